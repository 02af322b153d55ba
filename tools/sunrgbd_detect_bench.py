"""Times the SUN-RGBD inference tail behind the heads on one GPU -- decode (rule "sunrgbd") + rotated NMS per (frame, class) +
corners of the kept rows + matching + AP (detect.decode_detections, detect.rotate_nms_3d, detect.box3d_corners,
evaluate.match_detections_ap) -- for a validation-set-like load of synthetic head outputs, and, for context, the fp64 numpy
restatement of the same steps (tests/sunrgbd_detect_ref.py + oracle/box_ref.cube_nms: the reference's host loops) on the same
host and the same inputs.  The counterpart of tools/frustum_sunrgbd_bench.py, whose conventions it keeps.

python tools/sunrgbd_detect_bench.py [--frames 500] [--boxes 8] [--l2 40] [--iters 20] [--thresh 0.1] [--limit 900] [--no-host]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per child and one summary line.  The device child fails without a GPU; nothing falls back.

Load: `frames` images with `boxes` 2-D detections each (classes drawn from ten), L2 = 40 head rows per frustum (8 m at the 0.2 m
stride of cfgs/det_sample_sunrgbd.yaml).  Each frustum looks at one object: the rows within 0.6 m of its depth are foreground
and predict its box up to a few centimetres, so the NMS sees the clusters a trained model produces.  One in four objects is looked
at by two 2-D boxes; every object is a label box, one in five label boxes has no 2-D box.
Times: host wall clock per stage, synchronised, medians over --iters rounds after three warm-up rounds; `keep_read` is the read of
the keep lists between the NMS and the corners (it sizes the corner buffer).  A record for EXPERIMENTS.md; no test depends on a
time."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NB, NS, C = 12, 10, 10
MEAN_SIZE = np.array([[0.76, 1.4, 0.5], [2.1, 1.6, 0.9], [0.4, 1.2, 1.8], [0.6, 0.6, 0.8], [0.7, 1.4, 0.75], [0.5, 1.0, 1.0],
                      [0.5, 0.5, 0.6], [0.9, 1.9, 0.8], [0.8, 1.3, 0.7], [0.7, 0.45, 0.8]])


def scene(frames, boxes, L2, seed=3):
    """-> logits (B*L2, 69) float32, ref2 (B,3,L2), rot (B), rgb (B), unit_group (B), group_class (G), label rows (ng,7), their
    group (ng) -- groups are (frame, class); label-only groups come behind the detected ones."""
    rng = np.random.RandomState(seed)
    per = 2 * np.pi / NB
    lg_all, ref_all, rot_all, keys, labels, label_key = [], [], [], [], [], []
    z = (np.arange(L2) + 0.5) * (8.0 / L2)
    for f in range(frames):
        b = 0
        while b < boxes:
            c = rng.randint(C)
            size = MEAN_SIZE[c] * rng.uniform(0.85, 1.15, 3)
            obj = np.concatenate([[rng.uniform(-0.5, 0.5), rng.uniform(-0.2, 0.4), rng.uniform(1.5, 7.0)], size, [rng.uniform(-np.pi, np.pi)]])
            rot = rng.uniform(-0.5, 0.5)
            views = 2 if (rng.randint(4) == 0 and b + 1 < boxes) else 1
            cr, sr = np.cos(rot), np.sin(rot)                      # the object in label coordinates: rotate the frustum's by -rot
            labels.append(np.concatenate([[cr * obj[0] + sr * obj[2], obj[1], -sr * obj[0] + cr * obj[2]], size, [obj[6] + rot]]))
            label_key.append((f, c))
            for _ in range(views):
                lg = rng.normal(0, 0.5, (L2, 2 + 3 + 2 * NB + 4 * NS)).astype(np.float32)
                ref2 = np.stack([np.zeros(L2), np.zeros(L2), z])
                near = np.abs(z - obj[2]) < 0.6
                lg[:, 0], lg[:, 1] = np.where(near, -2.0, 2.0) + rng.normal(0, 0.3, L2), np.where(near, 2.0, -2.0) + rng.normal(0, 0.3, L2)
                lg[:, 2:5] = (obj[:3][None] - ref2.T) + rng.normal(0, 0.04, (L2, 3))
                ang = obj[6] % (2 * np.pi)
                k = int(np.round(ang / per)) % NB
                lg[:, 5 + k] += 6.0
                res = ang - k * per
                res = res - 2 * np.pi if res > np.pi else res
                lg[:, 5 + NB + k] = res / (per / 2) + rng.normal(0, 0.02, L2)
                lg[:, 5 + 2 * NB + c] += 6.0
                lg[:, 5 + 2 * NB + NS + 3 * c:5 + 2 * NB + NS + 3 * c + 3] = (size / MEAN_SIZE[c] - 1.0)[None] + rng.normal(0, 0.03, (L2, 3))
                lg_all.append(lg); ref_all.append(ref2); rot_all.append(rot); keys.append((f, c))
                b += 1
        for _ in range(max(1, boxes // 5)):                        # label boxes nobody looked at
            c = rng.randint(C)
            labels.append(np.concatenate([[rng.uniform(-3, 3), rng.uniform(-0.2, 0.4), rng.uniform(1.5, 7.0)], MEAN_SIZE[c], [rng.uniform(-3, 3)]]))
            label_key.append((f, c))
    groups = sorted(set(keys))
    groups += sorted(set(label_key) - set(groups))
    index = {k: i for i, k in enumerate(groups)}
    B = len(keys)
    return {"logits": np.concatenate(lg_all), "ref2": np.stack(ref_all).astype(np.float32), "rot": np.asarray(rot_all, dtype=np.float32),
            "rgb": rng.uniform(0.3, 1.0, B).astype(np.float32), "unit_group": np.asarray([index[k] for k in keys], dtype=np.int32),
            "group_class": np.asarray([k[1] for k in groups], dtype=np.int64), "labels": np.stack(labels),
            "label_group": np.asarray([index[k] for k in label_key], dtype=np.int64), "G_det": len(set(keys)), "B": B, "L2": L2}


def label_csr(sc):
    import sunrgbd_detect_ref as ref
    G = len(sc["group_class"])
    order = np.argsort(sc["label_group"], kind="stable")
    goff = np.concatenate([[0], np.cumsum(np.bincount(sc["label_group"], minlength=G))]).astype(np.int64)
    return ref.corners(sc["labels"][order]).astype(np.float32), goff


def every_class_is_labelled(sc):
    """eval_det evaluates the classes of the label boxes; with ten classes and hundreds of label boxes that is every class."""
    assert len(np.unique(sc["group_class"][np.unique(sc["label_group"])])) == C


def device_child(a):
    import torch
    from frustum_convnet_amd import detect, evaluate
    assert torch.cuda.is_available(), "the device measurement needs an MI355X"
    dev = torch.device("cuda:0")
    sc = scene(a.frames, a.boxes, a.l2)
    every_class_is_labelled(sc)
    gt_c, goff = label_csr(sc)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    lg, ref2, rot, rgb, ug = (up(sc[k]) for k in ("logits", "ref2", "rot", "rgb", "unit_group"))
    ms, gt = up(MEAN_SIZE.astype(np.float32)), up(gt_c)
    G, Gd, L2 = len(sc["group_class"]), sc["G_det"], sc["L2"]
    stages = {k: [] for k in ("decode", "nms", "keep_read", "corners", "match_ap", "total")}
    out = None
    for it in range(-3, a.iters):
        torch.cuda.synchronize()
        t = [time.perf_counter()]

        def lap():
            torch.cuda.synchronize()
            t.append(time.perf_counter())
        dets, valid = detect.decode_detections(lg, ref2, ms, rot, None, rgb, NB, NS, "nms", rule="sunrgbd"); lap()
        keep, cnt = detect.rotate_nms_3d(dets, valid, ug, L2, Gd, a.thresh, 300); lap()
        keep_h, cnt_h = keep.cpu().numpy(), cnt.cpu().numpy().astype(np.int64)
        assert (cnt_h >= 0).all()
        rows = np.concatenate([keep_h[g, :cnt_h[g]] for g in range(Gd)]).astype(np.int64)
        rows_d = torch.from_numpy(rows).to(dev); lap()
        cor = detect.box3d_corners(dets, rows_d)
        scores = dets[:, 7].index_select(0, rows_d); lap()
        doff = np.concatenate([[0], np.cumsum(cnt_h), np.full(G - Gd, cnt_h.sum())]).astype(np.int64)
        out = evaluate.match_detections_ap(cor, scores, doff, gt, goff, sc["group_class"], C, 0.25); lap()
        if it >= 0:
            for k, (x, y) in zip(("decode", "nms", "keep_read", "corners", "match_ap"), zip(t[:-1], t[1:])):
                stages[k].append((y - x) * 1e6)
            stages["total"].append((t[-1] - t[0]) * 1e6)
    print(json.dumps({"what": "device", "frames": a.frames, "frustums": sc["B"], "rows": sc["B"] * L2, "candidates": int(valid.sum()),
                      "groups": G, "kept": int(len(rows)), "label_boxes": int(len(gt_c)), "tp": int(out["tp"].sum()),
                      **{k + "_us": round(float(np.median(v)), 1) for k, v in stages.items()},
                      "ap": [round(float(x), 9) for x in out["ap"].cpu().numpy()]}), flush=True)


def host_child(a):
    import sunrgbd_detect_ref as ref
    from oracle import box_ref
    sc = scene(a.frames, a.boxes, a.l2)
    gt_c, goff = label_csr(sc)
    G, Gd, L2 = len(sc["group_class"]), sc["G_det"], sc["L2"]
    t = [time.perf_counter()]
    dets, sel, valid, _ = ref.decode(sc["logits"], sc["ref2"], MEAN_SIZE, sc["rot"], None, sc["rgb"], NB, NS, "nms")
    t.append(time.perf_counter())
    row_group = np.repeat(sc["unit_group"], L2)
    rows, cnt = [], []
    for g in range(Gd):
        cand = np.nonzero((row_group == g) & valid)[0]
        k = cand[np.asarray(box_ref.cube_nms(dets[cand], a.thresh), dtype=np.int64)] if len(cand) else cand
        rows.append(k); cnt.append(len(k))
    rows = np.concatenate(rows)
    t.append(time.perf_counter())
    cor = ref.corners(dets[rows]).astype(np.float32)
    t.append(time.perf_counter())
    doff = np.concatenate([[0], np.cumsum(cnt), np.full(G - Gd, sum(cnt))]).astype(np.int64)
    out = ref.evaluate(cor, dets[rows, 7].astype(np.float32), doff, gt_c, goff, sc["group_class"], C, 0.25)
    t.append(time.perf_counter())
    us = [(y - x) * 1e6 for x, y in zip(t[:-1], t[1:])]
    print(json.dumps({"what": "host_numpy", "candidates": int(valid.sum()), "kept": int(len(rows)), "tp": int(out["tp"].sum()),
                      "decode_us": round(us[0], 1), "nms_us": round(us[1], 1), "corners_us": round(us[2], 1), "match_ap_us": round(us[3], 1),
                      "total_us": round(sum(us), 1), "ap": [round(float(x), 9) for x in out["ap"]]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=500)
    ap.add_argument("--boxes", type=int, default=8)
    ap.add_argument("--l2", type=int, default=40)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--thresh", type=float, default=0.1)
    ap.add_argument("--limit", type=float, default=900.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child", choices=("device", "host"))
    a = ap.parse_args()
    if a.child:
        return (device_child if a.child == "device" else host_child)(a)
    rows = {}
    for which in ("device",) if a.no_host else ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [x for k in ("frames", "boxes", "l2", "iters", "thresh")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": which, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
        rows[which] = json.loads(p.stdout.strip().splitlines()[-1])
    if "host" in rows:
        dv, hs = rows["device"], rows["host"]
        print(json.dumps({"what": "summary", "device_total_us": dv["total_us"], "host_numpy_total_us": hs["total_us"],
                          "same_kept": dv["kept"] == hs["kept"], "same_tp": dv["tp"] == hs["tp"],
                          "ap_max_abs_diff": float(np.abs(np.asarray(dv["ap"]) - np.asarray(hs["ap"])).max())}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
