"""Times the KITTI evaluation on one GPU -- evaluate.kitti_eval end to end and its five launches one by one (fcn_kitti_overlaps,
_pass_a, _thresholds, _pass_b, _curves; csrc/kitti_eval.h) -- for a synthetic scene of the size of the KITTI validation split, and,
for context, the project's fp64 numpy restatement of the reference's evaluator (tests/kitti_eval_ref.py) on the same host's CPU
and the same scene.  The counterpart of tools/sunrgbd_detect_bench.py, whose conventions it keeps.

THE CPU SIDE IS THE PROJECT'S PYTHON RESTATEMENT, NOT THE REFERENCE'S BOOST BINARY (train/kitti_eval/evaluate_object_3d_offline.cpp
needs boost::geometry, which this project's build machines lack): it says what the referee of the tests costs, not what the
reference costs.

python tools/kitti_eval_bench.py [--frames 3769] [--labels 8] [--dets 10] [--iters 20] [--limit 1500] [--no-host]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per child and one summary line.  The device child fails without a GPU; nothing falls back.

Scene: `frames` frames with about `labels` labels (all seven types) and about `dets` detections each, 70 % of them about a label.
It is drawn without the knife-edge redraws of tests/kitti_eval_scenes.py (they cost more than the measurement), so a count may
differ between the fp32 device and the fp64 restatement where an overlap sits on a threshold; the summary line says how many do.
Times: hipEvent pairs on the current stream, medians over --iters rounds after three warm-up rounds; `end_to_end_us` is
evaluate.kitti_eval as a caller sees it (uploads of the offsets, allocation and zeroing of its buffers, five launches).  A record
for EXPERIMENTS.md; no test depends on a time."""
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


def scene(frames, labels, dets, seed=3):
    import kitti_eval_ref as ref
    import kitti_eval_scenes as scenes
    rng = np.random.default_rng(seed)
    own = {ref.CAR: 0, ref.VAN: 0, ref.PEDESTRIAN: 1, ref.PERSON_SITTING: 1, ref.CYCLIST: 2, ref.DONTCARE: 0, ref.OTHER: 0}
    out = []
    for _ in range(frames):
        types = [scenes.ALL_TYPES[i] for i in rng.choice(7, max(0, labels + rng.integers(-3, 4)), p=[0.45, 0.15, 0.1, 0.1, 0.05, 0.1, 0.05])]
        gt = [scenes.label(rng, t) for t in types]
        det, cls = [], []
        for _ in range(max(0, dets + rng.integers(-4, 5))):
            if gt and rng.uniform() < 0.7:
                i = rng.integers(len(gt))
                det.append(scenes.detection(rng, gt[i], rng.choice([0.02, 0.05, 0.12]), rng.uniform(0.05, 2.0)))
                cls.append(own[types[i]])
            else:
                t = [ref.CAR, ref.PEDESTRIAN, ref.CYCLIST][rng.integers(3)]
                det.append(scenes.detection(rng, scenes.label(rng, t), 0.0, rng.uniform(0.05, 2.0)))
                cls.append(own[t])
        out.append((np.asarray(det).reshape(-1, 13), np.asarray(cls, np.int32), np.asarray(gt).reshape(-1, 14), np.asarray(types, np.int32)))
    return scenes.pack(out)


def _summary(o):
    return {"n_gt": np.asarray(o["n_gt"]).tolist(), "num_thresholds": np.asarray(o["num_thresholds"]).tolist(),
            "tp_sum": int(np.asarray(o["tp"]).sum()), "fp_sum": int(np.asarray(o["fp"]).sum()), "fn_sum": int(np.asarray(o["fn"]).sum()),
            "ap": [round(float(x), 6) for x in np.asarray(o["ap"]).reshape(-1)]}


def device_child(a):
    import torch
    from frustum_convnet_amd import _native, evaluate
    assert torch.cuda.is_available(), "the device measurement needs an MI355X"
    dev = torch.device("cuda:0")
    sc = scene(a.frames, a.labels, a.dets)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    det, cls, gt, typ = up(sc["det"]), up(sc["det_class"]), up(sc["gt"]), up(sc["gt_type"])
    nd, ng, F = len(sc["det"]), len(sc["gt"]), len(sc["det_off"]) - 1
    ev = lambda: torch.cuda.Event(enable_timing=True)
    total, out = [], None
    for it in range(-3, a.iters):
        e0, e1 = ev(), ev()
        e0.record()
        out = evaluate.kitti_eval(det, cls, sc["det_off"], gt, typ, sc["gt_off"])
        e1.record()
        torch.cuda.synchronize()
        if it >= 0:
            total.append(e0.elapsed_time(e1) * 1e3)
    # the five launches one by one, on buffers allocated once
    poff = out["pair_off"]
    npairs = int(poff[-1])
    doff, goff, pof = up(sc["det_off"].astype(np.int32)), up(sc["gt_off"].astype(np.int32)), up(poff.astype(np.int32))
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    b = {"ov": z((npairs, 3), f32), "flags": z((10,), i32), "asg": z((27, nd, 2), i32), "tps": z((27, ng), f32), "srt": z((27, ng), f32),
         "tpc": z((27,), i32), "ngt": z((27,), i32), "nthr": z((27,), i32), "thr": z((27, 41), f64), "cnt": z((3, 27, 41), i32),
         "sim": z((F, 9, 41), f64), "prec": z((27, 41), f64), "aos": z((9, 41), f64), "ap": z((27,), f64), "aap": z((9,), f64)}
    p = lambda t: t.data_ptr() if t.numel() else None
    L, s = _native.lib(), _native.current_stream(dev)
    scn = (p(doff), p(goff), p(pof), F, p(det), p(cls), nd, p(gt), p(typ), ng, p(b["ov"]), npairs)
    calls = [("overlaps", lambda: L.fcn_kitti_overlaps(*scn, p(b["flags"]), s)),
             ("pass_a", lambda: L.fcn_kitti_pass_a(*scn, 7, p(b["asg"]), p(b["tps"]), p(b["tpc"]), p(b["ngt"]), s)),
             ("thresholds", lambda: L.fcn_kitti_thresholds(p(b["tps"]), p(b["tpc"]), p(b["ngt"]), ng, p(b["srt"]), p(b["thr"]), p(b["nthr"]), s)),
             ("pass_b", lambda: L.fcn_kitti_pass_b(*scn, 7, p(b["thr"]), p(b["nthr"]), p(b["asg"]), p(b["cnt"]), p(b["sim"]), s)),
             ("curves", lambda: L.fcn_kitti_curves(p(b["cnt"]), p(b["nthr"]), p(b["sim"]), F, p(b["flags"]), 7, p(b["prec"]), p(b["aos"]),
                                                   p(b["ap"]), p(b["aap"]), s))]
    split = {k: [] for k, _ in calls}
    for it in range(-3, a.iters):
        evs = [ev() for _ in range(len(calls) + 1)]
        evs[0].record()
        for i, (k, fn) in enumerate(calls):
            assert fn() == 0, k
            evs[i + 1].record()
        torch.cuda.synchronize()
        if it >= 0:
            for i, (k, _) in enumerate(calls):
                split[k].append(evs[i].elapsed_time(evs[i + 1]) * 1e3)
    assert torch.equal(b["ap"].view(3, 3, 3), out["ap"]) or bool(torch.isnan(out["ap"]).any())
    print(json.dumps({"what": "device", "frames": F, "detections": nd, "labels": ng, "pairs": npairs,
                      "end_to_end_us": round(float(np.median(total)), 1),
                      **{k + "_us": round(float(np.median(v)), 1) for k, v in split.items()},
                      "launches_us": round(float(sum(np.median(v) for v in split.values())), 1),
                      **_summary({k: v.cpu().numpy() if torch.is_tensor(v) else v for k, v in out.items()})}), flush=True)


def host_child(a):
    import kitti_eval_ref as ref
    sc = scene(a.frames, a.labels, a.dets)
    t0 = time.perf_counter()
    out = ref.evaluate(sc["det"], sc["det_class"], sc["det_off"], sc["gt"], sc["gt_type"], sc["gt_off"])
    t1 = time.perf_counter()
    print(json.dumps({"what": "host_numpy_restatement", "total_us": round((t1 - t0) * 1e6, 1), **_summary(out)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--labels", type=int, default=8)
    ap.add_argument("--dets", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--limit", type=float, default=1500.0)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child", choices=("device", "host"))
    a = ap.parse_args()
    if a.child:
        return (device_child if a.child == "device" else host_child)(a)
    rows = {}
    for which in ("device",) if a.no_host else ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [x for k in ("frames", "labels", "dets", "iters")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": which, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
        rows[which] = json.loads(p.stdout.strip().splitlines()[-1])
    if "host" in rows:
        dv, hs = rows["device"], rows["host"]
        dap, hap = np.asarray(dv["ap"], dtype=np.float64), np.asarray(hs["ap"], dtype=np.float64)
        print(json.dumps({"what": "summary", "device_end_to_end_us": dv["end_to_end_us"], "host_numpy_restatement_us": hs["total_us"],
                          "lists_with_other_thresholds": int((np.asarray(dv["num_thresholds"]) != np.asarray(hs["num_thresholds"])).sum()),
                          "same_n_gt": dv["n_gt"] == hs["n_gt"], "tp_fp_fn_device": [dv["tp_sum"], dv["fp_sum"], dv["fn_sum"]],
                          "tp_fp_fn_host": [hs["tp_sum"], hs["fp_sum"], hs["fn_sum"]],
                          "ap_max_abs_diff": float(np.nanmax(np.abs(dap - hap)))}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
