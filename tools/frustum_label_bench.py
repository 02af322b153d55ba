"""Times the labelled frustum extraction (frustum.frustum_training_candidates: fcn_frustum_label_count + the read of the 2 * D * S
selected and positive segment counts + fcn_frustum_label_fill) against the unlabelled one (frustum.frustum_candidates:
fcn_frustum_select_count / _fill) on the same scene, on one GPU: one full-size LiDAR frame and --boxes ground-truth boxes, each with
the 2-D box its corners project to.  The expectation to test: labelling costs next to nothing over selection, since the in-box test
runs on selected rows only.

python tools/frustum_label_bench.py [--points 120000] [--boxes 32] [--iters 200] [--limit 120]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per child and one summary line.  The children fail without a GPU; nothing falls back.

Times: `call` figures are device-event times around one entry point (they include the entry's read-back of box_frame and
frame_off, so they bound the kernel time from above); `candidates` is the host wall clock of the Python function per call,
synchronised.  Neither child clips the boxes (the training path never does), so both select the same rows.
A record for EXPERIMENTS.md; no test depends on a time.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from frustum_select_bench import P2, R0, V2C, W, H  # noqa: E402


def scene(points, boxes, seed=1):
    """One sweep of `points` rows (x, y, z, intensity) all around the car, 70 m out; `boxes` car-sized ground-truth boxes on the
    ground in front of the camera (rect camera coordinates, t the bottom centre) and the bounding rectangles of their projected
    corners, as a label file has them."""
    rng = np.random.RandomState(seed)
    r, a = rng.uniform(2.0, 70.0, points), rng.uniform(-np.pi, np.pi, points)
    pts = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 0.5, points), rng.uniform(0, 1, points)], 1).astype(np.float32)
    tz = rng.uniform(8.0, 50.0, boxes)
    gt = np.stack([rng.uniform(-0.4, 0.4, boxes) * tz, rng.uniform(1.4, 1.9, boxes), tz, rng.uniform(3.4, 4.4, boxes),
                   rng.uniform(1.5, 1.8, boxes), rng.uniform(1.4, 1.7, boxes), rng.uniform(-np.pi, np.pi, boxes)], 1)
    b2d = np.zeros((boxes, 4))
    for d, (tx, ty, tz_, l, w, h, ry) in enumerate(gt):
        c, s = np.cos(ry), np.sin(ry)
        xc = np.array([l / 2, l / 2, -l / 2, -l / 2] * 2)
        zc = np.array([w / 2, -w / 2, -w / 2, w / 2] * 2)
        cor = np.stack([c * xc + s * zc + tx, np.array([0.0] * 4 + [-h] * 4) + ty, -s * xc + c * zc + tz_, np.ones(8)])
        img = P2 @ cor
        u, v = img[0] / img[2], img[1] / img[2]
        b2d[d] = [u.min(), v.min(), u.max(), v.max()]
    return pts, np.array([0, points], dtype=np.int64), b2d, gt, np.zeros(boxes, dtype=np.int32)


def child(a):
    import torch
    from frustum_convnet_amd import _native, frustum
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    labelled = a.child == "labelled"
    pts, off, boxes, gt, bframe = scene(a.points, a.boxes)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_pts, t_off, t_gt, t_bf = up(pts), up(off), up(gt), up(bframe)
    cal = {"P": up(P2[None]), "V2C": up(V2C[None]), "R0": up(R0[None])}
    wh = up(np.array([[W, H]]))
    if labelled:                       # (boxes on the host: the reject rule reads them there)
        run = lambda: frustum.frustum_training_candidates(t_pts, t_off, cal, wh, boxes, t_bf, t_gt, min_box_height=0.0)
    else:
        run = lambda: frustum.frustum_candidates(t_pts, t_off, cal, wh, boxes, t_bf, clip_boxes=False)
    res = run()
    torch.cuda.synchronize()
    L, s = _native.lib(), _native.current_stream(dev)
    D, ps = len(bframe), pts.shape[1]
    S = -(-a.points // int(L.fcn_frustum_select_seg()))
    t_box = up(boxes)
    f64 = dict(dtype=torch.float64, device=dev)
    box2d, angle, corners = torch.zeros((D, 4), **f64), torch.zeros((D,), **f64), torch.zeros((D, 24), **f64)
    scnt, spos = (torch.zeros((D, S), dtype=torch.int32, device=dev) for _ in range(2))
    common = (t_pts.data_ptr(), t_off.data_ptr(), 1, ps, cal["P"].data_ptr(), cal["V2C"].data_ptr(), cal["R0"].data_ptr(),
              wh.data_ptr(), t_box.data_ptr(), t_bf.data_ptr(), D, S, 0, 2.0)
    if labelled:
        count = lambda: _native.check(L.fcn_frustum_label_count(*common, t_gt.data_ptr(), box2d.data_ptr(), angle.data_ptr(),
                                                                scnt.data_ptr(), spos.data_ptr(), corners.data_ptr(), s), "count")
    else:
        count = lambda: _native.check(L.fcn_frustum_select_count(*common, box2d.data_ptr(), angle.data_ptr(), scnt.data_ptr(), s), "count")
    count()
    soff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), scnt.reshape(-1).to(torch.int64).cumsum(0)])
    total = int(soff[-1])
    out = torch.empty((total, ps), dtype=torch.float32, device=dev)
    oseg = torch.empty((total,), dtype=torch.int64, device=dev)
    if labelled:
        fill = lambda: _native.check(L.fcn_frustum_label_fill(*common, t_gt.data_ptr(), soff.data_ptr(), out.data_ptr(),
                                                              oseg.data_ptr(), s), "fill")
    else:
        fill = lambda: _native.check(L.fcn_frustum_select_fill(*common, soff.data_ptr(), out.data_ptr(), s), "fill")
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.iters)]
    for it in range(-10, a.iters):                                 # ten warm-up rounds
        e = ev[max(it, 0)]
        e[0].record()
        count()
        e[1].record()
        fill()
        e[2].record()
    torch.cuda.synchronize()
    count_us = np.median([e[0].elapsed_time(e[1]) for e in ev]) * 1e3
    fill_us = np.median([e[1].elapsed_time(e[2]) for e in ev]) * 1e3
    t0 = time.perf_counter()
    for _ in range(a.iters):
        run()
    torch.cuda.synchronize()
    cand_us = (time.perf_counter() - t0) / a.iters * 1e6
    row = {"what": a.child, "points": a.points, "boxes": D, "segments": S, "workgroups": S * D, "selected_rows": total,
           "count_call_us": round(float(count_us), 2), "fill_call_us": round(float(fill_us), 2), "candidates_us": round(cand_us, 2)}
    if labelled:
        row.update(positive_rows=int(spos.sum()), labels_set=int(oseg.sum()), kept=len(res["kept"]))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--child", choices=("labelled", "unlabelled"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    rows = {}
    for which in ("unlabelled", "labelled"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [x for k in ("points", "boxes", "iters")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": which, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
        rows[which] = json.loads(p.stdout.strip().splitlines()[-1])
    un, lb = rows["unlabelled"], rows["labelled"]
    print(json.dumps({"what": "summary", "same_rows": un["selected_rows"] == lb["selected_rows"],
                      "labels_consistent": lb["positive_rows"] == lb["labels_set"],
                      "count_call_us": [un["count_call_us"], lb["count_call_us"]],
                      "fill_call_us": [un["fill_call_us"], lb["fill_call_us"]],
                      "candidates_us": [un["candidates_us"], lb["candidates_us"]]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
