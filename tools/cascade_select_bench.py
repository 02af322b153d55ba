"""Times the cascade link (cascade.refine_candidates: fcn_refine_select_count + the read of D counts + fcn_refine_select_fill) on
one GPU at a KITTI-like size, and, for context, the reference-style host selection of the same inputs (scipy.spatial.Delaunay
find_simplex over the frame's whole point cloud, once per box: kitti/prepare_data_refine.py:120-130, :729).

python tools/cascade_select_bench.py [--frames 8] [--points 20000] [--cands 64] [--iters 200] [--limit 120]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per child and one summary line.  The device child fails without a GPU; nothing falls back.

Times: `call` figures are device-event times around one entry point (they include the entry's read-back of the 2 * D candidate
indices, so they bound the kernel time from above); `link` is the host wall clock of refine_candidates per call, synchronised.
Bytes: what the launches move when every frame comes from HBM once per pass over it -- the count launch passes over a searched
frame once, the fill launch twice (it counts its quarters again before it writes), and the selected rows are written once;
candidates of one frame share it through the caches -- over the time, against the 8 TB/s HBM3E peak of the data sheet.
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

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet


def scene(frames, points, cands, seed=1):
    """`frames` scans of `points` rows (x, y, z, intensity) in a 80 m x 4 m x 70 m field of view; `cands` car-sized first-stage rows
    centred on scan points, spread over the frames."""
    rng = np.random.RandomState(seed)
    n = frames * points
    pts = np.stack([rng.uniform(-40, 40, n), rng.uniform(-1, 3, n), rng.uniform(0, 70, n), rng.uniform(0, 1, n)], 1).astype(np.float32)
    off = (np.arange(frames + 1) * points).astype(np.int64)
    cframe = (np.arange(cands) % frames).astype(np.int32)
    at = pts[cframe.astype(np.int64) * points + rng.randint(0, points, cands), :3]
    lwh = np.array([3.88, 1.63, 1.53]) * rng.uniform(0.8, 1.2, (cands, 3))
    dets = np.concatenate([at[:, :1], at[:, 1:2] + lwh[:, 2:3] / 2, at[:, 2:3], lwh, rng.uniform(-np.pi, np.pi, (cands, 1)),
                           rng.uniform(0, 1, (cands, 1))], 1).astype(np.float32)
    return pts, off, dets, np.arange(cands, dtype=np.int32), cframe


def device_child(a):
    import torch
    from frustum_convnet_amd import _native, cascade
    assert torch.cuda.is_available(), "the device measurement needs an MI355X"
    dev = torch.device("cuda:0")
    pts, off, dets, crow, cframe = scene(a.frames, a.points, a.cands)
    t = [torch.from_numpy(x).to(dev) for x in (pts, off, dets, crow, cframe)]
    res = cascade.refine_candidates(*t)
    torch.cuda.synchronize()
    counts = res["counts"]
    L, s = _native.lib(), _native.current_stream(dev)
    D, ps = len(crow), pts.shape[1]
    common = (t[0].data_ptr(), t[1].data_ptr(), a.frames, ps, t[2].data_ptr(), len(dets), t[3].data_ptr(), t[4].data_ptr(), D, 1.2)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.iters)]
    for it in range(-10, a.iters):                                 # ten warm-up rounds
        e = ev[max(it, 0)]
        e[0].record()
        _native.check(L.fcn_refine_select_count(*common, res["pred_box3d"].data_ptr(), res["pred_angle"].data_ptr(),
                                                res["pred_size"].data_ptr(), res["cnt"].data_ptr(), s), "count")
        e[1].record()
        _native.check(L.fcn_refine_select_fill(*common, res["off"].data_ptr(), res["points"].data_ptr(), s), "fill")
        e[2].record()
    torch.cuda.synchronize()
    count_us = np.median([e[0].elapsed_time(e[1]) for e in ev]) * 1e3
    fill_us = np.median([e[1].elapsed_time(e[2]) for e in ev]) * 1e3
    t0 = time.perf_counter()
    for _ in range(a.iters):
        cascade.refine_candidates(*t)
    torch.cuda.synchronize()
    link_us = (time.perf_counter() - t0) / a.iters * 1e6
    searched = len(set(cframe.tolist())) * a.points * ps * 4
    nbytes = 3 * searched + int(counts.sum()) * ps * 4           # count: one pass; fill: two passes + the rows written
    print(json.dumps({"what": "device", "frames": a.frames, "points": a.points, "cands": D, "selected_rows": int(counts.sum()),
                      "count_call_us": round(float(count_us), 2), "fill_call_us": round(float(fill_us), 2),
                      "link_us": round(link_us, 2), "bytes": nbytes,
                      "hbm_fraction_of_calls": round(nbytes / ((count_us + fill_us) * 1e-6) / HBM_PEAK, 5)}), flush=True)


def host_child(a):
    from scipy.spatial import Delaunay
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import cascade_ref
    pts, off, dets, crow, cframe = scene(a.frames, a.points, a.cands)
    t0 = time.perf_counter()
    total = 0
    for d in range(len(crow)):
        centre, size, ry = cascade_ref.enlarged_box(dets[crow[d]], 1.2)
        corners = cascade_ref.box_corners(centre, size, ry)
        frame = pts[off[cframe[d]]:off[cframe[d] + 1]]
        inds = Delaunay(corners).find_simplex(frame[:, :3]) >= 0
        total += len(frame[inds])
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "host_scipy", "cands": len(crow), "selected_rows": total, "seconds": round(dt, 4),
                      "us": round(dt * 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--child", choices=("device", "host"))
    a = ap.parse_args()
    if a.child:
        return (device_child if a.child == "device" else host_child)(a)
    rows = {}
    for which in ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [x for k in ("frames", "points", "cands", "iters")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": which, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
        rows[which] = json.loads(p.stdout.strip().splitlines()[-1])
    dv, hs = rows["device"], rows["host"]
    print(json.dumps({"what": "summary", "device_link_us": dv["link_us"], "host_scipy_us": hs["us"],
                      "same_rows": dv["selected_rows"] == hs["selected_rows"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
