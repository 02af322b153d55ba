"""Times the frustum extraction (frustum.frustum_candidates: fcn_frustum_select_count + the read of D * S segment counts +
fcn_frustum_select_fill) on one GPU for one full-size LiDAR frame and a 2-D detector's boxes, and, for context, the reference-style
host selection of the same inputs in numpy (project the frame once, mask it once per box: kitti/prepare_data.py:504-548).

python tools/frustum_select_bench.py [--points 120000] [--boxes 32] [--iters 200] [--limit 120]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per child and one summary line.  The device child fails without a GPU; nothing falls back.

Times: `call` figures are device-event times around one entry point (they include the entry's read-back of box_frame and
frame_off, so they bound the kernel time from above); `candidates` is the host wall clock of frustum_candidates per call,
synchronised.  Bytes: what the launches move when the frame comes from HBM once per pass over it -- the count launch passes over
the frame once, the fill launch twice (it counts its quarters again before it writes), and the selected rows are written once;
the boxes of one frame share it through the caches -- over the time, against the 8 TB/s HBM3E peak of the data sheet.
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

HBM_PEAK = 8.0e12          # bytes/s, MI355X data sheet
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
W, H = 1242.0, 375.0


def scene(points, boxes, seed=1):
    """One sweep of `points` rows (x, y, z, intensity) all around the car, 70 m out; `boxes` car-sized 2-D boxes in the image."""
    rng = np.random.RandomState(seed)
    r, a = rng.uniform(2.0, 70.0, points), rng.uniform(-np.pi, np.pi, points)
    pts = np.stack([r * np.cos(a), r * np.sin(a), rng.uniform(-2.0, 0.5, points), rng.uniform(0, 1, points)], 1).astype(np.float32)
    cx, cy = rng.uniform(60, W - 60, boxes), rng.uniform(150, 260, boxes)
    w, h = rng.uniform(40, 240, boxes), rng.uniform(30, 150, boxes)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    return pts, np.array([0, points], dtype=np.int64), b, np.zeros(boxes, dtype=np.int32)


def device_child(a):
    import torch
    from frustum_convnet_amd import _native, frustum
    assert torch.cuda.is_available(), "the device measurement needs an MI355X"
    dev = torch.device("cuda:0")
    pts, off, boxes, bframe = scene(a.points, a.boxes)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_pts, t_off, t_box, t_bf = up(pts), up(off), up(boxes), up(bframe)
    cal = {"P": up(P2[None]), "V2C": up(V2C[None]), "R0": up(R0[None])}
    wh = up(np.array([[W, H]]))
    res = frustum.frustum_candidates(t_pts, t_off, cal, wh, t_box, t_bf)
    torch.cuda.synchronize()
    counts = res["counts"]
    L, s = _native.lib(), _native.current_stream(dev)
    D, ps = len(bframe), pts.shape[1]
    seg = int(L.fcn_frustum_select_seg())
    S = -(-a.points // seg)
    scnt = torch.zeros((D, S), dtype=torch.int32, device=dev)
    common = (t_pts.data_ptr(), t_off.data_ptr(), 1, ps, cal["P"].data_ptr(), cal["V2C"].data_ptr(), cal["R0"].data_ptr(),
              wh.data_ptr(), t_box.data_ptr(), t_bf.data_ptr(), D, S, 1, 2.0)
    _native.check(L.fcn_frustum_select_count(*common, res["box2d"].data_ptr(), res["frustum_angle"].data_ptr(), scnt.data_ptr(), s), "count")
    soff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), scnt.reshape(-1).to(torch.int64).cumsum(0)])
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.iters)]
    for it in range(-10, a.iters):                                 # ten warm-up rounds
        e = ev[max(it, 0)]
        e[0].record()
        _native.check(L.fcn_frustum_select_count(*common, res["box2d"].data_ptr(), res["frustum_angle"].data_ptr(),
                                                 scnt.data_ptr(), s), "count")
        e[1].record()
        _native.check(L.fcn_frustum_select_fill(*common, soff.data_ptr(), res["points"].data_ptr(), s), "fill")
        e[2].record()
    torch.cuda.synchronize()
    count_us = np.median([e[0].elapsed_time(e[1]) for e in ev]) * 1e3
    fill_us = np.median([e[1].elapsed_time(e[2]) for e in ev]) * 1e3
    t0 = time.perf_counter()
    for _ in range(a.iters):
        frustum.frustum_candidates(t_pts, t_off, cal, wh, t_box, t_bf)
    torch.cuda.synchronize()
    cand_us = (time.perf_counter() - t0) / a.iters * 1e6
    nbytes = 3 * a.points * ps * 4 + int(counts.sum()) * ps * 4      # count: one pass; fill: two passes + the rows written
    print(json.dumps({"what": "device", "points": a.points, "boxes": D, "segments": S, "workgroups": S * D,
                      "selected_rows": int(counts.sum()), "count_call_us": round(float(count_us), 2),
                      "fill_call_us": round(float(fill_us), 2), "candidates_us": round(cand_us, 2), "bytes": nbytes,
                      "hbm_fraction_of_calls": round(nbytes / ((count_us + fill_us) * 1e-6) / HBM_PEAK, 5)}), flush=True)


def host_child(a):
    pts, off, boxes, bframe = scene(a.points, a.boxes)
    t0 = time.perf_counter()
    hom = np.hstack((pts[:, :3], np.ones((len(pts), 1))))
    rect = np.dot(R0, np.dot(hom, V2C.T).T).T
    img = np.dot(np.hstack((rect, np.ones((len(pts), 1)))), P2.T)
    u, v = img[:, 0] / img[:, 2], img[:, 1] / img[:, 2]
    pc_rect = np.zeros_like(pts)
    pc_rect[:, :3], pc_rect[:, 3] = rect, pts[:, 3]
    fov = (u < W) & (u >= 0) & (v < H) & (v >= 0) & (pts[:, 0] > 2.0)
    total = 0
    for b in boxes:
        x0, x1 = np.clip(b[[0, 2]], 0, W - 1)
        y0, y1 = np.clip(b[[1, 3]], 0, H - 1)
        total += len(pc_rect[(u < x1) & (u >= x0) & (v < y1) & (v >= y0) & fov])
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "host_numpy", "boxes": len(boxes), "selected_rows": total, "us": round(dt * 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=120000)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--child", choices=("device", "host"))
    a = ap.parse_args()
    if a.child:
        return (device_child if a.child == "device" else host_child)(a)
    rows = {}
    for which in ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [x for k in ("points", "boxes", "iters")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": which, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
        rows[which] = json.loads(p.stdout.strip().splitlines()[-1])
    dv, hs = rows["device"], rows["host"]
    print(json.dumps({"what": "summary", "device_candidates_us": dv["candidates_us"], "host_numpy_us": hs["us"],
                      "same_rows": dv["selected_rows"] == hs["selected_rows"]}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
