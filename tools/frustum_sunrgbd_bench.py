"""Times the SUN-RGBD frustum extraction (frustum.sunrgbd_candidates: fcn_frustum_sunrgbd_count + the read of D * S segment counts
+ fcn_frustum_sunrgbd_fill, csrc/frustum_sunrgbd.h) on one GPU for full-size depth frames and a 2-D detector's boxes, and, for
context, the reference-style host selection of the same inputs in numpy (project each frame once, mask it once per box:
sunrgbd/prepare_data.py:298-334).  The counterpart of tools/frustum_select_bench.py, whose conventions it keeps.

python tools/frustum_sunrgbd_bench.py [--frames 8] [--points 300000] [--stride 6] [--boxes 64] [--iters 100] [--limit 240]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per child and one summary line.  The device child fails without a GPU; nothing falls back.

Times: `call` figures are device-event times around one entry point (they include the entry's read-back of box_frame and
frame_off, so they bound the kernel time from above); `candidates` is the host wall clock of sunrgbd_candidates per call,
synchronised (its subsample draws, which are host work of the caller's generator, are switched off).  Bytes -- the algorithmic
bytes, tools/frustum_select_bench.py's accounting: every frame that has a box comes from HBM once per pass over it (the count launch
passes once, the fill launch twice -- it counts its quarters again before it writes) and the selected rows are written once; the
boxes of one frame share it through the caches -- over the time, in GB/s and against the 8 TB/s HBM3E peak of the data sheet.
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
K0 = np.array([[529.5, 0.0, 365.0], [0.0, 529.5, 265.0], [0.0, 0.0, 1.0]])
W, H = 730.0, 530.0


def rot_x(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def scene(frames, points, stride, boxes, seed=1):
    """`frames` depth frames of `points` rows (upright depth x, y, z, then r, g, b, ...) in a room 8 m deep; `boxes` furniture-sized
    2-D boxes spread over the frames in turn."""
    rng = np.random.RandomState(seed)
    n = frames * points
    y = rng.uniform(0.8, 8.0, n)
    pts = np.concatenate([np.stack([y * rng.uniform(-0.7, 0.7, n), y, y * rng.uniform(-0.5, 0.5, n)], 1),
                          rng.uniform(0, 1, (n, stride - 3))], 1).astype(np.float32)
    off = (np.arange(frames + 1) * points).astype(np.int64)
    K = np.stack([K0 + np.array([[0, 0, rng.uniform(-5, 5)], [0, 0, rng.uniform(-5, 5)], [0, 0, 0]]) for _ in range(frames)])
    Rt = np.stack([rot_x(rng.uniform(-0.25, 0.25)) for _ in range(frames)])
    cx, cy = rng.uniform(80, W - 80, boxes), rng.uniform(80, H - 80, boxes)
    w, h = rng.uniform(60, 260, boxes), rng.uniform(60, 220, boxes)
    b = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], 1)
    return pts, off, K, Rt, b, (np.arange(boxes) % frames).astype(np.int32)


def device_child(a):
    import torch
    from frustum_convnet_amd import _native, frustum
    assert torch.cuda.is_available(), "the device measurement needs an MI355X"
    dev = torch.device("cuda:0")
    pts, off, K, Rt, boxes, bframe = scene(a.frames, a.points, a.stride, a.boxes)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_pts, t_off, t_K, t_R, t_box, t_bf = up(pts), up(off), up(K.reshape(-1, 9)), up(Rt.reshape(-1, 9)), up(boxes), up(bframe)
    res = frustum.sunrgbd_candidates(t_pts, t_off, t_K, t_R, t_box, t_bf, cap=1 << 62)
    torch.cuda.synchronize()
    counts = res["counts"]
    L, s = _native.lib(), _native.current_stream(dev)
    D, ps = len(bframe), pts.shape[1]
    seg = int(L.fcn_frustum_select_seg())
    S = -(-a.points // seg)
    scnt = torch.zeros((D, S), dtype=torch.int32, device=dev)
    common = (t_pts.data_ptr(), t_off.data_ptr(), a.frames, ps, t_K.data_ptr(), t_R.data_ptr(), t_box.data_ptr(), t_bf.data_ptr(), D, S)
    _native.check(L.fcn_frustum_sunrgbd_count(*common, res["frustum_angle"].data_ptr(), scnt.data_ptr(), s), "count")
    soff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), scnt.reshape(-1).to(torch.int64).cumsum(0)])
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(a.iters)]
    for it in range(-10, a.iters):                                 # ten warm-up rounds
        e = ev[max(it, 0)]
        e[0].record()
        _native.check(L.fcn_frustum_sunrgbd_count(*common, res["frustum_angle"].data_ptr(), scnt.data_ptr(), s), "count")
        e[1].record()
        _native.check(L.fcn_frustum_sunrgbd_fill(*common, soff.data_ptr(), res["points"].data_ptr(), s), "fill")
        e[2].record()
    torch.cuda.synchronize()
    count_us = np.median([e[0].elapsed_time(e[1]) for e in ev]) * 1e3
    fill_us = np.median([e[1].elapsed_time(e[2]) for e in ev]) * 1e3
    t0 = time.perf_counter()
    for _ in range(a.iters):
        frustum.sunrgbd_candidates(t_pts, t_off, t_K, t_R, t_box, t_bf, cap=1 << 62)
    torch.cuda.synchronize()
    cand_us = (time.perf_counter() - t0) / a.iters * 1e6
    used = len(set(bframe.tolist()))
    nbytes = 3 * used * a.points * ps * 4 + int(counts.sum()) * ps * 4   # count: one pass; fill: two passes + the rows written
    gbs = nbytes / ((count_us + fill_us) * 1e-6) / 1e9
    print(json.dumps({"what": "device", "frames": a.frames, "points": a.points, "stride": ps, "boxes": D, "segments": S,
                      "workgroups": S * D, "selected_rows": int(counts.sum()), "count_call_us": round(float(count_us), 2),
                      "fill_call_us": round(float(fill_us), 2), "candidates_us": round(cand_us, 2), "bytes": nbytes,
                      "gb_per_s_of_calls": round(gbs, 1), "hbm_fraction_of_calls": round(gbs * 1e9 / HBM_PEAK, 5)}), flush=True)


def host_child(a):
    pts, off, K, Rt, boxes, bframe = scene(a.frames, a.points, a.stride, a.boxes)
    t0 = time.perf_counter()
    total = 0
    for f in range(a.frames):
        fr = pts[off[f]:off[f + 1]]
        cam = np.dot(Rt[f].T, fr[:, :3].T).T
        cam = np.stack([cam[:, 0], -cam[:, 2], cam[:, 1]], 1)
        uv = np.dot(cam, K[f].T)
        u, v = uv[:, 0] / uv[:, 2], uv[:, 1] / uv[:, 2]
        up = fr.copy()
        up[:, 1], up[:, 2] = -fr[:, 2], fr[:, 1]
        for b in boxes[bframe == f]:
            total += len(up[(u < b[2]) & (u >= b[0]) & (v < b[3]) & (v >= b[1])])
    dt = time.perf_counter() - t0
    print(json.dumps({"what": "host_numpy", "boxes": len(boxes), "selected_rows": total, "us": round(dt * 1e6, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=300000)
    ap.add_argument("--stride", type=int, default=6)
    ap.add_argument("--boxes", type=int, default=64)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--child", choices=("device", "host"))
    a = ap.parse_args()
    if a.child:
        return (device_child if a.child == "device" else host_child)(a)
    rows = {}
    for which in ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which] + [x for k in ("frames", "points", "stride", "boxes", "iters")
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
