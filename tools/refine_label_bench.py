"""Times the refinement stage's training link on one GPU: fcn_refine_match, fcn_refine_label_count, fcn_refine_label_fill
(csrc/refine_label.h) and the whole per-step sequence cascade.refine_training_candidates + RefineInputBuilder.build_device_train,
beside the inference link's one-workgroup-per-box selection (fcn_refine_select_count / _fill, csrc/refine_select.h) on the same
boxes.  The scene is KITTI-like: --frames image-FOV frames of --points rows in rect camera coordinates, --cands first-stage
detections spread over them, each next to a label box that holds a few hundred points, with A = 1 (no jitter) and A = 4 chained
jittered copies.

python tools/refine_label_bench.py [--frames 8] [--points 20000] [--cands 32] [--iters 200] [--limit 120]
    runs one child process per A, each under a time limit (--limit seconds), and prints one JSON line per child.  The children fail
    without a GPU; nothing falls back.

Times: `*_call_us` are medians of device-event times around one entry point (they include the entry's read-back of its index
lists, so they bound the kernel time from above); `sequence_us` is the host wall clock per call of the two Python functions,
synchronised.  The unlabelled selection runs on the un-jittered boxes (it has no jitter): at A = 1 both select the same rows.
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


def scene(frames, points, cands, seed=1):
    """frames x points rows (x, y, z, intensity); cands label boxes (tx, ty, tz, l, w, h, ry; t the bottom centre) dealt round the
    frames, 300 of each frame's rows drawn inside each of its boxes; one detection per label box: the label moved and scaled by a
    few percent (float32 rows)."""
    rng = np.random.RandomState(seed)
    frame_of = np.sort(np.arange(cands) % frames).astype(np.int32)
    tz = rng.uniform(8.0, 50.0, cands)
    gt = np.stack([rng.uniform(-0.4, 0.4, cands) * tz, rng.uniform(1.4, 1.9, cands), tz, rng.uniform(3.4, 4.4, cands),
                   rng.uniform(1.5, 1.8, cands), rng.uniform(1.4, 1.7, cands), rng.uniform(-np.pi, np.pi, cands)], 1)
    gt_off = np.concatenate([[0], np.cumsum(np.bincount(frame_of, minlength=frames))]).astype(np.int64)
    pts = np.stack([rng.uniform(-25.0, 25.0, frames * points), rng.uniform(-1.0, 2.5, frames * points),
                    rng.uniform(4.0, 60.0, frames * points), rng.uniform(0, 1, frames * points)], 1).astype(np.float32)
    for j, (tx, ty, tz_, l, w, h, ry) in enumerate(gt):
        n = 300
        a, dy, b = rng.uniform(-l / 2, l / 2, n), rng.uniform(-h, 0.0, n), rng.uniform(-w / 2, w / 2, n)
        c, s = np.cos(ry), np.sin(ry)
        at = frame_of[j] * points + rng.choice(points, n, replace=False)
        pts[at, :3] = np.stack([c * a + s * b + tx, dy + ty, -s * a + c * b + tz_], 1)
    dets = np.concatenate([gt + rng.uniform(-0.05, 0.05, gt.shape) * [1, 1, 1, 1, 1, 1, 1], rng.uniform(0, 1, (cands, 1))], 1)
    off = (np.arange(frames + 1) * points).astype(np.int64)
    return pts, off, dets.astype(np.float32), np.arange(cands, dtype=np.int32), frame_of, gt, gt_off


def child(a):
    import torch
    from frustum_convnet_amd import _native, cascade, inputs
    from frustum_convnet_amd.config import reset_cfg
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    A = a.child
    pts, off, dets, crow, cframe, gt, gt_off = scene(a.frames, a.points, a.cands)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    t_pts, t_off, t_dets, t_crow, t_cframe, t_gt, t_goff = (up(x) for x in (pts, off, dets, crow, cframe, gt, gt_off))
    D, R, G, F, ps = len(crow), len(dets), len(gt), a.frames, pts.shape[1]
    L, s = _native.lib(), _native.current_stream(dev)
    S = -(-a.points // int(L.fcn_frustum_select_seg()))
    U = D * A
    jit_h = None if A == 1 else np.random.RandomState(2).random_sample((D, A, 7))
    t_jit = None if jit_h is None else up(jit_h)
    gidx, best = cascade.match_detections(t_dets, t_crow, t_cframe, t_gt, t_goff, 0.5)
    reset_cfg()
    builder = inputs.RefineInputBuilder(512, strides=(0.1, 0.2, 0.4, 0.8), random_flip=True, random_shift=True)
    types = ["Car"] * D
    rng = np.random.RandomState(3)

    def sequence():
        sel = cascade.refine_training_candidates(t_pts, t_off, t_dets, t_crow, t_cframe, gidx, t_gt, jitter=t_jit)
        draws = inputs.draw_refine(sel["counts"], builder.npoints, True, True, rng=rng)
        return sel, builder.build_device_train(sel, types, draws=draws)
    sel, _ = sequence()
    torch.cuda.synchronize()
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    scnt, spos = torch.zeros((U, S), **i32), torch.zeros((U, S), **i32)
    boxes = [torch.zeros(shape, **f64) for shape in ((U, 24), (U,), (U, 3), (U, 24), (U,), (U, 3))]
    common = (t_pts.data_ptr(), t_off.data_ptr(), F, ps, t_dets.data_ptr(), R, t_crow.data_ptr(), t_cframe.data_ptr(), D, 1.2)
    label = common + (gidx.data_ptr(), t_gt.data_ptr(), G, A, None if t_jit is None else t_jit.data_ptr(), 0.05, S)
    match = lambda: _native.check(L.fcn_refine_match(t_dets.data_ptr(), R, t_crow.data_ptr(), t_cframe.data_ptr(), D, t_gt.data_ptr(),
                                                     G, t_goff.data_ptr(), F, 0.5, gidx.data_ptr(), best.data_ptr(), s), "match")
    count = lambda: _native.check(L.fcn_refine_label_count(*label, scnt.data_ptr(), spos.data_ptr(), *[b.data_ptr() for b in boxes], s),
                                  "count")
    count()
    soff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), scnt.reshape(-1).to(torch.int64).cumsum(0)])
    out = torch.empty((int(soff[-1]), ps), dtype=torch.float32, device=dev)
    fill = lambda: _native.check(L.fcn_refine_label_fill(*label, soff.data_ptr(), out.data_ptr(), s), "fill")
    # the inference link on the same (un-jittered) boxes: one workgroup per box over its whole frame
    cnt = torch.zeros((D,), **i32)
    pbox = [torch.zeros(shape, **f64) for shape in ((D, 24), (D,), (D, 3))]
    scount = lambda: _native.check(L.fcn_refine_select_count(*common, *[b.data_ptr() for b in pbox], cnt.data_ptr(), s), "select count")
    scount()
    ooff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), cnt.to(torch.int64).cumsum(0)])
    sout = torch.empty((int(ooff[-1]), ps), dtype=torch.float32, device=dev)
    sfill = lambda: _native.check(L.fcn_refine_select_fill(*common, ooff.data_ptr(), sout.data_ptr(), s), "select fill")
    calls = (("match", match), ("count", count), ("fill", fill), ("select_count", scount), ("select_fill", sfill))
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(calls) + 1)] for _ in range(a.iters)]
    for it in range(-10, a.iters):                                 # ten warm-up rounds
        e = ev[max(it, 0)]
        e[0].record()
        for k, (_, fn) in enumerate(calls):
            fn()
            e[k + 1].record()
    torch.cuda.synchronize()
    row = {"what": "A=%d" % A, "frames": F, "points_per_frame": a.points, "candidates": D, "units": U, "segments": S,
           "workgroups": S * U, "matched": int((gidx >= 0).sum()), "kept_units": len(sel["kept"]), "selected_rows": int(soff[-1]),
           "positive_rows": int(spos.sum()), "select_rows": int(ooff[-1])}
    for k, (name, _) in enumerate(calls):
        row[name + "_call_us"] = round(float(np.median([e[k].elapsed_time(e[k + 1]) for e in ev]) * 1e3), 2)
    t0 = time.perf_counter()
    for _ in range(a.iters):
        sequence()
    torch.cuda.synchronize()
    row["sequence_us"] = round((time.perf_counter() - t0) / a.iters * 1e6, 2)
    if A == 1:
        row["same_rows_as_select"] = bool(torch.equal(out.view(torch.int32), sout.view(torch.int32)))
    print(json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--cands", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=float, default=120.0)
    ap.add_argument("--child", type=int, choices=(1, 4))
    a = ap.parse_args()
    if a.child:
        return child(a)
    for A in (1, 4):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(A)] + [x for k in ("frames", "points", "cands", "iters")
                                                                                for x in ("--" + k, str(getattr(a, k)))]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": "A=%d" % A, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
