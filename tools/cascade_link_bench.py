"""Times one two-stage INFERENCE call -- a first-stage batch to second-stage detections -- on one GPU, three ways on the same scene:
  (a) TwoStageDetector.detect, the existing path: five host reads between the two stages, the second
      stage's batch size and window counts following the kept list;
  (b) cascade.CascadeLink.step() uncaptured;
  (c) the same step captured once into a graph and replayed: no host read, no upload, D candidates, B slots, fixed window counts.
The counterpart of tools/refine_train_source_bench.py, whose conventions it keeps.

python tools/cascade_link_bench.py [--frames 8] [--rows 120000] [--frustums 32] [--top-k 16] [--cands 64] [--batch 32] [--iters 200]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.
python tools/cascade_link_bench.py --selection-only N
    runs only the two selections below N times each, for a kernel trace (rocprofv3 --kernel-trace --stats) in a run of its own.

The scene (seeded, synthetic): bench.py's car and refine models (synthetic weights) and its car batch of `frustums` frustums in
`frames` groups, one frame per group; F frames of about `rows` rect-camera rows each: a uniform cloud and 300 rows around every box
the first stage keeps on that batch, so that the enlarged boxes hold points.  The window counts are what the existing path pads to
on this batch, the first stride two windows up.

Times: `wall_us`: the wall clock of one call synchronised, median over the iterations, the three paths alternating in blocks of
ten; `device_us`: the device-event time around the same call, median (for the existing path it includes the device's idle time
while the host reads).  `selection`: the device-event time of count + fill alone on the link's own candidate table -- the segmented
(S, D) grid of fcn_refine_detect_count / _fill against the one-workgroup-per-candidate grid of fcn_refine_select_count / _fill (whose
entries also read the two index lists back; the kernel trace of --selection-only separates the kernels from that).  All outputs are
checked finite and the three paths' detections compared.  A record for EXPERIMENTS.md; no test depends on a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def frames_around(d1, rows, frame_of_row, frames, n_rows, seed=1):
    """-> frame_points (n,4) float32, frame_off: a uniform cloud per frame with 300 rows around each kept box of that frame."""
    rng = np.random.RandomState(seed)
    pts, off = [], [0]
    for f in range(frames):
        n = int(n_rows * rng.uniform(0.95, 1.05))
        cloud = np.stack([rng.uniform(-40, 40, n), rng.uniform(-3.0, 3.0, n), rng.uniform(0, 80, n)], 1)
        at = 0
        for r in rows[frame_of_row == f]:
            c = np.array([d1[r, 0], d1[r, 1] - d1[r, 5] / 2.0, d1[r, 2]])
            cloud[at:at + 300] = c + rng.uniform(-1.0, 1.0, (300, 3)) * np.abs(d1[r, 3:6])[[0, 2, 1]] * 0.6
            at += 300
        rng.shuffle(cloud)
        pts.append(np.concatenate([cloud, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
        off.append(off[-1] + n)
    return np.concatenate(pts, 0), np.asarray(off, dtype=np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--frustums", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=16)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoints", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--selection-only", type=int, default=0)
    a = ap.parse_args()
    import torch
    import bench
    from frustum_convnet_amd import _native, cascade, inputs
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    F, B1, G, top_k, D, B = a.frames, a.frustums, a.frames, a.top_k, a.cands, a.batch
    m1 = bench.build_model(dev, "car").eval()
    data = bench.make_data("car", B1, a.npoints, 1234, dev)
    dd = {k: v.contiguous() for k, v in data.items() if k in ("point_cloud", "one_hot") or k.startswith("center_ref")}
    m2 = bench.build_model(dev, "refine").eval()                # (cfg now holds the refine configuration: the builder reads it)
    builder = inputs.RefineInputBuilder(a.npoints)
    L2 = int(dd["center_ref2"].shape[2])
    group = (np.arange(B1) * G // B1).astype(np.int32)
    frustum_frame, types = group.copy(), ["Car"] * B1
    ug = torch.from_numpy(group).to(dev)
    kw = dict(method="nms", thresh=0.1, top_k=top_k)
    # ---- the scene around the first stage's boxes, and the window counts the existing path pads to on it
    d1, _, keep1, cnt1 = m1.detect(dd, unit_group=ug, num_groups=G, **kw)
    keep_h, cnt_h = keep1.cpu().numpy(), cnt1.cpu().numpy()
    rows = np.concatenate([keep_h[g, :c] for g, c in enumerate(cnt_h) if c > 0]).astype(np.int64)
    pts_h, off = frames_around(d1.cpu().numpy().astype(np.float64), rows, frustum_frame[rows // L2], F, a.rows)
    pts = torch.from_numpy(pts_h).to(dev)
    two = cascade.TwoStageDetector(m1, m2, builder)
    cands = cascade.refine_candidates(pts, off, d1, rows.astype(np.int32), frustum_frame[rows // L2].astype(np.int32))
    widths = cands["pred_size"][:, 1].cpu().numpy()
    alive = cands["counts"] > 0
    print(json.dumps({"what": "scene", "kept_rows": int(len(rows)), "with_points": int(alive.sum()), "rows_selected": int(cands["counts"].sum()),
                      "width_min": float(widths[alive].min()), "width_max": float(widths[alive].max())}), flush=True)
    lpad = [builder._lpad(widths[alive])[0] + 2]
    for s in range(3):
        lpad.append((lpad[s] + 1) // 2)
    link = two.link(pts, off, frustum_frame, types, B1, L2, D, B, 1 << 20, lpad, 7, "nms", 0.1, unit_group=group, num_groups=G, top_k=top_k)
    L, p = _native.lib(), (lambda x: x.data_ptr())

    # ---- count + fill alone, on the link's own candidate table: the segmented grid against one workgroup per candidate
    link.step(dd)
    torch.cuda.synchronize()
    n_cand = int(link.n_cand.cpu()[0])
    crow, cframe = link.cand_row[:n_cand].clone(), link.cand_frame[:n_cand].clone()
    S, ps, R = link.S, link.ps, link.R
    f64 = dict(dtype=torch.float64, device=dev)
    hb, ha, hs = torch.zeros((n_cand, 24), **f64), torch.zeros((n_cand,), **f64), torch.zeros((n_cand, 3), **f64)
    scnt, wcnt = torch.zeros((n_cand, S), dtype=torch.int32, device=dev), torch.zeros((n_cand,), dtype=torch.int32, device=dev)
    common = (p(pts), p(link.frame_off), F, ps, p(d1), R, p(crow), p(cframe), n_cand, 1.2)
    stream = _native.current_stream(dev)
    _native.check(L.fcn_refine_detect_count(*common, S, p(scnt), p(hb), p(ha), p(hs), stream), "fcn_refine_detect_count")
    _native.check(L.fcn_refine_select_count(*common, p(hb), p(ha), p(hs), p(wcnt), stream), "fcn_refine_select_count")
    assert torch.equal(scnt.sum(1, dtype=torch.int32), wcnt)
    soff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), scnt.reshape(-1).cumsum(0)])
    woff = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), wcnt.cumsum(0)])
    total = int(woff[-1])
    out_s, out_w = (torch.zeros((total + 1, ps), dtype=torch.float32, device=dev) for _ in range(2))

    def segmented():
        _native.check(L.fcn_refine_detect_count(*common, S, p(scnt), p(hb), p(ha), p(hs), stream), "fcn_refine_detect_count")
        _native.check(L.fcn_refine_detect_fill(*common, S, p(soff), p(out_s), stream), "fcn_refine_detect_fill")

    def whole():
        _native.check(L.fcn_refine_select_count(*common, p(hb), p(ha), p(hs), p(wcnt), stream), "fcn_refine_select_count")
        _native.check(L.fcn_refine_select_fill(*common, p(woff), p(out_w), stream), "fcn_refine_select_fill")
    segmented(), whole()
    torch.cuda.synchronize()
    assert torch.equal(out_s, out_w) and total > 0
    if a.selection_only:
        for _ in range(a.selection_only):
            segmented(), whole()
        torch.cuda.synchronize()
        print(json.dumps({"what": "selection_only", "calls": a.selection_only, "candidates": n_cand, "S": S, "rows": total}), flush=True)
        return 0

    def host_call():
        return two.detect(dd, pts, off, frustum_frame, types, "nms", 0.1, unit_group=ug, num_groups=G, top_k=top_k, draws=host_draws)

    # ---- warm-up of both, then the capture (after a side-stream warm-up, as torch asks)
    host_draws = inputs.DeviceDraws(7, dev)
    for _ in range(5):
        res = host_call()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(5):
            link.step(dd)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    try:
        link.check()
    except ValueError as e:                                     # (empty slots flag the draws' bit 0: the summary reports the word)
        print(json.dumps({"what": "warm-up status", "status": str(e)}), flush=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = link.step(dd)
    torch.cuda.synchronize()
    names = ("host", "eager", "replay", "segmented", "whole")
    wall, devt = {k: [] for k in names}, {k: [] for k in names}
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(what, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ev[0].record()
        r = fn()
        ev[1].record()
        torch.cuda.synchronize()
        wall[what].append(time.perf_counter() - t0)
        devt[what].append(ev[0].elapsed_time(ev[1]) * 1e-3)
        return r

    for blk in range(a.iters // 10):                            # the paths alternate in blocks of ten
        for what, fn in (("host", host_call), ("replay", graph.replay), ("eager", lambda: link.step(dd)), ("segmented", segmented),
                         ("whole", whole)):
            for _ in range(10):
                r = timed(what, fn)
            if what == "host":
                res = r
    n_kept = int(out["n_kept"].cpu()[0])
    assert torch.isfinite(out["dets"]).all() and torch.isfinite(res["dets"]).all() and n_kept > 0
    # the same kept rows; equal detections are promised only at the existing path's own batch size and window counts
    same_rows = bool(np.array_equal(out["stage1_row"].cpu().numpy()[:n_kept], res["stage1_row"][:n_kept]))
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    shape = {"frames": F, "rows": int(off[-1]), "S": S, "B1": B1, "G": G, "top_k": top_k, "D": D, "B": B, "npoints": a.npoints, "lpad": lpad,
             "n_cand": n_cand, "n_kept": n_kept, "host_batch": int(len(res["stage1_row"]))}
    for what, name in (("host", "two_stage_detect"), ("eager", "cascade_link_eager"), ("replay", "cascade_link_replay"),
                       ("segmented", "selection_segmented"), ("whole", "selection_whole")):
        print(json.dumps(dict(shape, what=name, wall_us=us(wall[what]), wall_us_min=round(min(wall[what]) * 1e6, 1),
                              device_us=us(devt[what]), calls=len(wall[what]))), flush=True)
    print(json.dumps({"what": "summary", "host_wall_us": us(wall["host"]), "eager_wall_us": us(wall["eager"]),
                      "replay_wall_us": us(wall["replay"]), "replay_device_us": us(devt["replay"]),
                      "host_over_replay_wall": round(us(wall["host"]) / us(wall["replay"]), 2),
                      "selection_segmented_device_us": us(devt["segmented"]), "selection_whole_device_us": us(devt["whole"]),
                      "same_stage1_rows": same_rows, "status": int(link.status.cpu()[0]), "draws_status": int(link.draws.status.cpu()[0]),
                      "steps": int(link.draws.state.cpu()[0])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
