"""Times one two-stage INFERENCE call from LiDAR frames and 2-D boxes -- velodyne frames + a 2-D detector's boxes to second-stage
detections -- on one GPU, three ways on the same scene:
  (a) TwoStageDetector.detect_frames, the existing path: frustum_candidates, build_device and
      image_fov_points wait for the device before the first model launch, detect() five more times between the stages;
  (b) cascade.FrameCascade.step() uncaptured;
  (c) the same step captured once into a graph and replayed: no host read, no upload, fixed sizes.
And the front alone: frustum.FrameDetectSource(fov=True).step() against frustum_candidates + InputBuilder.build_device +
image_fov_points.  The counterpart of tools/cascade_link_bench.py, whose scene sizes and conventions it keeps.

python tools/frame_cascade_bench.py [--frames 8] [--rows 120000] [--boxes 32] [--top-k 16] [--cands 64] [--batch 32] [--iters 200]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.

The scene (seeded, synthetic): bench.py's car and refine models (synthetic weights); F frames of about `rows` velodyne rows each, a
uniform cloud in front of the car under a KITTI-like calibration (P2 of a KITTI sequence, the velodyne-to-camera axis swap, R0 = I,
1242 x 375 images); `boxes` 2-D boxes spread over the frames' images, one group per frame, every one tall and wide enough to pass
the skip rule.  The window counts are what the second stage needs on this scene, the first stride two windows up.

Times: `wall_us`: the wall clock of one call synchronised, median over the iterations, the paths alternating in blocks of ten;
`device_us`: the device-event time around the same call, median (for the existing paths it includes the device's idle time while
the host reads).  All outputs are checked finite and the paths' kept boxes compared.  A record for EXPERIMENTS.md; no test depends
on a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P2 = [[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]]
V2C = [[0.0, -1.0, 0.0, 0.0], [0.0, 0.0, -1.0, -0.08], [1.0, 0.0, 0.0, -0.27]]
WH = (1242.0, 375.0)


def scene(frames, n_rows, boxes, seed=1):
    """-> frame_points (n,4) float32 velodyne, frame_off, calib, img_wh (F,2), boxes2d (D,4), box_frame (D)."""
    rng = np.random.RandomState(seed)
    pts, off = [], [0]
    for f in range(frames):
        n = int(n_rows * rng.uniform(0.95, 1.05))
        pts.append(np.stack([rng.uniform(2.5, 80.0, n), rng.uniform(-40, 40, n), rng.uniform(-4.0, 4.0, n), rng.uniform(0, 1, n)], 1).astype(np.float32))
        off.append(off[-1] + n)
    calib = {"P": np.tile(np.asarray(P2)[None], (frames, 1, 1)), "V2C": np.tile(np.asarray(V2C)[None], (frames, 1, 1)),
             "R0": np.tile(np.eye(3)[None], (frames, 1, 1))}
    bframe = (np.arange(boxes) * frames // boxes).astype(np.int32)
    x0, y0 = rng.uniform(20, WH[0] - 260, boxes), rng.uniform(60, WH[1] - 200, boxes)
    b2d = np.stack([x0, y0, x0 + rng.uniform(90, 240, boxes), y0 + rng.uniform(60, 140, boxes)], 1)
    return np.concatenate(pts, 0), np.asarray(off, dtype=np.int64), calib, np.tile(np.asarray([WH]), (frames, 1)), b2d, bframe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--top-k", type=int, default=16)
    ap.add_argument("--cands", type=int, default=64)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoints", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    import torch
    import bench
    from frustum_convnet_amd import cascade, frustum, inputs
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    F, D1, G, top_k, D, B = a.frames, a.boxes, a.frames, a.top_k, a.cands, a.batch
    m1 = bench.build_model(dev, "car").eval()
    ib = inputs.InputBuilder(a.npoints)                          # (cfg holds the first stage's configuration here ...)
    m2 = bench.build_model(dev, "refine").eval()                # (... and the refine configuration here: the builders read it)
    rb = inputs.RefineInputBuilder(a.npoints)
    pts_h, off, calib, wh, b2d, bframe = scene(F, a.rows, D1)
    pts = torch.from_numpy(pts_h).to(dev)
    cal = {k: torch.from_numpy(v).to(dev) for k, v in calib.items()}
    types, prob, group = ["Car"] * D1, np.linspace(0.5, 0.95, D1), bframe.copy()
    two = cascade.TwoStageDetector(m1, m2, rb, input_builder=ib)
    cap1, cap2 = 1 << 20, 1 << 20

    def chain(lpad):
        fc = two.frame_link(pts, off, cal, wh, D1, D1, cap1, G, D, B, cap2, lpad, 7, "nms", 0.1, top_k=top_k)
        fc.source.set_boxes(b2d, bframe, types, prob, group)
        return fc
    # ---- the window counts the second stage needs on this scene, from a probe with room to spare
    probe = chain((64, 32, 16, 8))
    pr = probe.step()
    torch.cuda.synchronize()
    n1, n2 = int(pr["n_kept1"].cpu()[0]), int(pr["n_kept"].cpu()[0])
    widths = probe.link.pred_size.cpu().numpy()[probe.link.slot_unit.cpu().numpy()[:n2].astype(np.int64), 1]
    print(json.dumps({"what": "scene", "boxes": D1, "first_stage_slots": n1, "rows_first_stage": int(probe.source.counts.sum()),
                      "fov_rows": int(probe.link.frame_off.cpu()[-1]), "candidates": int(pr["n_cand"].cpu()[0]), "second_stage_slots": n2,
                      "rows_second_stage": int(probe.link.counts.sum()),
                      "width_min": float(widths.min()) if n2 else None, "width_max": float(widths.max()) if n2 else None}), flush=True)
    lpad = [(rb._lpad(widths)[0] if n2 else 14) + 2]
    for s in range(3):
        lpad.append((lpad[s] + 1) // 2)
    del probe, pr
    fc = chain(lpad)
    src = frustum.FrameDetectSource(pts, off, cal, wh, ib, D1, D1, cap1, 7, G, fov=True).set_boxes(b2d, bframe, types, prob, group)
    d1, d2 = inputs.DeviceDraws(7, dev), inputs.DeviceDraws(8, dev)

    def host_call():
        return two.detect_frames(pts, off, cal, wh, b2d, bframe, types, prob, "nms", 0.1, unit_group=group, num_groups=G, top_k=top_k,
                                 draws=d1, refine_draws=d2)

    def host_front():
        sel = frustum.frustum_candidates(pts, off, cal, wh, b2d, bframe)
        batch = ib.build_device(sel, cal["P"], types, prob, draws=d1)
        return batch, frustum.image_fov_points(pts, off, cal, wh)

    # ---- warm-up of all, then the captures (after a side-stream warm-up, as torch asks)
    for _ in range(5):
        res = host_call()
        front = host_front()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(5):
            fc.step()
            src.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for part in (fc, src):
        try:
            part.check()
        except ValueError as e:                                 # (empty slots flag the draws' bit 0: the summary reports the words)
            print(json.dumps({"what": "warm-up status", "status": str(e)}), flush=True)
    graph, sgraph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fc.step()
    with torch.cuda.graph(sgraph):
        sout = src.step()
    torch.cuda.synchronize()
    names = ("host", "eager", "replay", "host_front", "source_eager", "source_replay")
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
        for what, fn in (("host", host_call), ("replay", graph.replay), ("eager", fc.step), ("host_front", host_front),
                         ("source_replay", sgraph.replay), ("source_eager", src.step)):
            for _ in range(10):
                r = timed(what, fn)
            if what == "host":
                res = r
            if what == "host_front":
                front = r
    n1, n2 = int(out["n_kept1"].cpu()[0]), int(out["n_kept"].cpu()[0])
    assert torch.isfinite(out["dets"]).all() and n1 > 0 and all(torch.isfinite(v).all() for v in out["batch1"].values())
    assert res["dets"] is None or torch.isfinite(res["dets"]).all()
    same_boxes = bool(np.array_equal(out["slot_box"].cpu().numpy()[:n1], res["kept"][:n1]) and len(res["kept"]) == n1)
    same_front = bool(np.array_equal(sout["slot_box"].cpu().numpy()[:n1], front[0]["kept"]) and torch.equal(src.fov_off, front[1][1]))
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    shape = {"frames": F, "rows": int(off[-1]), "S": fc.source.S, "boxes": D1, "B1": D1, "G": G, "top_k": top_k, "D": D, "B": B,
             "npoints": a.npoints, "lpad": lpad, "n_kept1": n1, "n_cand": int(out["n_cand"].cpu()[0]), "n_kept2": n2,
             "host_batch2": int(len(res["stage1_row"]))}
    for what, name in (("host", "detect_frames"), ("eager", "frame_cascade_eager"), ("replay", "frame_cascade_replay"),
                       ("host_front", "candidates_build_device_fov"), ("source_eager", "frame_detect_source_eager"),
                       ("source_replay", "frame_detect_source_replay")):
        print(json.dumps(dict(shape, what=name, wall_us=us(wall[what]), wall_us_min=round(min(wall[what]) * 1e6, 1),
                              device_us=us(devt[what]), calls=len(wall[what]))), flush=True)
    st = lambda *w: int(sum(int(x.cpu()[0]) for x in w))
    print(json.dumps({"what": "summary", "host_wall_us": us(wall["host"]), "eager_wall_us": us(wall["eager"]),
                      "replay_wall_us": us(wall["replay"]), "replay_device_us": us(devt["replay"]),
                      "host_over_replay_wall": round(us(wall["host"]) / us(wall["replay"]), 2),
                      "front_host_wall_us": us(wall["host_front"]), "front_replay_wall_us": us(wall["source_replay"]),
                      "front_replay_device_us": us(devt["source_replay"]),
                      "front_host_over_replay_wall": round(us(wall["host_front"]) / us(wall["source_replay"]), 2),
                      "same_kept_boxes": same_boxes, "same_front": same_front, "status": st(fc.source.status, fc.link.status),
                      "draws_status": st(fc.source.draws.status, fc.link.draws.status), "steps": int(fc.source.draws.state.cpu()[0])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
