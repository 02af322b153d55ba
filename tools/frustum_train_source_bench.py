"""Times one KITTI first-stage training INPUT step -- freshly perturbed label boxes to the InputBuilder batch -- at the workload's
own shape on one GPU, both ways:
  (a) the existing path: frustum.perturb_boxes2d on the host, frustum.frustum_training_candidates (two launches around a host
      read of the segment counts; each entry reads box_frame / frame_off back), InputBuilder.build_device_train(draws=DeviceDraws);
  (b) frustum.FrameTrainSource.step() captured once into a graph and replayed: no host read, no upload, a fixed batch of B slots.
The counterpart of tools/device_draw_bench.py, whose conventions it keeps.

python tools/frustum_train_source_bench.py [--frames 8] [--rows 120000] [--batch 32] [--boxes 48] [--iters 200]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.

The scene (seeded, synthetic): F sweeps of about `rows` velodyne rows each under a KITTI calibration; 12 labels per frame -- nine
objects with points of their own at 8-45 m, two beyond 55 m whose label boxes are under 25 px (the height rule drops them), one
without a point inside (the label rule drops it).  Both paths try D labels per step, drawn without replacement from the F * 12.

Times: (a) `wall_us`: the wall clock of one step synchronised, median over the iterations, the two paths alternating in blocks of
ten.  (b) `replay_device_us`: the device-event time around one graph replay, median; `replay_wall_us`: the wall clock of one replay
synchronised; `eager_wall_us`: step() uncaptured, synchronised.  `few_share`: the share of the timed steps in which fewer than B of
the D boxes survived (status bit 1) -- how to size D.  Both paths' batches are checked finite.  A record for EXPERIMENTS.md; no
test depends on a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = np.asarray([[721.5377, 0, 609.5593, 44.85728], [0, 721.5377, 172.854, 0.2163791], [0, 0, 1, 0.002745884]])
V2C = np.asarray([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                  [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
R0 = np.asarray([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
W, H = 1242.0, 375.0
PER_FRAME = 12


def rect_to_velo(rect):
    ref = np.linalg.solve(R0, rect.T)
    return np.linalg.solve(V2C[:, :3], ref - V2C[:, 3:4]).T


def corners(gt):
    tx, ty, tz, l, w, h, ry = gt
    x = np.asarray([l / 2, l / 2, -l / 2, -l / 2] * 2)
    y = np.asarray([0.0] * 4 + [-h] * 4)
    z = np.asarray([w / 2, -w / 2, -w / 2, w / 2] * 2)
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([c * x + s * z + tx, y + ty, -s * x + c * z + tz], 1)


def scene(frames, rows, seed=1):
    """-> frame_points (n,4) float32, frame_off, calib, img_size, gt_box2d, gt_box3d, box_frame, types."""
    rng = np.random.RandomState(seed)
    pts, off, gt2d, gt3d, bframe, types = [], [0], [], [], [], []
    for f in range(frames):
        n = int(rows * rng.uniform(0.95, 1.05))
        sweep = np.stack([rng.uniform(3, 70, n), rng.uniform(-30, 30, n), rng.uniform(-2.2, 1.0, n)], 1)
        at = 0
        for k in range(PER_FRAME):
            kind = "far" if k >= 10 else ("empty" if k == 9 else "object")
            z = rng.uniform(56, 65) if kind == "far" else 8.0 + 4.0 * k + rng.uniform(0, 2)
            x = rng.uniform(-0.35, 0.35) * z
            t = ("Car", "Pedestrian", "Cyclist")[k % 3]
            l, w, h = {"Car": (3.9, 1.6, 1.5), "Pedestrian": (0.8, 0.6, 1.8), "Cyclist": (1.8, 0.6, 1.7)}[t]
            gt = np.asarray([x, 1.65 if kind != "empty" else -4.0, z, l, w, h, rng.uniform(-np.pi, np.pi)])
            img = np.concatenate([corners(gt), np.ones((8, 1))], 1) @ P.T
            u, v = img[:, 0] / img[:, 2], img[:, 1] / img[:, 2]
            box = [max(u.min(), 0.0), max(v.min(), 0.0), min(u.max(), W - 1), min(v.max(), H - 1)]
            if kind == "empty":                                 # a label in the air: its image box is made to lie in the image
                box = [500.0, 20.0, 580.0, 80.0]
            if kind != "empty":                                 # the object's own returns: a few hundred rows inside its box
                m = int(rng.uniform(150, 600))
                a, dy, b = rng.uniform(-l / 2, l / 2, m), rng.uniform(-h, 0, m), rng.uniform(-w / 2, w / 2, m)
                c, s = np.cos(gt[6]), np.sin(gt[6])
                sweep[at:at + m] = rect_to_velo(np.stack([c * a + s * b + gt[0], dy + gt[1], -s * a + c * b + gt[2]], 1))
                at += m
            gt2d.append(box), gt3d.append(gt), bframe.append(f), types.append(t)
        rng.shuffle(sweep)
        pts.append(np.concatenate([sweep, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
        off.append(off[-1] + n)
    calib = {"P": np.tile(P.reshape(1, 12), (frames, 1)), "V2C": np.tile(V2C.reshape(1, 12), (frames, 1)),
             "R0": np.tile(R0.reshape(1, 9), (frames, 1))}
    return (np.concatenate(pts, 0), np.asarray(off, dtype=np.int64), calib, np.tile([[W, H]], (frames, 1)), np.asarray(gt2d),
            np.asarray(gt3d), np.asarray(bframe, dtype=np.int32), types)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--boxes", type=int, default=48)
    ap.add_argument("--npoints", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    import torch
    from frustum_convnet_amd import frustum, inputs
    from frustum_convnet_amd.config import reset_cfg
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    reset_cfg()
    pts_h, off, calib, wh, gt2d, gt3d, bframe, types = scene(a.frames, a.rows)
    G, B, D = len(bframe), a.batch, a.boxes
    pts = torch.from_numpy(pts_h).to(dev)
    cal = {k: torch.from_numpy(v).to(dev) for k, v in calib.items()}
    b = inputs.InputBuilder(a.npoints, random_flip=True, random_shift=True)
    capacity = 1 << 20
    src = frustum.FrameTrainSource(pts, off, cal, wh, gt2d, gt3d, bframe, types, b, B, D, capacity, 7)
    dd = inputs.DeviceDraws(11, dev)
    rng = np.random.RandomState(5)
    kept_hist = []

    def host_step():
        lab = rng.choice(G, D, False)
        boxes = frustum.perturb_boxes2d(gt2d[lab], wh[bframe[lab]], 0.1, rng=rng)
        sel = frustum.frustum_training_candidates(pts, off, cal, wh, boxes, bframe[lab], gt3d[lab], gt_box2d=gt2d[lab])
        kept_hist.append(len(sel["kept"]))
        return b.build_device_train(sel, cal["P"], [types[g] for g in lab], draws=dd)

    # ---- warm-up of both, then the capture (after a side-stream warm-up, as torch asks)
    for _ in range(5):
        out_h = host_step()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(5):
            src.step()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    try:
        src.check()
    except ValueError:                                          # (fewer than B survivors in a warm-up step: counted below, not an error)
        pass
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.step()
    torch.cuda.synchronize()
    kept_hist.clear()
    host_wall, replay_wall, replay_dev, eager_wall, few = [], [], [], [], 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for blk in range(a.iters // 10):                            # the two paths alternate in blocks of ten
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out_h = host_step()
            torch.cuda.synchronize()
            host_wall.append(time.perf_counter() - t0)
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            graph.replay()
            ev[1].record()
            torch.cuda.synchronize()
            replay_wall.append(time.perf_counter() - t0)
            replay_dev.append(ev[0].elapsed_time(ev[1]) * 1e-3)
            few += int(src.n_kept.cpu()[0]) < B
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            src.step()
            torch.cuda.synchronize()
            eager_wall.append(time.perf_counter() - t0)
            few += int(src.n_kept.cpu()[0]) < B
    assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point())
    assert all(torch.isfinite(v).all() for v in out_h.values() if isinstance(v, torch.Tensor) and v.is_floating_point())
    status = int(src.status.cpu()[0])
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    shape = {"frames": a.frames, "rows": int(off[-1]), "S": src.S, "labels": G, "B": B, "D": D, "npoints": a.npoints}
    print(json.dumps(dict(shape, what="host_path", wall_us=us(host_wall), wall_us_min=round(min(host_wall) * 1e6, 1),
                          kept_min=int(min(kept_hist)), kept_median=float(np.median(kept_hist)))), flush=True)
    print(json.dumps(dict(shape, what="train_source", replay_device_us=us(replay_dev), replay_wall_us=us(replay_wall),
                          replay_wall_us_min=round(min(replay_wall) * 1e6, 1), eager_wall_us=us(eager_wall),
                          few_share=round(few / (len(replay_wall) + len(eager_wall)), 4), status=status,
                          rows_selected=int(src.off.cpu()[-1]), steps=int(src.draws_box.state.cpu()[0]))), flush=True)
    print(json.dumps({"what": "summary", "host_wall_us": us(host_wall), "replay_wall_us": us(replay_wall),
                      "replay_device_us": us(replay_dev), "host_over_replay_wall": round(us(host_wall) / us(replay_wall), 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
