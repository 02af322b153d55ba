"""Times one SUN-RGBD training INPUT step -- freshly perturbed label boxes to the SunrgbdInputBuilder batch -- at the workload's own
shape on one GPU, three ways:
  (a) the existing path: frustum.perturb_boxes2d_sunrgbd on the host, frustum.sunrgbd_training_candidates (its launches around
      host reads of the segment counts and of the post-subsample positives, rng.choice(n, 2048, replace=False) on the host for every
      frustum over 2048 rows), SunrgbdInputBuilder.build_device_train(draws=DeviceDraws);
  (b) frustum.SunrgbdTrainSource.step() uncaptured;
  (c) the same step captured once into a graph and replayed: no host read, no upload, a fixed batch of B slots.
The counterpart of tools/frustum_train_source_bench.py, whose conventions it keeps.

python tools/sunrgbd_train_source_bench.py [--frames 8] [--rows 300000] [--batch 32] [--boxes 48] [--iters 100]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.

The scene (seeded, synthetic): F depth frames of about `rows` upright-depth rows (x, y, z, r, g, b) each under one camera matrix
and tilt; 12 labels per frame -- ten objects with points of their own at 2-6.5 m, one with three points inside (the bar of five
drops it) and one in the air.  Both paths try D labels per step, drawn without replacement from the F * 12.

Times: `wall_us`: the wall clock of one step synchronised, median over the iterations, the three ways alternating in blocks of ten.
`replay_device_us`: the device-event time around one graph replay, median.  `few_share`: the share of the timed steps in which
fewer than B of the D boxes survived (status bit 1) -- how to size D.  `rows_filled`: the rows the fill stored per step (ALL
pre-kept boxes are filled: how to size `capacity`).  The batches are checked finite.  A record for EXPERIMENTS.md; no test depends
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

K = np.asarray([[529.5, 0.0, 365.0], [0.0, 529.5, 265.0], [0.0, 0.0, 1.0]])
RT = np.asarray([[0.979589, 0.012593, -0.200614], [0.012593, 0.992231, 0.123772], [0.200614, -0.123772, 0.971820]])
PER_FRAME = 12
TYPES = ("bed", "table", "sofa", "chair", "toilet", "desk", "dresser", "night_stand", "bookshelf", "bathtub")


def project(xyz):
    d = xyz @ RT                                                # Rtilt^T . p, row-wise
    c = np.stack([d[:, 0], -d[:, 2], d[:, 1]], 1)
    img = c @ K.T
    return img[:, 0] / img[:, 2], img[:, 1] / img[:, 2]


def corners(gt):
    cx, cy, cz, l, w, h, heading = gt
    x = np.asarray([-l, l, l, -l] * 2)
    y = np.asarray([w, w, -w, -w] * 2)
    z = np.asarray([h] * 4 + [-h] * 4)
    c, s = np.cos(-heading), np.sin(-heading)
    return np.stack([c * x - s * y + cx, s * x + c * y + cy, z + cz], 1)


def scene(frames, rows, seed=1):
    """-> frame_points (n,6) float32, frame_off, K (F,3,3), Rtilt (F,3,3), gt_box2d, gt_box3d (half extents), box_frame, types."""
    rng = np.random.RandomState(seed)
    pts, off, gt2d, gt3d, bframe, types = [], [0], [], [], [], []
    for f in range(frames):
        n = int(rows * rng.uniform(0.95, 1.05))
        room = np.stack([rng.uniform(-3.5, 3.5, n), rng.uniform(1.0, 7.0, n), rng.uniform(-1.3, 1.6, n)], 1)
        at = 0
        for k in range(PER_FRAME):
            kind = "air" if k == 11 else ("few" if k == 10 else "object")
            y = 2.0 + 0.4 * k + rng.uniform(0, 0.3)
            ext = [0.02, 0.02, 0.02] if kind == "few" else [rng.uniform(0.2, 0.5), rng.uniform(0.15, 0.35), rng.uniform(0.2, 0.4)]
            gt = np.asarray([rng.uniform(-0.35, 0.35) * y, y, rng.uniform(-0.6, 0.2) if kind != "air" else 4.0] + ext +
                            [rng.uniform(-np.pi, np.pi)])
            u, v = project(corners(gt))
            box = [u.min(), v.min(), u.max(), v.max()]
            if kind != "object":                                # a label above the room, a tiny one: their image boxes are given
                box = [300.0, 100.0, 420.0, 200.0] if kind == "air" else [u.min() - 30, v.min() - 30, u.max() + 30, v.max() + 30]
            if kind != "air":                                   # the object's own surface: rows inside its box
                m = 3 if kind == "few" else int(rng.uniform(1500, 12000))
                a, b, dz = rng.uniform(-gt[3], gt[3], m), rng.uniform(-gt[4], gt[4], m), rng.uniform(-gt[5], gt[5], m)
                c, s = np.cos(-gt[6]), np.sin(-gt[6])
                room[at:at + m] = np.stack([c * a - s * b + gt[0], s * a + c * b + gt[1], dz + gt[2]], 1)
                at += m
            gt2d.append(box), gt3d.append(gt), bframe.append(f), types.append(TYPES[k % len(TYPES)])
        rng.shuffle(room)
        pts.append(np.concatenate([room, rng.uniform(0, 1, (n, 3))], 1).astype(np.float32))
        off.append(off[-1] + n)
    return (np.concatenate(pts, 0), np.asarray(off, dtype=np.int64), np.tile(K[None], (frames, 1, 1)), np.tile(RT[None], (frames, 1, 1)),
            np.asarray(gt2d), np.asarray(gt3d), np.asarray(bframe, dtype=np.int32), types)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=300000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--boxes", type=int, default=48)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--capacity", type=int, default=4 << 20)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    import torch
    from frustum_convnet_amd import frustum, inputs
    from frustum_convnet_amd.config import reset_cfg
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    reset_cfg()
    pts_h, off, Kf, Rf, gt2d, gt3d, bframe, types = scene(a.frames, a.rows)
    G, B, D = len(bframe), a.batch, a.boxes
    pts = torch.from_numpy(pts_h).to(dev)
    Kd, Rd = torch.from_numpy(Kf).to(dev), torch.from_numpy(Rf).to(dev)
    b = inputs.SunrgbdInputBuilder(a.npoints, (0.1, 0.2, 0.4, 0.8, 1.6), 8.0, random_flip=True, random_shift=True)
    src = frustum.SunrgbdTrainSource(pts, off, Kd, Rd, gt2d, gt3d, bframe, types, b, B, D, a.capacity, 7, cap=a.cap)
    dd = inputs.DeviceDraws(11, dev)
    rng = np.random.RandomState(5)
    kept_hist, sub_hist = [], []

    def host_step():
        lab = rng.choice(G, D, False)
        boxes = frustum.perturb_boxes2d_sunrgbd(gt2d[lab], 0.1, rng=rng)
        sel = frustum.sunrgbd_training_candidates(pts, off, Kd, Rd, boxes, bframe[lab], gt3d[lab], cap=a.cap, rng=rng)
        kept_hist.append(len(sel["kept"]))
        sub_hist.append(sum(x is not None for x in sel.get("sub", [])))
        return b.build_device_train(sel, Kd, Rd, [types[g] for g in lab], draws=dd)

    # ---- warm-up of both, then the capture (after a side-stream warm-up, as torch asks)
    for _ in range(3):
        out_h = host_step()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        for _ in range(3):
            src.step()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    try:
        src.check()
    except ValueError as e:                                     # (fewer than B survivors in a warm-up step: counted below, not an error)
        if "bit 2" in str(e):
            raise
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.step()
    torch.cuda.synchronize()
    kept_hist.clear(), sub_hist.clear()
    host_wall, replay_wall, replay_dev, eager_wall, filled, few = [], [], [], [], [], 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    for blk in range(a.iters // 10):                            # the three ways alternate in blocks of ten
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
            filled.append(int(src.seg_off.cpu()[-1]))
        for _ in range(10):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            src.step()
            torch.cuda.synchronize()
            eager_wall.append(time.perf_counter() - t0)
            few += int(src.n_kept.cpu()[0]) < B
            filled.append(int(src.seg_off.cpu()[-1]))
    assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point())
    assert all(torch.isfinite(v).all() for v in out_h.values() if isinstance(v, torch.Tensor) and v.is_floating_point())
    status = int(src.status.cpu()[0])
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    shape = {"frames": a.frames, "rows": int(off[-1]), "S": src.S, "labels": G, "B": B, "D": D, "npoints": a.npoints, "cap": a.cap}
    print(json.dumps(dict(shape, what="host_path", wall_us=us(host_wall), wall_us_min=round(min(host_wall) * 1e6, 1),
                          kept_min=int(min(kept_hist)), kept_median=float(np.median(kept_hist)),
                          subsampled_median=float(np.median(sub_hist)))), flush=True)
    print(json.dumps(dict(shape, what="train_source", replay_device_us=us(replay_dev), replay_wall_us=us(replay_wall),
                          replay_wall_us_min=round(min(replay_wall) * 1e6, 1), eager_wall_us=us(eager_wall),
                          few_share=round(few / (len(replay_wall) + len(eager_wall)), 4), status=status,
                          rows_filled_median=float(np.median(filled)), rows_filled_max=int(max(filled)), capacity=a.capacity,
                          steps=int(src.draws_box.state.cpu()[0]))), flush=True)
    print(json.dumps({"what": "summary", "host_wall_us": us(host_wall), "eager_wall_us": us(eager_wall), "replay_wall_us": us(replay_wall),
                      "replay_device_us": us(replay_dev), "host_over_replay_wall": round(us(host_wall) / us(replay_wall), 2)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
