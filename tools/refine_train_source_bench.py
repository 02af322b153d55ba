"""Times one refine-stage training INPUT step -- first-stage detections and the frames' label boxes to the RefineInputBuilder batch
-- on one GPU, three ways on the same scene:
  (a) the existing per-step path (INTEGRATION.md section 13's loop): cascade.match_detections, gt_idx read back, the host's
      draw_box3d_jitter for the matched candidates, cascade.refine_training_candidates (two launches around a host read of the
      segment counts; each entry reads its index lists back), RefineInputBuilder.build_device_train(draws=DeviceDraws);
  (b) cascade.RefineTrainSource.step() uncaptured;
  (c) the same step captured once into a graph and replayed: no host read, no upload, a fixed batch of B slots.
The counterpart of tools/frustum_train_source_bench.py, whose conventions it keeps.

python tools/refine_train_source_bench.py [--frames 8] [--rows 120000] [--batch 32] [--dets 24] [--copies 2] [--iters 200]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.

The scene (seeded, synthetic): F frames of about `rows` rect-camera rows each; 12 labels per frame with a few hundred rows of their
own; one detection per label -- ten of them the label box shifted, resized and turned a little (most match, a narrow box now and
then falls under the IoU bar), two far from every label (they match nothing).  Both paths try D detections per step with A chained
jittered copies each, drawn without replacement from the F * 12.

Times: `wall_us`: the wall clock of one step synchronised, median over the iterations, the three paths alternating in blocks of
ten; `device_us`: the device-event time around the same step, median.  `few_share`: the share of the source's timed steps in which
fewer than B units survived (status bit 1) -- how to size D * A; `rows_median`: the median rows filled per step.  All batches are
checked finite.  A record for EXPERIMENTS.md; no test depends on a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PER_FRAME = 12
STRIDES = (0.1, 0.2, 0.4, 0.8)
SIZES = {"Car": (3.9, 1.6, 1.5), "Pedestrian": (0.8, 0.6, 1.8), "Cyclist": (1.8, 0.6, 1.7)}


def scene(frames, rows, seed=1):
    """-> frame_points (n,4) float32, frame_off, dets (R,8) float32, det_frame, det_types, gt_box3d (G,7), gt_off."""
    rng = np.random.RandomState(seed)
    pts, off, dets, dframe, types, gts, goff = [], [0], [], [], [], [], [0]
    for f in range(frames):
        n = int(rows * rng.uniform(0.95, 1.05))
        cloud = np.stack([rng.uniform(-30, 30, n), rng.uniform(-1.0, 2.0, n), rng.uniform(3, 70, n)], 1)
        at = 0
        for k in range(PER_FRAME):
            t = ("Car", "Pedestrian", "Cyclist")[k % 3]
            l, w, h = SIZES[t]
            z = 8.0 + 4.0 * k + rng.uniform(0, 2)
            gt = np.asarray([rng.uniform(-0.35, 0.35) * z, 1.65, z, l, w, h, rng.uniform(-np.pi, np.pi)])
            m = int(rng.uniform(150, 600))                      # the object's own returns
            a, dy, b = rng.uniform(-l / 2, l / 2, m), rng.uniform(-h, 0, m), rng.uniform(-w / 2, w / 2, m)
            c, s = np.cos(gt[6]), np.sin(gt[6])
            cloud[at:at + m] = np.stack([c * a + s * b + gt[0], dy + gt[1], -s * a + c * b + gt[2]], 1)
            at += m
            det = gt.copy()
            if k >= 10:                                         # a false positive: far from every label
                det[0] += 25.0
            else:
                det[:3] += rng.uniform(-0.1, 0.1, 3)
                det[3:6] *= rng.uniform(0.95, 1.05, 3)
                det[6] += rng.uniform(-0.05, 0.05)
            gts.append(gt), dets.append(np.concatenate([det, [rng.uniform(0.3, 1.0)]])), dframe.append(f), types.append(t)
        rng.shuffle(cloud)
        pts.append(np.concatenate([cloud, rng.uniform(0, 1, (n, 1))], 1).astype(np.float32))
        off.append(off[-1] + n)
        goff.append(len(gts))
    return (np.concatenate(pts, 0), np.asarray(off, dtype=np.int64), np.asarray(dets, dtype=np.float32),
            np.asarray(dframe, dtype=np.int32), types, np.asarray(gts), np.asarray(goff, dtype=np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--dets", type=int, default=24)
    ap.add_argument("--copies", type=int, default=2)
    ap.add_argument("--npoints", type=int, default=512)
    ap.add_argument("--iters", type=int, default=200)
    a = ap.parse_args()
    import torch
    from frustum_convnet_amd import cascade, inputs
    from frustum_convnet_amd.config import reset_cfg
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    reset_cfg()
    pts_h, off, dets_h, dframe, types, gt, goff = scene(a.frames, a.rows)
    R, B, D, A = len(dframe), a.batch, a.dets, a.copies
    pts, dets = torch.from_numpy(pts_h).to(dev), torch.from_numpy(dets_h).to(dev)
    b = inputs.RefineInputBuilder(a.npoints, strides=STRIDES, random_flip=True, random_shift=True)
    # the widest box any unit can have: the widest detection enlarged by 1.2 and stretched by 5 % per chained copy
    wmax = float(dets_h[:, 4].max()) * 1.2 * 1.05 ** A
    lpad = [int(np.ceil(wmax / s)) + 1 for s in STRIDES]
    capacity = 1 << 20
    src = cascade.RefineTrainSource(pts, off, dets, dframe, types, gt, goff, b, B, D, A, capacity, lpad, 7)
    dd = inputs.DeviceDraws(11, dev)
    rng = np.random.RandomState(5)
    kept_hist, rows_hist = [], []

    def host_step():
        crow = rng.choice(R, D, False).astype(np.int32)
        cframe = dframe[crow]
        gidx, _ = cascade.match_detections(dets, crow, cframe, gt, goff, 0.5)
        matched = np.nonzero(gidx.cpu().numpy() >= 0)[0]
        jitter = np.zeros((D, A, 7))
        jitter[matched] = cascade.draw_box3d_jitter(len(matched), A, rng=rng)
        sel = cascade.refine_training_candidates(pts, off, dets, crow, cframe, gidx, gt, jitter=jitter)
        kept_hist.append(len(sel["kept"]))
        return b.build_device_train(sel, [types[r] for r in crow], draws=dd)

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
    wall = {"host": [], "eager": [], "replay": []}
    devt = {"host": [], "eager": [], "replay": []}
    few = 0
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

    for blk in range(a.iters // 10):                            # the three paths alternate in blocks of ten
        for _ in range(10):
            out_h = timed("host", host_step)
        for what, fn in (("replay", graph.replay), ("eager", src.step)):
            for _ in range(10):
                timed(what, fn)
                few += int(src.n_kept.cpu()[0]) < B
                rows_hist.append(int(src.off.cpu()[-1]))
    assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point())
    assert all(torch.isfinite(v).all() for v in out_h.values() if isinstance(v, torch.Tensor) and v.is_floating_point())
    status = int(src.status.cpu()[0])
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    shape = {"frames": a.frames, "rows": int(off[-1]), "S": src.S, "dets": R, "B": B, "D": D, "A": A, "npoints": a.npoints, "lpad": lpad}
    print(json.dumps(dict(shape, what="host_path", wall_us=us(wall["host"]), wall_us_min=round(min(wall["host"]) * 1e6, 1),
                          device_us=us(devt["host"]), kept_min=int(min(kept_hist)), kept_median=float(np.median(kept_hist)))), flush=True)
    for what in ("eager", "replay"):
        print(json.dumps(dict(shape, what="train_source_" + what, wall_us=us(wall[what]), wall_us_min=round(min(wall[what]) * 1e6, 1),
                              device_us=us(devt[what]))), flush=True)
    print(json.dumps({"what": "summary", "host_wall_us": us(wall["host"]), "eager_wall_us": us(wall["eager"]),
                      "replay_wall_us": us(wall["replay"]), "replay_device_us": us(devt["replay"]),
                      "host_over_replay_wall": round(us(wall["host"]) / us(wall["replay"]), 2),
                      "few_share": round(few / (len(wall["replay"]) + len(wall["eager"])), 4), "rows_median": float(np.median(rows_hist)),
                      "status": status, "steps": int(src.draws_jitter.state.cpu()[0])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
