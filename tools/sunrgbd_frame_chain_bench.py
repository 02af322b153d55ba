"""Times one SUN-RGBD INFERENCE call from depth frames and 2-D boxes -- upright-depth frames + a 2-D detector's boxes to the corners,
scores and group offsets of the kept detections -- on one GPU, three ways on the same scene, in one run:
  (a) SunrgbdDetector.detect_frames, the existing path: sunrgbd_candidates reads box_frame / frame_off and the D * S segment counts
      back and draws rng.choice(n, cap, replace=False) on the host for every frustum over `cap` rows, build_device builds the kept
      list on the host and uploads the subsamples, detect_frames reads the keep lists back and uploads the kept rows again;
  (b) evaluate.SunrgbdFrameChain.step() uncaptured;
  (c) the same step captured once into a graph and replayed: no host read, no upload, fixed sizes.
And the front alone: frustum.SunrgbdDetectSource.step() against sunrgbd_candidates + SunrgbdInputBuilder.build_device.  The
counterpart of tools/frame_cascade_bench.py, whose conventions it keeps.

python tools/sunrgbd_frame_chain_bench.py [--frames 8] [--rows 300000] [--boxes 32] [--npoints 2048] [--cap 2048] [--top-k 300]
                                          [--iters 100]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.

The scene (seeded, synthetic) is that of tools/sunrgbd_train_source_bench.py: bench.py's five-scale model (synthetic weights); F depth
frames of about `rows` upright-depth rows (x, y, z, r, g, b) each under one camera matrix and tilt, ten objects per frame with points
of their own; the 2-D boxes are the image boxes of the first boxes / F objects of every frame.  B = D = `boxes`: every box has a slot,
so both paths keep the same boxes (the summary says so: `same_kept_boxes`); the host path draws its resample with DeviceDraws too,
which favours it.  The two paths draw from different streams (numpy's on the host, the counter-based one on the device), so they are
compared on their kept boxes, not on their rows.

Times: `wall_us`: the wall clock of one call synchronised, median over the iterations, the paths alternating in blocks of ten;
`device_us`: the device-event time around the same call, median (for the existing paths it includes the device's idle time while
the host reads).  All outputs are checked finite.  A record for EXPERIMENTS.md; no test depends on a time.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=300000)
    ap.add_argument("--boxes", type=int, default=32)
    ap.add_argument("--npoints", type=int, default=2048)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--top-k", type=int, default=300)
    ap.add_argument("--capacity", type=int, default=4 << 20)
    ap.add_argument("--iters", type=int, default=100)
    a = ap.parse_args()
    import torch
    import bench
    from sunrgbd_train_source_bench import PER_FRAME, scene
    from frustum_convnet_amd import evaluate, frustum, inputs
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    F, D = a.frames, a.boxes
    model = bench.build_model(dev, "sunrgbd").eval()            # (cfg holds the SUN-RGBD configuration from here on)
    b = inputs.SunrgbdInputBuilder(a.npoints)
    pts_h, off, Kf, Rf, gt2d, _, gframe, gtypes = scene(F, a.rows)
    per = -(-D // F)
    pick = np.asarray([f * PER_FRAME + k for f in range(F) for k in range(min(per, 10))][:D])      # objects only
    b2d, bframe, types = gt2d[pick], gframe[pick], [gtypes[i] for i in pick]
    prob = np.linspace(0.5, 0.95, D)
    pts = torch.from_numpy(pts_h).to(dev)
    Kd, Rd = torch.from_numpy(Kf).to(dev), torch.from_numpy(Rf).to(dev)
    det = evaluate.SunrgbdDetector(model, b)
    chain = det.frame_link(pts, off, Kd, Rd, D, D, a.capacity, 7, "nms", 0.1, top_k=a.top_k, cap=a.cap)
    chain.source.set_boxes(b2d, bframe, types, prob)
    src = frustum.SunrgbdDetectSource(pts, off, Kd, Rd, b, D, D, a.capacity, 7, cap=a.cap).set_boxes(b2d, bframe, types, prob)
    dd = inputs.DeviceDraws(7, dev)
    off_d = torch.from_numpy(off).to(dev)

    def host_call():
        return det.detect_frames(pts, off_d, Kd, Rd, b2d, bframe, types, prob, "nms", 0.1, top_k=a.top_k, draws=dd)

    def host_front():
        sel = frustum.sunrgbd_candidates(pts, off_d, Kd, Rd, b2d, bframe, cap=a.cap)
        return b.build_device(sel, Kd, Rd, types, prob, draws=dd)

    # ---- warm-up of all, then the captures (after a side-stream warm-up, as torch asks)
    for _ in range(3):
        res = host_call()
        front = host_front()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            chain.step()
            src.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for part in (chain, src):
        try:
            part.check()
        except ValueError as e:                                 # (empty slots flag the draws' bit 0: the summary reports the words)
            print(json.dumps({"what": "warm-up status", "status": str(e)}), flush=True)
    graph, sgraph = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = chain.step()
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

    for blk in range(max(1, a.iters // 10)):                    # the paths alternate in blocks of ten
        for what, fn in (("host", host_call), ("replay", graph.replay), ("eager", chain.step), ("host_front", host_front),
                         ("source_replay", sgraph.replay), ("source_eager", src.step)):
            for _ in range(10):
                r = timed(what, fn)
            if what == "host":
                res = r
            if what == "host_front":
                front = r
    t0 = time.perf_counter()
    got = chain.result()
    result_us = (time.perf_counter() - t0) * 1e6
    n = int(out["n_kept"].cpu()[0])
    assert torch.isfinite(out["dets"]).all() and n > 0 and all(torch.isfinite(v).all() for v in out["batch"].values())
    assert res["dets"] is not None and torch.isfinite(res["dets"]).all() and torch.isfinite(got["corners"]).all()
    same_boxes = bool(np.array_equal(got["kept"], res["kept"]))
    same_front = bool(np.array_equal(sout["slot_box"].cpu().numpy()[:int(sout["n_kept"].cpu()[0])], front["kept"]))
    us = lambda v: round(float(np.median(v)) * 1e6, 1)
    shape = {"frames": F, "rows": int(off[-1]), "S": chain.source.S, "boxes": D, "B": D, "G": chain.G, "top_k": a.top_k,
             "npoints": a.npoints, "cap": a.cap, "n_kept": n, "host_kept": int(len(res["kept"])),
             "subsampled_slots": int((chain.source.sub_len > 0).sum()), "rows_filled": int(chain.source.counts.sum()),
             "kept_rows": int(len(got["rows"])), "host_kept_rows": int(len(res["rows"]))}
    for what, name in (("host", "detect_frames"), ("eager", "frame_chain_eager"), ("replay", "frame_chain_replay"),
                       ("host_front", "candidates_build_device"), ("source_eager", "detect_source_eager"),
                       ("source_replay", "detect_source_replay")):
        print(json.dumps(dict(shape, what=name, wall_us=us(wall[what]), wall_us_min=round(min(wall[what]) * 1e6, 1),
                              device_us=us(devt[what]), calls=len(wall[what]))), flush=True)
    st = lambda *w: int(sum(int(x.cpu()[0]) for x in w))
    print(json.dumps({"what": "summary", "host_wall_us": us(wall["host"]), "eager_wall_us": us(wall["eager"]),
                      "replay_wall_us": us(wall["replay"]), "replay_device_us": us(devt["replay"]),
                      "host_over_replay_wall": round(us(wall["host"]) / us(wall["replay"]), 2),
                      "front_host_wall_us": us(wall["host_front"]), "front_replay_wall_us": us(wall["source_replay"]),
                      "front_replay_device_us": us(devt["source_replay"]),
                      "front_host_over_replay_wall": round(us(wall["host_front"]) / us(wall["source_replay"]), 2),
                      "result_read_us": round(result_us, 1), "same_kept_boxes": same_boxes, "same_front": same_front,
                      "status": st(chain.source.status, chain.status),
                      "draws_status": st(chain.source.draws.status, chain.source.draws_sub.status),
                      "steps": int(chain.source.draws.state.cpu()[0])}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
