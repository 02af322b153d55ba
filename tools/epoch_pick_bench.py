"""Times the epoch sampler (inputs.EpochSampler, C-ABI fcn_epoch_pick, csrc/epoch_pick.h) on one GPU, beside what it replaces:
  (a) the kernel: one fcn_epoch_pick at G = 4096, 16 384, 65 536 and 262 144 labels, D = 48, at the first, a middle and the last
      window of an epoch (advance = 0, so the window stays), and in the same run fcn_draw_batch at B = 1, N = D over the same G --
      what pick=True costs a training source today;
  (b) the step: tools/frustum_train_source_bench.py's scene through frustum.FrameTrainSource.step(), captured and replayed, with
      pick=True and with pick="epoch", the two alternating over --repeats rounds.
The counterpart of tools/device_draw_bench.py, whose conventions it keeps.

python tools/epoch_pick_bench.py [--iters 200] [--repeats 3] [--frames 8] [--rows 120000] [--batch 32] [--boxes 48]
    prints one JSON line per measurement and one summary line.  It fails without a GPU; nothing falls back.

Times: `device_us` is the device-event time around one call into given buffers, median over the iterations (the draw is two
launches issued from the host, so its figure holds the gap between them); `in_graph_us` the device-event time of a replayed graph of
20 such calls, over 20 (no host between the launches: what a captured step pays).  `replay_device_us` is the device-event time
around one replay of the captured step, median per round; `spread_us` the distance between the largest and the smallest round median
of the pick=True step: an epoch figure within that distance of the pick=True figure is not a measured difference.  A record for
EXPERIMENTS.md; no test depends on a time.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GS = (4096, 16384, 65536, 262144)
K = 20


def timed(torch, call, iters):
    """(device_us of one call, in_graph_us per call of a replayed graph of K calls)."""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(iters)]
    for it in range(-10, iters):                                    # ten warm-up rounds
        e = ev[max(it, 0)]
        e[0].record()
        call()
        e[1].record()
    torch.cuda.synchronize()
    device_us = float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e3
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(K):
            call()
    gev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(20)]
    for it in range(-3, 20):
        e = gev[max(it, 0)]
        e[0].record()
        graph.replay()
        e[1].record()
    torch.cuda.synchronize()
    return round(device_us, 2), round(float(np.median([e[0].elapsed_time(e[1]) for e in gev])) * 1e3 / K, 2)


def kernels(a, torch, inputs, dev):
    D = a.boxes
    for G in GS:
        cd = torch.tensor([G], dtype=torch.int64, device=dev)
        T = G // D
        s = inputs.EpochSampler(7, dev)
        out = torch.zeros((D,), dtype=torch.int32, device=dev)
        for name, t in (("first", 0), ("middle", T // 2), ("last", T - 1)):
            s.state.copy_(torch.tensor([3, t], dtype=torch.int64))
            torch.cuda.synchronize()
            d_us, g_us = timed(torch, lambda: s.pick(cd, D, out=out, advance=False), a.iters)
            s.check()
            print(json.dumps({"what": "epoch_pick", "G": G, "D": D, "window": name, "turn": t, "device_us": d_us, "in_graph_us": g_us}),
                  flush=True)
        dd = inputs.DeviceDraws(7, dev)
        o = dd.draw(cd, D, False, False)
        d_us, g_us = timed(torch, lambda: dd.draw(cd, D, False, False, out=o), a.iters)
        dd.check()
        print(json.dumps({"what": "draw_batch", "G": G, "D": D, "B": 1, "device_us": d_us, "in_graph_us": g_us}), flush=True)


def steps(a, torch, inputs, dev):
    from frustum_convnet_amd import frustum
    from frustum_train_source_bench import scene
    pts_h, off, calib, wh, gt2d, gt3d, bframe, types = scene(a.frames, a.rows)
    G, B, D = len(bframe), a.batch, a.boxes
    pts = torch.from_numpy(pts_h).to(dev)
    cal = {k: torch.from_numpy(v).to(dev) for k, v in calib.items()}
    b = inputs.InputBuilder(a.npoints, random_flip=True, random_shift=True)
    graphs = {}
    for pick in (True, "epoch"):
        src = frustum.FrameTrainSource(pts, off, cal, wh, gt2d, gt3d, bframe, types, b, B, D, 1 << 20, 7, pick=pick)
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(5):
                src.step()
        torch.cuda.current_stream().wait_stream(stream)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = src.step()
        torch.cuda.synchronize()
        graphs[pick] = (src, graph, out)
    rounds = {True: [], "epoch": []}
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(a.iters)]
    for r in range(a.repeats):                                      # the two modes alternate
        for pick in (True, "epoch"):
            src, graph, out = graphs[pick]
            for it in range(-5, a.iters):
                e = ev[max(it, 0)]
                e[0].record()
                graph.replay()
                e[1].record()
            torch.cuda.synchronize()
            rounds[pick].append(round(float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e3, 1))
    shape = {"frames": a.frames, "rows": int(off[-1]), "labels": G, "B": B, "D": D, "npoints": a.npoints}
    for pick in (True, "epoch"):
        src, graph, out = graphs[pick]
        assert all(torch.isfinite(v).all() for v in out.values() if v.is_floating_point())
        extra = {} if src.sampler is None else {"epoch_state": [int(x) for x in src.sampler.state.cpu().tolist()],
                                                "turns_per_epoch": src.sampler.steps_per_epoch(G, D)}
        print(json.dumps(dict(shape, what="train_source", pick=pick, replay_device_us=rounds[pick],
                              steps=int(src.draws_box.state.cpu()[0]), **extra)), flush=True)
    t_med, e_med = float(np.median(rounds[True])), float(np.median(rounds["epoch"]))
    spread = max(rounds[True]) - min(rounds[True])
    print(json.dumps({"what": "summary", "pick_true_us": t_med, "pick_epoch_us": e_med, "epoch_minus_true_us": round(e_med - t_med, 1),
                      "spread_us": round(spread, 1), "slower_beyond_spread": bool(e_med - t_med > spread)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--rows", type=int, default=120000)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--boxes", type=int, default=48)
    ap.add_argument("--npoints", type=int, default=1024)
    a = ap.parse_args()
    import torch
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    reset_cfg()
    kernels(a, torch, inputs, dev)
    steps(a, torch, inputs, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
