"""Captured training step (forward, backward, Adam through FlatTrainState) of the car configuration at B=32, N=1024 with batch-
statistics BatchNorm and with frozen BatchNorm (PointNetDet.freeze_bn), timed with device events, the two graphs replayed in
alternating rounds in one process so that both see the same clocks.  Prints one JSON line: median step time per mode and the
frozen / training ratio.

    python tools/frozen_bn_timing.py [--rounds 8] [--steps 20]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (model / batch builders only)


def capture(frozen, data, dev):
    from frustum_convnet_amd.train_state import FlatTrainState
    m = bench.build_model(dev, "car")
    if frozen:
        m.freeze_bn()
    st = FlatTrainState(m, lr=1e-4, weight_decay=1e-4)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # warm-up outside capture (allocator, workspaces)
        for _ in range(2):
            lo, _ = m(data)
            m.backward(lo["total_loss"])
            st.adam_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        lo, _ = m(data)
        m.backward(lo["total_loss"])
        st.adam_step()
    return g, m, st, lo      # (the graph writes the optimiser state and the loss: they must outlive every replay)


def time_graph(g, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--npoint", type=int, default=1024)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    data = bench.make_data("car", a.batch, a.npoint, 1, dev)
    graphs = {"train": capture(False, data, dev), "frozen": capture(True, data, dev)}
    for g, *_ in graphs.values():
        time_graph(g, 3)
    ms = {k: [] for k in graphs}
    for r in range(a.rounds):
        for k in (("train", "frozen") if r % 2 == 0 else ("frozen", "train")):
            ms[k].append(time_graph(graphs[k][0], a.steps))
    med = {k: statistics.median(v) for k, v in ms.items()}
    print(json.dumps({"workload": "car_b%d_n%d captured step" % (a.batch, a.npoint), "rounds": a.rounds, "steps": a.steps,
                      "train_ms": round(med["train"], 4), "frozen_ms": round(med["frozen"], 4),
                      "frozen_over_train": round(med["frozen"] / med["train"], 4),
                      "train_rounds_ms": [round(x, 4) for x in ms["train"]],
                      "frozen_rounds_ms": [round(x, 4) for x in ms["frozen"]]}))


if __name__ == "__main__":
    main()
