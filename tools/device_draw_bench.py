"""Times the batch builders' random draws at B = 32 on one GPU, both ways: the host path every builder defaults to -- read the
per-sample row counts back, inputs.draw() / draw_sunrgbd() in numpy (np.random.choice per sample: a full permutation of n rows
where n >= N), upload the (B, N) int32 table and the scalars -- against inputs.DeviceDraws.draw (C-ABI fcn_draw_batch,
csrc/draws.h), which writes the same four arrays on the device.  The counterpart of tools/frustum_sunrgbd_bench.py, whose
conventions it keeps.

python tools/device_draw_bench.py [--batch 32] [--iters 200] [--limit 240]
    runs the two measurements in child processes of their own, each under a time limit (--limit seconds), and prints one JSON
    line per workload and child and one summary line per workload.  The children fail without a GPU; nothing falls back.

Workloads (row counts of synthetic frustums, synth.make_records; the points themselves play no part):
    car      N = 1024, n ~ U(1200, 2400)          cfgs/det_sample.yaml          (every row without replacement)
    people   N = 1024, n ~ U(100, 1500)           cfgs/det_sample_people.yaml   (mostly with replacement)
    refine   N =  512, n ~ U(200, 1600)           cfgs/refine_car.yaml
    sunrgbd  N = 2048, n ~ U(1000, 30000), a box over 2048 rows subsampled to 2048 (composed in the kernel); + the height shift

Times: host `wall_us` is the wall clock of one count read + draw + upload, synchronised, median over the iterations.  Device
`device_us` is the device-event time around one DeviceDraws.draw into given buffers (two launches issued from the host, so it
holds the gap between them), median; `in_graph_us` the device-event time of a replayed graph of 20 such calls, over 20 (no host
between the launches: what a captured step pays per draw); `wall_us` the wall clock of one call synchronised, median;
`enqueue_us` the host time of the call alone (what a training loop pays when it does not wait).  A record for EXPERIMENTS.md; no test depends on a time.
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

WORKLOADS = (("car", 1024, (1200, 2400), False), ("people", 1024, (100, 1500), False), ("refine", 512, (200, 1600), False),
             ("sunrgbd", 2048, (1000, 30000), True))
CAP = 2048


def counts_of(name, batch, n_raw):
    from frustum_convnet_amd import synth
    u = synth.uniform01(1234, synth.stream_id("draw_bench_" + name), (batch,))
    return (n_raw[0] + u * (n_raw[1] - n_raw[0])).astype(np.int64)


def subsamples(counts):
    rng = np.random.RandomState(3)
    return [np.sort(rng.choice(int(n), CAP, False)).astype(np.int32) if n > CAP else None for n in counts]


def host_child(a):
    import torch
    from frustum_convnet_amd import inputs
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev, non_blocking=True)
    for name, N, n_raw, sun in WORKLOADS:
        counts = counts_of(name, a.batch, n_raw)
        sub = subsamples(counts) if sun else None
        cd = up(counts)
        compose = lambda ch: inputs.SunrgbdInputBuilder._compose(None, ch, sub)     # (the host's composition; no builder state)
        np.random.seed(1)
        ts = []
        for it in range(-5, a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            c = cd.cpu().numpy()                                        # the count read
            if sun:
                rows = np.asarray([n if s is None else len(s) for n, s in zip(c, sub)])
                d = inputs.draw_sunrgbd(rows, N, True, True)
                t = (up(compose(d[0])),) + tuple(up(x) for x in d[1:])
            else:
                d = inputs.draw(c, N, True, True)
                t = tuple(up(x) for x in d)
            torch.cuda.synchronize()
            if it >= 0:
                ts.append(time.perf_counter() - t0)
        print(json.dumps({"what": "host", "workload": name, "batch": a.batch, "N": N, "rows_min": int(counts.min()),
                          "rows_max": int(counts.max()), "wall_us": round(float(np.median(ts)) * 1e6, 1),
                          "upload_bytes": int(sum(x.numel() * x.element_size() for x in t))}), flush=True)


def device_child(a):
    import torch
    from frustum_convnet_amd import inputs
    assert torch.cuda.is_available(), "the measurement needs an MI355X"
    dev = torch.device("cuda:0")
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    for name, N, n_raw, sun in WORKLOADS:
        counts = counts_of(name, a.batch, n_raw)
        cd = up(counts)
        kw = {}
        if sun:
            sub = subsamples(counts)
            lens = [0 if s is None else len(s) for s in sub]
            kw = {"sub": up(np.concatenate([s for s in sub if s is not None])), "sub_off": up(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64))}
        dd = inputs.DeviceDraws(7, dev)
        out = dd.draw(cd, N, True, True, hshift=sun, **kw)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(a.iters)]
        for it in range(-10, a.iters):                                  # ten warm-up rounds
            e = ev[max(it, 0)]
            e[0].record()
            dd.draw(cd, N, True, True, hshift=sun, out=out, **kw)
            e[1].record()
        torch.cuda.synchronize()
        device_us = float(np.median([e[0].elapsed_time(e[1]) for e in ev])) * 1e3
        wall, enq = [], []
        for _ in range(a.iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dd.draw(cd, N, True, True, hshift=sun, out=out, **kw)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            enq.append(t1 - t0)
        # back to back inside one captured graph: no host between the launches (what a captured training step pays per draw)
        K = 20
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(K):
                dd.draw(cd, N, True, True, hshift=sun, out=out, **kw)
        gev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(20)]
        for it in range(-3, 20):
            e = gev[max(it, 0)]
            e[0].record()
            graph.replay()
            e[1].record()
        torch.cuda.synchronize()
        graph_us = float(np.median([e[0].elapsed_time(e[1]) for e in gev])) * 1e3 / K
        dd.check()
        print(json.dumps({"what": "device", "workload": name, "batch": a.batch, "N": N, "device_us": round(device_us, 2),
                          "in_graph_us": round(graph_us, 2),
                          "wall_us": round(float(np.median(wall)) * 1e6, 1), "enqueue_us": round(float(np.median(enq)) * 1e6, 1),
                          "steps_drawn": int(dd.state.cpu()[0])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--limit", type=float, default=240.0)
    ap.add_argument("--child", choices=("device", "host"))
    a = ap.parse_args()
    if a.child:
        return (device_child if a.child == "device" else host_child)(a)
    rows = {}
    for which in ("host", "device"):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--batch", str(a.batch), "--iters", str(a.iters)]
        p = subprocess.run(cmd, timeout=a.limit, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(p.stdout)
        if p.returncode != 0:
            print(json.dumps({"what": which, "error": "exit status %d" % p.returncode}), flush=True)
            return 1
        for line in p.stdout.strip().splitlines():
            r = json.loads(line)
            rows[(which, r["workload"])] = r
    for name, _, _, _ in WORKLOADS:
        h, d = rows[("host", name)], rows[("device", name)]
        print(json.dumps({"what": "summary", "workload": name, "host_wall_us": h["wall_us"], "device_wall_us": d["wall_us"],
                          "device_us": d["device_us"], "in_graph_us": d["in_graph_us"], "host_over_device_wall": round(h["wall_us"] / d["wall_us"], 1)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
