"""A/B of the single-launch eval PointNet (fuse_eval, FCN_FUSED_EVAL) against the layered eval path on one GPU.

python tools/fused_eval_ab.py [--rounds 3]
    alternates FCN_FUSED_EVAL=0 / 1 in fresh child processes; each child takes bench.py's own inference measurement (eval forward
    + decode, hipGraph replay: the `inference` row of `bench.py --full`) for the configurations below and its detect() row; prints
    one JSON line per child and the medians per setting.
python tools/fused_eval_ab.py --trace 12
    12 eager eval forwards of the car configuration, 30 ms apart: the program to put behind `rocprofv3 --kernel-trace --stats --`.
python tools/fused_eval_ab.py --timeline kernel_trace.csv
    the last forward of such a trace launch by launch (forwards are split at the 30 ms gaps), the launch count and the time per
    kernel name."""
import argparse
import collections
import csv
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS = (("car", "split"), ("car", "bf16"), ("car", "bf16ops"), ("people", "split"), ("refine", "split"), ("sunrgbd", "split"))


def child(min_time):
    import torch
    import bench
    dev = torch.device("cuda:0")
    out = {"fused_eval": os.environ.get("FCN_FUSED_EVAL", "0")}
    for cfg, prec in ROWS:
        r = bench.measure_inference(cfg, 32, dev, min_time, prec)
        out["%s/%s" % (cfg, prec)] = r["value"]
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    d = bench.detect_row(dev, 32)
    out["detect frames/s"] = d["value"]
    out["detect launch"] = d["launch"]
    print(json.dumps(out), flush=True)


def trace(n):
    import torch
    import bench
    from frustum_convnet_amd import precision as fprec
    dev = torch.device("cuda:0")
    fprec.set_precision("split")
    model = bench.build_model(dev, "car").eval()
    data = bench.make_data("car", 32, bench.CFGS["car"][3], 1234, dev)
    data = {k: v for k, v in data.items() if k in ("point_cloud", "one_hot") or k.startswith("center_ref")}
    with torch.no_grad():
        for _ in range(n):
            model(data)
            torch.cuda.synchronize()
            time.sleep(0.03)
    print("fused_eval", model.feat_net.nets[0].fused_eval if hasattr(model.feat_net.nets[0], "fused_eval") else None)


def timeline(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    cuts = [0] + [i for i in range(1, len(rows)) if int(rows[i]["Start_Timestamp"]) - int(rows[i - 1]["End_Timestamp"]) > 15e6]
    fw = [rows[a:b] for a, b in zip(cuts, cuts[1:] + [len(rows)])]
    print("forwards %d, launches per forward %s" % (len(fw), [len(f) for f in fw]))
    last = fw[-1]
    t0 = int(last[0]["Start_Timestamp"])
    print("last forward: %d launches, first start to last end %.1f us, sum of kernel times %.1f us" % (
        len(last), (int(last[-1]["End_Timestamp"]) - t0) / 1e3,
        sum(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in last) / 1e3))
    for r in last:
        s, e = (int(r["Start_Timestamp"]) - t0) / 1e3, (int(r["End_Timestamp"]) - t0) / 1e3
        print("%8.1f %7.1f  %-70s wg=%d x %s" % (s, e - s, r["Kernel_Name"].split("(")[0][:70],
                                                 int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"]), r["Workgroup_Size_X"]))
    # medians over the forwards after the first three, per kernel name and position of the name within the forward
    agg = collections.OrderedDict()
    for f in fw[3:]:
        seen = collections.Counter()
        for r in f:
            n = r["Kernel_Name"].split("(")[0][:70]
            seen[n] += 1
            agg.setdefault((n, seen[n]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("median us per launch over forwards 4..%d (name, occurrence within the forward):" % len(fw))
    for (n, k), v in agg.items():
        print("%7.1f  %-70s #%d" % (statistics.median(v), n, k))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-time", type=float, default=0.5)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--trace", type=int, default=0)
    ap.add_argument("--timeline", default=None)
    a = ap.parse_args()
    if a.timeline:
        return timeline(a.timeline)
    if a.child:
        return child(a.min_time)
    if a.trace:
        return trace(a.trace)
    res = {"0": [], "1": []}
    for _ in range(a.rounds):
        for flag in ("0", "1"):
            env = dict(os.environ, FCN_FUSED_EVAL=flag)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--min-time", str(a.min_time)], env=env,
                               stdout=subprocess.PIPE, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit("child with FCN_FUSED_EVAL=%s ended with %d" % (flag, r.returncode))    # (nothing more is started)
            line = r.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            res[flag].append(json.loads(line))
    keys = [k for k in res["0"][0] if k not in ("fused_eval", "detect launch")]
    print("%-18s %12s %12s %8s" % ("median of %d" % a.rounds, "layered", "fused", "ratio"))
    for k in keys:
        m0, m1 = (statistics.median(r[k] for r in res[f]) for f in ("0", "1"))
        print("%-18s %12.1f %12.1f %8.3f" % (k, m0, m1, m1 / m0))


if __name__ == "__main__":
    main()
