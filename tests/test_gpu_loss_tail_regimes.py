"""-m gpu: the fused loss tail (csrc/loss_tail.hip: fcn_det_loss_tail, fcn_det_loss_tail_rows2) and the IoU metric kernel
(csrc/box_iou.hip: fcn_det_iou_metrics) on SYNTHETIC logits that reach every branch of the kernels by construction, against
oracle.det_ref.loss_tail in float64 (autograd for d total / d logits) and oracle.box_ref.iou_metrics.

The golden fixtures feed these kernels the logits of an untrained network with one foreground row per frustum (the census
of `test_fixture_census_is_printed` shows which branches they reach).  Here the generator starts from the labels, writes the
logits row that encodes each label exactly, and perturbs it per loss term on a ladder 0, 1e-3, 0.03, 0.3, 1, 3, 10 (times
a factor in [0.6, 1.4]), so both sides of the four Huber terms, exact zeros, the flipped label box winning the corner
minimum, decoded angles above pi, label headings on bin edges / +-pi / negative / above 2 pi, every size class, both
accuracy outcomes and class logits from a tie to +-90 are all present; `census()` counts them from float64 quantities and
the test asserts a minimum of CENSUS_MIN = 5 rows per row regime (3 frustums per heading regime) for every batch of at
least 1000 rows (smaller batches draw from the same generator; a batch of one row cannot hold every regime).

No row sits on a kink: a row whose float64 distance to dist = 3, |e| = 1, n = 1, cd = 1, d1 = d2 or iou3d = thresh is below
KINK = 1e-3 of the quantity is drawn again, class-logit margins are exactly 0 or >= 6e-4, arg-max margins of the heading /
size scores are >= 2 by construction, and label headings that are not ON an edge on purpose keep 1e-3 rad from every bin
edge.  Headings placed on an edge on purpose keep their rows in the comparison: the label bin is recomputed in float32
numpy with the kernel's pymod formula (with and without the fused multiply-add a compiler may contract it to; an edge value
on which the two disagree is moved to its next float32 neighbour) and given to the float64 referee.  The share of rows left
out of any comparison is 0, and asserted.

Bars.  Loss scalars 1e-4 * max(1, |ref|), accuracies 1e-6, whole-tensor gradient 1e-4 * max|ref| + 1e-7, IoU metrics 1e-4,
1e-4, 1e-6: the project's existing bars.  Per-row gradient: max|got - ref| over the row's 2 + 39 / 2 + 67 entries divided by
max(largest |ref| entry of that row, ROW_FLOOR / nfg) -- every gradient entry carries the factor 1 / nfg, a row's largest
entry is typically 1 / nfg to 20 / nfg, so the floor is about 1e-3 of a typical row.  The float32 evaluation of the oracle on
the same inputs (all shapes below, both instantiations) misses the float64 one by at most 1.42e-4 in that measure
(the worst rows are the nearly converged ones: corner differences of ~1e-3 m between coordinates of up to 60 m)
(`test_generator_terminates_and_float32_oracle_error`, which prints it); the kernel is allowed ROW_BAR = 4 x that
= 5.7e-4 (two float32 evaluations in different operation order, device cosf / sinf / expf not correctly rounded).  The rows
with saturated class logits are covered by the same measure (their float64 gradient is ~0, so the floor makes it absolute:
5.7e-4 * 1e-2 / nfg).  Measured for the kernel, worst row of all cases: 1.56e-4 on an MI355X, 9.6e-5 under
the host emulation (EXPERIMENTS.md, "Loss tail, decode, IoU and NMS off the fixture regime")."""
import numpy as np
import pytest
import torch

from helpers import load_golden, golden_inputs
from oracle import box_ref, det_ref

pytestmark = pytest.mark.gpu

NB = 12
PER64 = 2 * np.pi / NB
HALF64 = PER64 / 2
PER32 = np.float32(6.283185307179586 / NB)
HALF32 = np.float32(6.283185307179586 / NB / 2.0)
TWO_PI32 = np.float32(6.283185307179586)
W = (1.0, 10.0, 20.0, 20.0)            # BOX, CORNER, HEAD_REG, SIZE_REG (oracle.det_ref.LOSS_W)
THRESH = 0.7
LADDER = (0.0, 1e-3, 0.03, 0.3, 1.0, 3.0, 10.0)
KINK = 1e-3
CENSUS_MIN = 5
CENSUS_MIN_FRUSTUMS = 3
ROW_FLOOR = 1e-2
ROW_BAR = 5.7e-4                       # 4 x 1.42e-4 (float32 oracle vs float64 oracle, worst row of all shapes)

SHAPES = [(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (7, 9), (4, 16), (5, 13), (127, 1), (2, 64), (3, 43), (149, 7), (32, 140),
          (33, 140), (10, 252)]
MODES = ["nfg0", "allfg", "allignored", "lastfg"]


def mean_size32(ns):
    return (det_ref.MEAN_SIZE if ns == 3 else det_ref.MEAN_SIZE_SUNRGBD).astype(np.float32)


def _pymod32(a, b, fma):
    a, b = np.float32(a), np.float32(b)
    f = np.floor(a / b).astype(np.float32)
    if fma:
        return np.float32(np.float64(a) - np.float64(b) * np.float64(f))
    return np.float32(a - np.float32(b * f))


def head_bin32(h, fma=False):
    """The kernel's label bin and residual (loss_tail.hip: pymod, shifted, hc, hres) in float32 numpy."""
    ga = _pymod32(h, TWO_PI32, fma)
    sh = _pymod32(np.float32(ga + HALF32), TWO_PI32, fma)
    hc = int(min(max(int(np.floor(np.float32(sh / PER32))), 0), NB - 1))
    center = np.float32(np.float32(np.float32(hc) * PER32) + HALF32)
    if fma:
        center = np.float32(np.float64(np.float32(hc)) * np.float64(PER32) + np.float64(HALF32))
    return hc, np.float32(np.float32(sh - center) / HALF32)


def _edge(k, m=0):
    return np.float32(k * PER64 - HALF64 + 2 * np.pi * m)


def _up(x):
    return np.nextafter(np.float32(x), np.float32(np.inf))


def _down(x):
    return np.nextafter(np.float32(x), np.float32(-np.inf))


def special_headings():
    """Label headings the fixtures never see: on bin edges (k * per - half) and their float32 neighbours, exactly +-pi,
    negative, above 2 pi, below -2 pi."""
    out = [_edge(0), np.float32(np.pi), np.float32(-np.pi), np.float32(-2.0), np.float32(7.5), _up(_edge(6)), _down(_edge(3)),
           np.float32(-7.0), _edge(1), np.float32(np.pi), np.float32(9.0), _edge(7), _up(_edge(9)), _down(_edge(11)),
           _edge(4, 1), np.float32(-np.pi), _edge(5, -1)]
    for k in range(NB):
        out += [_edge(k), _up(_edge(k)), _down(_edge(k))]
    return out


def edge_distance64(h):
    sh = ((np.float64(h) % (2 * np.pi)) + HALF64) % (2 * np.pi)
    fr = sh / PER64 - np.floor(sh / PER64)
    return min(fr, 1 - fr) * PER64


def make_batch(ns, B, L2, seed, mode="mixed"):
    """-> (logits (R, 2 + nc) float32, data dict of numpy arrays, hc (B,) int64 float32 label bins, info)."""
    rng = np.random.default_rng(seed)
    nc = 3 + 2 * NB + 4 * ns
    R = B * L2
    ms = mean_size32(ns)
    q = lambda x: (np.round(np.asarray(x, np.float64) * 1024) / 1024).astype(np.float32)      # multiples of 2^-10: differences exact
    lab = rng.choice(np.array([1, 0, -1]), size=R, p=[0.45, 0.4, 0.15]).astype(np.int64)
    if mode == "nfg0":
        lab[lab == 1] = 0
    elif mode == "allfg":
        lab[:] = 1
    elif mode == "allignored":
        lab[:] = -1
    elif mode == "lastfg":
        lab[lab == 1] = 0
        lab[R - 1] = 1
    center = q(np.stack([rng.uniform(-10, 10, B), rng.uniform(0.5, 2, B), rng.uniform(5, 60, B)], 1))
    ref2 = q(center[:, :, None] + rng.normal(0, 1, (B, 3, L2)))
    size_class = (np.arange(B) % ns).astype(np.int64)
    rng.shuffle(size_class)
    size = (ms[size_class] * rng.uniform(0.7, 1.4, (B, 3))).astype(np.float32)
    heading = rng.uniform(-np.pi, np.pi, B).astype(np.float32)
    spec = special_headings()
    zero_fr = np.zeros(B, dtype=bool)
    on_edge = np.zeros(B, dtype=bool)
    moved = 0
    for b in range(B):
        if b % 2 == 0:
            heading[b] = spec[(b // 2) % len(spec)]
            while head_bin32(heading[b], False)[0] != head_bin32(heading[b], True)[0]:       # contraction-dependent bin
                heading[b] = _up(heading[b])
                moved += 1
            on_edge[b] = edge_distance64(heading[b]) < 1e-5
        elif b % 4 == 1:                      # the perfect row is EXACT in float32: heading = fl(k * per), size = the cluster mean
            zero_fr[b] = True
            heading[b] = np.float32(np.float32(rng.integers(0, 6)) * PER32)
            size[b] = ms[size_class[b]]
        if not on_edge[b]:
            while edge_distance64(heading[b]) < KINK and not zero_fr[b]:
                heading[b] = np.float32(rng.uniform(-np.pi, np.pi))
    hc = np.array([head_bin32(h)[0] for h in heading], dtype=np.int64)
    hres = np.array([head_bin32(h)[1] for h in heading], dtype=np.float32)
    d = {"cls_label": lab.reshape(B, L2), "center_ref2": ref2, "box3d_center": center, "box3d_heading": heading.reshape(B, 1),
         "box3d_size": size, "size_class": size_class.reshape(B, 1)}
    logits = np.zeros((R, 2 + nc), dtype=np.float32)
    f32 = np.float32

    def unit(n):
        v = rng.normal(0, 1, n)
        return v / np.linalg.norm(v)

    def scale(top=len(LADDER)):
        return LADDER[rng.integers(0, top)] * rng.uniform(0.6, 1.4)

    def fill(r):
        b, l = divmod(r, L2)
        row = logits[r]
        row[:] = rng.normal(0, 1, 2 + nc).astype(f32)
        # class logits: a tie, margins up the ladder, saturated +-30 / +-90 -- for both targets and for ignored rows
        m = (0.0, 1e-3, 0.03, 0.3, 1.0, 3.0, 10.0, 30.0, 90.0)[rng.integers(0, 9)]
        m *= rng.uniform(0.6, 1.4) * (1 if rng.random() < 0.5 else -1)
        base = f32(rng.normal(0, 1))
        row[0], row[1] = base, f32(base + f32(m))
        if abs(float(row[1]) - float(row[0])) < 6e-4:
            row[1] = row[0]
        if lab[r] != 1:
            return
        all_zero = zero_fr[b] and rng.random() < 0.3
        flip = (not all_zero) and rng.random() < 0.15
        s_c, s_h, s_s = (0.0, 0.0, 0.0) if all_zero else (scale(), scale(5 if flip else len(LADDER)), scale())
        o = row[2:]
        o[0:3] = (center[b] - ref2[b, :, l]) + (s_c * unit(3)).astype(f32)
        k = hc[b]
        hs = np.clip(rng.normal(0, 0.5, NB), -2, 2)
        hs[k if rng.random() < 0.7 else (k + rng.integers(1, NB)) % NB] = 4.0
        o[3:3 + NB] = hs.astype(f32)
        hr = rng.normal(0, 0.3, NB).astype(f32)
        sg = 1.0 if rng.random() < 0.5 else -1.0
        hr[k] = hres[b] + f32(sg * s_h) + f32((12.0 if rng.random() < 0.5 else -12.0) if flip else 0.0)
        o[3 + NB:3 + 2 * NB] = hr
        sc = int(size_class[b])
        ss = np.clip(rng.normal(0, 0.5, ns), -2, 2)
        ss[sc if rng.random() < 0.7 else (sc + rng.integers(1, ns)) % ns] = 4.0
        o[3 + 2 * NB:3 + 2 * NB + ns] = ss.astype(f32)
        sr = rng.normal(0, 0.3, (ns, 3)).astype(f32)
        sr[sc] = (size[b] - ms[sc]) / ms[sc] + (s_s * unit(3)).astype(f32)
        o[3 + 2 * NB + ns:] = sr.reshape(-1)

    for r in range(R):
        fill(r)
    redrawn, rows = 0, np.nonzero(lab == 1)[0]
    for _ in range(200):
        if len(rows) == 0:
            break
        a = analyse(logits, d, ns, hc, rows)
        bad = ((np.abs(a["dist"] - 3) < 3 * KINK) | (np.abs(np.abs(a["e"]) - 1) < KINK) | (np.abs(a["n"] - 1) < KINK)
               | (np.abs(a["cd"] - 1) < KINK) | (np.abs(a["d1"] - a["d2"]) < KINK * np.maximum(a["d1"], a["d2"]))
               | (np.abs(a["iou3d"] - THRESH) < KINK))
        rows = rows[bad]
        redrawn += len(rows)
        for r in rows:
            fill(int(r))
    else:
        raise AssertionError("the generator did not move every row off the kinks")
    return logits, d, hc, {"redrawn": redrawn, "edge_moved": moved, "on_edge": on_edge, "zero_fr": zero_fr}


def analyse(logits, d, ns, hc_b, rows=None, with_iou=True):
    """float64 per-row quantities of the foreground rows `rows` (default: all of them)."""
    nc = 3 + 2 * NB + 4 * ns
    B, L2 = d["cls_label"].shape
    lab = d["cls_label"].reshape(-1)
    if rows is None:
        rows = np.nonzero(lab == 1)[0]
    rows = np.asarray(rows, dtype=np.int64)
    b = rows // L2
    ar = np.arange(len(rows))
    o = logits[rows, 2:2 + nc].astype(np.float64)
    ref2 = d["center_ref2"].transpose(0, 2, 1).reshape(-1, 3)[rows].astype(np.float64)
    cl = d["box3d_center"][b].astype(np.float64)
    hl = d["box3d_heading"].reshape(-1)[b].astype(np.float64)
    sl = d["box3d_size"][b].astype(np.float64)
    sc = d["size_class"].reshape(-1)[b]
    ms = mean_size32(ns).astype(np.float64)
    ex = ms[sc]
    hc = np.asarray(hc_b)[b]
    out = {"rows": rows, "b": b, "sc": sc}
    out["dist"] = np.linalg.norm(cl - ref2 - o[:, :3], axis=1)
    dl = hl % (2 * np.pi) - hc * PER64
    hres = ((dl + np.pi) % (2 * np.pi) - np.pi) / HALF64
    out["e"] = o[ar, 3 + NB + hc] - hres
    so = 3 + 2 * NB + ns + 3 * sc
    sel = o[ar[:, None], so[:, None] + np.arange(3)[None]]
    out["n"] = np.linalg.norm((sl - ex) / ex - sel, axis=1)
    pre = hc * PER64 + o[ar, 3 + NB + hc] * HALF64
    out["ang_pre"] = pre
    ang = np.where(pre > np.pi, pre - 2 * np.pi, pre)
    cp = box_ref.boxes3d2corners(np.concatenate([ref2 + o[:, :3], sel * ex + ex, ang[:, None]], 1))
    cg = box_ref.boxes3d2corners(np.concatenate([cl, sl, hl[:, None]], 1))
    cf = box_ref.boxes3d2corners(np.concatenate([cl, sl, hl[:, None] + np.pi], 1))
    out["d1"] = np.linalg.norm(cp - cg, axis=2).mean(1) if len(rows) else np.zeros(0)
    out["d2"] = np.linalg.norm(cp - cf, axis=2).mean(1) if len(rows) else np.zeros(0)
    out["cd"] = np.minimum(out["d1"], out["d2"])
    hs, ss = o[:, 3:3 + NB], o[:, 3 + 2 * NB:3 + 2 * NB + ns]
    out["head_hit"] = np.argmax(hs, 1) == hc if len(rows) else np.zeros(0, bool)
    out["size_hit"] = np.argmax(ss, 1) == sc if len(rows) else np.zeros(0, bool)
    for name, s in (("head_margin", hs), ("size_margin", ss)):
        t = np.sort(s, 1)
        out[name] = t[:, -1] - t[:, -2] if len(rows) else np.zeros(0)
    if with_iou:
        # the metric kernel decodes with the ARG-MAX bins (oracle.box_ref.iou_metrics)
        iou = np.zeros((len(rows), 2))
        ah, a_s = (np.argmax(hs, 1), np.argmax(ss, 1)) if len(rows) else (np.zeros(0, int), np.zeros(0, int))
        pa = ah * PER64 + o[ar, 3 + NB + ah] * HALF64
        pa = np.where(pa > np.pi, pa - 2 * np.pi, pa)
        so2 = 3 + 2 * NB + ns + 3 * a_s
        sel2 = o[ar[:, None], so2[:, None] + np.arange(3)[None]]
        pb = np.concatenate([ref2 + o[:, :3], sel2 * ms[a_s] + ms[a_s], pa[:, None]], 1)
        if len(rows):
            iou = box_ref.iou_pair(box_ref.boxes3d2corners(pb), cg)
        out["iou2d"], out["iou3d"] = iou[:, 0], iou[:, 1]
    return out


def census(logits, d, ns, hc_b, on_edge=None):
    """Rows (frustums for the heading regimes) per regime, from float64 quantities only."""
    a = analyse(logits, d, ns, hc_b)
    lab = d["cls_label"].reshape(-1)
    c0, c1 = logits[:, 0].astype(np.float64), logits[:, 1].astype(np.float64)
    m = c1 - c0
    c = {}
    for name, v, k in (("center", a["dist"], 3.0), ("head_res", np.abs(a["e"]), 1.0), ("size_res", a["n"], 1.0)):
        c[name + "_zero"] = int((v < 1e-6).sum())
        c[name + "_quadratic"] = int(((v >= 1e-6) & (v < k)).sum())
        c[name + "_linear"] = int((v > k).sum())
    cd, fl = a["cd"], a["d2"] < a["d1"]
    c["corner_zero"] = int((cd < 1e-5).sum())
    c["corner_quadratic"] = int(((cd >= 1e-5) & (cd < 1)).sum())
    c["corner_linear"] = int((cd > 1).sum())
    c["flipped_quadratic"] = int((fl & (cd < 1)).sum())
    c["flipped_linear"] = int((fl & (cd > 1)).sum())
    c["angle_above_pi_before_wrap"] = int((a["ang_pre"] > np.pi).sum())
    c["head_acc_hit"], c["head_acc_miss"] = int(a["head_hit"].sum()), int((~a["head_hit"]).sum())
    c["size_acc_hit"], c["size_acc_miss"] = int(a["size_hit"].sum()), int((~a["size_hit"]).sum())
    for k in range(ns):
        c["size_class_%d" % k] = int((a["sc"] == k).sum())
    for t, name in ((0, "bg"), (1, "fg"), (-1, "ignored")):
        s = lab == t
        c["cls_%s_tie" % name] = int((s & (m == 0)).sum())
        c["cls_%s_saturated_fg" % name] = int((s & (m > 15)).sum())
        c["cls_%s_saturated_bg" % name] = int((s & (m < -15)).sum())
    c["iou_at_or_above_thresh"] = int((a["iou3d"] >= THRESH).sum())
    c["iou_below_thresh"] = int((a["iou3d"] < THRESH).sum())
    fr = np.unique(a["b"])
    h = d["box3d_heading"].reshape(-1)[fr].astype(np.float64)
    f = {"heading_on_bin_edge": int(sum(edge_distance64(x) < 1e-5 for x in h)),
         "heading_pm_pi": int((np.abs(np.abs(h) - np.pi) < 1e-6).sum()), "heading_negative": int((h < 0).sum()),
         "heading_above_2pi": int((h > 2 * np.pi).sum())}
    return c, f, a


def _t(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dtype) if dtype is not None and t.dtype.is_floating_point else t


def referee(logits, d, ns, hc, dtype=torch.float64):
    """oracle.det_ref.loss_tail in `dtype` -> (losses dict of floats, (cls, head, size) accuracies, nfg, gradient rows (R, 2 + nc))."""
    nc = 3 + 2 * NB + 4 * ns
    B, L2 = d["cls_label"].shape
    lg = _t(logits[:, :2 + nc], dtype).clone().requires_grad_(True)
    cls_raw = lg[:, :2].reshape(B, L2, 2).permute(0, 2, 1)
    reg_raw = lg[:, 2:].reshape(B, L2, nc).permute(0, 2, 1)
    data = {k: _t(v, dtype) for k, v in d.items()}
    out = det_ref.loss_tail(cls_raw, reg_raw, data, nb=NB, ncls=ns, mean_size=mean_size32(ns).astype(np.float64),
                            head_bin=_t(hc))
    out["total_loss"].backward()
    lab = d["cls_label"].reshape(-1)
    keep, fg = lab != -1, lab == 1
    pred = (logits[:, 1] > logits[:, 0]).astype(np.int64)
    cls_acc = float((pred[keep] == (lab[keep] >= 1)).mean()) if keep.any() else 0.0
    o = logits[:, 2:2 + nc]
    b = np.arange(B * L2) // L2
    head_acc = float((np.argmax(o[fg, 3:3 + NB], 1) == hc[b[fg]]).mean()) if fg.any() else 0.0
    size_acc = float((np.argmax(o[fg, 3 + 2 * NB:3 + 2 * NB + ns], 1) == d["size_class"].reshape(-1)[b[fg]]).mean()) if fg.any() else 0.0
    return ({k: float(v.detach()) for k, v in out.items()}, (cls_acc, head_acc, size_acc), int(fg.sum()),
            lg.grad.detach().double().numpy())


def row_error(got, ref, nfg):
    """Worst row of max|got - ref| / max(largest |ref| of the row, ROW_FLOOR / nfg) -- over ALL rows (share left out: 0)."""
    floor = ROW_FLOOR / (nfg + 1e-14)
    err = np.abs(got - ref).max(1) / np.maximum(np.abs(ref).max(1), floor)
    assert err.shape[0] == ref.shape[0]
    return float(err.max()), int(err.argmax())


# ---------------------------------------------------------------------------------------------------------------- kernels
def _dev(d, ns):
    t = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
    t["mean_size"] = torch.from_numpy(mean_size32(ns)).cuda()
    return t


def _label_args(t):
    return (t["cls_label"], t["center_ref2"], t["box3d_center"], t["box3d_heading"], t["box3d_size"], t["size_class"],
            t["mean_size"])


def run_planar(logits, d, ns):
    from frustum_convnet_amd import loss_fused
    nc = 3 + 2 * NB + 4 * ns
    B, L2 = d["cls_label"].shape
    t = _dev(d, ns)
    lg = torch.from_numpy(logits[:, :2 + nc]).reshape(B, L2, 2 + nc).permute(0, 2, 1).contiguous().cuda()
    cls_raw = lg[:, :2].contiguous().requires_grad_(True)
    reg_raw = lg[:, 2:].contiguous().requires_grad_(True)
    losses, acc, nfg = loss_fused.det_loss_tail(cls_raw, reg_raw, *_label_args(t), NB, ns, W)
    losses["total_loss"].backward()
    g = torch.cat([cls_raw.grad, reg_raw.grad], 1).permute(0, 2, 1).reshape(B * L2, 2 + nc)
    return ({k: float(v) for k, v in losses.items()}, tuple(float(x) for x in acc), float(nfg), g.cpu().numpy())


def padded(logits, ns, fill=np.nan):
    ld = 64 if ns == 3 else 128
    out = np.full((logits.shape[0], ld), fill, dtype=np.float32)
    out[:, :logits.shape[1]] = logits
    return out


def run_rows_raw(logits_ld, d, ns, scratch=None):
    """fcn_det_loss_tail_rows2 straight through the C-ABI: the gradient buffer is pre-filled with NaN.
    -> (out16 numpy, gradient (R, ld) numpy, total)."""
    from frustum_convnet_amd import _native
    B, L2 = d["cls_label"].shape
    t = _dev(d, ns)
    lg = torch.from_numpy(logits_ld).cuda()
    out = torch.full((16,), float("nan"), dtype=torch.float32).cuda()
    total = torch.full((1,), float("nan"), dtype=torch.float32).cuda()
    dlog = torch.full(lg.shape, float("nan"), dtype=torch.float32).cuda()
    with torch.cuda.device(lg.device):
        rc = _native.lib().fcn_det_loss_tail_rows2(lg.data_ptr(), *[x.data_ptr() for x in _label_args(t)], B, L2, NB, ns,
                                                   *W, out.data_ptr(), dlog.data_ptr(),
                                                   None if scratch is None else scratch.data_ptr(), total.data_ptr(),
                                                   _native.current_stream(lg.device))
    _native.check(rc, "fcn_det_loss_tail_rows2")
    torch.cuda.synchronize()
    return out.cpu().numpy(), dlog.cpu().numpy(), float(total[0])


def run_rows_binding(logits_ld, d, ns, scratch=None):
    from frustum_convnet_amd import loss_fused
    B, L2 = d["cls_label"].shape
    t = _dev(d, ns)
    lg = torch.from_numpy(logits_ld).cuda().requires_grad_(True)
    losses, acc, nfg = loss_fused.det_loss_tail_rows(lg, B, L2, *_label_args(t), NB, ns, W, scratch=scratch)
    losses["total_loss"].backward()
    return ({k: float(v) for k, v in losses.items()}, tuple(float(x) for x in acc), float(nfg), lg.grad.cpu().numpy())


def run_metrics(metrics, logits_ld, d, ns):
    B, L2 = d["cls_label"].shape
    t = _dev(d, ns)
    out = metrics(torch.from_numpy(logits_ld).cuda(), B, L2, t["cls_label"], t["center_ref2"], t["box3d_center"],
                  t["box3d_heading"], t["box3d_size"], t["mean_size"], NB, ns, THRESH)
    metrics.join()
    torch.cuda.synchronize()
    return out.cpu().numpy()


def expected_metrics(a):
    if len(a["rows"]) == 0:
        return 0.0, 0.0, 0.0
    return float(a["iou2d"].mean()), float(a["iou3d"].mean()), float((a["iou3d"] >= THRESH).mean())


def check_losses(tag, got, ref):
    losses, acc, nfg = got
    rl, ra, rn = ref
    for k, v in rl.items():
        assert np.isfinite(losses[k]), (tag, k, losses[k])
        assert abs(losses[k] - v) <= 1e-4 * max(1.0, abs(v)), (tag, k, losses[k], v)
    for i, k in enumerate(("cls_acc", "head_acc", "size_acc")):
        assert abs(acc[i] - ra[i]) < 1e-6, (tag, k, acc[i], ra[i])
    assert int(nfg) == rn, (tag, nfg, rn)


def check_grad(tag, got, ref, nfg):
    assert np.isfinite(got).all(), tag
    assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max() + 1e-7, (tag, np.abs(got - ref).max(), np.abs(ref).max())
    worst, row = row_error(got, ref, nfg)
    assert worst <= ROW_BAR, (tag, "row", row, worst)
    return worst


def out16_as_result(out):
    names = ("total_loss", "cls_loss", "center_loss", "head_cls_loss", "head_res_loss", "size_cls_loss", "size_res_loss",
             "corners_loss")
    return ({k: float(out[i]) for i, k in enumerate(names)}, (float(out[8]), float(out[9]), float(out[10])), float(out[11]))


def assert_census(c, f, B):
    low = {k: v for k, v in c.items() if v < CENSUS_MIN}
    assert not low, ("regimes below %d rows" % CENSUS_MIN, low)
    if B >= 32:
        lowf = {k: v for k, v in f.items() if v < CENSUS_MIN_FRUSTUMS}
        assert not lowf, ("heading regimes below %d frustums" % CENSUS_MIN_FRUSTUMS, lowf)


def _seed(ns, B, L2, mode="mixed"):
    return 1000 * ns + 37 * B + L2 + 7919 * (["mixed"] + MODES).index(mode)


def _one_batch(ns, B, L2, mode):
    nc = 3 + 2 * NB + 4 * ns
    R = B * L2
    logits, d, hc, info = make_batch(ns, B, L2, _seed(ns, B, L2, mode), mode)
    c, f, a = census(logits, d, ns, hc)
    if mode == "mixed" and R >= 1000:
        assert_census(c, f, B)
    # no compared row on a kink (the rows are ALL compared)
    assert (a["head_margin"] >= 1.0).all() and (a["size_margin"] >= 1.0).all()
    m = np.abs(logits[:, 1].astype(np.float64) - logits[:, 0])
    assert ((m == 0) | (m >= 5e-4)).all()
    rl, ra, rn, rg = referee(logits, d, ns, hc)
    ref = (rl, ra, rn)
    tag = "ns%d B%d L2 %d %s" % (ns, B, L2, mode)
    worst = {}
    # planar (B, C, L2)
    pl = run_planar(logits, d, ns)
    check_losses(tag + " planar", pl[:3], ref)
    worst["planar"] = check_grad(tag + " planar", pl[3].astype(np.float64), rg, rn)
    # row-major: pad columns of the logits NaN, the gradient buffer NaN before the launch
    lp = padded(logits, ns)
    ld = lp.shape[1]
    assert ld == (64 if ns == 3 else 128)
    out, g, total = run_rows_raw(lp, d, ns)
    check_losses(tag + " rows", out16_as_result(out), ref)
    assert total == float(out[0]) and (out[12:] == 0).all()
    assert (g[:, 2 + nc:] == 0).all(), tag + ": pad columns of the gradient rows must be exactly 0"
    worst["rows"] = check_grad(tag + " rows", g[:, :2 + nc].astype(np.float64), rg, rn)
    # the same per-row arithmetic in both layouts
    assert np.array_equal(g[:, :2 + nc], pl[3]), (tag, "planar vs rows", np.abs(g[:, :2 + nc] - pl[3]).max())
    # pad columns are never read: finite junk instead of NaN changes nothing
    out_j, g_j, _ = run_rows_raw(padded(logits, ns, fill=1e30), d, ns)
    assert np.array_equal(g_j, g)
    # with the persistent scratch: same gradient, scalars summed in workgroup order
    from frustum_convnet_amd import loss_fused
    scratch = loss_fused.loss_scratch(B, L2, "cuda")
    out_s, g_s, total_s = run_rows_raw(lp, d, ns, scratch)
    check_losses(tag + " rows+scratch", out16_as_result(out_s), ref)
    assert np.array_equal(g_s, g) and total_s == float(out_s[0])
    assert int(scratch.cpu().view(torch.int32)[0]) == 0, "arrival ticket not reset"
    out_s2, g_s2, _ = run_rows_raw(lp, d, ns, scratch)
    assert np.array_equal(out_s2, out_s) and np.array_equal(g_s2, g_s)
    # the autograd binding hands the same numbers through
    bl = run_rows_binding(lp, d, ns, scratch)
    assert np.array_equal(bl[3], g)
    assert bl[0]["total_loss"] == float(out_s[0]) and bl[2] == float(out_s[11])
    # IoU metrics on the same batch
    from frustum_convnet_amd.loss_fused import IouMetrics
    got = run_metrics(IouMetrics(), lp, d, ns)
    e2, e3, et = expected_metrics(a)
    e2o, e3o, eto = box_ref.iou_metrics(
        logits[:, 2:], d["center_ref2"].transpose(0, 2, 1).reshape(R, 3), [(int(r), int(r // L2)) for r in a["rows"]],
        d["box3d_center"], d["box3d_heading"].reshape(-1), d["box3d_size"], mean_size32(ns), nb=NB, ns=ns, thresh=THRESH)
    assert abs(e2 - e2o) < 1e-12 and abs(e3 - e3o) < 1e-12 and et == eto
    assert abs(got[0] - e2) < 1e-4 and abs(got[1] - e3) < 1e-4 and abs(got[2] - et) < 1e-6, (tag, got, (e2, e3, et))
    assert int(got[3]) == rn
    print("%s: nfg %d redrawn %d edge values moved %d | worst per-row gradient error planar %.2e rows %.2e (bar %.1e) | "
          "IoU_2D %.4f IoU_3D %.4f IoU>=%.1f %.4f" % (tag, rn, info["redrawn"], info["edge_moved"], worst["planar"],
                                                      worst["rows"], ROW_BAR, got[0], got[1], THRESH, got[2]))
    if mode == "mixed" and R >= 1000:
        print("  census rows:", c)
        print("  census frustums:", f)
    return c


@pytest.mark.parametrize("ns", [3, 10])
@pytest.mark.parametrize("B,L2", SHAPES)
def test_loss_tail_regimes(B, L2, ns):
    _one_batch(ns, B, L2, "mixed")


@pytest.mark.parametrize("ns", [3, 10])
@pytest.mark.parametrize("mode", MODES)
def test_loss_tail_label_extremes(mode, ns):
    """nfg = 0 (every foreground mean 0, gradients finite), nfg = R, every row ignored (nkeep = 0), and the only
    foreground row in the LAST row of an odd R (the label the 16-byte count loop leaves to thread 0)."""
    B, L2 = (5, 13) if mode in ("lastfg", "nfg0") else (2, 64)
    c = _one_batch(ns, B, L2, mode)
    if mode == "allfg":
        assert c["head_acc_hit"] + c["head_acc_miss"] == B * L2


@pytest.mark.parametrize("ns", [3, 10])
def test_scratch_is_ready_for_the_next_launch(ns):
    """Three launches with different inputs (different R, so different workgroup counts) on ONE scratch buffer equal three
    launches on fresh buffers, bit for bit."""
    from frustum_convnet_amd import loss_fused
    shapes = [(7, 9), (3, 43), (5, 13)]
    scratch = loss_fused.loss_scratch(3, 43, "cuda")
    for B, L2 in shapes:
        logits, d, hc, _ = make_batch(ns, B, L2, _seed(ns, B, L2) + 1)
        lp = padded(logits, ns)
        o1, g1, _ = run_rows_raw(lp, d, ns, scratch)
        o2, g2, _ = run_rows_raw(lp, d, ns, loss_fused.loss_scratch(B, L2, "cuda"))
        assert np.array_equal(o1, o2) and np.array_equal(g1, g2), (B, L2)
        check_losses("scratch %dx%d" % (B, L2), out16_as_result(o1), referee(logits, d, ns, hc)[:3])


@pytest.mark.parametrize("ns", [3, 10])
def test_iou_metrics_scratch_resets_between_launches(ns):
    """Launches with different nfg (one of them 0) through ONE IouMetrics object: the kernel's sums start from zero."""
    from frustum_convnet_amd.loss_fused import IouMetrics
    met = IouMetrics()
    for B, L2, mode in (3, 43, "mixed"), (5, 13, "nfg0"), (7, 9, "mixed"), (2, 64, "allfg"):
        logits, d, hc, _ = make_batch(ns, B, L2, _seed(ns, B, L2, mode) + 2, mode)
        a = analyse(logits, d, ns, hc)
        got = run_metrics(met, padded(logits, ns), d, ns)
        e2, e3, et = expected_metrics(a)
        assert abs(got[0] - e2) < 1e-4 and abs(got[1] - e3) < 1e-4 and abs(got[2] - et) < 1e-6, (mode, got, (e2, e3, et))
        assert int(got[3]) == len(a["rows"])
        if mode == "mixed":
            assert 0 < et < 1            # both sides of the threshold are populated


def test_generator_terminates_and_float32_oracle_error():
    """Oracle only (no kernel): the generator terminates for every shape with every regime populated where the census is
    asserted, and the float32 evaluation of the oracle misses the float64 one by the number ROW_BAR is derived from."""
    worst = 0.0
    for ns in (3, 10):
        for B, L2 in SHAPES:
            logits, d, hc, info = make_batch(ns, B, L2, _seed(ns, B, L2))
            if B * L2 >= 1000:
                c, f, _ = census(logits, d, ns, hc)
                assert_census(c, f, B)
            r64, r32 = referee(logits, d, ns, hc), referee(logits, d, ns, hc, torch.float32)
            e, row = row_error(r32[3], r64[3], r64[2])
            worst = max(worst, e)
            for k, v in r64[0].items():
                assert abs(r32[0][k] - v) <= 1e-4 * max(1.0, abs(v)), (ns, B, L2, k)
    print("float32 oracle vs float64 oracle: worst per-row gradient error %.3e -> ROW_BAR %.1e" % (worst, ROW_BAR))
    assert 4 * worst <= ROW_BAR          # the bar stays tied to the measurement it came from


def test_fixture_census_is_printed():
    """The same census on the four small golden fixtures (their recorded train logits): printed, not asserted -- the
    evidence for what the fixtures do and do not reach (EXPERIMENTS.md)."""
    for case in ("car_b4_n512", "people_b2_n512", "refine_b4_n512", "sunrgbd_b4_n1024"):
        g = load_golden(case)
        dn = golden_inputs(g)
        cls, reg = g["cls_train"], g["reg_train"]
        B, nc, L2 = reg.shape
        ns = (nc - 3 - 2 * NB) // 4
        logits = np.concatenate([cls, reg], 1).transpose(0, 2, 1).reshape(B * L2, 2 + nc).astype(np.float32)
        d = {k: np.asarray(dn[k]) for k in ("cls_label", "center_ref2", "box3d_center", "box3d_heading", "box3d_size",
                                            "size_class")}
        d["box3d_heading"] = d["box3d_heading"].reshape(B, 1).astype(np.float32)
        d["size_class"] = d["size_class"].reshape(B, 1).astype(np.int64)
        hc = np.array([head_bin32(h)[0] for h in d["box3d_heading"].reshape(-1)], dtype=np.int64)
        c, f, a = census(logits, d, ns, hc)
        print(case, "R", B * L2, "nfg", len(a["rows"]), {k: v for k, v in c.items() if not k.startswith("size_class")}, f)
