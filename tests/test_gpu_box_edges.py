"""-m gpu: the rotated-box kernels of csrc/box_iou.hip (iou_pair_kernel, decode_kernel, nms_kernel) at the shapes and inputs
the golden fixtures do not reach: box pairs with coincident / collinear edges, extreme aspect ratios and sizes, at depths of
5 to 80 m; decode with more positions than threads, arg-max ties and every selection branch; NMS with up to 4096 (and 4097)
candidates, every rows_per_unit regime, equal scores and duplicate boxes.  Referees: oracle.box_ref in float64 on the SAME
float32 inputs the kernel receives (and closed forms for the box families, checked on the float64 oracle)."""
import numpy as np
import pytest
import torch

from oracle import box_ref, det_ref

pytestmark = pytest.mark.gpu

DEPTHS = ((0.0, 5.0), (-12.0, 20.0), (25.0, 40.0), (-40.0, 80.0))          # (x, z) of the pair's centre
IOU_BAR = 5e-5                                                            # the suite's bar for iou_pair (test_gpu_box.py)


# ----------------------------------------------------------------------------------------------------- box pair families
def _rot(dx, dz, ry):
    """offset (dx along the box's length axis, dz along its width axis) in world x-z for heading ry (boxes3d2corners)."""
    return np.cos(ry) * dx + np.sin(ry) * dz, -np.sin(ry) * dx + np.cos(ry) * dz


def iou_families():
    """-> list of (family, box a (7), box b (7), (iou2d, iou3d) closed form or None), centred near the origin."""
    out = []
    box = lambda x, y, z, l, w, h, r: np.array([x, y, z, l, w, h, r], dtype=np.float64)
    for l, w, h, r in ((3.9, 1.6, 1.5, 0.0), (3.9, 1.6, 1.5, 0.7), (0.8, 0.6, 1.8, -2.3), (1.0, 1.0, 1.0, np.pi / 4)):
        a = box(0, 1, 0, l, w, h, r)
        out.append(("identical", a, a.copy(), (1.0, 1.0)))
        m = min(l, w)
        i90 = m * m / (2 * l * w - m * m)
        out.append(("turned_90", a, box(0, 1, 0, l, w, h, r + np.pi / 2), (i90, i90)))
        out.append(("turned_180", a, box(0, 1, 0, l, w, h, r + np.pi), (1.0, 1.0)))
        # sharing one full edge, half an edge, one corner: nothing but the boundary in common
        for name, dx, dz in (("full_edge", l, 0.0), ("full_edge_w", 0.0, w), ("half_edge", l, w / 2), ("one_corner", l, w)):
            ox, oz = _rot(dx, dz, r)
            out.append((name, a, box(ox, 1, oz, l, w, h, r), (0.0, 0.0)))
        # a quarter-size box inside, two of its edges on a's edges
        ox, oz = _rot(l / 4, w / 4, r)
        out.append(("contained_shared_edge", a, box(ox, 1, oz, l / 2, w / 2, h, r), (0.25, 0.25)))
        # y extents that only touch / overlap by half
        out.append(("y_touch", a, box(0, 1 + h, 0, l, w, h, r), (1.0, 0.0)))
        out.append(("y_half", a, box(0, 1 + h / 2, 0, l, w, h, r), (1.0, 1.0 / 3.0)))
        # heading differences of 1e-4 rad
        out.append(("heading_1e-4", a, box(0, 1, 0, l, w, h, r + 1e-4), None))
        out.append(("heading_-1e-4_shift", a, box(0.01, 1, -0.02, l, w, h, r - 1e-4), None))
    # a 45 degree square inside / across an axis-aligned square
    for s, S in ((1.0, 2.0), (1.0, np.sqrt(2.0)), (2.0, 2.4), (3.0, 3.5)):
        D = s / np.sqrt(2.0)
        inter = s * s if S / 2 >= D - 1e-12 else s * s - 4 * (D - S / 2) ** 2
        i2 = inter / (s * s + S * S - inter)
        out.append(("square_45", box(0, 1, 0, s, s, 1.5, np.pi / 4), box(0, 1, 0, S, S, 1.5, 0.0), (i2, i2)))
    # long thin boxes (40 : 1) crossing at their centres: the intersection is a rhombus of area w^2 / sin(theta)
    for L, w, th in ((40.0, 1.0, np.pi / 2), (40.0, 1.0, 0.3), (8.0, 0.2, 1.1), (20.0, 0.5, 2.5)):
        inter = w * w / abs(np.sin(th))
        i2 = inter / (2 * L * w - inter)
        out.append(("thin_crossing", box(0, 1, 0, L, w, 1.5, 0.2), box(0, 1, 0, L, w, 1.5, 0.2 + th), (i2, i2)))
    # sizes from 1e-2 m to 50 m: the same box moved by half its length along its own axis -> 1 / 3
    for s in (1e-2, 0.1, 1.0, 10.0, 50.0):
        for r in (0.0, 0.9):
            ox, oz = _rot(s, 0.0, r)
            out.append(("size_%g" % s, box(0, 1, 0, 2 * s, s, s, r), box(ox, 1, oz, 2 * s, s, s, r), (1.0 / 3.0, 1.0 / 3.0)))
    return out


def iou_family_arrays(x, z):
    """The families moved to (x, z): float32 corner arrays as the kernel receives them, the float64 oracle ON those float32
    corners, the closed forms (NaN where there is none) and the names."""
    fam = iou_families()
    a = np.array([f[1] for f in fam]); b = np.array([f[2] for f in fam])
    a[:, 0] += x; a[:, 2] += z; b[:, 0] += x; b[:, 2] += z
    ca, cb = box_ref.boxes3d2corners(a).astype(np.float32), box_ref.boxes3d2corners(b).astype(np.float32)
    closed = np.array([f[3] if f[3] is not None else (np.nan, np.nan) for f in fam], dtype=np.float64)
    return a, b, ca, cb, box_ref.iou_pair(ca, cb), closed, [f[0] for f in fam]


def test_iou_family_closed_forms_hold_for_the_oracle():
    """The float64 oracle on the exact (float64) boxes reproduces every closed form: the families are what they claim to be."""
    fam = iou_families()
    a = np.array([f[1] for f in fam]); b = np.array([f[2] for f in fam])
    got = box_ref.iou_pair(box_ref.boxes3d2corners(a), box_ref.boxes3d2corners(b))
    for i, f in enumerate(fam):
        if f[3] is not None:
            assert abs(got[i, 0] - f[3][0]) < 1e-9 and abs(got[i, 1] - f[3][1]) < 1e-9, (f[0], got[i], f[3])


def test_iou_pair_families_at_depth():
    from frustum_convnet_amd import detect
    worst_all = 0.0
    for x, z in DEPTHS:
        a, b, ca, cb, exp, closed, names = iou_family_arrays(x, z)
        got = detect.box3d_iou_pair(torch.from_numpy(ca).cuda(), torch.from_numpy(cb).cuda()).cpu().numpy().astype(np.float64)
        err = np.abs(got - exp).max(1)
        i = int(err.argmax())
        print("iou_pair families at x %+5.0f m z %3.0f m: worst |kernel - float64 oracle| %.2e (%s), %d pairs"
              % (x, z, err[i], names[i], len(names)))
        worst_all = max(worst_all, float(err[i]))
        assert np.isfinite(got).all()
        assert err[i] < IOU_BAR, (x, z, names[i], got[i], exp[i])
    assert worst_all < IOU_BAR


# ------------------------------------------------------------------------------------------------------------------ decode
NB = 12


def _decode_expect(logits, ref2, mean_size, rot, refc, rgb, ns, method, b, L2):
    """One frustum through oracle.box_ref.decode_detections, as test_gpu_box.test_decode_matches_oracle does."""
    nc = 3 + 2 * NB + 4 * ns
    rows = logits[b * L2:(b + 1) * L2].astype(np.float64)
    o = rows[:, 2:2 + nc]
    per = 2 * np.pi / NB
    ah = np.argmax(o[:, 3:3 + NB], 1); a_s = np.argmax(o[:, 3 + 2 * NB:3 + 2 * NB + ns], 1)
    ang = ah * per + o[np.arange(L2), 3 + NB + ah] * per / 2
    ang = np.where(ang > np.pi, ang - 2 * np.pi, ang)
    sr = np.stack([o[np.arange(L2), 3 + 2 * NB + ns + 3 * a_s + j] for j in range(3)], 1)
    size = sr * mean_size[a_s] + mean_size[a_s]
    ctr = o[:, :3] + ref2[b].T
    # the oracle decides on float32 probabilities like the reference (torch softmax in fp32)
    p32 = torch.softmax(torch.from_numpy(logits[b * L2:(b + 1) * L2, :2].copy()), -1).numpy()
    return box_ref.decode_detections(p32.astype(np.float64), ctr, ang, size, float(rot[b]),
                                     np.zeros(3) if refc is None else refc[b].astype(np.float64),
                                     1.0 if rgb is None else float(rgb[b]), method), ang


def _decode_batch(rng, B, L2, ns, ld):
    nc = 3 + 2 * NB + 4 * ns
    logits = np.zeros((B * L2, ld), dtype=np.float32)
    logits[:, :2 + nc] = rng.normal(0, 1.0, (B * L2, 2 + nc)).astype(np.float32)
    # class margins clipped to +-4 and one clear best row per frustum: the float32 softmax of the oracle and the kernel's
    # own expf formula round differently, so the arg-max must not hang on the last bit (ties are placed on purpose below)
    logits[:, 1] = logits[:, 0] + np.clip(rng.normal(0, 1.4, B * L2), -4, 4).astype(np.float32)
    best = rng.integers(0, L2, B)
    for b in range(B):
        logits[b * L2 + best[b], 1] = logits[b * L2 + best[b], 0] + np.float32(6.0)
    logits[:, 2 + 3 + 2 * NB + ns:2 + nc] *= 0.3                            # size residuals: mostly positive sizes
    ref2 = rng.normal(0, 1, (B, 3, L2)).astype(np.float32) + np.array([0, 1, 20], dtype=np.float32)[None, :, None]
    return logits, ref2, best


def _run_decode(logits, ref2, mean_size, rot, refc, rgb, ns, B, L2, tag):
    from frustum_convnet_amd import detect
    t = lambda x: None if x is None else torch.from_numpy(x).cuda()
    worst_ang = [np.inf, -np.inf]
    for method in ("nms", "top"):
        dets, valid = detect.decode_detections(t(logits), t(ref2), t(mean_size), t(rot), t(refc), t(rgb), NB, ns, method)
        dets, valid = dets.cpu().numpy(), valid.cpu().numpy()
        assert set(np.unique(valid)) <= {0, 1}
        for b in range(B):
            (exp_rows, idx), ang = _decode_expect(logits, ref2, mean_size, rot, refc, rgb, ns, method, b, L2)
            got_idx = np.nonzero(valid[b * L2:(b + 1) * L2])[0].tolist()
            assert got_idx == idx, (tag, method, b, got_idx[:8], idx[:8])
            if idx:
                assert np.abs(dets[b * L2 + np.array(idx)] - exp_rows).max() < 2e-4, (tag, method, b)
                worst_ang = [min(worst_ang[0], ang[idx].min()), max(worst_ang[1], ang[idx].max())]
    return worst_ang


@pytest.mark.parametrize("ns,ld", [(3, 64), (10, 128)])
@pytest.mark.parametrize("B,L2", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 700)])
def test_decode_shapes(B, L2, ns, ld):
    """L2 below / at / above the 256 threads of a workgroup (later trips of both loops), one frustum, one position."""
    rng = np.random.default_rng(100 * L2 + ns)
    logits, ref2, _ = _decode_batch(rng, B, L2, ns, ld)
    mean_size = (det_ref.MEAN_SIZE if ns == 3 else det_ref.MEAN_SIZE_SUNRGBD).astype(np.float32)
    rot = np.array([-4.0, 0.4, 3.5][:B], dtype=np.float32)                 # both signs, beyond +-pi
    refc = rng.normal(0, 1, (B, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, B).astype(np.float32)
    _run_decode(logits, ref2, mean_size, rot, refc, rgb, ns, B, L2, "shapes")
    _run_decode(logits, ref2, mean_size, rot, None, None, ns, B, L2, "shapes, no ref_center / rgb_prob")


@pytest.mark.parametrize("ns,ld", [(3, 64), (10, 128)])
def test_decode_ties_and_selection_branches(ns, ld):
    """L2 = 700 (three trips).  Frustum 0: the best p_fg is shared by BIT-IDENTICAL foreground rows at 3, 259, 515 (different
    threads, different trips) -> 'top' takes the first; 1: the same rows but no foreground anywhere -> both methods take the
    first; 2: p_fg == 1.0f at 600, 10 and 300 from DIFFERENT saturated logits -> the first (10); 3: every position
    foreground; 4: no foreground and the arg-max row decodes to a zero-size box -> nothing valid; 5: decoded angles just
    below and just above pi (the wrap) in the selected rows."""
    rng = np.random.default_rng(11 + ns)
    B, L2 = 6, 700
    nc = 3 + 2 * NB + 4 * ns
    logits, ref2, best = _decode_batch(rng, B, L2, ns, ld)
    R = lambda b, l: b * L2 + l
    for b in (0, 1):
        logits[R(b, 0):R(b + 1, 0), 1] = logits[R(b, 0):R(b + 1, 0), 0] - np.abs(logits[R(b, 0):R(b + 1, 0), 1] - logits[R(b, 0):R(b + 1, 0), 0]) - 1
        row = logits[R(b, 3)].copy()
        row[1] = row[0] + (np.float32(2.5) if b == 0 else np.float32(-0.25))     # frustum 1: the best p_fg is still background
        for l in (3, 259, 515):
            logits[R(b, l)] = row
    logits[R(2, 0):R(3, 0), 1] = logits[R(2, 0):R(3, 0), 0] - 1
    for l, m in ((600, 40.0), (10, 60.0), (300, 50.0)):
        logits[R(2, l), 1] = logits[R(2, l), 0] + np.float32(m)
    logits[R(3, 0):R(4, 0), 1] = logits[R(3, 0):R(4, 0), 0] + np.abs(logits[R(3, 0):R(4, 0), 1] - logits[R(3, 0):R(4, 0), 0]) + 0.5
    logits[R(4, 0):R(5, 0), 1] = logits[R(4, 0):R(5, 0), 0] - np.abs(logits[R(4, 0):R(5, 0), 1] - logits[R(4, 0):R(5, 0), 0]) - 1
    logits[R(4, 333), 1] = logits[R(4, 333), 0] - np.float32(0.125)
    logits[R(4, 333), 2 + 3 + 2 * NB + ns:2 + nc] = -1.0
    for l, res in ((5, -0.01), (400, 0.01), (699, 0.5)):                  # bin 6 is centred on pi
        logits[R(5, l), 1] = logits[R(5, l), 0] + np.float32(1.0)
        logits[R(5, l), 2 + 3:2 + 3 + NB] = 0
        logits[R(5, l), 2 + 3 + 6] = 3.0
        logits[R(5, l), 2 + 3 + NB + 6] = res
    mean_size = (det_ref.MEAN_SIZE if ns == 3 else det_ref.MEAN_SIZE_SUNRGBD).astype(np.float32)
    rot = np.array([-4.0, -0.3, 0.4, 3.5, 0.0, -3.3], dtype=np.float32)
    refc = rng.normal(0, 1, (B, 3)).astype(np.float32)
    rgb = rng.uniform(0, 1, B).astype(np.float32)
    # the inputs are what the docstring says (float32 softmax, as the oracle decides)
    p1 = torch.softmax(torch.from_numpy(logits[:, :2].copy()), -1).numpy()[:, 1].reshape(B, L2)
    assert p1[0].argmax() == 3 and p1[0, 3] == p1[0, 259] == p1[0, 515] == p1[0].max() and p1[0, 3] > 0.5
    assert p1[1].argmax() == 3 and p1[1, 3] == p1[1, 515] and p1[1].max() < 0.5
    assert p1[2, 600] == p1[2, 10] == p1[2, 300] == 1.0 and (p1[2] == 1.0).sum() == 3
    assert (p1[3] > 0.5).all() and (p1[4] < 0.5).all() and p1[4].argmax() == 333
    ang = _run_decode(logits, ref2, mean_size, rot, refc, rgb, ns, B, L2, "ties")
    _run_decode(logits, ref2, mean_size, rot, None, None, ns, B, L2, "ties, no ref_center / rgb_prob")
    assert ang[0] < -3.1 and ang[1] > 3.1                                 # both sides of the wrap were decoded


# --------------------------------------------------------------------------------------------------------------------- NMS
NMS_IOU_MARGIN = 1e-3        # an examined pair's float64 iou3d this close to thresh: float32 may decide differently -> re-draw
NMS_GAP_MARGIN = 1e-4        # a deciding hull gap this close to 0 (coordinates up to 85 m: float32 ulp 8e-6) -> re-draw


class Ambiguous(Exception):
    pass


def fast_nms(dets, thresh, top_k):
    """oracle.box_ref.cube_nms (stable order: later row first among equal scores) with the axis-aligned hull test of
    box_ref.py (`standup_iou <= 0`) pre-computed for all pairs by numpy, so that only overlapping pairs are clipped: the same
    decisions, in seconds for 4096 candidates.  Raises Ambiguous when a decision sits within the margins above."""
    dets = np.asarray(dets, dtype=np.float64)
    n = len(dets)
    if n == 0:
        return []
    order = dets[:, 7].argsort(kind="stable")[::-1]
    corners = box_ref.boxes3d2corners(dets[:, :7])
    lo, hi = corners.min(1), corners.max(1)
    gap = np.full((n, n), np.inf)
    for q in range(3):
        gap = np.minimum(gap, np.minimum(hi[:, None, q], hi[None, :, q]) - np.maximum(lo[:, None, q], lo[None, :, q]))
    np.fill_diagonal(gap, -np.inf)
    if (np.abs(gap) < NMS_GAP_MARGIN).any():
        raise Ambiguous("hull gap")
    rank = np.empty(n, dtype=np.int64); rank[order] = np.arange(n)
    suppressed = np.zeros(n, dtype=bool)
    keep = []
    for i in order:
        if suppressed[i]:
            continue
        keep.append(int(i))
        for j in np.nonzero((gap[i] > 0) & ~suppressed & (rank > rank[i]))[0]:
            v = box_ref.iou_pair(corners[i:i + 1], corners[j:j + 1])[0, 1]
            if abs(v - thresh) < NMS_IOU_MARGIN:
                raise Ambiguous("iou")
            if v >= thresh:
                suppressed[j] = True
    return keep[:top_k]


def cluster_dets(rng, n, scores="distinct"):
    """n car-sized boxes in clusters of 3 on a grid of 9 x 9 cells x 17 levels (9 m apart in x and z, 4 m in y: x in +-40 m,
    z 8..84 m).  Inside a cluster a box is the cluster's box moved along its width axis: a near-duplicate (3-D IoU ~0.9),
    half overlapping (~0.45) or apart (IoU 0, but the axis-aligned hulls of the turned boxes still overlap) -- decisions on
    every side of the hull test and of thresh, few of them near either.
    scores: 'distinct', 'blocks' (runs of exactly equal scores among distinct ones), 'equal' (all equal)."""
    ncl = (n + 2) // 3
    ncell = 9 * 9 * 17
    cell = rng.permutation(ncell)[:ncl] if ncl <= ncell else rng.integers(0, ncell, ncl)
    cx, cz, cy = (cell % 9) * 9.0 - 36.0, ((cell // 9) % 9) * 9.0 + 10.0, (cell // 81) * 4.0
    k = np.arange(n) // 3
    ry = rng.uniform(-np.pi, np.pi, ncl + 1)[k]
    kind = rng.integers(0, 3, n)
    off = np.where(kind == 0, rng.normal(0, 0.03, n), np.where(kind == 1, rng.uniform(0.55, 0.7, n), rng.uniform(2.5, 2.7, n)))
    d = np.zeros((n, 8), dtype=np.float64)
    d[:, 0] = cx[k] + np.sin(ry) * off + rng.normal(0, 0.02, n)
    d[:, 1] = cy[k] + rng.normal(0, 0.03, n)
    d[:, 2] = cz[k] + np.cos(ry) * off + rng.normal(0, 0.02, n)
    d[:, 3:6] = np.array([3.9, 1.6, 1.5]) * rng.uniform(0.97, 1.03, (n, 3))
    d[:, 6] = ry + rng.normal(0, 0.02, n)
    if scores == "distinct":
        d[:, 7] = rng.permutation(n) / max(n, 1) + 0.5
    elif scores == "equal":
        d[:, 7] = 1.75
    else:
        d[:, 7] = np.round(rng.uniform(0, 1, n) * 8) / 8 + 1.0          # nine values: long runs of equal float32 scores
        sel = rng.random(n) < 0.3
        d[sel, 7] = rng.uniform(1, 2, int(sel.sum()))
    d = d[rng.permutation(n)]
    return d.astype(np.float32)


def drawn(make, thresh, top_k=300):
    """Draw candidate sets until none of the reference's decisions is ambiguous; -> (dets float32, keep, number of re-draws)."""
    for attempt in range(50):
        d = make(attempt)
        try:
            return d, fast_nms(d, thresh, top_k), attempt
        except Ambiguous:
            continue
    raise AssertionError("no unambiguous candidate set in 50 draws")


def assemble(groups, rows_per_unit, rng, with_valid=True, extra_groups=0):
    """groups: list of (n_g, 8) arrays -> dets (U * rows_per_unit, 8), valid (or None: every unit full), unit_group (U,),
    rows[g] = global row of each candidate of group g.  Units of the groups are interleaved; the unused slots of a unit are
    spread over it and hold NaN (the kernel must never read an invalid row)."""
    units = []                       # (group, candidate indices of this unit)
    for g, d in enumerate(groups):
        n = len(d)
        nu = max(1, (n + rows_per_unit - 1) // rows_per_unit)
        cut = np.linspace(0, n, nu + 1).astype(int) if with_valid else np.arange(0, n + 1, rows_per_unit)
        if not with_valid:
            assert n % rows_per_unit == 0 and n > 0
        for u in range(len(cut) - 1):
            units.append((g, np.arange(cut[u], cut[u + 1])))
    by_g = {}
    for u in units:
        by_g.setdefault(u[0], []).append(u)
    order = []                       # round-robin over the groups: units of several groups interleaved, each group's in order
    while any(by_g.values()):
        for g in sorted(by_g):
            if by_g[g]:
                order.append(by_g[g].pop(0))
    U = len(order)
    dets = np.full((U * rows_per_unit, 8), np.nan, dtype=np.float32)
    valid = np.zeros(U * rows_per_unit, dtype=np.int32)
    ug = np.zeros(U, dtype=np.int32)
    rows = [np.zeros(len(d), dtype=np.int64) for d in groups]
    for u, (g, idx) in enumerate(order):
        ug[u] = g
        slots = np.sort(rng.permutation(rows_per_unit)[:len(idx)]) if with_valid else np.arange(rows_per_unit)
        dets[u * rows_per_unit + slots] = groups[g][idx]
        valid[u * rows_per_unit + slots] = 1
        rows[g][idx] = u * rows_per_unit + slots
    return dets, (valid if with_valid else None), ug, rows


def run_nms(dets, valid, ug, rows_per_unit, G, thresh, top_k=300):
    from frustum_convnet_amd import detect
    keep, cnt = detect.rotate_nms_3d(torch.from_numpy(dets).cuda(), None if valid is None else torch.from_numpy(valid).cuda(),
                                     torch.from_numpy(ug), rows_per_unit, G, thresh, top_k=top_k)
    return keep.cpu().numpy(), cnt.cpu().numpy()


def check_groups(tag, keep, cnt, rows, expect, top_k):
    for g, e in enumerate(expect):
        if e is None:
            assert cnt[g] == -1, (tag, g, cnt[g])
            continue
        exp = [int(rows[g][k]) for k in e][:top_k]
        assert int(cnt[g]) == len(exp), (tag, g, int(cnt[g]), len(exp))
        got = keep[g, :len(exp)].tolist()
        assert got == exp, (tag, g, [(i, a, b) for i, (a, b) in enumerate(zip(got, exp)) if a != b][:5])


NMS_LAUNCHES = {
    # name: (rows_per_unit, [(n, scores)], with_valid, thresh, top_k)
    "small_r16": (16, [(0, "distinct"), (1, "distinct"), (2, "equal"), (255, "blocks"), (256, "distinct"), (257, "blocks"),
                       (40, "equal")], True, 0.1, 300),
    "r1_novalid": (1, [(37, "blocks"), (1, "distinct"), (130, "equal")], False, 0.1, 300),
    "r300_n1000": (300, [(1000, "blocks"), (300, "distinct")], True, 0.1, 5000),
    "r300_novalid": (300, [(600, "blocks")], False, 0.25, 5000),
    "r1024_n4096_4097": (1024, [(4096, "blocks"), (4097, "distinct"), (257, "blocks")], True, 0.1, 5000),
    "r1024_novalid_4096": (1024, [(4096, "distinct")], False, 0.1, 5000),
    "topk_1": (16, [(60, "blocks")], True, 0.1, 1),
    "topk_below_kept": (16, [(257, "blocks")], True, 0.1, 7),
}


@pytest.mark.parametrize("name", list(NMS_LAUNCHES))
def test_nms_sizes_ties_and_units(name):
    """Keep lists must match the stable-order reference EXACTLY, group by group; a group above 4096 candidates answers -1
    while the other groups of the launch are still right; a group id that no unit carries and a group without a valid row
    keep nothing.  The share of skipped candidate sets is 0: an ambiguous draw is replaced, never dropped."""
    rpu, specs, with_valid, thresh, top_k = NMS_LAUNCHES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    groups, expect, redraws = [], [], 0
    for gi, (n, scores) in enumerate(specs):
        if n > 4096:                         # no reference needed: the kernel must refuse the group
            groups.append(cluster_dets(np.random.default_rng(gi + 1), n, scores)); expect.append(None)
            continue
        d, keep, att = drawn(lambda attempt: cluster_dets(np.random.default_rng([sum(map(ord, name)), gi, attempt]), n, scores),
                             thresh, 1 << 30)          # the whole keep list: check_groups cuts it at top_k
        groups.append(d); expect.append(keep); redraws += att
    dets, valid, ug, rows = assemble(groups, rpu, rng, with_valid)
    G = len(groups) + 1                      # the last group id is carried by no unit
    expect.append([]); rows.append(np.zeros(0, dtype=np.int64))
    if with_valid:
        assert (valid == 0).any() or all(len(g) % rpu == 0 for g in groups)
    keep, cnt = run_nms(dets, valid, ug, rpu, G, thresh, top_k)
    check_groups(name, keep, cnt, rows, expect, top_k)
    kept = [len(e) for e in expect if e is not None]
    if name == "topk_below_kept":
        assert kept[0] > top_k
    print("nms %s: groups n = %s kept %s (top_k %d), candidate sets re-drawn %d, skipped 0" %
          (name, [len(g) for g in groups], kept, top_k, redraws))


def test_nms_duplicates_and_tie_order():
    """Exact duplicates of a box: with equal scores the LATER row is examined first and suppresses the earlier ones; with
    distinct scores the best one survives.  All-equal scores on boxes that do not overlap: the keep list is the rows in
    DESCENDING row order (np.argsort(kind='stable')[::-1])."""
    rng = np.random.default_rng(5)
    base = cluster_dets(rng, 30, "distinct").astype(np.float64)
    base[:, 0] = np.arange(30) * 7.0 - 100; base[:, 1] = 0; base[:, 2] = 30        # apart: nothing suppresses anything
    dup = base[[4, 4, 4, 9, 9, 17]].copy()
    dup[:3, 7] = 1.5                         # three copies of box 4, equal scores
    dup[3:5, 7] = (1.2, 1.9)                 # two copies of box 9, the later one better
    dup[5, 7] = base[17, 7] - 0.25           # a worse copy of box 17
    base[4, 7] = 1.5
    d = np.concatenate([base, dup]).astype(np.float32)
    exp = fast_nms(d, 0.1, 300)
    assert exp == box_ref.cube_nms(d, 0.1)
    assert 32 in exp and 4 not in exp and 30 not in exp and 31 not in exp          # the last copy of box 4 wins
    assert 34 in exp and 9 not in exp and 17 in exp and 35 not in exp
    eq = base.copy(); eq[:, 7] = 2.0
    assert fast_nms(eq.astype(np.float32), 0.1, 300) == list(range(29, -1, -1))
    for rpu in (1, 16):
        groups = [d, eq.astype(np.float32)]
        dets, valid, ug, rows = assemble(groups, rpu, rng, with_valid=rpu > 1)
        if rpu == 1:
            valid = None
        keep, cnt = run_nms(dets, valid, ug, rpu, 2, 0.1)
        check_groups("duplicates rpu %d" % rpu, keep, cnt, rows, [exp, list(range(29, -1, -1))], 300)


def test_fast_nms_equals_cube_nms():
    """The pre-computed hull matrix changes nothing: same keep lists as oracle.box_ref.cube_nms (oracle only, no kernel)."""
    for n, scores in ((1, "distinct"), (2, "equal"), (120, "blocks"), (255, "blocks"), (90, "equal")):
        d, keep, _ = drawn(lambda attempt: cluster_dets(np.random.default_rng([n, attempt]), n, scores), 0.1)
        assert keep == box_ref.cube_nms(d, 0.1), (n, scores)
        assert len(keep) < n or n <= 2
