"""TEST INFRASTRUCTURE: named edge cases of the batch-builder kernels (csrc/inputs.hip: prepare_inputs_kernel behind
fcn_prepare_inputs / _infer / _sunrgbd, prepare_inputs_refine_kernel behind fcn_prepare_inputs_refine) OFF the three recorded
fixtures: records, draws and the expected batch of oracle/inputs_ref.py for every case.  Pure numpy; nothing here touches the
code under test.  tests/test_gpu_inputs_edges.py runs the cases on the device (and tests/test_emu_gpu_subset.py on the host
emulation), tests/test_inputs_cases.py checks the generators themselves without a GPU.

A case is a dict: kind ("refine" | "kitti" | "sunrgbd"), rec (the fixtures' packed layout, what the oracle takes), npoints,
strides, max_depth (first stage), flip / shift (the builder's switches), want (the oracle's collated batch; refine: + lens),
labels (per sample what the oracle's generate_labels saw, in fp64: centre, size, angle, stride-2 centres) and what the case
claims: rows ({sample: expected cls_label row}), zero_faces ({(sample, box, window)}: stride-2 centres EXACTLY on a face of
the positive (box 0) / ignore (box 1) box) and tie_rows ({sample}: fallback rows whose two smallest distances are EQUAL).

Exact label comparison is only fair where the fp64 oracle is not itself on a knife edge, so check_margins() holds for every
case: each stride-2 centre's distance to the nearest face plane of both boxes, and in fallback rows the gap between the
smallest and the second-smallest distance, is either exactly 0 where the case says so or > MARGIN.  No case is exempt.

np.arange(z1, z2, s) yields z1 + i * ((z1 + s) - z1) where the kernel computes z1 + i * s: for strides that are not exact in
binary the two differ in the last fp64 bits -- harmless under the float bar, but the tie and face cases use binary strides."""
import contextlib
import functools
import os

import numpy as np

from oracle import inputs_ref

HERE = os.path.dirname(os.path.abspath(__file__))
MARGIN = 1e-9
REFINE_STRIDES = (0.1, 0.2, 0.4, 0.8)
BINARY_STRIDES = (0.125, 0.25, 0.5, 1.0)
KITTI_FLOAT_KEYS = ("point_cloud", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "box3d_center", "box3d_heading",
                    "box3d_size", "rot_angle")
SUNRGBD_FLOAT_KEYS = KITTI_FLOAT_KEYS + ("center_ref5",)
REFINE_FLOAT_KEYS = KITTI_FLOAT_KEYS + ("ref_center",)


def fixture(name):
    return {k: np.array(v) for k, v in np.load(os.path.join(HERE, "golden", name + ".npz")).items()}


# ------------------------------------------------------------------------------------------------------------- the oracle
@contextlib.contextmanager
def _capture(fn_name, store):
    """Records what the oracle's label function is handed (centre, size, angle, stride-2 centres: after rotation, flip and
    shift, in fp64), so the margins are measured on the oracle's own numbers."""
    orig = getattr(inputs_ref, fn_name)

    def wrap(center, size, angle, ref):
        store.append(dict(center=np.array(center, dtype=np.float64), size=np.array(size, dtype=np.float64), angle=float(angle),
                          ref=np.array(ref, dtype=np.float64)))
        return orig(center, size, angle, ref)
    setattr(inputs_ref, fn_name, wrap)
    try:
        yield
    finally:
        setattr(inputs_ref, fn_name, orig)


def _expected(case):
    rec, labels = case["rec"], []
    if case["kind"] == "refine":
        offs = np.concatenate([[0], np.cumsum(rec["raw_counts"])])
        items = []
        with _capture("generate_labels_refine", labels):
            for b in range(len(rec["raw_counts"])):
                sl = slice(int(offs[b]), int(offs[b + 1]))
                items.append(inputs_ref.prepare_sample_refine(
                    rec["raw_points"][sl], rec["pred_corners"][b], float(rec["pred_angle"][b]), rec["pred_size"][b],
                    rec["box3d_corners"][b], float(rec["heading"][b]), rec["size"][b], rec["draw_choice"][b],
                    float(rec["draw_coin"][b]), float(rec["draw_normal"][b]), case["strides"], case["flip"], case["shift"]))
        want = inputs_ref.collate_refine(items)
        want["lens"] = np.array([[it["center_ref%d" % (s + 1)].shape[-1] for s in range(4)] for it in items], dtype=np.int32)
        want["size_class"] = np.zeros((len(items), 1), dtype=np.int64)                       # every record is a 'Car'
    elif case["kind"] == "kitti":
        with _capture("generate_labels", labels):
            want = inputs_ref.prepare_batch(rec, case["strides"], case["max_depth"], case["flip"], case["shift"])
        want["size_class"] = np.zeros((len(rec["raw_counts"]), 1), dtype=np.int64)           # every record is a 'Car'
    else:
        with _capture("generate_labels", labels):
            want = inputs_ref.prepare_batch_sunrgbd(rec, case["strides"], case["max_depth"], case["flip"], case["shift"])
        want["size_class"] = np.array(rec["size_class"], dtype=np.int64).reshape(-1, 1)
    case["want"], case["labels"] = want, labels
    return case


BOX_SCALES = {"refine": (0.3, 0.6), "kitti": (0.5, 1.0), "sunrgbd": (0.5, 1.0)}


def margins(case):
    """Per sample: face (2, L) -- each stride-2 centre's distance to the nearest face plane of the positive and the ignore box
    -- and gap -- in a fallback row (no centre inside the positive box) the second-smallest minus the smallest distance to the
    box centre (inf for a single window), else None."""
    out = []
    for lab in case["labels"]:
        c, s = np.cos(lab["angle"]), np.sin(lab["angle"])
        d = lab["ref"] - lab["center"][None, :]
        loc = np.stack([c * d[:, 0] - s * d[:, 2], d[:, 1], s * d[:, 0] + c * d[:, 2]])      # along l, h, w
        face = []
        for k in BOX_SCALES[case["kind"]]:
            l, w, h = lab["size"] * k
            half = np.array([l / 2.0, h / 2.0, w / 2.0])[:, None]
            face.append(np.abs(np.abs(loc) - half).min(0))
        gap = None
        if inputs_ref.in_box(lab["ref"], lab["center"], lab["size"] * BOX_SCALES[case["kind"]][0], lab["angle"]).sum() == 0:
            dis = np.sort(np.sqrt(((lab["ref"] - lab["center"][None, :]) ** 2).sum(1)))
            gap = float(dis[1] - dis[0]) if len(dis) > 1 else float("inf")
        out.append(dict(face=np.stack(face), gap=gap))
    return out


def check_margins(case):
    """The condition of the module docstring, with no case left out.  Returns (smallest non-zero face margin, smallest non-zero
    gap, number of exact faces, number of exact ties) for the report."""
    zero_faces, tie_rows = case.get("zero_faces", set()), case.get("tie_rows", set())
    face_min, gap_min = float("inf"), float("inf")
    for b, m in enumerate(margins(case)):
        for box in range(2):
            for l, v in enumerate(m["face"][box]):
                if (b, box, l) in zero_faces:
                    assert v == 0.0, (case["name"], "centre meant to lie exactly on a face", b, box, l, v)
                else:
                    assert v > MARGIN, (case["name"], "centre on a knife edge", b, box, l, v)
                    face_min = min(face_min, float(v))
        if b in tie_rows:
            assert m["gap"] == 0.0, (case["name"], "row meant to be an exact tie", b, m["gap"])
        elif m["gap"] is not None:
            assert m["gap"] > MARGIN, (case["name"], "fallback on a knife edge", b, m["gap"])
            gap_min = min(gap_min, m["gap"])
    assert all(b < len(case["labels"]) for b in tie_rows) and all(b < len(case["labels"]) for (b, _, _) in zero_faces)
    return face_min, gap_min, len(zero_faces), len(tie_rows)


def check_rows(case):
    """The label rows a case spells out, on the oracle's batch."""
    for b, row in case.get("rows", {}).items():
        got = case["want"]["cls_label"][b].tolist()
        assert got == list(row), (case["name"], b, got, list(row))


def _finish(case):
    _expected(case)
    check_margins(case)
    check_rows(case)
    return case


def records(case):
    """The case's packed arrays as the list of records the public builders take."""
    rec = case["rec"]
    offs = np.concatenate([[0], np.cumsum(rec["raw_counts"])])
    out = []
    for b in range(len(rec["raw_counts"])):
        sl = slice(int(offs[b]), int(offs[b + 1]))
        r = {"points": rec["raw_points"][sl], "box3d": rec["box3d_corners"][b], "heading": float(rec["heading"][b]),
             "size": rec["size"][b], "type": "Car"}
        if case["kind"] == "refine":
            r.update(pred_box3d=rec["pred_corners"][b], pred_angle=float(rec["pred_angle"][b]), pred_size=rec["pred_size"][b])
        else:
            r.update(seg=rec["raw_seg"][sl], box2d=rec["box2d"][b], frustum_angle=float(rec["frustum_angle"][b]))
            if case["kind"] == "kitti":
                r["P"] = rec["P"][b]
            else:
                r.update(K=rec["K"][b], Rtilt=rec["Rtilt"][b], type=str(rec["types"][b]))
        out.append(r)
    return out


def draws(case):
    rec = case["rec"]
    d = (rec["draw_choice"], rec["draw_coin"], rec["draw_normal"])
    return d + (rec["draw_hshift"],) if case["kind"] == "sunrgbd" else d


def _choice(rng, counts, N):
    """np.random.choice as the loaders call it: with replacement only when the record has fewer points than N."""
    return np.stack([rng.choice(int(n), N, int(n) < N) for n in counts]).astype(np.int32)


# ------------------------------------------------------------------------------------------------------------ refine cases
def _refine_rec(samples, counts, N, pt_stride, rng):
    """samples: dicts with pc (3) predicted centre, pangle, psize (l, w, h), local (3) the label box's centre IN THE PREDICTED
    FRAME (before flip and shift), rel its heading relative to the prediction, size (l, w, h), coin, normal."""
    pts, rec = [], {k: [] for k in ("pred_corners", "pred_angle", "pred_size", "box3d_corners", "heading", "size", "draw_coin",
                                    "draw_normal")}
    for smp, n in zip(samples, counts):
        pc, pa = np.asarray(smp["pc"], dtype=np.float64), float(smp["pangle"])
        c, s = np.cos(pa), np.sin(pa)
        lx, ly, lz = smp["local"]
        world = pc + np.array([lx * c + lz * s, ly, -lx * s + lz * c])            # the inverse of rotate_along_y by pangle
        psize, size = np.asarray(smp["psize"], dtype=np.float64), np.asarray(smp["size"], dtype=np.float64)
        rec["pred_corners"].append(inputs_ref.box_corners(pc, psize, pa))
        rec["pred_angle"].append(pa)
        rec["pred_size"].append(psize)
        rec["box3d_corners"].append(inputs_ref.box_corners(world, size, pa + smp["rel"]))
        rec["heading"].append(pa + smp["rel"])
        rec["size"].append(size)
        rec["draw_coin"].append(float(smp["coin"]))
        rec["draw_normal"].append(float(smp["normal"]))
        p = rng.normal(size=(int(n), pt_stride)) * np.concatenate([psize[[0, 2, 1]] / 2.0 + 0.3, np.ones(pt_stride - 3)])
        p[:, :3] += pc[None, :]
        pts.append(p.astype(np.float32))
    rec = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    rec["raw_points"] = np.concatenate(pts, 0)
    rec["raw_counts"] = np.asarray(counts, dtype=np.int64)
    rec["draw_choice"] = _choice(rng, counts, N)
    return rec


def _refine_case(name, samples, counts, N, flip, shift, strides=REFINE_STRIDES, pt_stride=4, seed=0, **claims):
    rec = _refine_rec(samples, counts, N, pt_stride, np.random.RandomState(seed))
    return _finish(dict(name=name, kind="refine", rec=rec, npoints=N, strides=tuple(strides), flip=flip, shift=shift, **claims))


def _seeded_refine_samples(rng, B):
    out = []
    for b in range(B):
        psize = np.array([rng.uniform(3.2, 4.6), rng.uniform(1.4, 2.1), rng.uniform(1.3, 1.9)])
        out.append(dict(pc=rng.uniform(-10, 10, 3) + np.array([0.0, 0.0, 25.0]), pangle=rng.uniform(-np.pi, np.pi), psize=psize,
                        local=rng.uniform(-0.3, 0.3, 3), rel=rng.uniform(-0.2, 0.2), size=psize * rng.uniform(0.8, 1.1, 3),
                        coin=rng.random_sample(), normal=rng.randn()))
    return out


def _flip_shift_matrix(flip, shift):
    """Coin exactly 0.5 (must not flip), just above it, and 0; normal beyond both sides of the +-2 stride_1 clamp and inside."""
    rng = np.random.RandomState(31)
    samples = _seeded_refine_samples(rng, 3)
    for smp, coin, normal in zip(samples, (0.5, 0.5000001, 0.0), (-5.0, 5.0, 0.01)):
        smp["coin"], smp["normal"] = coin, normal
    case = _refine_case("flip_shift_matrix-f%ds%d" % (flip, shift), samples, (80, 300, 513), 300, flip, shift, seed=32)
    if shift:                                       # the clamp is really hit on both sides, and one draw stays inside it
        raw = [smp["normal"] * np.sqrt(smp["size"][0] ** 2 + smp["size"][1] ** 2) * 0.1 for smp in samples]
        s1 = 2.0 * case["strides"][0]
        assert raw[0] < -s1 and raw[1] > s1 and 0.0 < raw[2] < s1, raw
    return case


def _fallback_samples(on):
    a = dict(pc=(1.5, 1.0, 20.0), pangle=0.3, psize=(4.0, 1.6, 1.5), local=(0.05, 0.02, 0.07), rel=0.05, size=(3.9, 1.6, 1.5))
    # B: 5 windows on stride 2 (centres -0.35 .. 0.45); the label box, 0.05 a side, lies 3 m beyond the far end
    b = dict(pc=(-4.0, 1.2, 31.0), pangle=-1.1, psize=(2.0, 0.9, 1.5), local=(0.01, 0.02, 0.45 + 3.0), rel=0.1,
             size=(0.05, 0.05, 0.05))
    # C: one window on every stride
    c = dict(pc=(7.0, 0.8, 12.0), pangle=2.5, psize=(0.5, 0.05, 0.4), local=(0.3, 0.1, 0.2), rel=-0.3, size=(1.0, 0.6, 0.5))
    for smp, coin, normal in zip((a, b, c), (0.9, 0.2, 0.7), (0.3, -1.2, 2.0)):
        smp["coin"], smp["normal"] = (coin, normal) if on else (0.0, 0.0)
    return [a, b, c]


def _fallback_last_padded(on, only=None):
    """B's fallback lands on its LAST real window (index 4 of 5) in a row padded to A's 8: the padding must repeat the +1 that
    thread 0 has just written.  C has one window on every stride: its whole row is that window's label.  only = 0 / 1 / 2: the
    same sample alone (B = 1): Lpad is its own count and nothing is padded."""
    samples, counts = _fallback_samples(on), (200, 60, 1)
    rows = {1: [0, 0, 0, 0, 1, 1, 1, 1], 2: [1] * 8}
    name = "fallback_last_padded-" + ("on" if on else "off")
    if only is not None:
        samples, counts = [samples[only]], (counts[only],)
        rows = {1: {0: [0, 0, 0, 0, 1]}, 2: {0: [1]}}.get(only, {})
        name = "fallback_last_padded-alone%d" % only
    case = _refine_case(name, samples, counts, 128, on, on, seed=41, rows=rows)
    lens = case["want"]["lens"]
    if only is None:
        assert lens[:, 1].tolist() == [8, 5, 1] and lens[2].tolist() == [1, 1, 1, 1], lens
        m = margins(case)
        assert m[1]["gap"] is not None and int(np.argmin(np.sqrt(((case["labels"][1]["ref"] - case["labels"][1]["center"]) ** 2).sum(1)))) == 4
    else:                                           # alone: no padding anywhere
        assert [case["want"]["center_ref%d" % (s + 1)].shape[-1] for s in range(4)] == lens[0].tolist()
        assert case["want"]["cls_label"].shape == (1, int(lens[0, 1]))
    return case


def _fallback_wide_padding():
    """fallback_last_padded's sample B next to a sample with 300 windows: the +1 thread 0 writes on B's last real window (4)
    is repeated over 295 padded positions, by every wave of the workgroup and on a second trip -- not just by thread 0's own
    wave, as in the 8-wide row."""
    a = dict(pc=(3.0, 1.0, 40.0), pangle=0.7, psize=(4.0, 60.0, 1.5), local=(0.05, 0.02, 0.07), rel=0.05, size=(3.9, 1.6, 1.5),
             coin=0.0, normal=0.0)
    b = dict(_fallback_samples(False)[1])
    case = _refine_case("fallback_wide_padding", [a, b], (40, 60), 64, False, False, seed=45,
                        rows={1: [0, 0, 0, 0] + [1] * 296})
    assert case["want"]["lens"][:, 1].tolist() == [300, 5]
    return case


def _long_windows():
    """Predicted width 60: 600 / 300 / 150 / 75 windows, so a thread of the 256 makes a second trip through the stride-2 row.
    Sample 0: a tiny label box whose nearest window (280) is only reached on that trip; sample 1: a large label box with +1 and
    -1 labels on both sides of index 256.  One point per sample."""
    z = lambda i: -30.0 + 0.1 + 0.2 * i
    s0 = dict(pc=(3.0, 1.0, 40.0), pangle=0.7, psize=(4.0, 60.0, 1.5), local=(0.02, 0.01, z(280) + 0.03), rel=0.1,
              size=(0.05, 0.05, 0.05), coin=0.0, normal=0.0)
    s1 = dict(pc=(-2.0, 1.1, 45.0), pangle=-0.4, psize=(4.0, 60.0, 1.5), local=(0.1, 0.05, z(256) + 0.04), rel=0.02,
              size=(8.0, 20.0, 4.0), coin=0.0, normal=0.0)
    case = _refine_case("long_windows", [s0, s1], (3, 1), 1, False, False, seed=51)
    want = case["want"]
    assert want["lens"].tolist() == [[600, 300, 150, 75]] * 2 and want["point_cloud"].shape == (2, 3, 1)
    assert np.nonzero(want["cls_label"][0])[0].tolist() == [280] and margins(case)[0]["gap"] is not None
    row = want["cls_label"][1]
    for v in (1, -1):
        assert (row[:256] == v).any() and (row[256:] == v).any(), v
    assert row[255] == 1 and row[256] == 1 and row[0] == 0 and row[-1] == 0
    return case


def _exact_tie():
    """Binary strides, predicted angle 0, predicted box at the origin, width 4: the stride-2 centres are -1.875 + 0.25 i exactly.
    A label box of side 2^-6 at z = -1.5 / 0 / 1.5 is EXACTLY midway between two of them: the lower index gets the +1, like
    np.argmin."""
    samples = [dict(pc=(0.0, 0.0, 0.0), pangle=0.0, psize=(2.0, 4.0, 1.5), local=(0.0, 0.0, z), rel=0.0, size=(2.0 ** -6,) * 3,
                    coin=0.0, normal=0.0) for z in (-1.5, 0.0, 1.5)]
    rows = {b: [1 if i == hit else 0 for i in range(16)] for b, hit in enumerate((1, 7, 13))}
    case = _refine_case("exact_tie", samples, (7, 30, 12), 64, False, False, strides=BINARY_STRIDES, seed=61, rows=rows,
                        tie_rows={0, 1, 2})
    for lab, hit in zip(case["labels"], (1, 7, 13)):
        dis = np.sqrt(((lab["ref"] - lab["center"][None, :]) ** 2).sum(1))
        assert dis[hit] == dis[hit + 1] == dis.min() == 0.125 and (dis == dis.min()).sum() == 2, dis
    return case


def _ragged_n(N, pt_stride):
    """Resampling: records of 5, 50 and 700 points against N below, between and above them."""
    rng = np.random.RandomState(700 + N)
    return _refine_case("ragged_n-%d-%d" % (N, pt_stride), _seeded_refine_samples(rng, 3), (5, 50, 700), N, True, True,
                        pt_stride=pt_stride, seed=71 + N)


# ------------------------------------------------------------------------------------------------------- first-stage cases
def _kitti_rec(samples, counts, N, rng, pt_stride=4):
    """samples: dicts with P (3,4), box2d (4), fangle, center (3) the label box's centre IN THE CENTRE VIEW (after the rotation by
    pi/2 + fangle, before flip and shift), heading (world), size (l, w, h), coin, normal."""
    keys = ("box2d", "P", "box3d_corners", "heading", "size", "frustum_angle", "draw_coin", "draw_normal")
    rec, pts, seg = {k: [] for k in keys}, [], []
    for smp, n in zip(samples, counts):
        rot = np.pi / 2.0 + smp["fangle"]
        c, s = np.cos(rot), np.sin(rot)
        xr, y, zr = smp["center"]
        world = np.array([xr * c + zr * s, y, -xr * s + zr * c])                 # the inverse of rotate_along_y by rot
        size = np.asarray(smp["size"], dtype=np.float64)
        rec["box2d"].append(smp["box2d"]); rec["P"].append(smp["P"]); rec["frustum_angle"].append(smp["fangle"])
        rec["box3d_corners"].append(inputs_ref.box_corners(world, size, smp["heading"]))
        rec["heading"].append(smp["heading"]); rec["size"].append(size)
        rec["draw_coin"].append(smp["coin"]); rec["draw_normal"].append(smp["normal"])
        p = rng.normal(size=(int(n), pt_stride)) * 1.5
        p[:, :3] += world[None, :]
        pts.append(p.astype(np.float32))
        seg.append(rng.randint(0, 2, int(n)).astype(np.int64))
    rec = {k: np.asarray(v, dtype=np.float64) for k, v in rec.items()}
    rec["raw_points"], rec["raw_seg"] = np.concatenate(pts, 0), np.concatenate(seg, 0)
    rec["raw_counts"] = np.asarray(counts, dtype=np.int64)
    rec["draw_choice"] = _choice(rng, counts, N)
    return rec


def _kitti_case(name, samples, counts, N, strides, max_depth, flip, shift, seed, **claims):
    rec = _kitti_rec(samples, counts, N, np.random.RandomState(seed))
    return _finish(dict(name=name, kind="kitti", rec=rec, npoints=N, strides=tuple(strides), max_depth=float(max_depth),
                        flip=flip, shift=shift, **claims))


P_AXIS = np.array([[700.0, 0.0, 600.0, 0.0], [0.0, 700.0, 180.0, 0.0], [0.0, 0.0, 1.0, 0.0]])


def _on_axis(z, size, coin=0.0, normal=0.0):
    """2-D box centred on the principal point, frustum_angle = -pi/2: rot = 0 exactly and the window centres are (0, 0, depth)."""
    return dict(P=P_AXIS, box2d=(560.0, 150.0, 640.0, 210.0), fangle=-np.pi / 2.0, center=(0.0, 0.0, z), heading=0.0, size=size,
                coin=coin, normal=normal)


def _kitti_long_l2():
    """L2 = 280 > 256 windows: the per-thread minimum over two windows and the (distance, index) order of the cross-thread
    reduction.  Stride-2 centres are 0.125 + 0.25 i exactly; the boxes at 10 and 66 are exact ties (39 | 40, 263 | 264: the
    lower index wins, 263 on a thread's second trip), the one at 0 falls back to window 0, the one at 69.875 sits on window 279."""
    samples = [_on_axis(z, (2.0 ** -6,) * 3) for z in (0.0, 10.0, 66.0, 69.875)]
    hits = (0, 39, 263, 279)
    rows = {b: [1 if i == h else 0 for i in range(280)] for b, h in enumerate(hits)}
    case = _kitti_case("kitti_long_l2", samples, (40, 9, 70, 64), 64, BINARY_STRIDES, 70.0, False, False, 81, rows=rows,
                       tie_rows={1, 2})
    assert [case["want"]["center_ref%d" % (s + 1)].shape[-1] for s in range(4)] == [560, 280, 140, 70]
    assert all(float(lab["ref"][0, 2]) == 0.125 and not lab["ref"][:, :2].any() for lab in case["labels"])
    assert float(case["want"]["rot_angle"][0, 0]) == 0.0
    gaps = [m["gap"] for m in margins(case)]
    assert gaps[0] == 0.25 and gaps[1] == 0.0 and gaps[2] == 0.0 and gaps[3] is None, gaps
    return case


def _kitti_face_inclusive():
    """Stride 2 = 0.5: centres 0.25 + 0.5 i.  A label box with w = 2 at z = 10.25 has its half-box faces EXACTLY on the centres
    9.75 and 10.75 (+1: a face counts as inside) and its full-box faces exactly on 9.25 and 11.25 (-1)."""
    row = [0] * 140
    row[18:23] = [-1, 1, 1, 1, -1]
    case = _kitti_case("kitti_face_inclusive", [_on_axis(10.25, (1.0, 2.0, 1.0))], (33,), 40, (0.25, 0.5, 1.0, 2.0), 70.0, False,
                       False, 82, rows={0: row}, zero_faces={(0, 0, 19), (0, 0, 21), (0, 1, 18), (0, 1, 22)})
    lab = case["labels"][0]
    dz = lab["ref"][:, 2] - lab["center"][2]
    assert dz[18:23].tolist() == [-1.0, -0.5, 0.0, 0.5, 1.0] and lab["angle"] == 0.0
    return case


def _off_axis(rng, z, normal):
    f = rng.uniform(650.0, 750.0)
    P = np.array([[f, 0.0, rng.uniform(580, 640), rng.uniform(30, 60)], [0.0, f, rng.uniform(160, 200), rng.uniform(-1, 1)],
                  [0.0, 0.0, 1.0, 0.003]])
    u, v = rng.uniform(300, 900), rng.uniform(150, 220)
    fangle = -np.arctan2(f, u - P[0, 2])                                        # the ray through the 2-D box centre, roughly
    return dict(P=P, box2d=(u - 40.0, v - 30.0, u + 40.0, v + 30.0), fangle=float(fangle),
                center=(rng.uniform(-0.4, 0.4), rng.uniform(0.8, 1.4), z), heading=rng.uniform(-np.pi, np.pi),
                size=(rng.uniform(3.4, 4.4), rng.uniform(1.5, 1.9), rng.uniform(1.4, 1.8)), coin=rng.random_sample(), normal=normal)


def _kitti_shift_clamps(which):
    """Both clamps of the depth shift: +-0.5 dist on the draw, and the clip of the shifted centre to [0, max_depth]."""
    rng = np.random.RandomState(91 if which == "ends" else 92)
    if which == "ends":
        plan = [(0.3, -5.0), (0.3, 5.0), (69.8, -5.0), (69.8, 5.0)]
    else:
        plan = [(33.0, -5.0), (35.0, 5.0), (37.0, 0.01)]
    samples = [_off_axis(rng, z, n) for z, n in plan]
    case = _kitti_case("kitti_shift_clamps-" + which, samples, (90, 300, 700, 17)[:len(plan)], 257, (0.25, 0.5, 1.0, 2.0), 70.0,
                       True, True, 93)
    cz = [float(lab["center"][2]) for lab in case["labels"]]                    # after the shift
    dist = [float(np.sqrt(s["size"][0] ** 2 + s["size"][1] ** 2)) for s in samples]
    if which == "ends":
        assert abs(cz[0]) < 1e-12 and abs(cz[3] - 70.0) < 1e-12, cz              # the clip to [0, max_depth], both ends
        assert abs(cz[1] - (0.3 + 0.5 * dist[1])) < 1e-9 and abs(cz[2] - (69.8 - 0.5 * dist[2])) < 1e-9, cz
    else:
        want = [33.0 - 0.5 * dist[0], 35.0 + 0.5 * dist[1], 37.0 + 0.01 * dist[2] * 0.2]
        assert np.abs(np.array(cz) - want).max() < 1e-9, (cz, want)
    return case


SUN_COIN = (0.5, 0.5000001, 0.0, 1.0, 0.49, 0.9)
SUN_NORMAL = (-5.0, 5.0, 0.0, 0.01, -0.01, 2.0)
SUN_HSHIFT = (0.0, 0.999999, 0.5, 0.25, 0.75, 0.1)


def _sunrgbd(flip, shift, tiny, N):
    """The SUN-RGBD fixture's records with forced draws; tiny: boxes shrunk to 2 % (every row falls back to the nearest centre
    through K and Rtilt).  shift off is the kernel's path without a height-shift pointer."""
    g = fixture("inputs_sunrgbd_b6")
    rec = {k: g[k] for k in ("raw_points", "raw_seg", "raw_counts", "box2d", "K", "Rtilt", "box3d_corners", "heading", "size",
                             "frustum_angle", "types")}
    rec["size_class"] = g["ref_size_class"]
    if tiny:
        rec["size"] = rec["size"] * 0.02
        mid = rec["box3d_corners"].mean(1, keepdims=True)
        rec["box3d_corners"] = mid + 0.02 * (rec["box3d_corners"] - mid)
    rec["draw_choice"] = _choice(np.random.RandomState(200 + N), rec["raw_counts"], N)
    rec["draw_coin"], rec["draw_normal"], rec["draw_hshift"] = (np.array(v, dtype=np.float64) for v in (SUN_COIN, SUN_NORMAL, SUN_HSHIFT))
    case = _finish(dict(name="sunrgbd-f%ds%d-%s-n%d" % (flip, shift, "tiny" if tiny else "rec", N), kind="sunrgbd", rec=rec, npoints=N,
                        strides=tuple(float(s) for s in g["meta_strides"]), max_depth=float(g["meta_max_depth"]), flip=flip,
                        shift=shift))
    cls = case["want"]["cls_label"]
    if tiny:
        assert ((cls == 1).sum(1) == 1).all() and not (cls == -1).any() and all(m["gap"] is not None for m in margins(case))
    else:
        assert ((cls == 1).sum(1) >= 1).all()
    assert case["want"]["point_cloud"].shape == (6, 3, N) and cls.shape == (6, 40)
    return case


# ------------------------------------------------------------------------------------------------------------------- index
FLIP_SHIFT = [(f, s) for f in (False, True) for s in (False, True)]
REFINE_CASES = {}
for _f, _s in FLIP_SHIFT:
    REFINE_CASES["flip_shift_matrix-f%ds%d" % (_f, _s)] = functools.partial(_flip_shift_matrix, _f, _s)
REFINE_CASES["fallback_last_padded-off"] = functools.partial(_fallback_last_padded, False)
REFINE_CASES["fallback_last_padded-on"] = functools.partial(_fallback_last_padded, True)
for _b in range(3):
    REFINE_CASES["fallback_last_padded-alone%d" % _b] = functools.partial(_fallback_last_padded, False, _b)
REFINE_CASES["fallback_wide_padding"] = _fallback_wide_padding
REFINE_CASES["long_windows"] = _long_windows
REFINE_CASES["exact_tie"] = _exact_tie
for _n in (1, 100, 257, 1024):
    for _p in (3, 4):
        REFINE_CASES["ragged_n-%d-%d" % (_n, _p)] = functools.partial(_ragged_n, _n, _p)

KITTI_CASES = {"kitti_long_l2": _kitti_long_l2, "kitti_face_inclusive": _kitti_face_inclusive,
               "kitti_shift_clamps-ends": functools.partial(_kitti_shift_clamps, "ends"),
               "kitti_shift_clamps-mid": functools.partial(_kitti_shift_clamps, "mid")}

SUNRGBD_CASES = {}
for _f, _s in FLIP_SHIFT:
    for _t in (False, True):
        for _n in (1, 257, 2048):
            SUNRGBD_CASES["sunrgbd-f%ds%d-%s-n%d" % (_f, _s, "tiny" if _t else "rec", _n)] = functools.partial(_sunrgbd, _f, _s, _t, _n)

CASES = dict(REFINE_CASES, **KITTI_CASES, **SUNRGBD_CASES)


@functools.lru_cache(maxsize=None)
def built(name):
    """A case with the oracle's batch, computed once and shared (read-only) by the tests that use it."""
    case = CASES[name]()
    assert case["name"] == name, (case["name"], name)
    return case
