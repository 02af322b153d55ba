"""-m gpu: the training side of the frustum extraction -- fcn_frustum_label_count / _fill (csrc/frustum_label.h) through the C-ABI,
frustum.frustum_training_candidates against the reference's recorded run, InputBuilder.build_device_train against build() on host
records, and one training step on its batch.  The referee is the fp64 numpy restatement of tests/frustum_label_ref.py (pinned to
the reference by tests/test_frustum_label_referee.py).  The scene's shape logic (frame lengths from fcn_frustum_select_seg(),
calibrations, back-projection) is test_gpu_frustum.py's.  tests/test_emu_frustum_label.py runs the same functions on the host
emulation of the kernels."""
import functools
import os

import numpy as np
import pytest
import torch

import frustum_label_ref
import frustum_ref
from test_gpu_frustum import (BADARG, _back_project, _bits, _calib, _check_rows, _common, _dev, _input_builder, _lengths, _p, _seg,
                              _seg_counts)
from test_gpu_frustum import _count as _select_count
from test_gpu_frustum import _fill as _select_fill

pytestmark = pytest.mark.gpu
MARGIN = 1e-6                      # m: the inputs keep this distance from every face plane (as the golden fixture does)
MARGIN_PX = 1e-6                   # px: and this from every 2-D edge
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_label.npz")
# tx, ty, tz, l, w, h, ry: rect camera coordinates, t the bottom centre.  MAIN, SECOND: every frame; QUARTER: behind the clip
# distance but nearer than any background point (they start at 3 m); AIR: above the image.  Pairwise disjoint.
MAIN = (0.0, 1.6, 20.0, 8.0, 6.0, 3.0, 0.4)
SECOND = (-2.0, 1.5, 12.0, 5.0, 4.0, 2.5, -2.0)
QUARTER = (0.0, 0.3, 2.4, 0.8, 0.6, 0.4, 1.0)
AIR = (0.0, -6.0, 20.0, 3.9, 1.6, 1.5, 2.6)
INNER_2D = [300.25, 100.5, 700.75, 300.0]


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def _inside_box(rng, n, gt, V2C, R0):
    """n float32 velodyne points drawn inside the 3-D box."""
    l, w, h, ry = gt[3], gt[4], gt[5], gt[6]
    a, dy, b = rng.uniform(-l / 2, l / 2, n), rng.uniform(-h, 0.0, n), rng.uniform(-w / 2, w / 2, n)
    c, s = np.cos(ry), np.sin(ry)
    rect = np.stack([c * a + s * b + gt[0], dy + gt[1], -s * a + c * b + gt[2]])
    ref = np.linalg.solve(R0, rect)
    return np.linalg.solve(V2C[:, :3], ref - V2C[:, 3:4]).T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scene(stride):
    """F = 10 frames of the lengths the kernels' paths turn on; per frame the whole-image box with MAIN beside it and an inner box
    with SECOND; the longest frame also has QUARTER (positives in one wave's quarter of one segment only) and AIR (none).
    Row i of a frame lies inside MAIN when i % 7 == 0, inside SECOND when i % 11 == 3; points keep the margins.  Returns the
    inputs and the referee's answer."""
    seg = _seg()
    lengths = _lengths(seg)
    F = len(lengths)
    rng = np.random.RandomState(300 + stride)
    P, V2C, R0, wh = _calib(F)
    boxes, bframe, gt = [], [], []
    for f in range(F):
        W, H = wh[f]
        boxes += [[-50.0, -50.0, W + 50.0, H + 50.0], INNER_2D]
        gt += [MAIN, SECOND]
        bframe += [f, f]
    W, H = wh[F - 1]
    boxes += [[-50.0, -50.0, W + 50.0, H + 50.0], [-50.0, -50.0, W + 50.0, H + 50.0]]
    gt += [QUARTER, AIR]
    bframe += [F - 1, F - 1]
    boxes, gt, bframe = np.asarray(boxes, dtype=np.float64), np.asarray(gt, dtype=np.float64), np.asarray(bframe, dtype=np.int32)
    q_lo = seg + 2 * (seg // 4)                                      # segment 1, wave 2's quarter of a full segment
    frames = []
    for f, n in enumerate(lengths):
        W, H = wh[f]
        i = np.arange(n)
        owner = np.where(i % 7 == 0, 0, np.where(i % 11 == 3, 1, -1))
        if f == F - 1:
            owner[(i >= q_lo + 5) & (i < q_lo + seg // 4 - 5) & (i % 13 == 1) & (owner < 0)] = 2
        mine = np.nonzero(bframe == f)[0]
        xyz = np.zeros((n, 3), dtype=np.float32)
        todo = np.ones(n, dtype=bool)
        for _ in range(100):
            for k, box in enumerate((MAIN, SECOND, QUARTER)):
                m = todo & (owner == k)
                xyz[m] = _inside_box(rng, int(m.sum()), box, V2C[f], R0[f])
            m = todo & (owner < 0)
            xyz[m] = _back_project(rng, int(m.sum()), P[f], V2C[f], R0[f], W, H, inside=n <= 255)
            rect, u, v = frustum_ref.project(xyz, P[f], V2C[f], R0[f])
            todo = np.zeros(n, dtype=bool)
            for d in mine:
                todo |= frustum_label_ref.face_distance(rect.astype(np.float32), gt[d]) < MARGIN
                todo |= frustum_ref.edge_distance(u, v, boxes[d], W, H) < MARGIN_PX
            if not todo.any():
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (n, stride - 3)).astype(np.float32)], 1))
    pts = np.concatenate(frames, 0)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ref = frustum_label_ref.select_labeled(pts, off, P, V2C, R0, wh, boxes, bframe, gt)
    S = 3
    ref["seg_cnt"] = _seg_counts(ref["index"], S, seg)
    ref["seg_pos"] = _seg_counts([ix[sg > 0] for ix, sg in zip(ref["index"], ref["seg"])], S, seg)
    D = len(bframe)
    big, quarter, air = D - 4, D - 2, D - 1                          # the longest frame's whole-image box, QUARTER, AIR
    assert min(e.min() for e in ref["face"] if len(e)) >= MARGIN and min(e.min() for e in ref["edge"] if len(e)) >= MARGIN_PX
    assert (ref["seg_pos"][big] > 0).all() and (ref["seg_pos"][big] % 64 != 0).all()      # every segment, no multiple of 64
    assert (ref["seg_pos"][big + 1] > 0).all() and (ref["seg_pos"][big + 1] < ref["seg_cnt"][big + 1]).all()
    qi = ref["index"][quarter][ref["seg"][quarter] > 0]
    assert len(qi) > 10 and qi.min() >= q_lo and qi.max() < q_lo + seg // 4                # one wave's quarter only
    assert ref["pos"][air] == 0 and ref["counts"][air] > seg
    assert ref["pos"][2] == 1 and ref["counts"][2] == 1 and ref["counts"][0] == 0          # the frames of 1 and 0 rows
    return {"pts": pts, "off": off, "P": P, "V2C": V2C, "R0": R0, "wh": wh, "boxes": boxes, "bframe": bframe, "gt": gt,
            "ref": ref, "S": S, "seg": seg, "lengths": lengths, "big": big, "quarter": quarter, "air": air}


KEYS = ("pts", "off", "P", "V2C", "R0", "wh", "boxes", "bframe", "gt")


def _tensors(sc, **over):
    return {k: _dev(over.get(k, sc[k])) for k in KEYS}


def _count(t, S, clipd=2.0):
    """The raw labelled count on device tensors -> rc, outputs (sentinel-filled first)."""
    from frustum_convnet_amd import _native
    D = t["bframe"].numel()
    f64 = dict(dtype=torch.float64, device="cuda")
    o = {"box2d": torch.full((D, 4), -7.0, **f64), "angle": torch.full((D,), -7.0, **f64),
         "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
         "spos": torch.full((D, S), -7, dtype=torch.int32, device="cuda"), "corners": torch.full((D, 24), -7.0, **f64)}
    rc = _native.lib().fcn_frustum_label_count(*_common(t, S, False, clipd), _p(t["gt"]), _p(o["box2d"]), _p(o["angle"]),
                                               _p(o["scnt"]), _p(o["spos"]), _p(o["corners"]), _native.current_stream())
    torch.cuda.synchronize()
    return rc, o


def _fill(t, S, seg_counts, clipd=2.0, guard=5):
    """The raw labelled fill -> rc, rows, labels, the `guard` poisoned entries behind each, seg_off."""
    from frustum_convnet_amd import _native
    ps = t["pts"].shape[1]
    soff = np.concatenate([[0], np.cumsum(np.asarray(seg_counts).reshape(-1))]).astype(np.int64)
    n = int(soff[-1])
    out = torch.full((n + guard, ps), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((n + guard,), -7, dtype=torch.int64, device="cuda")
    soff_d = _dev(soff)
    rc = _native.lib().fcn_frustum_label_fill(*_common(t, S, False, clipd), _p(t["gt"]), _p(soff_d), _p(out), _p(oseg),
                                              _native.current_stream())
    torch.cuda.synchronize()
    out, oseg = out.cpu().numpy(), oseg.cpu().numpy()
    return rc, out[:n], oseg[:n], (out[n:], oseg[n:]), soff


def _guards_intact(guard):
    return bool((guard[0] == -7.0).all() and (guard[1] == -7).all())


@pytest.mark.parametrize("stride", [3, 4, 5])
def test_label_entry_points_match_the_referee(stride):
    sc = _scene(stride)
    ref, S = sc["ref"], sc["S"]
    t = _tensors(sc)
    rc, o = _count(t, S)
    assert rc == 0
    scnt, spos = o["scnt"].cpu().numpy(), o["spos"].cpu().numpy()
    print("cnt", scnt.sum(1).tolist(), "pos", spos.sum(1).tolist(), "referee pos", ref["pos"].tolist())
    assert np.array_equal(scnt, ref["seg_cnt"]) and np.array_equal(spos, ref["seg_pos"])       # per segment
    assert np.array_equal(o["box2d"].cpu().numpy(), sc["boxes"])                                # (no clipping)
    aerr = np.abs(o["angle"].cpu().numpy() - ref["frustum_angle"])
    cerr = np.abs(o["corners"].cpu().numpy().reshape(-1, 8, 3) - ref["corners"])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all()
    assert np.abs(ref["corners"]).max() < 100.0
    rc, rows, seg, guard, soff = _fill(t, S, scnt)
    assert rc == 0 and _guards_intact(guard)
    _check_rows(rows, np.concatenate(ref["rows"], 0), "stride %d" % stride)
    assert seg.dtype == np.int64 and np.array_equal(seg, np.concatenate(ref["seg"]))
    assert np.array_equal(soff[::S], np.concatenate([[0], np.cumsum(ref["counts"])]))
    rc2, rows2, seg2, _, _ = _fill(t, S, scnt)
    rc3, o3 = _count(t, S)
    assert rc2 == 0 and np.array_equal(_bits(rows2), _bits(rows)) and np.array_equal(seg2, seg)  # identical over two runs
    assert rc3 == 0 and all(torch.equal(o3[k], o[k]) for k in o)
    # labelling does not disturb selection: the unlabelled pair on the same inputs gives the same counts and rows, bit for bit
    rc, so = _select_count(t, S, False)
    assert rc == 0 and torch.equal(so["scnt"], o["scnt"]) and torch.equal(so["box2d"], o["box2d"]) and torch.equal(so["angle"], o["angle"])
    rc, srows, sguard, _ = _select_fill(t, S, scnt, False)
    assert rc == 0 and np.array_equal(_bits(srows), _bits(rows))
    # more segments than any frame needs: the surplus ones count 0
    rc, o5 = _count(t, S + 2)
    assert rc == 0 and np.array_equal(o5["spos"].cpu().numpy()[:, :S], ref["seg_pos"]) and (o5["spos"].cpu().numpy()[:, S:] == 0).all()
    assert np.array_equal(o5["scnt"].cpu().numpy()[:, :S], ref["seg_cnt"]) and (o5["scnt"].cpu().numpy()[:, S:] == 0).all()


def test_label_rows_that_are_not_16_byte_aligned():
    """pt_stride 4 takes 16-byte accesses only when the buffers allow it: a view that starts 4 bytes into an allocation must give
    the aligned run's counts, positives, rows and labels through the word-by-word path, bit for bit."""
    sc = _scene(4)
    S = sc["S"]
    t = _tensors(sc)
    rc, o = _count(t, S)
    rc_f, rows_a, seg_a, _, _ = _fill(t, S, o["scnt"].cpu().numpy())
    assert rc == 0 and rc_f == 0 and np.array_equal(o["scnt"].cpu().numpy(), sc["ref"]["seg_cnt"])
    flat = torch.zeros(sc["pts"].size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = t["pts"].reshape(-1)
    t["pts"] = flat[1:].view(-1, 4)
    assert t["pts"].data_ptr() % 16 == 4
    rc, o2 = _count(t, S)
    assert rc == 0 and all(torch.equal(o2[k], o[k]) for k in o)
    rc, rows, seg, guard, _ = _fill(t, S, o2["scnt"].cpu().numpy())
    assert rc == 0 and _guards_intact(guard)
    assert np.array_equal(_bits(rows), _bits(rows_a)) and np.array_equal(seg, seg_a)


def test_points_exactly_on_a_face_are_inside_and_one_step_out_is_outside():
    """An axis-aligned box (ry = 0) with dyadic centre and sizes, identity V2C / R0 and a plain pinhole P: the float32 rect row IS
    the input row.  Per face: one float32 step inside, exactly on it, one step outside -> 1, 1, 0."""
    gt = np.asarray([[4.0, 1.0, 16.0, 2.0, 1.0, 0.5, 0.0]])          # x in [3, 5], y in [0.5, 1], z in [15.5, 16.5]
    centre = np.asarray([4.0, 0.75, 16.0], dtype=np.float32)
    rows, want = [], []
    for axis, (lo, hi) in enumerate(((3.0, 5.0), (0.5, 1.0), (15.5, 16.5))):
        for face, outward in ((lo, -np.inf), (hi, np.inf)):
            f32 = np.float32(face)
            assert float(f32) == face
            for val, inside in ((np.nextafter(f32, np.float32(-outward)), 1), (f32, 1), (np.nextafter(f32, np.float32(outward)), 0)):
                p = centre.copy()
                p[axis] = val
                rows.append(p)
                want.append(inside)
    pts = np.concatenate([np.asarray(rows, dtype=np.float32), np.full((len(rows), 1), 0.5, dtype=np.float32)], 1)
    want = np.asarray(want, dtype=np.int64)
    eye = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)
    P = np.asarray([[[700.0, 0.0, 600.0, 0.0], [0.0, 700.0, 180.0, 0.0], [0.0, 0.0, 1.0, 0.0]]])
    sc = {"pts": pts, "off": np.asarray([0, len(pts)], dtype=np.int64), "P": P, "V2C": eye[None], "R0": np.eye(3)[None],
          "wh": np.asarray([[1242.0, 375.0]]), "boxes": np.asarray([[0.0, 0.0, 1242.0, 375.0]]),
          "bframe": np.zeros(1, dtype=np.int32), "gt": gt}
    assert np.array_equal(frustum_label_ref.in_box(pts[:, :3], gt[0]).astype(np.int64), want)       # (the referee says the same)
    assert want.sum() == 12 and len(want) == 18
    t = _tensors(sc)
    rc, o = _count(t, 1)
    assert rc == 0 and o["scnt"].cpu().numpy().tolist() == [[18]] and o["spos"].cpu().numpy().tolist() == [[12]]
    rc, got, seg, guard, _ = _fill(t, 1, [[18]])
    assert rc == 0 and _guards_intact(guard)
    assert np.array_equal(_bits(got), _bits(pts))                     # the rect row is the input row, bit for bit
    assert np.array_equal(seg, want)
    assert np.array_equal(o["corners"].cpu().numpy().reshape(8, 3), frustum_label_ref.corners(gt[0]))    # cos 0, sin 0: exact


def test_slices_bound_both_stores():
    """seg_off bounds the writes to out_pts AND out_seg: with offsets that grant one segment 100 rows fewer than it selects and
    one box no row at all, both buffers hold the slices and nothing else; neighbours and the poisoned entries behind are unchanged."""
    sc = _scene(4)
    S, seg, ref = sc["S"], sc["seg"], sc["ref"]
    t = _tensors(sc)
    counts = ref["seg_cnt"].copy()
    d, s, none = sc["big"], 1, sc["big"] + 1
    assert counts[d, s] > 200 and counts[none].sum() > 0 and ref["pos"][none] > 0
    counts[d, s] -= 100
    counts[none] = 0                                                 # (how the host leaves a rejected box out)
    rc, rows, lab, guard, soff = _fill(t, S, counts)
    assert rc == 0 and _guards_intact(guard)
    assert len(rows) == ref["counts"].sum() - 100 - ref["counts"][none] == len(lab)
    for dd in range(len(counts)):
        for ss in range(S):
            i = dd * S + ss
            m = (ref["index"][dd] // seg) == ss
            _check_rows(rows[soff[i]:soff[i + 1]], ref["rows"][dd][m][:counts[dd, ss]], "")
            assert np.array_equal(lab[soff[i]:soff[i + 1]], ref["seg"][dd][m][:counts[dd, ss]]), (dd, ss)
    # every box granted nothing: nothing is written at all
    rc, rows, lab, guard, _ = _fill(t, S, np.zeros_like(counts))
    assert rc == 0 and len(rows) == 0 and len(lab) == 0 and _guards_intact(guard)


def test_label_bad_arguments_are_refused_with_nothing_written():
    from frustum_convnet_amd import _native
    sc = _scene(3)
    S = sc["S"]
    t = _tensors(sc)
    L = _native.lib()
    s = _native.current_stream()
    D = t["bframe"].numel()
    rc, o = _count(t, S)
    assert rc == 0
    scnt = o["scnt"].cpu().numpy()
    # S too small for the longest frame: refused, nothing launched
    rc, ob = _count(t, S - 1)
    assert rc == BADARG and all((ob[k].cpu().numpy() == -7).all() for k in ob)
    f64 = dict(dtype=torch.float64, device="cuda")
    w = {"box2d": torch.full((D, 4), -7.0, **f64), "angle": torch.full((D,), -7.0, **f64),
         "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
         "spos": torch.full((D, S), -7, dtype=torch.int32, device="cuda"), "corners": torch.full((D, 24), -7.0, **f64)}
    good = _common(t, S, False) + [_p(t["gt"]), _p(w["box2d"]), _p(w["angle"]), _p(w["scnt"]), _p(w["spos"]), _p(w["corners"]), s]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 18, 19):              # NULL pointers
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_label_count(*bad) == BADARG, i
    for i, v in ((3, 2), (11, 0), (11, -1), (10, -1), (2, -1), (10, 65536)):  # pt_stride 2, S < 1, negative sizes, D > 65535
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_label_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((w[k].cpu().numpy() == -7).all() for k in w)               # nothing written by any of them
    assert L.fcn_frustum_label_count(*good) == 0                           # (the same list is accepted when nothing is wrong)
    torch.cuda.synchronize()
    assert torch.equal(w["spos"], o["spos"]) and torch.equal(w["corners"], o["corners"])
    soff = _dev(np.concatenate([[0], np.cumsum(scnt.reshape(-1))]).astype(np.int64))
    out = torch.full((int(scnt.sum()), 3), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((int(scnt.sum()),), -7, dtype=torch.int64, device="cuda")
    goodf = good[:15] + [_p(soff), _p(out), _p(oseg), s]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_frustum_label_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (11, 0), (11, -1), (11, S - 1), (10, -1), (2, -1), (10, 65536)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_frustum_label_fill(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (oseg.cpu().numpy() == -7).all()
    assert L.fcn_frustum_label_fill(*goodf) == 0
    torch.cuda.synchronize()
    assert np.array_equal(oseg.cpu().numpy(), np.concatenate(sc["ref"]["seg"]))


@pytest.mark.parametrize("what", ["frame_high", "frame_negative"])
def test_out_of_range_box_frame_is_reported_and_never_dereferenced(what):
    from frustum_convnet_amd import frustum, _native
    sc = _scene(4)
    S, ref = sc["S"], sc["ref"]
    F = len(sc["lengths"])
    bframe = sc["bframe"].copy()
    bad = sc["big"]
    bframe[bad] = F if what == "frame_high" else -1
    t = _tensors(sc, bframe=bframe)                                  # exactly sized buffers: nothing beyond them can be read
    rc, o = _count(t, S)
    assert rc == BADARG
    scnt, spos = o["scnt"].cpu().numpy(), o["spos"].cpu().numpy()
    want_c, want_p = ref["seg_cnt"].copy(), ref["seg_pos"].copy()
    want_c[bad], want_p[bad] = 0, 0
    assert np.array_equal(scnt, want_c) and np.array_equal(spos, want_p)    # its counts are 0, every other box is processed
    box, ang, cor = o["box2d"].cpu().numpy(), o["angle"].cpu().numpy(), o["corners"].cpu().numpy()
    assert (box[bad] == -7.0).all() and ang[bad] == -7.0 and (cor[bad] == -7.0).all()   # nothing else of it is written
    ok = np.arange(len(bframe)) != bad
    assert np.array_equal(box[ok], sc["boxes"][ok]) and (np.abs(cor[ok].reshape(-1, 8, 3) - ref["corners"][ok]) <= 1e-12).all()
    rc, rows, lab, guard, _ = _fill(t, S, scnt)
    assert rc == BADARG and _guards_intact(guard)
    _check_rows(rows, np.concatenate([r for d, r in enumerate(ref["rows"]) if d != bad], 0), what)
    assert np.array_equal(lab, np.concatenate([r for d, r in enumerate(ref["seg"]) if d != bad]))
    with pytest.raises(_native.NativeError):
        frustum.frustum_training_candidates(t["pts"], t["off"], {"P": t["P"], "V2C": t["V2C"], "R0": t["R0"]}, t["wh"], t["boxes"],
                                            t["bframe"], t["gt"])


def _golden_sel():
    from frustum_convnet_amd import frustum
    g = _golden()
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    sel = frustum.frustum_training_candidates(_dev(g["points"]), _dev(g["off"]), cal, g["img_wh"], g["ref_boxes"], g["box_frame"],
                                              g["gt_box3d"], gt_box2d=g["gt_box2d"])
    return g, cal, sel


def test_training_candidates_equal_the_references_recorded_run():
    """frustum_training_candidates on the golden fixture's frames, perturbed boxes and labels against what the reference's own
    functions produced: the kept boxes, every label, rows, corners, angles."""
    g, cal, sel = _golden_sel()
    kept = np.nonzero(~g["ref_reject"])[0]
    K = len(kept)
    assert np.array_equal(sel["kept"], kept) and sel["kept"].dtype == np.int64 and 0 < K < len(g["box_frame"])
    counts = g["ref_mask"].sum(1)[kept]
    assert np.array_equal(sel["counts"], counts) and sel["counts"].dtype == np.int64
    assert np.array_equal(sel["cnt"].cpu().numpy(), counts) and sel["cnt"].dtype == torch.int32
    assert np.array_equal(sel["pos"].cpu().numpy(), g["ref_label"].sum(1)[kept]) and sel["pos"].dtype == torch.int32
    off_h = sel["off"].cpu().numpy()
    assert np.array_equal(off_h, np.concatenate([[0], np.cumsum(counts)])) and sel["off"].dtype == torch.int64
    assert np.array_equal(sel["box2d"].cpu().numpy(), g["ref_boxes"][kept])
    assert np.array_equal(sel["box_frame"].cpu().numpy(), g["box_frame"][kept]) and sel["box_frame"].dtype == torch.int32
    assert np.array_equal(sel["heading"].cpu().numpy(), g["gt_box3d"][kept, 6])
    assert np.array_equal(sel["size"].cpu().numpy(), g["gt_box3d"][kept, 3:6])
    aerr = np.abs(sel["frustum_angle"].cpu().numpy() - g["ref_angle"][kept])
    cerr = np.abs(sel["box3d"].cpu().numpy() - g["ref_corners"][kept])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all() and sel["box3d"].shape == (K, 8, 3)
    pts_h, seg_h = sel["points"].cpu().numpy(), sel["seg"].cpu().numpy()
    assert sel["points"].dtype == torch.float32 and sel["seg"].dtype == torch.int64 and len(pts_h) == len(seg_h) == counts.sum()
    for k, d in enumerate(kept):
        f = g["box_frame"][d]
        n = int(g["off"][f + 1] - g["off"][f])
        m = g["ref_mask"][d, :n]
        fr = slice(int(g["off"][f]), int(g["off"][f + 1]))
        want = np.concatenate([g["ref_rect"][fr][m], g["points"][fr][m, 3:]], 1)
        _check_rows(pts_h[off_h[k]:off_h[k + 1]], want, "box %d" % d)
        assert np.array_equal(seg_h[off_h[k]:off_h[k + 1]], g["ref_label"][d, :n][m].astype(np.int64)), d
    for k in ("box2d", "frustum_angle", "box3d", "heading", "size"):
        assert sel[k].dtype == torch.float64 and sel[k].is_cuda, k
    assert sorted(sel.keys()) == sorted(["points", "seg", "off", "box2d", "frustum_angle", "box3d", "heading", "size", "box_frame",
                                         "cnt", "pos", "kept", "counts"])
    # gt_box2d defaults to the boxes that select: the small box's PERTURBED height decides then
    g2 = _golden()
    cal = {k: _dev(g2[k]) for k in ("P", "V2C", "R0")}
    from frustum_convnet_amd import frustum
    sel2 = frustum.frustum_training_candidates(_dev(g2["points"]), _dev(g2["off"]), cal, g2["img_wh"], g2["ref_boxes"],
                                               g2["box_frame"], g2["gt_box3d"], min_box_height=10.0)
    hh = g2["ref_boxes"][:, 3] - g2["ref_boxes"][:, 1]
    assert sel2["kept"].tolist() == [d for d in range(len(hh)) if hh[d] >= 10.0 and g2["ref_label"][d].any()]
    assert len(sel2["kept"]) == K + 1


def _records(sel, g, types):
    """Host records of build() from the DOWNLOADED training candidates."""
    pts_h, seg_h, off_h = sel["points"].cpu().numpy(), sel["seg"].cpu().numpy(), sel["off"].cpu().numpy()
    box_h, ang_h, cor_h = sel["box2d"].cpu().numpy(), sel["frustum_angle"].cpu().numpy(), sel["box3d"].cpu().numpy()
    head_h, size_h, bf_h = sel["heading"].cpu().numpy(), sel["size"].cpu().numpy(), sel["box_frame"].cpu().numpy()
    return [{"points": pts_h[off_h[k]:off_h[k + 1]], "seg": seg_h[off_h[k]:off_h[k + 1]], "box2d": box_h[k], "P": g["P"][bf_h[k]],
             "box3d": cor_h[k], "heading": float(head_h[k]), "size": size_h[k], "frustum_angle": float(ang_h[k]),
             "type": types[d]} for k, d in enumerate(sel["kept"])]


def test_build_device_train_equals_build_on_host_records():
    """InputBuilder.build_device_train on the device candidates against build(records) on host records made from the DOWNLOADED
    candidates, same draws, flip and shift on: every key bit-identical."""
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    g, cal, sel = _golden_sel()
    reset_cfg()
    N = 192
    b = inputs.InputBuilder(N, strides=(0.25, 0.5, 1.0, 2.0), max_depth=70.0, random_flip=True, random_shift=True)
    types = [str(x) for x in g["types"]]
    counts = sel["counts"]
    assert (counts < N).any() and (counts > N).any()                  # both resample modes
    draws = inputs.draw(counts, N, True, True, rng=np.random.RandomState(3))
    assert (draws[1] > 0.5).any() and (draws[1] <= 0.5).any()         # flipped and unflipped samples
    got = b.build_device_train(sel, cal["P"], types, draws=draws)
    want = b.build(_records(sel, g, types), draws=draws)
    torch.cuda.synchronize()
    assert sorted(got.keys()) == sorted(want.keys()) and "seg_label" in got and "one_hot" in got
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    cls = got["cls_label"].cpu().numpy()
    assert ((cls == 1).sum(1) >= 1).all()                             # a 1 in every row
    assert (got["seg_label"].cpu().numpy().sum(1) > 0).all()
    assert len(set(got["size_class"].cpu().numpy().ravel().tolist())) == 3      # Car, Pedestrian, Cyclist
    # without the labels' per-point output; into given buffers; drawn like the reference when no draws are given
    got2 = b.build_device_train(sel, cal["P"], types, draws=draws, with_seg=False)
    assert "seg_label" not in got2 and torch.equal(got2["point_cloud"].cpu(), want["point_cloud"].cpu())
    out = b.alloc(len(sel["kept"]))
    got3 = b.build_device_train(sel, cal["P"], types, draws=draws, out=out)
    assert got3["point_cloud"].data_ptr() == out["point_cloud"].data_ptr() and torch.equal(got3["seg_label"].cpu(), want["seg_label"].cpu())
    np.random.seed(5)
    got4 = b.build_device_train(sel, cal["P"], types)
    np.random.seed(5)
    want4 = b.build(_records(sel, g, types))
    assert all(torch.equal(got4[k].cpu(), want4[k].cpu()) for k in want4)


def test_one_training_step_on_the_device_built_batch():
    """The hash-initialised car_b4_n512 model: the losses from the build_device_train batch equal those from the build(records)
    batch bit for bit, are finite, and backward() runs."""
    from helpers import load_golden
    from test_gpu_model import _model
    from frustum_convnet_amd import inputs
    g, cal, sel = _golden_sel()
    g1 = load_golden("car_b4_n512")
    m = _model(g1).train()
    b = inputs.InputBuilder(int(g1["meta_npoint"]), random_flip=True, random_shift=True)      # (cfg holds the model's strides)
    types = [str(x) for x in g["types"]]
    draws = inputs.draw(sel["counts"], b.npoints, True, True, rng=np.random.RandomState(4))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    losses, _ = m(b.build_device_train(sel, cal["P"], types, draws=draws))
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    got = {k: v.detach().cpu().clone() for k, v in losses.items()}
    m.load_state_dict(sd)                                             # (the running statistics moved)
    losses2, _ = m(b.build(_records(sel, g, types), draws=draws))
    torch.cuda.synchronize()
    print({k: float(v) for k, v in got.items()})
    for k, v in losses2.items():
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], v.detach().cpu()), k
    assert float(got["total_loss"]) > 0


def test_empty_results_launch_nothing_behind_them():
    from frustum_convnet_amd import frustum, _native
    g = _golden()
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    rejected = np.nonzero(g["ref_reject"])[0]
    pts, off = _dev(g["points"]), _dev(g["off"])
    L = _native.lib()
    calls = []
    real = L.fcn_frustum_label_fill
    try:
        L.fcn_frustum_label_fill = lambda *a: calls.append(a) or real(*a)
        # only boxes the reject rule drops: 'kept' alone, and the fill is not launched
        sel = frustum.frustum_training_candidates(pts, off, cal, g["img_wh"], g["ref_boxes"][rejected], g["box_frame"][rejected],
                                                  g["gt_box3d"][rejected], gt_box2d=g["gt_box2d"][rejected])
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and sel["kept"].dtype == np.int64 and calls == []
        # D = 0
        sel = frustum.frustum_training_candidates(pts, off, cal, g["img_wh"], np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros((0, 7)))
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and calls == []
        # F = 0: no frame to search
        sel = frustum.frustum_training_candidates(torch.zeros((0, 4), dtype=torch.float32, device="cuda"), np.zeros(1, np.int64),
                                                  {"P": np.zeros((0, 12)), "V2C": np.zeros((0, 12)), "R0": np.zeros((0, 9))},
                                                  np.zeros((0, 2)), g["ref_boxes"][:2], np.zeros(2, np.int32), g["gt_box3d"][:2])
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and calls == []
        ok = frustum.frustum_training_candidates(pts, off, cal, g["img_wh"], g["ref_boxes"], g["box_frame"], g["gt_box3d"],
                                                 gt_box2d=g["gt_box2d"])
        assert len(calls) == 1 and len(ok["kept"]) > 0                # (the spy sees the launch when there is one)
    finally:
        L.fcn_frustum_label_fill = real
    b = _input_builder(64)
    assert list(b.build_device_train(sel, cal["P"], [])) == ["kept"]
    # the entry points themselves: D = 0 touches nothing, F = 0 zeroes both counts
    sc = _scene(3)
    t = _tensors(sc)
    t0 = dict(t, boxes=_dev(np.zeros((0, 4))), bframe=_dev(np.zeros(0, np.int32)), gt=_dev(np.zeros((0, 7))))
    rc, o = _count(t0, sc["S"])
    assert rc == 0 and o["scnt"].numel() == 0
    rc, rows, lab, guard, _ = _fill(t0, sc["S"], np.zeros((0, sc["S"]), np.int64))
    assert rc == 0 and rows.shape == (0, 3) and _guards_intact(guard)
    tf = dict(t, off=_dev(np.zeros(1, np.int64)))
    rc, o = _count(tf, sc["S"])
    assert rc == 0 and (o["scnt"].cpu().numpy() == 0).all() and (o["spos"].cpu().numpy() == 0).all()
    assert (o["box2d"].cpu().numpy() == -7.0).all() and (o["corners"].cpu().numpy() == -7.0).all()
    rc, rows, lab, guard, _ = _fill(tf, sc["S"], np.zeros((t["bframe"].numel(), sc["S"]), np.int64))
    assert rc == 0 and len(rows) == 0 and _guards_intact(guard)
