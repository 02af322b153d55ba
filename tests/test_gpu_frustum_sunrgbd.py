"""-m gpu: the SUN-RGBD frustum extraction on the device -- fcn_frustum_sunrgbd_count / _fill / _label_count / _label_fill and
fcn_frustum_subset_pos (csrc/frustum_sunrgbd.h) and fcn_prepare_inputs_sunrgbd_infer through the C-ABI,
frustum.sunrgbd_candidates / sunrgbd_training_candidates against the reference's recorded run, and
SunrgbdInputBuilder.build_device / build_device_train against the reference loader's batches, against build() on host records, and
in one training step of the five-scale model.  The referee is the fp64 numpy restatement of tests/frustum_sunrgbd_ref.py (pinned to
the reference by tests/test_frustum_sunrgbd_referee.py).  Every shape derives from fcn_frustum_select_seg().
tests/test_emu_frustum_sunrgbd.py runs the same functions on the host emulation of the kernels."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

import frustum_sunrgbd_ref as ref
from test_gpu_frustum import BADARG, NAN_PAYLOAD, _bits, _dev, _lengths, _p, _seg, _seg_counts

pytestmark = pytest.mark.gpu
MARGIN = 1e-6                      # m: the inputs keep this distance from every face plane (as the golden fixture does)
MARGIN_PX = 1e-6                   # px: and this from every 2-D edge
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_sunrgbd.npz")
FLOAT_KEYS = ("point_cloud", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "center_ref5", "box3d_center",
              "box3d_heading", "box3d_size", "rot_angle")
# cx, cy, cz, l, w, h (HALF extents), heading: upright depth.  MAIN, SECOND: every frame; QUARTER: nearer than any background row
# (they start at 1.5 m); AIR: above every row.  Pairwise disjoint.
MAIN = (0.2, 3.0, -0.1, 0.9, 0.6, 0.5, 0.4)
SECOND = (-0.8, 4.6, 0.2, 0.5, 0.4, 0.45, -2.0)
QUARTER = (0.0, 0.9, 0.0, 0.2, 0.15, 0.15, 1.0)
AIR = (0.0, 3.0, 5.0, 0.5, 0.5, 0.3, 2.6)
WHOLE_2D = [-60.0, -60.0, 800.0, 600.0]
INNER_2D = [150.25, 100.5, 450.75, 400.0]
# the kernels load a row in one 16-byte piece (stride 4, 16-byte aligned) or word by word; "4+4", "4+8", "6+4": that stride in a
# buffer that starts 4 / 8 bytes behind a 16-byte boundary (word by word)
STRIDES = [3, 5, 6, 7, 4, "4+4", "4+8", "6+4"]


@functools.lru_cache(maxsize=None)
def _golden():
    return dict(np.load(GOLDEN))


def _calib(F):
    """Frame f takes calibration f % 2 of the golden fixture (a real tilt with small off-diagonal terms; two camera matrices)."""
    g = _golden()
    i = np.arange(F) % 2
    return g["K"][i].copy(), g["Rtilt"][i].copy()


def _inside(rng, n, gt):
    """n float32 upright-depth points drawn inside the 3-D box."""
    l, w, h, heading = gt[3], gt[4], gt[5], gt[6]
    a, b, dz = rng.uniform(-l, l, n), rng.uniform(-w, w, n), rng.uniform(-h, h, n)
    c, s = np.cos(-heading), np.sin(-heading)
    return np.stack([c * a - s * b + gt[0], s * a + c * b + gt[1], dz + gt[2]], 1).astype(np.float32)


def _back_project(rng, n, K, Rt):
    """n float32 upright-depth points from random pixels in and up to 100 px around the image, at 1.5 ... 6 m; one in sixteen
    BEHIND the camera (the reference has no guard: such a row is selected when it projects into the box)."""
    u, v, z = rng.uniform(-100.0, 830.0, n), rng.uniform(-100.0, 630.0, n), rng.uniform(1.5, 6.0, n)
    z = np.where(rng.randint(16, size=n) == 0, -z, z)
    c0, c1 = (u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1]
    return (Rt @ np.stack([c0, z, -c1])).T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scene(stride):
    """F = 10 frames of the lengths the kernels' paths turn on; per frame a box wider than the image with MAIN beside it and an
    inner box with SECOND; the longest frame also has QUARTER (positives in one wave's quarter of one segment only) and AIR
    (none).  Row i of a frame lies inside MAIN when i % 7 == 0, inside SECOND when i % 11 == 3; rows keep the margins.  Three rows
    of the longest frame that the boxes would select carry a NaN, +inf, -inf coordinate; one selected row a NaN payload in a
    passthrough column.  Returns the inputs and the referee's answer."""
    seg = _seg()
    lengths = _lengths(seg)
    F = len(lengths)
    rng = np.random.RandomState(500 + stride)
    K, Rt = _calib(F)
    boxes, bframe, gt = [], [], []
    for f in range(F):
        boxes += [WHOLE_2D, INNER_2D]
        gt += [MAIN, SECOND]
        bframe += [f, f]
    boxes += [WHOLE_2D, WHOLE_2D]
    gt += [QUARTER, AIR]
    bframe += [F - 1, F - 1]
    boxes, gt, bframe = np.asarray(boxes, dtype=np.float64), np.asarray(gt, dtype=np.float64), np.asarray(bframe, dtype=np.int32)
    q_lo = seg + 2 * (seg // 4)                                      # segment 1, wave 2's quarter of a full segment
    frames = []
    for f, n in enumerate(lengths):
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
                xyz[m] = _inside(rng, int(m.sum()), box)
            m = todo & (owner < 0)
            xyz[m] = _back_project(rng, int(m.sum()), K[f], Rt[f])
            u, v, _ = ref.project(xyz, K[f], Rt[f])
            todo = np.zeros(n, dtype=bool)
            for d in mine:
                todo |= ref.face_distance(xyz, gt[d]) < MARGIN
                todo |= ref.edge_distance(u, v, boxes[d]) < MARGIN_PX
            if not todo.any():
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (n, stride - 3)).astype(np.float32)], 1))
    pts = np.concatenate(frames, 0)
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    big = int(off[-2])
    u, v, _ = ref.project(pts[big:, :3], K[F - 1], Rt[F - 1])
    hit = np.nonzero(ref.box_mask(pts[big:, :3], u, v, boxes[-4]))[0]                # rows the longest frame's wide box selects
    poison = [hit[hit > seg][0], hit[3], hit[hit > 2 * seg][0]]
    pts[big + poison[0], 0], pts[big + poison[1], 1], pts[big + poison[2], 2] = np.nan, np.inf, -np.inf
    if stride > 3:
        pts[big + hit[len(hit) // 2]:big + hit[len(hit) // 2] + 1, 3].view(np.uint32)[0] = NAN_PAYLOAD
    out = ref.select(pts, off, K, Rt, boxes, bframe, gt)
    S = 3
    out["seg_cnt"] = _seg_counts(out["index"], S, seg)
    out["seg_pos"] = _seg_counts([ix[sg > 0] for ix, sg in zip(out["index"], out["seg"])], S, seg)
    D = len(bframe)
    wide, quarter, air = D - 4, D - 2, D - 1                         # the longest frame's wide box, QUARTER, AIR
    assert not set(poison) & set(out["index"][wide].tolist())        # the non-finite rows are never selected
    assert min(e.min() for e in out["face"] if len(e)) >= MARGIN and min(e.min() for e in out["edge"] if len(e)) >= MARGIN_PX
    assert (out["seg_pos"][wide] > 0).all() and (out["seg_pos"][wide] % 64 != 0).all() and (out["seg_cnt"][wide] % 64 != 0).all()
    assert (out["seg_pos"][wide + 1] > 0).all() and (out["seg_pos"][wide + 1] < out["seg_cnt"][wide + 1]).all()
    assert out["counts"][wide] < lengths[-1]                          # (not everything is selected)
    qi = out["index"][quarter][out["seg"][quarter] > 0]
    assert len(qi) > 10 and qi.min() >= q_lo and qi.max() < q_lo + seg // 4                # one wave's quarter only
    assert out["pos"][air] == 0 and out["counts"][air] > seg
    assert out["pos"][2] == 1 and out["counts"][2] == 1 and out["counts"][0] == 0          # the frames of 1 and 0 rows
    assert any((dep < 0).any() for dep in out["depth"])                                      # rows behind the camera
    return {"pts": pts, "off": off, "K": K, "Rt": Rt, "boxes": boxes, "bframe": bframe, "gt": gt, "ref": out, "S": S, "seg": seg,
            "lengths": lengths, "wide": wide, "quarter": quarter, "air": air}


KEYS = ("pts", "off", "K", "Rt", "boxes", "bframe", "gt")


def _tensors(sc, shift=0, **over):
    t = {k: _dev(over.get(k, sc[k])) for k in KEYS}
    if shift:                                                        # the same rows, `shift` bytes behind a 16-byte boundary
        n, ps = t["pts"].shape
        w = shift // 4
        buf = torch.zeros((n * ps + 4,), dtype=torch.float32, device="cuda")
        buf[w:w + n * ps] = t["pts"].reshape(-1)
        t["pts"] = buf[w:w + n * ps].view(n, ps)
        assert t["pts"].data_ptr() % 16 == shift
    return t


def _common(t, S, ps=None):
    return [_p(t["pts"]), _p(t["off"]), t["off"].numel() - 1, t["pts"].shape[1] if ps is None else ps, _p(t["K"]), _p(t["Rt"]),
            _p(t["boxes"]), _p(t["bframe"]), t["bframe"].numel(), S]


def _count(t, S, label=True):
    """The raw count on device tensors -> rc, outputs (sentinel-filled first)."""
    from frustum_convnet_amd import _native
    D = t["bframe"].numel()
    f64 = dict(dtype=torch.float64, device="cuda")
    o = {"angle": torch.full((D,), -7.0, **f64), "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda")}
    if label:
        o.update(spos=torch.full((D, S), -7, dtype=torch.int32, device="cuda"), corners=torch.full((D, 24), -7.0, **f64))
        rc = _native.lib().fcn_frustum_sunrgbd_label_count(*_common(t, S), _p(t["gt"]), _p(o["angle"]), _p(o["scnt"]), _p(o["spos"]),
                                                           _p(o["corners"]), _native.current_stream())
    else:
        rc = _native.lib().fcn_frustum_sunrgbd_count(*_common(t, S), _p(o["angle"]), _p(o["scnt"]), _native.current_stream())
    torch.cuda.synchronize()
    return rc, o


def _fill(t, S, seg_counts, label=True, guard=5):
    """The raw fill -> rc, rows, labels (None unlabelled), the `guard` poisoned entries behind each, seg_off."""
    from frustum_convnet_amd import _native
    ps = t["pts"].shape[1]
    soff = np.concatenate([[0], np.cumsum(np.asarray(seg_counts).reshape(-1))]).astype(np.int64)
    n = int(soff[-1])
    out = torch.full((n + guard, ps), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((n + guard,), -7, dtype=torch.int64, device="cuda")
    soff_d = _dev(soff)
    if label:
        rc = _native.lib().fcn_frustum_sunrgbd_label_fill(*_common(t, S), _p(t["gt"]), _p(soff_d), _p(out), _p(oseg),
                                                          _native.current_stream())
    else:
        rc = _native.lib().fcn_frustum_sunrgbd_fill(*_common(t, S), _p(soff_d), _p(out), _native.current_stream())
    torch.cuda.synchronize()
    out, oseg = out.cpu().numpy(), oseg.cpu().numpy()
    return rc, out[:n], oseg[:n], (out[n:], oseg[n:]), soff


def _guards_intact(guard, label=True):
    return bool((guard[0] == -7.0).all() and ((guard[1] == -7).all()))


def _same_rows(got, want, what=""):
    """Bit-identical, every column: the xyz of a stored row are the input's bits under a swap and a sign."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), what


@pytest.mark.parametrize("stride", STRIDES, ids=[str(s) for s in STRIDES])
def test_entry_points_match_the_referee(stride):
    stride, shift = (int(x) for x in stride.split("+")) if isinstance(stride, str) else (stride, 0)
    sc = _scene(stride)
    out, S = sc["ref"], sc["S"]
    t = _tensors(sc, shift=shift)
    rc, o = _count(t, S)
    assert rc == 0
    scnt, spos = o["scnt"].cpu().numpy(), o["spos"].cpu().numpy()
    print("cnt", scnt.sum(1).tolist(), "pos", spos.sum(1).tolist(), "referee pos", out["pos"].tolist())
    assert np.array_equal(scnt, out["seg_cnt"]) and np.array_equal(spos, out["seg_pos"])       # per segment
    aerr = np.abs(o["angle"].cpu().numpy() - out["frustum_angle"])
    cerr = np.abs(o["corners"].cpu().numpy().reshape(-1, 8, 3) - out["corners"])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all()
    assert np.abs(out["corners"]).max() < 100.0
    rc, rows, seg, guard, soff = _fill(t, S, scnt)
    assert rc == 0 and _guards_intact(guard)
    _same_rows(rows, np.concatenate(out["rows"], 0), "stride %d + %d bytes" % (stride, shift))
    assert seg.dtype == np.int64 and np.array_equal(seg, np.concatenate(out["seg"]))
    assert np.array_equal(soff[::S], np.concatenate([[0], np.cumsum(out["counts"])]))
    if rows.shape[1] > 3:
        assert (_bits(rows[:, 3]) == NAN_PAYLOAD).sum() >= 1                                     # the payload came through
    rc2, rows2, seg2, _, _ = _fill(t, S, scnt)
    rc3, o3 = _count(t, S)
    assert rc2 == 0 and np.array_equal(_bits(rows2), _bits(rows)) and np.array_equal(seg2, seg)  # identical over two runs
    assert rc3 == 0 and all(torch.equal(o3[k], o[k]) for k in o)
    # the unlabelled pair on the same inputs: the same counts, angles and rows, bit for bit
    rc, so = _count(t, S, label=False)
    assert rc == 0 and torch.equal(so["scnt"], o["scnt"]) and torch.equal(so["angle"], o["angle"])
    rc, srows, sseg, sguard, _ = _fill(t, S, scnt, label=False)
    assert rc == 0 and np.array_equal(_bits(srows), _bits(rows)) and (sseg == -7).all() and _guards_intact(sguard)
    # more segments than any frame needs: the surplus ones count 0
    rc, o5 = _count(t, S + 2)
    assert rc == 0 and np.array_equal(o5["spos"].cpu().numpy()[:, :S], out["seg_pos"]) and (o5["spos"].cpu().numpy()[:, S:] == 0).all()
    assert np.array_equal(o5["scnt"].cpu().numpy()[:, :S], out["seg_cnt"]) and (o5["scnt"].cpu().numpy()[:, S:] == 0).all()


def test_points_exactly_on_a_face_are_inside_and_one_step_out_is_outside():
    """An axis-aligned box (heading 0: cos and sin are exact) with dyadic centroid and half extents, identity Rtilt and a plain
    pinhole K.  Per face: one float32 step inside, exactly on it, one step outside -> 1, 1, 0."""
    gt = np.asarray([[0.5, 4.0, 0.5, 1.0, 0.5, 0.25, 0.0]])          # x in [-0.5, 1.5], y in [3.5, 4.5], z in [0.25, 0.75]
    centre = np.asarray([0.5, 4.0, 0.5], dtype=np.float32)
    rows, want = [], []
    for axis, (lo, hi) in enumerate(((-0.5, 1.5), (3.5, 4.5), (0.25, 0.75))):
        for face, outward in ((lo, -np.inf), (hi, np.inf)):
            f32 = np.float32(face)
            assert float(f32) == face
            for val, inside in ((np.nextafter(f32, np.float32(-outward)), 1), (f32, 1), (np.nextafter(f32, np.float32(outward)), 0)):
                p = centre.copy()
                p[axis] = val
                rows.append(p)
                want.append(inside)
    pts = np.concatenate([np.asarray(rows, dtype=np.float32), np.full((len(rows), 3), 0.5, dtype=np.float32)], 1)
    want = np.asarray(want, dtype=np.int64)
    sc = {"pts": pts, "off": np.asarray([0, len(pts)], dtype=np.int64), "K": np.asarray([[[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]]]),
          "Rt": np.eye(3)[None], "boxes": np.asarray([[0.0, 0.0, 640.0, 480.0]]), "bframe": np.zeros(1, dtype=np.int32), "gt": gt}
    assert np.array_equal(ref.in_box(pts[:, :3], gt[0]).astype(np.int64), want)                     # (the referee says the same)
    assert want.sum() == 12 and len(want) == 18
    t = _tensors(sc)
    rc, o = _count(t, 1)
    assert rc == 0 and o["scnt"].cpu().numpy().tolist() == [[18]] and o["spos"].cpu().numpy().tolist() == [[12]]
    rc, got, seg, guard, _ = _fill(t, 1, [[18]])
    assert rc == 0 and _guards_intact(guard)
    _same_rows(got, ref.to_upright_camera(pts))
    assert np.array_equal(seg, want)
    assert np.array_equal(o["corners"].cpu().numpy().reshape(8, 3), ref.corners(gt[0]))             # cos 0, sin 0: exact


def test_slices_bound_both_stores():
    """seg_off bounds the writes to out_pts AND out_seg: with offsets that grant one segment 100 rows fewer than it selects and
    one box no row at all, both buffers hold the slices and nothing else; the poisoned entries behind are unchanged."""
    sc = _scene(6)
    S, seg, out = sc["S"], sc["seg"], sc["ref"]
    t = _tensors(sc)
    counts = out["seg_cnt"].copy()
    d, s, none = sc["wide"], 1, sc["wide"] + 1
    assert counts[d, s] > 200 and counts[none].sum() > 0 and out["pos"][none] > 0
    counts[d, s] -= 100
    counts[none] = 0                                                 # (how the host leaves a rejected box out)
    for label in (True, False):
        rc, rows, lab, guard, soff = _fill(t, S, counts, label=label)
        assert rc == 0 and _guards_intact(guard)
        assert len(rows) == out["counts"].sum() - 100 - out["counts"][none] == len(lab)
        for dd in range(len(counts)):
            for ss in range(S):
                i = dd * S + ss
                m = (out["index"][dd] // seg) == ss
                _same_rows(rows[soff[i]:soff[i + 1]], out["rows"][dd][m][:counts[dd, ss]])
                if label:
                    assert np.array_equal(lab[soff[i]:soff[i + 1]], out["seg"][dd][m][:counts[dd, ss]]), (dd, ss)
        # every box granted nothing: nothing is written at all
        rc, rows, lab, guard, _ = _fill(t, S, np.zeros_like(counts), label=label)
        assert rc == 0 and len(rows) == 0 and len(lab) == 0 and _guards_intact(guard)


def test_bad_arguments_are_refused_with_nothing_written():
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
    for label in (True, False):                                      # S too small for the longest frame: refused, nothing launched
        rc, ob = _count(t, S - 1, label=label)
        assert rc == BADARG and all((ob[k].cpu().numpy() == -7).all() for k in ob)
    f64 = dict(dtype=torch.float64, device="cuda")
    w = {"angle": torch.full((D,), -7.0, **f64), "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
         "spos": torch.full((D, S), -7, dtype=torch.int32, device="cuda"), "corners": torch.full((D, 24), -7.0, **f64)}
    sizes = ((3, 2), (9, 0), (9, -1), (8, -1), (2, -1), (8, 65536))   # pt_stride 2, S < 1, negative sizes, D > 65535
    good = _common(t, S) + [_p(t["gt"]), _p(w["angle"]), _p(w["scnt"]), _p(w["spos"]), _p(w["corners"]), s]
    goodu = _common(t, S) + [_p(w["angle"]), _p(w["scnt"]), s]
    for fn, lst, nulls in ((L.fcn_frustum_sunrgbd_label_count, good, (0, 1, 4, 5, 6, 7, 10, 11, 12, 13, 14)),
                           (L.fcn_frustum_sunrgbd_count, goodu, (0, 1, 4, 5, 6, 7, 10, 11))):
        for i in nulls:                                              # NULL pointers
            bad = list(lst)
            bad[i] = None
            assert fn(*bad) == BADARG, i
        for i, v in sizes:
            bad = list(lst)
            bad[i] = v
            assert fn(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((w[k].cpu().numpy() == -7).all() for k in w)               # nothing written by any of them
    assert L.fcn_frustum_sunrgbd_label_count(*good) == 0                   # (the same list is accepted when nothing is wrong)
    torch.cuda.synchronize()
    assert torch.equal(w["spos"], o["spos"]) and torch.equal(w["corners"], o["corners"])
    soff = _dev(np.concatenate([[0], np.cumsum(scnt.reshape(-1))]).astype(np.int64))
    out = torch.full((int(scnt.sum()), 3), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((int(scnt.sum()),), -7, dtype=torch.int64, device="cuda")
    goodf = _common(t, S) + [_p(t["gt"]), _p(soff), _p(out), _p(oseg), s]
    goodfu = _common(t, S) + [_p(soff), _p(out), s]
    for fn, lst, nulls in ((L.fcn_frustum_sunrgbd_label_fill, goodf, (0, 1, 4, 5, 6, 7, 10, 11, 12, 13)),
                           (L.fcn_frustum_sunrgbd_fill, goodfu, (0, 1, 4, 5, 6, 7, 10, 11))):
        for i in nulls:
            bad = list(lst)
            bad[i] = None
            assert fn(*bad) == BADARG, i
        for i, v in sizes + ((9, S - 1),):
            bad = list(lst)
            bad[i] = v
            assert fn(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (oseg.cpu().numpy() == -7).all()
    assert L.fcn_frustum_sunrgbd_label_fill(*goodf) == 0
    torch.cuda.synchronize()
    assert np.array_equal(oseg.cpu().numpy(), np.concatenate(sc["ref"]["seg"]))
    # fcn_frustum_subset_pos
    pos = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    z64, z32 = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int32, device="cuda")
    goods = [_p(z64), _p(z64), _p(z32), _p(z32), _p(z64), 2, _p(pos), s]
    for i in (0, 1, 2, 3, 4, 6):
        bad = list(goods)
        bad[i] = None
        assert L.fcn_frustum_subset_pos(*bad) == BADARG, i
    bad = list(goods)
    bad[5] = -1
    assert L.fcn_frustum_subset_pos(*bad) == BADARG
    torch.cuda.synchronize()
    assert (pos.cpu().numpy() == -7).all()
    bad[5] = 0
    assert L.fcn_frustum_subset_pos(*bad) == 0 and (pos.cpu().numpy() == -7).all()     # U == 0 touches nothing


@pytest.mark.parametrize("what", ["frame_high", "frame_negative"])
def test_out_of_range_box_frame_is_reported_and_never_dereferenced(what):
    from frustum_convnet_amd import frustum, _native
    sc = _scene(6)
    S, out = sc["S"], sc["ref"]
    F = len(sc["lengths"])
    bframe = sc["bframe"].copy()
    bad = sc["wide"]
    bframe[bad] = F if what == "frame_high" else -1
    t = _tensors(sc, bframe=bframe)                                  # exactly sized buffers: nothing beyond them can be read
    ok = np.arange(len(bframe)) != bad
    for label in (True, False):
        rc, o = _count(t, S, label=label)
        assert rc == BADARG
        scnt = o["scnt"].cpu().numpy()
        want_c, want_p = out["seg_cnt"].copy(), out["seg_pos"].copy()
        want_c[bad], want_p[bad] = 0, 0
        assert np.array_equal(scnt, want_c)                          # its counts are 0, every other box is processed
        ang = o["angle"].cpu().numpy()
        assert ang[bad] == -7.0 and (np.abs(ang[ok] - out["frustum_angle"][ok]) <= 1e-12).all()
        if label:
            cor = o["corners"].cpu().numpy()
            assert np.array_equal(o["spos"].cpu().numpy(), want_p) and (cor[bad] == -7.0).all()      # nothing else of it is written
            assert (np.abs(cor[ok].reshape(-1, 8, 3) - out["corners"][ok]) <= 1e-12).all()
        rc, rows, lab, guard, _ = _fill(t, S, scnt, label=label)
        assert rc == BADARG and _guards_intact(guard)
        _same_rows(rows, np.concatenate([r for d, r in enumerate(out["rows"]) if d != bad], 0), what)
        if label:
            assert np.array_equal(lab, np.concatenate([r for d, r in enumerate(out["seg"]) if d != bad]))
    with pytest.raises(_native.NativeError):
        frustum.sunrgbd_training_candidates(t["pts"], t["off"], t["K"], t["Rt"], t["boxes"], t["bframe"], t["gt"])
    with pytest.raises(_native.NativeError):
        frustum.sunrgbd_candidates(t["pts"], t["off"], t["K"], t["Rt"], t["boxes"], t["bframe"])


def test_subset_pos_equals_numpy():
    """Units with and without a subsample, one of a single index, one whose subsample repeats an index, sizes on both sides of the
    workgroup's stride; an out-of-range index is skipped, never dereferenced (the label buffer is exactly sized)."""
    from frustum_convnet_amd import _native
    rng = np.random.RandomState(11)
    cnt = np.asarray([300, 1, 255, 257, 5000, 0, 64], dtype=np.int32)
    starts = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.int64)
    seg = (rng.uniform(size=int(cnt.sum())) < 0.3).astype(np.int64)
    sub = [rng.choice(300, 100, replace=False), None, rng.choice(255, 255, replace=False), np.asarray([256]),
           rng.choice(5000, 2048, replace=False), None, np.asarray([3, 3, 3, 70, -1, 64])]
    lens = [0 if x is None else len(x) for x in sub]
    sub_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    flat = np.concatenate([x for x in sub if x is not None]).astype(np.int32)
    want = []
    for u in range(len(cnt)):
        mine = seg[starts[u]:starts[u] + cnt[u]]
        ix = np.arange(cnt[u]) if sub[u] is None else np.asarray([k for k in sub[u] if 0 <= k < cnt[u]], dtype=np.int64)
        want.append(int(mine[ix].sum()))
    assert want[0] > 0 and want[4] > 100 and want[5] == 0
    pos = torch.full((len(cnt) + 3,), -7, dtype=torch.int32, device="cuda")
    d = [_dev(x) for x in (seg, starts, cnt, flat, sub_off)]
    rc = _native.lib().fcn_frustum_subset_pos(*[_p(x) for x in d], len(cnt), _p(pos), _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and pos.cpu().numpy()[:len(cnt)].tolist() == want and (pos.cpu().numpy()[len(cnt):] == -7).all()


def _fixture_inputs(g, which):
    dev = {k: _dev(g[k]) for k in ("points", "off", "K", "Rtilt")}
    if which == "train":
        rep = np.repeat(g["gt_box3d"], int(g["meta_augment"]), 0)
        return dev, g["train_boxes"], g["train_box_frame"], rep
    return dev, g["det_boxes"], g["det_frame"], None


def _train_sel():
    from frustum_convnet_amd import frustum
    g = _golden()
    dev, boxes, bframe, gt = _fixture_inputs(g, "train")
    sel = frustum.sunrgbd_training_candidates(dev["points"], dev["off"], dev["K"], dev["Rtilt"], boxes, bframe, gt,
                                              sub=ref.fixture_sub(g, "train"))
    return g, dev, sel


def _det_sel():
    from frustum_convnet_amd import frustum
    g = _golden()
    dev, boxes, bframe, _ = _fixture_inputs(g, "det")
    sel = frustum.sunrgbd_candidates(dev["points"], dev["off"], dev["K"], dev["Rtilt"], boxes, bframe, sub=ref.fixture_sub(g, "det"))
    return g, dev, sel


def _frame_rows(g, d_frame, index):
    """The reference's record rows from its stored indices: the frame's rows, in upright camera coordinates."""
    return ref.to_upright_camera(g["points"][int(g["off"][d_frame]):int(g["off"][d_frame + 1])][index])


def test_training_candidates_equal_the_references_recorded_run():
    """sunrgbd_training_candidates on the fixture's frames, recorded perturbed boxes and recorded subsample draws against what the
    reference's own extract_frustum_data pickled: the kept boxes, rows, labels, the float32 box2d, corners, angles."""
    g, dev, sel = _train_sel()
    kept = g["train_kept"]
    K = len(kept)
    assert np.array_equal(sel["kept"], kept) and sel["kept"].dtype == np.int64 and 0 < K < len(g["train_boxes"])
    recs = ref.fixture_records(g, "train")
    off_h, cnt_h = sel["off"].cpu().numpy(), sel["cnt"].cpu().numpy()
    pts_h, seg_h = sel["points"].cpu().numpy(), sel["seg"].cpu().numpy()
    assert sel["points"].dtype == torch.float32 and sel["seg"].dtype == torch.int64 and sel["off"].dtype == torch.int64
    assert off_h.shape == (K + 1,) and off_h[-1] == len(pts_h) == len(seg_h) and np.array_equal(cnt_h, sel["counts"])
    pos_h = sel["pos"].cpu().numpy()
    for k, (d, index, label) in enumerate(recs):
        rows, lab = pts_h[off_h[k]:off_h[k] + cnt_h[k]], seg_h[off_h[k]:off_h[k] + cnt_h[k]]
        pick = slice(None) if sel["sub"][k] is None else sel["sub"][k]
        _same_rows(rows[pick], _frame_rows(g, int(g["train_box_frame"][d]), index), "box %d" % d)
        assert np.array_equal(lab[pick], label) and pos_h[k] == label.sum(), d
        assert (sel["sub"][k] is None) == (cnt_h[k] <= int(g["meta_cap"]))
    assert np.array_equal(sel["box2d"].cpu().numpy(), g["train_box2d"].astype(np.float64))          # the float32 value, widened
    assert not np.array_equal(sel["box2d"].cpu().numpy(), g["train_boxes"][kept])
    assert np.array_equal(sel["box_frame"].cpu().numpy(), g["train_box_frame"][kept]) and sel["box_frame"].dtype == torch.int32
    assert np.array_equal(sel["heading"].cpu().numpy(), g["train_heading"]) and np.array_equal(sel["size"].cpu().numpy(), g["train_size"])
    aerr = np.abs(sel["frustum_angle"].cpu().numpy() - g["train_angle"])
    cerr = np.abs(sel["box3d"].cpu().numpy() - g["train_box3d"])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all() and sel["box3d"].shape == (K, 8, 3)
    for k in ("box2d", "frustum_angle", "box3d", "heading", "size"):
        assert sel[k].dtype == torch.float64 and sel[k].is_cuda, k
    assert sel["cnt"].dtype == torch.int32 and sel["pos"].dtype == torch.int32 and sel["counts"].dtype == np.int64
    assert sorted(sel.keys()) == sorted(["points", "seg", "off", "box2d", "frustum_angle", "box3d", "heading", "size", "box_frame",
                                         "cnt", "pos", "kept", "counts", "sub"])
    # the three ways a box leaves: fewer than 5 positives in all; 5 or more of which its subsample keeps fewer (its rows stay in
    # the packed buffer, unlisted); and, drawn here instead of handed in, the same rule under other draws
    gone = set(range(len(g["train_boxes"]))) - set(kept.tolist())
    assert set(g["meta_few"].tolist()) <= gone and set(g["meta_subfew"][g["meta_subfew_dropped"]].tolist()) <= gone
    assert len(pts_h) > cnt_h.sum()
    from frustum_convnet_amd import frustum
    dv, boxes, bframe, gt = _fixture_inputs(g, "train")
    np.random.seed(3)
    sel2 = frustum.sunrgbd_training_candidates(dv["points"], dv["off"], dv["K"], dv["Rtilt"], boxes, bframe, gt)
    np.random.seed(3)
    want_sub = frustum.draw_frustum_subsample(ref.select(g["points"], g["off"], g["K"], g["Rtilt"], boxes, bframe)["counts"])
    assert all((a is None) == (want_sub[d] is None) and (a is None or np.array_equal(a, want_sub[d])) for a, d in zip(sel2["sub"], sel2["kept"]))
    assert set(kept.tolist()) - set(g["meta_big"].tolist()) <= set(sel2["kept"].tolist())
    with pytest.raises(ValueError):
        bad = ref.fixture_sub(g, "train")
        bad[int(g["meta_big"][0])] = np.asarray([0, 10 ** 6])
        frustum.sunrgbd_training_candidates(dv["points"], dv["off"], dv["K"], dv["Rtilt"], boxes, bframe, gt, sub=bad)


def test_candidates_equal_the_references_recorded_run():
    g, dev, sel = _det_sel()
    D = len(g["det_boxes"])
    mine = ref.select(g["points"], g["off"], g["K"], g["Rtilt"], g["det_boxes"], g["det_frame"])
    assert np.array_equal(sel["counts"], mine["counts"]) and np.array_equal(sel["cnt"].cpu().numpy(), mine["counts"])
    off_h, pts_h = sel["off"].cpu().numpy(), sel["points"].cpu().numpy()
    assert np.array_equal(off_h, np.concatenate([[0], np.cumsum(mine["counts"])])) and sel["off"].dtype == torch.int64
    assert np.array_equal(sel["box2d"].cpu().numpy(), g["det_boxes"])                              # unrounded
    for k, (d, index, _) in enumerate(ref.fixture_records(g, "det")):
        rows = pts_h[off_h[d]:off_h[d + 1]]
        pick = slice(None) if sel["sub"][d] is None else sel["sub"][d]
        _same_rows(rows[pick], _frame_rows(g, int(g["det_frame"][d]), index), "detection %d" % d)
        assert abs(float(sel["frustum_angle"][d]) - g["det_angle"][k]) <= 1e-12
    assert sorted(sel.keys()) == sorted(["points", "off", "box2d", "frustum_angle", "cnt", "box_frame", "counts", "sub"])
    assert len(sel["sub"]) == D and sum(x is not None for x in sel["sub"]) == 2


def _builder(g, flip, shift):
    from frustum_convnet_amd.config import reset_cfg
    from frustum_convnet_amd.inputs import SunrgbdInputBuilder
    reset_cfg()
    return SunrgbdInputBuilder(int(g["meta_npoint"]), tuple(g["meta_strides"]), float(g["meta_max_depth"]), random_flip=flip,
                               random_shift=shift)


def _close(got, want, key):
    """The bar of test_gpu_inputs.py::test_sunrgbd_builder_matches_reference_batch."""
    assert got.shape == want.shape and got.dtype == np.float32, key
    d = np.abs(got.astype(np.float64) - want.astype(np.float64)).max()
    assert d <= 1e-6 * max(1.0, np.abs(want).max()), (key, d)


def _records(sel, g, types, boxes_key):
    """Host records of build() from the DOWNLOADED candidates: each box's rows with its subsample applied."""
    pts_h, off_h, cnt_h = sel["points"].cpu().numpy(), sel["off"].cpu().numpy(), sel["cnt"].cpu().numpy()
    seg_h = sel["seg"].cpu().numpy()
    box_h, ang_h, cor_h = sel["box2d"].cpu().numpy(), sel["frustum_angle"].cpu().numpy(), sel["box3d"].cpu().numpy()
    head_h, size_h, bf_h = sel["heading"].cpu().numpy(), sel["size"].cpu().numpy(), sel["box_frame"].cpu().numpy()
    recs = []
    for k, d in enumerate(sel["kept"]):
        pick = slice(None) if sel["sub"][k] is None else sel["sub"][k]
        recs.append({"points": pts_h[off_h[k]:off_h[k] + cnt_h[k]][pick], "seg": seg_h[off_h[k]:off_h[k] + cnt_h[k]][pick],
                     "box2d": box_h[k], "K": g["K"][bf_h[k]], "Rtilt": g["Rtilt"][bf_h[k]], "box3d": cor_h[k],
                     "heading": float(head_h[k]), "size": size_h[k], "frustum_angle": float(ang_h[k]), "type": types[d]})
    return recs


def test_build_device_train_equals_the_loaders_batch_and_build():
    """SunrgbdInputBuilder.build_device_train with the recorded draws against the batch the reference's own ProviderDataset +
    default_collate made of the reference's own pickle, at the bars of test_sunrgbd_builder_matches_reference_batch; and against
    build() on host records made from the same selection: every key bit-identical."""
    g, dev, sel = _train_sel()
    b = _builder(g, True, True)
    types = [str(x) for x in g["train_types"]]
    draws = (g["train_draw_choice"], g["train_draw_coin"], g["train_draw_normal"], g["train_draw_hshift"])
    rows = np.asarray([c if s is None else len(s) for c, s in zip(sel["counts"], sel["sub"])])
    assert (rows < b.npoints).any() and (rows > b.npoints).any() and (rows == int(g["meta_cap"])).any()
    assert (draws[1] > 0.5).any() and (draws[1] <= 0.5).any()
    got = b.build_device_train(sel, dev["K"], dev["Rtilt"], types, draws=draws)
    torch.cuda.synchronize()
    for k in ("cls_label", "seg_label", "size_class", "one_hot"):
        assert torch.equal(got[k].cpu(), torch.from_numpy(g["train_batch_" + k])), k
    for k in FLOAT_KEYS:
        _close(got[k].cpu().numpy(), g["train_batch_" + k], k)
    assert sorted(got.keys()) == sorted(k[len("train_batch_"):] for k in g if k.startswith("train_batch_"))
    want = b.build(_records(sel, g, types, "train"), draws=draws)
    torch.cuda.synchronize()
    assert sorted(got.keys()) == sorted(want.keys())
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    got2 = b.build_device_train(sel, dev["K"], dev["Rtilt"], types, draws=draws, with_seg=False)
    assert "seg_label" not in got2 and torch.equal(got2["point_cloud"].cpu(), want["point_cloud"].cpu())
    np.random.seed(5)                                                 # drawn like the reference when no draws are given
    got3 = b.build_device_train(sel, dev["K"], dev["Rtilt"], types)
    np.random.seed(5)
    want3 = b.build(_records(sel, g, types, "train"))
    assert all(torch.equal(got3[k].cpu(), want3[k].cpu()) for k in want3)


def test_build_device_equals_the_loaders_batch():
    """build_device with the recorded draws against the reference loader's from_rgb_detection batch of the reference's own
    detection pickle: the skipped detection (fewer than 5 rows), the subsampled ones, every key."""
    g, dev, sel = _det_sel()
    b = _builder(g, False, False)
    types, prob = [str(x) for x in g["det_types"]], g["det_prob"]
    got = b.build_device(sel, dev["K"], dev["Rtilt"], types, prob, draws=(g["det_draw_choice"],))
    torch.cuda.synchronize()
    assert np.array_equal(got["kept"], g["det_kept"]) and int(g["meta_det_tiny"]) not in got["kept"]
    assert sorted(k for k in got if k != "kept") == sorted(k[len("det_batch_"):] for k in g if k.startswith("det_batch_"))
    assert torch.equal(got["one_hot"].cpu(), torch.from_numpy(g["det_batch_one_hot"]))
    assert torch.equal(got["rgb_prob"].cpu(), torch.from_numpy(g["det_batch_rgb_prob"]))
    for k in ("point_cloud", "rot_angle", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "center_ref5"):
        _close(got[k].cpu().numpy(), g["det_batch_" + k], k)
    np.random.seed(9)                                                 # drawn from the RECORDS' row counts when no draws are given
    got2 = b.build_device(sel, dev["K"], dev["Rtilt"], types, prob)
    np.random.seed(9)
    from frustum_convnet_amd import inputs
    rows = np.minimum(sel["counts"], int(g["meta_cap"]))[got["kept"]]
    got3 = b.build_device(sel, dev["K"], dev["Rtilt"], types, prob, draws=inputs.draw_sunrgbd(rows, b.npoints, False, False))
    assert torch.equal(got2["point_cloud"].cpu(), got3["point_cloud"].cpu())
    with pytest.raises(ValueError):
        b.build_device(sel, dev["K"], dev["Rtilt"], types[:-1], prob)


def test_one_training_step_on_the_device_built_batch():
    """The five-scale model with hash-initialised weights: the losses from the build_device_train batch equal those from the
    build(records) batch bit for bit, are finite, and backward() runs."""
    from frustum_convnet_amd.config import cfg, reset_cfg
    from frustum_convnet_amd import det_base_sunrgbd, frustum, synth
    g = _golden()
    dev, boxes, bframe, gt = _fixture_inputs(g, "train")
    use = np.asarray([0, 2, 10])                                      # three of the kept boxes, a subsampled one among them
    pick = g["train_kept"][use]
    sub = ref.fixture_sub(g, "train")
    sel = frustum.sunrgbd_training_candidates(dev["points"], dev["off"], dev["K"], dev["Rtilt"], boxes[pick], bframe[pick], gt[pick],
                                              sub=[sub[d] for d in pick])
    assert len(sel["kept"]) == 3 and sel["sub"][2] is not None and sel["sub"][0] is None
    b = _builder(g, True, True)
    cfg.DATA.HEIGHT_HALF = tuple(float(x) for x in g["meta_strides"])
    cfg.DATA.STRIDE = cfg.DATA.HEIGHT_HALF
    cfg.DATA.DATASET_NAME = "SUNRGBD"
    cfg.DATA.MAX_DEPTH = float(g["meta_max_depth"])
    try:
        types = [str(x) for x in g["train_types"][pick]]
        draws = tuple(g["train_draw_" + k][use] for k in ("choice", "coin", "normal", "hshift"))
        m = det_base_sunrgbd.PointNetDet(3, num_vec=10, num_classes=2)
        synth.fill_state_dict(m.state_dict(), seed=7)
        m = m.cuda().train()
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        losses, _ = m(b.build_device_train(sel, dev["K"], dev["Rtilt"], types, draws=draws))
        losses["total_loss"].backward()
        torch.cuda.synchronize()
        grads = [p.grad for p in m.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(x).all() for x in grads)
        got = {k: v.detach().cpu().clone() for k, v in losses.items()}
        m.load_state_dict(sd)                                         # (the running statistics moved)
        losses2, _ = m(b.build(_records(sel, g, types, "train"), draws=draws))
        torch.cuda.synchronize()
        print({k: float(v) for k, v in got.items()})
        for k, v in losses2.items():
            assert torch.isfinite(got[k]).all() and torch.equal(got[k], v.detach().cpu()), k
        assert float(got["total_loss"]) > 0
    finally:
        reset_cfg()


def test_empty_results_launch_nothing_behind_them():
    from frustum_convnet_amd import frustum, _native
    g = _golden()
    dev, boxes, bframe, gt = _fixture_inputs(g, "train")
    sub = ref.fixture_sub(g, "train")
    few = g["meta_few"]
    L = _native.lib()
    calls = []
    names = ("fcn_frustum_sunrgbd_label_fill", "fcn_frustum_sunrgbd_fill", "fcn_frustum_subset_pos", "fcn_prepare_inputs_sunrgbd",
             "fcn_prepare_inputs_sunrgbd_infer")
    real = {n: getattr(L, n) for n in names}
    args = (dev["points"], dev["off"], dev["K"], dev["Rtilt"])
    try:
        for n in names:
            setattr(L, n, (lambda n: lambda *a: calls.append(n) or real[n](*a))(n))
        # only boxes under the bar before the fill: 'kept' alone, and neither the fill nor the recount is launched
        sel = frustum.sunrgbd_training_candidates(*args, boxes[few], bframe[few], gt[few])
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and sel["kept"].dtype == np.int64 and calls == []
        # only boxes that fall under it after their subsample: filled, recounted, and then 'kept' alone
        lost = g["meta_subfew"][g["meta_subfew_dropped"]]
        sel = frustum.sunrgbd_training_candidates(*args, boxes[lost], bframe[lost], gt[lost], sub=[sub[d] for d in lost])
        assert list(sel.keys()) == ["kept"] and calls == ["fcn_frustum_sunrgbd_label_fill", "fcn_frustum_subset_pos"]
        del calls[:]
        # no box is subsampled: no recount
        small = g["train_kept"][:2]
        sel = frustum.sunrgbd_training_candidates(*args, boxes[small], bframe[small], gt[small])
        assert len(sel["kept"]) == 2 and calls == ["fcn_frustum_sunrgbd_label_fill"]
        del calls[:]
        # D = 0, and F = 0: no frame to search
        sel = frustum.sunrgbd_training_candidates(*args, np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros((0, 7)))
        assert list(sel.keys()) == ["kept"] and calls == []
        none = (torch.zeros((0, 6), dtype=torch.float32, device="cuda"), np.zeros(1, np.int64), np.zeros((0, 9)), np.zeros((0, 9)))
        sel = frustum.sunrgbd_training_candidates(*none, boxes[:2], np.zeros(2, np.int32), gt[:2])
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and calls == []
        b = _builder(g, False, False)
        assert list(b.build_device_train(sel, dev["K"], dev["Rtilt"], [])) == ["kept"] and calls == []
        # the inference side: boxes that select nothing -> no fill, and no batch launch behind it
        away = np.asarray([[5000.0, 5000.0, 5100.0, 5100.0]] * 2)
        det = frustum.sunrgbd_candidates(*args, away, np.zeros(2, np.int32))
        assert det["points"].shape == (0, 6) and det["counts"].tolist() == [0, 0] and det["sub"] == [None, None] and calls == []
        assert list(b.build_device(det, dev["K"], dev["Rtilt"], ["bed", "bed"], [0.5, 0.5])) == ["kept"] and calls == []
        det = frustum.sunrgbd_candidates(*none, away, np.zeros(2, np.int32))
        assert det["counts"].tolist() == [0, 0] and calls == []
        det = frustum.sunrgbd_candidates(*args, np.zeros((0, 4)), np.zeros(0, np.int32))
        assert det["points"].shape == (0, 6) and det["off"].cpu().numpy().tolist() == [0] and calls == []
    finally:
        for n in names:
            setattr(L, n, real[n])
    # the entry points themselves: D = 0 touches nothing, F = 0 zeroes the counts, frames that are all empty select nothing
    sc = _scene(3)
    t = _tensors(sc)
    t0 = dict(t, boxes=_dev(np.zeros((0, 4))), bframe=_dev(np.zeros(0, np.int32)), gt=_dev(np.zeros((0, 7))))
    tf = dict(t, off=_dev(np.zeros(1, np.int64)))
    te = dict(t, off=_dev(np.zeros(len(sc["lengths"]) + 1, np.int64)))
    D = t["bframe"].numel()
    for label in (True, False):
        rc, o = _count(t0, sc["S"], label=label)
        assert rc == 0 and o["scnt"].numel() == 0
        rc, rows, lab, guard, _ = _fill(t0, sc["S"], np.zeros((0, sc["S"]), np.int64), label=label)
        assert rc == 0 and rows.shape == (0, 3) and _guards_intact(guard)
        rc, o = _count(tf, sc["S"], label=label)
        assert rc == 0 and (o["scnt"].cpu().numpy() == 0).all() and (o["angle"].cpu().numpy() == -7.0).all()
        assert not label or ((o["spos"].cpu().numpy() == 0).all() and (o["corners"].cpu().numpy() == -7.0).all())
        rc, rows, lab, guard, _ = _fill(tf, sc["S"], np.zeros((D, sc["S"]), np.int64), label=label)
        assert rc == 0 and len(rows) == 0 and _guards_intact(guard)
        rc, o = _count(te, sc["S"], label=label)
        assert rc == 0 and (o["scnt"].cpu().numpy() == 0).all() and (np.abs(o["angle"].cpu().numpy() - sc["ref"]["frustum_angle"]) <= 1e-12).all()
        rc, rows, lab, guard, _ = _fill(te, sc["S"], np.zeros((D, sc["S"]), np.int64), label=label)
        assert rc == 0 and len(rows) == 0 and _guards_intact(guard)


def test_infer_entry_point_refuses_bad_arguments():
    from frustum_convnet_amd import _native
    from frustum_convnet_amd._native import Inp5Desc
    B, N, L5 = 2, 8, [4, 3, 2, 2, 1]
    f32 = dict(dtype=torch.float32, device="cuda")
    raw, off = torch.ones((16, 6), **f32), _dev(np.asarray([0, 8, 16], dtype=np.int64))
    choice = torch.zeros((B, N), dtype=torch.int32, device="cuda")
    fang, box = _dev(np.zeros(B)), _dev(np.asarray([[0.0, 0.0, 10.0, 10.0]] * B))
    K, R = _dev(np.tile(np.asarray([500.0, 0, 320, 0, 500, 240, 0, 0, 1]), (B, 1))), _dev(np.tile(np.eye(3).reshape(9), (B, 1)))
    pc, rot = torch.full((B, 3, N), -7.0, **f32), torch.full((B, 1), -7.0, **f32)
    refs_t = [torch.full((B, 3, l), -7.0, **f32) for l in L5]
    refs = (ctypes.c_void_p * 5)(*[r.data_ptr() for r in refs_t])
    mk = lambda **kw: Inp5Desc(kw.get("B", B), kw.get("N", N), kw.get("ps", 6), (ctypes.c_int32 * 5)(*kw.get("L", L5)),
                               (ctypes.c_double * 5)(0.1, 0.2, 0.4, 0.8, 1.6), 8.0, kw.get("flip", 0), kw.get("shift", 0))
    fn = _native.lib().fcn_prepare_inputs_sunrgbd_infer
    s = _native.current_stream()
    good = [_p(raw), _p(off), _p(choice), _p(fang), _p(box), _p(K), _p(R), _p(pc), refs, _p(rot), s]
    for i in (0, 1, 2, 3, 4, 5, 6, 7, 9):
        bad = list(good)
        bad[i] = None
        assert fn(ctypes.byref(mk()), *bad) == BADARG, i
    for kw in (dict(B=0), dict(N=0), dict(ps=2), dict(flip=1), dict(shift=1), dict(L=[4, 3, 0, 2, 1])):
        assert fn(ctypes.byref(mk(**kw)), *good) == BADARG, kw
    torch.cuda.synchronize()
    assert (pc.cpu().numpy() == -7.0).all() and (rot.cpu().numpy() == -7.0).all() and all((r.cpu().numpy() == -7.0).all() for r in refs_t)
    assert fn(ctypes.byref(mk()), *good) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(pc).all() and all(torch.isfinite(r).all() for r in refs_t) and (rot.cpu().numpy() != -7.0).all()
