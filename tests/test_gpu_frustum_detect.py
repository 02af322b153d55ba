"""-m gpu: the capturable inference front -- fcn_frustum_detect_count / _plan / _fill and fcn_frustum_fov_plan
(csrc/frustum_detect_plan.h) through the C-ABI against the numpy restatement of tests/frustum_detect_plan_ref.py (pinned to the
host path by tests/test_frustum_detect_plan_referee.py) and against the reading selection fcn_frustum_select_count / _fill;
frustum.FrameDetectSource against the path it replaces (frustum_candidates + InputBuilder.build_device + image_fov_points) and the
reference's recorded run of tests/golden/frustum_select.npz; cascade.FrameCascade against TwoStageDetector.detect_frames; both under
a captured graph.  Scenes and helpers are those of tests/test_gpu_frustum.py, the models those of tests/test_gpu_cascade.py
(hash-initialised car_b4_n512 and refine_b4_n512, N = 512, top_k = 6).  tests/test_emu_frustum_detect.py runs the same functions on
the host emulation of the kernels (all but the graph captures)."""
import numpy as np
import pytest
import torch

import frustum_detect_plan_ref as R
from test_gpu_frustum import BADARG, _back_project, _bits, _cal, _check_rows, _common, _count, _dev, _fill, _golden, _input_builder, _p
from test_gpu_frustum import _scene, _tensors
from test_gpu_refine_plan import _guarded, _intact

pytestmark = pytest.mark.gpu
LIMIT = 10002                      # FCN_E_LIMIT
SEED = 20241020
TYPES9 = ["Car", "Pedestrian", "Cyclist"] * 3
BATCH_KEYS = ("point_cloud", "rot_angle", "rgb_prob", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "one_hot")


# ------------------------------------------------------------------------------------------------ the plan
PLAN_OUT = (("slot_box", torch.int32, lambda D, S, B: (B,)), ("n_kept", torch.int32, lambda D, S, B: (1,)),
            ("seg_off", torch.int64, lambda D, S, B: (D * S + 1,)), ("off", torch.int64, lambda D, S, B: (B + 1,)),
            ("counts", torch.int64, lambda D, S, B: (B,)))


def _plan_equals(cnt, box, frame, nb, B1, capacity, F, hthr=5.0, pthr=1.0):
    """The raw entry on exactly sized, guarded inputs and poisoned, guarded outputs, held to the restatement (every output is
    poisoned first, so equality also says that every output is written) -> the restatement's tuple."""
    from frustum_convnet_amd import _native
    cnt = np.asarray(cnt)
    D, S = cnt.shape
    o = {k: _guarded(shape(D, S, B1), dt, -7) for k, dt, shape in PLAN_OUT}
    status, sbuf = _guarded((1,), torch.int32, 0)
    ins = []
    for a, dt in ((cnt.astype(np.int32), torch.int32), (np.asarray(box, dtype=np.float64).reshape(D, 4), torch.float64),
                  (np.asarray(frame, dtype=np.int32).reshape(D), torch.int32), (np.asarray([nb], dtype=np.int32), torch.int32)):
        v, buf = _guarded(a.shape, dt, -7)
        v.copy_(_dev(a))
        ins.append((v, buf))
    rc = _native.lib().fcn_frustum_detect_plan(*[_p(v) for v, _ in ins], hthr, pthr, D, S, B1, capacity, F,
                                               *[_p(o[k][0]) for k, _, _ in PLAN_OUT], _p(status), _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(_intact(buf, -7) for _, buf in o.values()) and _intact(sbuf, 0) and all(_intact(buf, -7) for _, buf in ins)
    got = {k: v.cpu().numpy() for k, (v, _) in o.items()}
    want = R.plan(cnt, box, frame, nb, hthr, pthr, B1, capacity, F)
    for k, w in (("slot_box", want[0]), ("seg_off", want[2]), ("off", want[3]), ("counts", want[4])):
        assert got[k].dtype == w.dtype and got[k].tobytes() == w.tobytes(), k
    assert int(got["n_kept"][0]) == want[1] and int(status.cpu()[0]) == want[5]
    return want


def _table(D=12, S=3, F=4, seed=0):
    """Counts, boxes and frames kept off every knife edge; boxes 1 and 6 without a row, box 3 too low, box 8 too narrow."""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(1, 900, (D, S))
    cnt[[1, 6]] = 0
    cnt[4, S - 1] = 0 if S > 1 else cnt[4, S - 1]
    x0, y0 = rs.uniform(0, 500, D), rs.uniform(0, 200, D)
    w, h = rs.uniform(20, 200, D), rs.uniform(20, 100, D)
    h[3], w[8] = 3.0, 0.25
    return cnt, np.stack([x0, y0, x0 + w, y0 + h], 1), rs.randint(0, F, D).astype(np.int32)


SURVIVORS = [0, 2, 4, 5, 7, 9, 10, 11]


@pytest.mark.parametrize("case", ["n_boxes_0", "n_boxes_D", "n_boxes_D_plus_1", "n_boxes_negative", "frame_minus_1", "frame_F",
                                  "exactly_B1", "B1_plus_1", "no_survivor"])
def test_plan_box_count_frames_and_slots(case):
    cnt, box, frame = _table()
    D = 12
    if case.startswith("n_boxes"):
        nb = {"n_boxes_0": 0, "n_boxes_D": D, "n_boxes_D_plus_1": D + 1, "n_boxes_negative": -3}[case]
        slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, frame, nb, D, 1 << 40, 4)
        assert st == (R.ST_RANGE if nb in (D + 1, -3) else 0) and n == (0 if nb <= 0 else 8)
        assert slot_box[:n].tolist() == SURVIVORS[:n] and (slot_box[n:] == D).all()
        if n == 0:
            assert not seg_off.any() and off.tolist() == [1 << 40] * D + [0] and not counts.any()
        assert _plan_equals(cnt, box, frame, 5, D, 1 << 40, 4)[0][:4].tolist() == [0, 2, 4, D]        # boxes 5.. are not live
        assert _plan_equals(cnt, box, frame, -2 ** 31, 3, 100, 4)[5] == R.ST_RANGE and _plan_equals(cnt, box, frame, 2 ** 31 - 1, 3, 1 << 40, 4)[1] == 3
    elif case.startswith("frame"):
        bad = frame.copy()
        bad[5], bad[1] = (-1, -2 ** 31) if case == "frame_minus_1" else (4, 2 ** 31 - 1)       # a survivor and a box without rows
        slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, bad, D, D, 1 << 40, 4)
        assert st == R.ST_RANGE and slot_box[:n].tolist() == [d for d in SURVIVORS if d != 5]
        assert seg_off[5 * 3] == seg_off[6 * 3]                             # an empty slice: the fill stores nothing for it
        assert _plan_equals(cnt, box, bad, 1, D, 1 << 40, 4)[5] == 0        # beyond n_boxes a frame is nobody's business
    elif case == "exactly_B1":
        slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, frame, D, 8, 1 << 40, 4)
        assert n == 8 and st == 0 and slot_box.tolist() == SURVIVORS and np.array_equal(counts, cnt[SURVIVORS].sum(1))
        assert off[8] == cnt[SURVIVORS].sum() and np.array_equal(off[:8], seg_off[np.asarray(SURVIVORS) * 3])
        slot_box, n, _, off, counts, st = _plan_equals(cnt, box, frame, D, 10, 1000, 4)      # two empty slots: the spare row, no bit
        assert n == 8 and (slot_box[8:] == D).all() and (off[8:10] == 1000).all() and not counts[8:].any() and st == R.ST_TRUNC
    elif case == "B1_plus_1":
        slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, frame, D, 7, 1 << 40, 4)
        assert n == 7 and st == R.ST_MANY and slot_box.tolist() == SURVIVORS[:7] and off[7] == cnt[SURVIVORS[:7]].sum()
        assert seg_off[11 * 3] == seg_off[-1]                               # the dropped survivor holds no rows
    else:
        for c, b in ((cnt * 0, box), (cnt, box * 0)):
            slot_box, n, seg_off, off, counts, st = _plan_equals(c, b, frame, D, 4, 1000, 4)
            assert n == 0 and st == 0 and not seg_off.any() and off.tolist() == [1000] * 4 + [0] and (slot_box == D).all()


def test_plan_knife_edges():
    one = lambda h, w, c, hthr=5.0, pthr=1.0: _plan_equals([[c]], [[0.0, 0.0, w, h]], [0], 1, 1, 100, 1, hthr, pthr)[1]
    assert one(5.0, 8.0, 3) == 1 and one(np.nextafter(5.0, 0.0), 8.0, 3) == 0          # height == threshold; one ulp under
    assert one(8.0, 1.0, 3) == 1 and one(8.0, np.nextafter(1.0, 0.0), 3) == 0           # width exactly 1
    assert one(8.0, 8.0, 7, pthr=7.0) == 1 and one(8.0, 8.0, 6, pthr=7.0) == 0          # count == lidar_point_threshold
    assert one(8.0, 8.0, 0, pthr=0.0) == 0 and one(8.0, 8.0, 1, pthr=0.0) == 1          # threshold 0 keeps no empty box
    assert one(np.nan, 8.0, 3) == 1                                                     # (numpy's comparison: NaN < 5 is False)
    assert _plan_equals([[7]], [[0.0, 0.0, 9.0, 9.0]], [0], 1, 1, 100, 1)[3].tolist() == [0, 7]     # B1 = D = S = 1


@pytest.mark.parametrize("S", [1, 3])
def test_plan_capacity_and_segments(S):
    cnt, box, frame = _table(S=S)
    D = 12
    held = SURVIVORS
    total = int(cnt[held].sum())
    assert _plan_equals(cnt, box, frame, D, 8, total, 4)[5] == 0            # exactly met: no bit 2
    slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, frame, D, 8, total - 1, 4)
    assert st == R.ST_TRUNC and off[8] == total - 1 and counts[7] == cnt[11].sum() - 1 and seg_off[-1] == total - 1
    first = int(cnt[0].sum())
    cut = first + int(cnt[2, 0]) - 1 if S == 3 else first + 5               # inside box 2's first segment
    slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, frame, D, 8, cut, 4)
    assert st == R.ST_TRUNC and counts[:3].tolist() == [first, cut - first, 0] and n == 8 and (seg_off[2 * S + 1:] == cut).all()
    assert _plan_equals(cnt, box, frame, D, 8, 0, 4)[2].any() == False


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [255, 256, 257])
def test_plans_where_a_threads_run_goes_from_one_box_to_two(D, S):
    """The run-per-thread split is csrc/slot_plan.h's, shared by every plan: over 256 threads, 255 and 256 boxes are runs of one
    (the last thread's empty, then not), 257 boxes are runs of two with threads 129.. owning nothing.  B1 = D, some boxes without
    a row or too low, a capacity one row short of the total; then the FOV form over as many frames."""
    from frustum_convnet_amd import _native
    rs = np.random.RandomState(4 * D + S)
    cnt = rs.randint(0, 900, (D, S)) * (rs.uniform(size=(D, 1)) < 0.8)
    box = np.tile(np.asarray([[10.0, 20.0, 110.0, 90.0]]), (D, 1))
    box[::7, 3] = 22.0
    frame = rs.randint(0, 4, D)
    total = int(R.plan(cnt, box, frame, D, 5.0, 1.0, D, 1 << 40, 4)[2][-1])
    slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, frame, D, D, total - 1, 4)
    assert 0 < n < D and st == R.ST_TRUNC and seg_off[-1] == total - 1 and counts.sum() == total - 1
    seg_off, sbuf = _guarded((D * S + 1,), torch.int64, -7)
    fov_off, fbuf = _guarded((D + 1,), torch.int64, -7)
    cnt_d = _dev(cnt.astype(np.int32))
    total = int(cnt.sum())
    assert _native.lib().fcn_frustum_fov_plan(_p(cnt_d), D, S, total - 1, _p(seg_off), _p(fov_off), _native.current_stream()) == 0
    torch.cuda.synchronize()
    ws, wf = R.fov_plan(cnt, total - 1)
    assert _intact(sbuf, -7) and _intact(fbuf, -7) and seg_off.cpu().numpy().tobytes() == ws.tobytes() and fov_off.cpu().numpy().tobytes() == wf.tobytes()
    assert wf[-1] == total - 1


def test_plan_at_its_limits_and_refusals():
    from frustum_convnet_amd import _native, frustum
    L, s = _native.lib(), _native.current_stream()
    max_d, max_segs = frustum.FrameDetectSource.limits()
    assert (max_d, max_segs) == (2048, 65536)
    rs = np.random.RandomState(1)
    for D, S in ((max_d, max_segs // max_d), (777, 5)):                     # the largest plan; more boxes than threads, sums beyond 2^31
        hi = 50 if D == max_d else 2 ** 31 - 1
        cnt = rs.randint(0, hi, (D, S)) * (rs.uniform(size=(D, 1)) < 0.6)
        box = np.tile(np.asarray([[10.0, 20.0, 110.0, 90.0]]), (D, 1))
        box[::7, 3] = 22.0
        slot_box, n, seg_off, off, counts, st = _plan_equals(cnt, box, rs.randint(0, 9, D), D, D, 1 << 50, 9)
        assert 300 < n < D and st == 0 and (np.diff(slot_box[:n]) > 0).all()
        _plan_equals(cnt, box, rs.randint(-1, 10, D), D - 5, 300, 1 << 36 if D == 777 else 9000, 9)
    # ---- refusals: nothing is written
    cnt, box, frame = _table()
    D, S, B = 12, 3, 4
    po = {k: torch.full(shape(D, S, B), -7, dtype=dt, device="cuda") for k, dt, shape in PLAN_OUT}
    po["status"] = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    pin = (_dev(cnt.astype(np.int32)), _dev(box), _dev(frame), _dev(np.asarray([D], np.int32)))
    good = [_p(x) for x in pin] + [5.0, 1.0, D, S, B, 10000, 4] + [_p(po[k]) for k in ("slot_box", "n_kept", "seg_off", "off", "counts", "status")] + [s]
    for i in (0, 1, 2, 3, 11, 12, 13, 14, 15, 16):
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_detect_plan(*bad) == BADARG, i
    for i, v, rc in ((6, -1, BADARG), (7, 0, BADARG), (8, 0, BADARG), (9, -1, BADARG), (10, -1, BADARG), (4, float("nan"), BADARG),
                     (5, float("nan"), BADARG), (6, max_d + 1, LIMIT), (8, max_d + 1, LIMIT), (7, max_segs // D + 1, LIMIT)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_detect_plan(*bad) == rc, (i, v)
    fo = (torch.full((D * S + 1,), -7, dtype=torch.int64, device="cuda"), torch.full((D + 1,), -7, dtype=torch.int64, device="cuda"))
    goodf = [_p(pin[0]), D, S, 10000, _p(fo[0]), _p(fo[1]), s]
    for i in (0, 4, 5):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_frustum_fov_plan(*bad) == BADARG, i
    for i, v, rc in ((1, -1, BADARG), (2, 0, BADARG), (3, -1, BADARG), (2, max_segs // D + 1, LIMIT)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_frustum_fov_plan(*bad) == rc, (i, v)
    assert L.fcn_frustum_detect_plan_limits(None, None) == BADARG
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in list(po.values()) + list(fo))
    # count and fill: the reading entries' argument refusals, and n_boxes
    sc = _scene(3)
    t = _tensors(sc)
    nb = _dev(np.asarray([30], np.int32))
    w = {"box2d": torch.full((30, 4), -7.0, dtype=torch.float64, device="cuda"), "angle": torch.full((30,), -7.0, dtype=torch.float64, device="cuda"),
         "scnt": torch.full((30, 3), -7, dtype=torch.int32, device="cuda")}
    good = _common(t, 3, True) + [_p(nb), _p(w["box2d"]), _p(w["angle"]), _p(w["scnt"]), s]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17):
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_detect_count(*bad) == BADARG, i
    for i, v in ((3, 2), (11, 0), (11, -1), (10, -1), (2, -1), (10, 65536)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_detect_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in w.values())
    soff = torch.zeros(91, dtype=torch.int64, device="cuda")
    out = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    goodf = good[:15] + [_p(soff), _p(out), s]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 14, 15, 16):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_frustum_detect_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (11, 0), (10, -1), (10, 65536)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_frustum_detect_fill(*bad) == BADARG, (i, v)
    assert L.fcn_frustum_detect_fill(*goodf) == 0                           # (every slice empty: nothing to write)
    zero = list(good)
    zero[2] = 0                                                             # F = 0: the counts are zeroed, nothing else is written
    assert L.fcn_frustum_detect_count(*zero) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and not w["scnt"].cpu().numpy().any() and (w["box2d"].cpu().numpy() == -7.0).all()


# ------------------------------------------------------------------------------------------------ count / fill behind n_boxes
def _dcount(t, S, nb, clip=True):
    from frustum_convnet_amd import _native
    D = t["bframe"].numel()
    o = {"box2d": torch.full((D, 4), -7.0, dtype=torch.float64, device="cuda"),
         "angle": torch.full((D,), -7.0, dtype=torch.float64, device="cuda"),
         "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda")}
    nbt, nbuf = _guarded((1,), torch.int32, -7)
    nbt.fill_(nb)
    rc = _native.lib().fcn_frustum_detect_count(*_common(t, S, clip), _p(nbt), _p(o["box2d"]), _p(o["angle"]), _p(o["scnt"]),
                                                _native.current_stream())
    torch.cuda.synchronize()
    assert _intact(nbuf, -7)
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _dfill(t, S, nb, seg_off, rows, clip=True, guard=5):
    """The raw fill entry into a poisoned buffer of `rows` rows between `guard` poisoned rows -> rc, the rows, the guards intact."""
    from frustum_convnet_amd import _native
    ps = t["pts"].shape[1]
    buf = torch.full((rows + 2 * guard, ps), -7.0, dtype=torch.float32, device="cuda")
    soff, nbt = _dev(np.asarray(seg_off, dtype=np.int64)), _dev(np.asarray([nb], np.int32))
    rc = _native.lib().fcn_frustum_detect_fill(*_common(t, S, clip), _p(nbt), _p(soff), _p(buf[guard:]), _native.current_stream())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return rc, h[guard:guard + rows], bool((h[:guard] == -7.0).all() and (h[guard + rows:] == -7.0).all())


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("stride", [4, 5])
def test_selection_equals_the_reading_selection_byte_for_byte(stride, clip):
    """The scene of tests/test_gpu_frustum.py (frames of 0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1 and 2 * seg + 100 rows, three
    boxes each) with every box live; then with the boxes from 17 on beyond n_boxes and two frames out of range: they store nothing."""
    sc = _scene(stride)
    S = sc["S"]
    t = _tensors(sc)
    rc, want = _count(t, S, clip)
    assert rc == 0
    want = {k: v.cpu().numpy() for k, v in want.items()}
    rcf, wrows, _, wsoff = _fill(t, S, want["scnt"], clip)
    assert rcf == 0 and len(wrows) > 1000
    rc, got = _dcount(t, S, 30, clip)
    assert rc == 0
    for k in ("scnt", "box2d", "angle"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    rc, rows, intact = _dfill(t, S, 30, wsoff, len(wrows), clip)
    assert rc == 0 and intact and np.array_equal(_bits(rows), _bits(wrows))
    # ---- boxes 17.. are not live; box 3 has frame F, box 10 frame -1 (exactly sized tables: nothing beyond them can be read)
    bframe = sc["bframe"].copy()
    bframe[3], bframe[10] = len(sc["lengths"]), -1
    t2 = _tensors(sc, bframe=bframe)
    rc, got = _dcount(t2, S, 17, clip)
    dead = np.asarray([d in (3, 10) or d >= 17 for d in range(30)])
    assert rc == 0 and not got["scnt"][dead].any() and np.array_equal(got["scnt"][~dead], want["scnt"][~dead])
    assert (got["box2d"][dead] == -7.0).all() and (got["angle"][dead] == -7.0).all()
    assert got["box2d"][~dead].tobytes() == want["box2d"][~dead].tobytes() and got["angle"][~dead].tobytes() == want["angle"][~dead].tobytes()
    rc, rows, intact = _dfill(t2, S, 17, wsoff, len(wrows), clip)          # granted the live run's rows: the dead store none of them
    assert rc == 0 and intact
    for d in range(30):
        a, b = int(wsoff[d * S]), int(wsoff[(d + 1) * S])
        assert (rows[a:b] == -7.0).all() if dead[d] else np.array_equal(_bits(rows[a:b]), _bits(wrows[a:b])), d
    assert want["scnt"][dead].sum() > 1000
    for nb in (0, -5):
        rc, got = _dcount(t, S, nb, clip)
        assert rc == 0 and not got["scnt"].any() and (got["box2d"] == -7.0).all()
        rc, rows, intact = _dfill(t, S, nb, wsoff, len(wrows), clip)
        assert rc == 0 and intact and (rows == -7.0).all()


def _exact_frames():
    """Frames of exactly seg, seg + 1 and 0 rows, every row inside the image and in front of the clip distance, one whole-image box
    and one inner box per frame (the last frame's boxes find nothing)."""
    g = _golden()
    seg = 4096
    rng = np.random.RandomState(5)
    P, V2C, R0, wh = (g[k][[0, 1, 0]].copy() for k in ("P", "V2C", "R0", "img_wh"))
    lengths = (seg, seg + 1, 0)
    frames = [np.concatenate([_back_project(rng, n, P[f], V2C[f], R0[f], wh[f][0], wh[f][1], True), rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1)
              for f, n in enumerate(lengths)]
    boxes = np.asarray([b for f in range(3) for b in ([-50.0, -50.0, wh[f][0] + 50.0, wh[f][1] + 50.0], [300.25, 100.5, 700.75, 300.0])])
    return {"pts": np.concatenate(frames, 0), "off": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "P": P, "V2C": V2C,
            "R0": R0, "wh": wh, "boxes": boxes, "bframe": np.repeat(np.arange(3), 2).astype(np.int32)}


def test_count_plan_fill_on_frames_of_4096_4097_and_0_rows():
    """count -> plan -> fill, the capacity exactly met and one row short, into a buffer of exactly capacity + 1 rows between guard
    rows; equal to frustum_candidates' rows of the boxes the existing rule keeps."""
    from frustum_convnet_amd import frustum
    sc = _exact_frames()
    t = _tensors(sc)
    rc, o = _dcount(t, 2, 6)
    assert rc == 0 and o["scnt"][0].tolist() == [4096, 0] and o["scnt"][2].tolist() == [4096, 1] and not o["scnt"][4:].any()
    assert 0 < o["scnt"][1].sum() < 4096 and o["scnt"][3, 1] <= 1
    sel = frustum.frustum_candidates(t["pts"], t["off"], _cal(t), t["wh"], t["boxes"], t["bframe"])
    assert np.array_equal(sel["counts"], o["scnt"].sum(1)) and sel["box2d"].cpu().numpy().tobytes() == o["box2d"].tobytes()
    want_rows, woff = sel["points"].cpu().numpy(), sel["off"].cpu().numpy()
    total = int(o["scnt"].sum())
    for cap, bit in ((total, 0), (total - 1, R.ST_TRUNC)):
        slot_box, n, seg_off, off, counts, st = _plan_equals(o["scnt"], o["box2d"], sc["bframe"], 6, 5, cap, 3)
        assert st == bit and n == 4 and slot_box.tolist() == [0, 1, 2, 3, 6] and seg_off[-1] == cap and off[4] == cap
        rc, rows, intact = _dfill(t, 2, 6, seg_off, cap + 1)
        assert rc == 0 and intact and (rows[cap] == -7.0).all() and np.array_equal(_bits(rows[:cap]), _bits(want_rows[:cap]))
        assert np.array_equal(off[:4], woff[:4]) and counts[:3].tolist() == sel["counts"][:3].tolist()


def test_fov_plan_equals_image_fov_points_byte_for_byte():
    from frustum_convnet_amd import frustum, _native
    sc = _scene(4)
    S, F, n = sc["S"], len(sc["lengths"]), len(sc["pts"])
    t = _tensors(sc)
    want_pts, want_off = frustum.image_fov_points(t["pts"], t["off"], _cal(t), t["wh"])
    want_pts, want_off = want_pts.cpu().numpy(), want_off.cpu().numpy()
    fov = dict(t, boxes=_dev(np.concatenate([np.zeros((F, 2)), sc["wh"]], 1)), bframe=_dev(np.arange(F, dtype=np.int32)))
    rc, o = _dcount(fov, S, F, clip=False)
    assert rc == 0 and 0 < o["scnt"].sum() == want_off[-1] < n
    seg_off, sbuf = _guarded((F * S + 1,), torch.int64, -7)
    fov_off, fbuf = _guarded((F + 1,), torch.int64, -7)
    cnt_d = _dev(o["scnt"])
    assert _native.lib().fcn_frustum_fov_plan(_p(cnt_d), F, S, n, _p(seg_off), _p(fov_off), _native.current_stream()) == 0
    torch.cuda.synchronize()
    ws, wf = R.fov_plan(o["scnt"], n)
    assert _intact(sbuf, -7) and _intact(fbuf, -7) and seg_off.cpu().numpy().tobytes() == ws.tobytes() and fov_off.cpu().numpy().tobytes() == wf.tobytes()
    assert fov_off.cpu().numpy().tobytes() == want_off.tobytes()
    rc, rows, intact = _dfill(fov, S, F, ws, int(ws[-1]), clip=False)
    assert rc == 0 and intact and np.array_equal(_bits(rows), _bits(want_pts))
    small = R.fov_plan(o["scnt"], 100)                                      # the clamp bounds the stores whatever the counts hold
    assert _native.lib().fcn_frustum_fov_plan(_p(cnt_d), F, S, 100, _p(seg_off), _p(fov_off), _native.current_stream()) == 0
    torch.cuda.synchronize()
    assert seg_off.cpu().numpy().tobytes() == small[0].tobytes() and fov_off.cpu().numpy().tobytes() == small[1].tobytes() and small[0].max() == 100


# ------------------------------------------------------------------------------------------------ FrameDetectSource
def _source(builder, B1, D=9, capacity=4000, seed=SEED, fov=False, boxes=True, **kw):
    from frustum_convnet_amd import frustum
    g = _golden()
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    a = dict(frame_points=_dev(g["points"]), frame_off=g["off"], calib=cal, img_size=g["img_wh"], spare_group=9)
    a.update(kw)
    src = frustum.FrameDetectSource(a.pop("frame_points"), a.pop("frame_off"), a.pop("calib"), a.pop("img_size"), builder, B1, D, capacity,
                                    seed, a.pop("spare_group"), fov=fov, **a)
    if boxes:
        src.set_boxes(g["boxes"], g["box_frame"], TYPES9, np.linspace(0.2, 0.95, 9))
    return src


def _existing(builder, draws, boxes=None, bframe=None, types=TYPES9, prob=None, points=None, **kw):
    """The path the source replaces, on the golden frames: frustum_candidates + build_device -> sel, batch."""
    from frustum_convnet_amd import frustum
    g = _golden()
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    boxes, bframe = (g["boxes"] if boxes is None else boxes), (g["box_frame"] if bframe is None else bframe)
    prob = np.linspace(0.2, 0.95, 9) if prob is None else prob
    sel = frustum.frustum_candidates(_dev(g["points"]) if points is None else points, _dev(g["off"]), cal, g["img_wh"], boxes, bframe)
    return sel, builder.build_device(sel, cal["P"], types, prob, draws=draws, **kw)


def _host(x):
    return {k: v.cpu().clone() for k, v in x.items() if isinstance(v, torch.Tensor)}


def test_source_equals_the_existing_path_and_the_recorded_run():
    """B1 = the survivors, the capacity exactly met, the source's own choice table handed to the existing path: the batch equals
    build_device(frustum_candidates(...)) bit for bit in every key; the slots, boxes, angles and rows are the reference's recorded
    run of the golden fixture, held to it as tests/test_gpu_frustum.py holds the existing path."""
    g = _golden()
    b = _input_builder(256)
    kept = np.nonzero(~g["ref_skip"])[0]
    counts = g["ref_mask"].sum(1)
    src = _source(b, len(kept), capacity=int(counts[kept].sum()), fov=True)
    assert src.S == 1 and src.points.shape == (int(counts[kept].sum()) + 1, 4)
    got = src.step()
    torch.cuda.synchronize()
    src.check()                                                             # nothing dropped, no empty slot: no bit
    assert sorted(got.keys()) == sorted(BATCH_KEYS + ("slot_box", "slot_frame", "slot_class", "slot_group", "n_kept"))
    sel, want = _existing(b, (src.t["choice"].clone(),))
    assert np.array_equal(want.pop("kept"), kept) and sorted(want.keys()) == sorted(BATCH_KEYS)
    for k in BATCH_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k].cpu(), want[k].cpu()), k
    assert got["slot_box"].cpu().numpy().tolist() == kept.tolist() and int(got["n_kept"].cpu()[0]) == len(kept)
    assert np.array_equal(got["slot_frame"].cpu().numpy(), g["box_frame"][kept]) and got["slot_group"].cpu().numpy().tolist() == kept.tolist()
    assert got["slot_class"].cpu().numpy().tolist() == [b.classes.index(TYPES9[d]) for d in kept]
    # ---- the recorded run
    assert np.array_equal(src.counts.cpu().numpy(), counts[kept]) and np.array_equal(src.seg_cnt.cpu().numpy().sum(1), counts)
    assert np.array_equal(src.box2d.cpu().numpy()[:9], g["ref_box2d"]) and np.array_equal(src.t["box2d"].cpu().numpy(), g["ref_box2d"][kept])
    assert (np.abs(src.angle.cpu().numpy()[:9] - g["ref_angle"]) <= 1e-12).all()
    pts_h, off_h = src.points.cpu().numpy(), src.off.cpu().numpy()
    assert np.array_equal(off_h, np.concatenate([[0], np.cumsum(counts[kept])]))
    for i, d in enumerate(kept):
        f = g["box_frame"][d]
        m = g["ref_mask"][d, :int(g["off"][f + 1] - g["off"][f])]
        want_rows = np.concatenate([g["ref_rect"][g["off"][f]:g["off"][f + 1]][m], g["points"][g["off"][f]:g["off"][f + 1]][m, 3:]], 1)
        _check_rows(pts_h[off_h[i]:off_h[i + 1]], want_rows, "box %d" % d)
    from frustum_convnet_amd import frustum
    fp, fo = frustum.image_fov_points(src.frames[0], g["off"], {k: _dev(g[k]) for k in ("P", "V2C", "R0")}, g["img_wh"])
    assert torch.equal(src.fov_off.cpu(), fo.cpu()) and torch.equal(src.fov_points[:int(fo[-1])].cpu(), fp.cpu())
    # ---- other thresholds, clip_boxes off: the existing path's kept list again
    for kw in (dict(img_height_threshold=3, lidar_point_threshold=12), dict(lidar_point_threshold=10 ** 6), dict(clip_boxes=False)):
        s2 = _source(b, 9, **kw)
        s2.step()
        torch.cuda.synchronize()
        from frustum_convnet_amd import frustum
        cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
        sel2 = frustum.frustum_candidates(_dev(g["points"]), _dev(g["off"]), cal, g["img_wh"], g["boxes"], g["box_frame"], 2.0, kw.get("clip_boxes", True))
        thr = {k: v for k, v in kw.items() if k != "clip_boxes"}
        k2 = b.build_device(sel2, cal["P"], TYPES9, np.linspace(0.2, 0.95, 9), **thr)["kept"]
        n = int(s2.n_kept.cpu()[0])
        assert n == len(k2) and s2.slot_box.cpu().numpy()[:n].tolist() == k2.tolist() and (s2.slot_box.cpu().numpy()[n:] == 9).all()


def test_source_with_empty_slots():
    """B1 = survivors + 2: the filled slots' rows equal the existing path's, the empty slots hold the spare row's frustum over no rows,
    finite and the same every step; too few slots are said."""
    g = _golden()
    b = _input_builder(256)
    kept = np.nonzero(~g["ref_skip"])[0]
    n = len(kept)
    src = _source(b, n + 2)
    first = _host(src.step())
    torch.cuda.synchronize()
    sel, want = _existing(b, (src.t["choice"][:n].clone(),))
    for k in BATCH_KEYS:
        assert torch.equal(first[k][:n], want[k].cpu()), k
        assert torch.isfinite(first[k]).all(), k
    assert first["slot_box"].tolist() == kept.tolist() + [9, 9] and first["slot_group"].tolist() == kept.tolist() + [9, 9]
    assert first["slot_frame"][n:].tolist() == [0, 0] and first["slot_class"][n:].tolist() == [0, 0] and not first["rgb_prob"][n:].any()
    assert first["one_hot"][n:].tolist() == [[1.0, 0.0, 0.0]] * 2 and not src.t["choice"][n:].cpu().numpy().any()
    assert src.off.cpu().numpy()[n:n + 2].tolist() == [src.capacity] * 2 and not src.points[src.capacity].cpu().numpy().any()
    src.set_boxes(g["boxes"][::-1].copy(), g["box_frame"][::-1].copy(), TYPES9[::-1], np.linspace(0.2, 0.95, 9)[::-1].copy())
    second = _host(src.step())
    torch.cuda.synchronize()
    assert second["slot_box"].tolist() == sorted(8 - kept).copy() + [9, 9] and int(src.draws.state.cpu()[0]) == 2
    for k in BATCH_KEYS:
        assert torch.equal(first[k][n:], second[k][n:]), k
    with pytest.raises(ValueError, match="bit 0") as e:                     # the draws' own bit: an empty slot has no row either
        src.check()
    assert "bit 8" not in str(e.value) and "bit 10" not in str(e.value) and "bit 2" not in str(e.value)
    small = _source(b, n - 1, capacity=100)
    small.step()
    assert small.slot_box.cpu().numpy().tolist() == kept[:n - 1].tolist()
    with pytest.raises(ValueError, match="bit 8") as e:
        small.check()
    assert "bit 2" in str(e.value) and "bit 10" not in str(e.value)          # (bit 0 too: the slots behind the cut hold no row)
    assert small.counts.cpu().numpy().sum() == 100 and small.off.cpu().numpy()[-1] == 100


def test_source_check_names_the_bits_and_clears():
    b = _input_builder(256)
    src = _source(b, 4)
    src.check()
    for bit, name in ((R.ST_TRUNC, "bit 2"), (R.ST_MANY, "bit 8"), (R.ST_RANGE, "bit 10")):
        src.status.fill_(bit)
        with pytest.raises(ValueError, match=name) as e:
            src.check()
        assert int(src.status.cpu()[0]) == 0 and sum("bit %d:" % i in str(e.value) for i in (0, 1, 2, 4, 8, 10)) == 1
    src.draws.status.fill_(1)
    with pytest.raises(ValueError, match="bit 0"):
        src.check()
    assert int(src.draws.status.cpu()[0]) == 0
    src.check()
    # the kernels' own bit 10: a live box whose frame is out of range, then n_boxes beyond the table; both cleared by check()
    src.box_frame[1] = 2
    src.step()
    with pytest.raises(ValueError, match="bit 10"):
        src.check()
    assert 1 not in src.slot_box.cpu().numpy().tolist()
    src.box_frame[1] = 0
    src.n_boxes.fill_(10)
    src.step()
    with pytest.raises(ValueError, match="bit 10"):
        src.check()
    assert src.slot_box.cpu().numpy().tolist() == [0, 1, 2, 5]


def test_source_refusals():
    from frustum_convnet_amd import frustum
    g = _golden()
    b = _input_builder(256)
    pts = _dev(g["points"])
    src = _source(b, 4)
    assert src.frames[0].data_ptr() != pts.data_ptr() and _source(b, 4, frame_points=pts).frames[0].data_ptr() == pts.data_ptr()   # held
    for kw in (dict(frame_off=[0, 4800, 2600]), dict(frame_off=[0]), dict(frame_off=[0, 2600, 10 ** 6]), dict(frame_points=pts.double()),
               dict(frame_points=pts[:, :2].contiguous()), dict(frame_points=pts[::2]), dict(frame_points=g["points"]),
               dict(B1=0), dict(B1=10), dict(D=0), dict(D=2049), dict(capacity=0), dict(spare_group=-1), dict(spare_group=2 ** 31),
               dict(img_height_threshold=float("nan")), dict(lidar_point_threshold=float("inf")), dict(clip_distance=float("nan")),
               dict(img_size=g["img_wh"][:1]), dict(calib={k: g[k][:1] for k in ("P", "V2C", "R0")})):
        kw = dict(kw)
        with pytest.raises(ValueError):
            _source(b, kw.pop("B1", 4), D=kw.pop("D", 9), capacity=kw.pop("capacity", 4000), boxes=False, **kw)
    with pytest.raises(ValueError):                                         # D * S beyond the plan's segments
        _source(b, 4, D=2048, boxes=False, frame_points=torch.zeros((4096 * 40, 4), dtype=torch.float32, device="cuda"), frame_off=[0, 4096 * 40, 4096 * 40])
    boxes, fr, prob = g["boxes"], g["box_frame"], np.linspace(0.2, 0.95, 9)
    for args in ((boxes, fr[:8], TYPES9, prob), (boxes, fr, TYPES9[:8], prob), (boxes, fr, TYPES9, prob[:8]), (boxes, fr, TYPES9, prob, [0] * 8),
                 (np.concatenate([boxes, boxes[:1]]), np.concatenate([fr, fr[:1]]), TYPES9 + ["Car"], np.concatenate([prob, prob[:1]])),
                 (boxes, np.where(np.arange(9) == 4, 2, fr), TYPES9, prob), (boxes, np.where(np.arange(9) == 4, -1, fr), TYPES9, prob),
                 (boxes, fr.astype(np.float64), TYPES9, prob), (boxes, fr, ["Tram"] + TYPES9[1:], prob), (boxes, fr, TYPES9, prob, [9] + [0] * 8),
                 (boxes, fr, TYPES9, prob, [-1] + [0] * 8), (np.where(np.arange(36).reshape(9, 4) == 5, np.nan, boxes), fr, TYPES9, prob),
                 (boxes, fr, TYPES9, np.where(np.arange(9) == 2, np.inf, prob))):
        with pytest.raises(ValueError):
            src.set_boxes(*args)
    assert int(src.n_boxes.cpu()[0]) == 9 and np.array_equal(src.boxes2d.cpu().numpy()[:9], boxes)      # a refusal writes nothing
    assert src.boxes2d.cpu().numpy()[9].tolist() == [0, 0, 1, 1] and int(src.box_group.cpu()[9]) == 9
    assert int(src.set_boxes(boxes[:0], fr[:0], [], prob[:0]).n_boxes.cpu()[0]) == 0
    src.step()
    torch.cuda.synchronize()
    assert int(src.n_kept.cpu()[0]) == 0 and (src.slot_box.cpu().numpy() == 9).all() and int(src.status.cpu()[0]) == 0
    with pytest.raises(ValueError):
        src.bind(slot_frame=torch.zeros((5,), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        src.bind(fov_off=torch.zeros((3,), dtype=torch.int64, device="cuda"))        # fov=False: there is no such output
    with pytest.raises(ValueError):
        _source(b, 4, fov=True).bind(fov_off=torch.zeros((3,), dtype=torch.int32, device="cuda"))
    assert frustum.FrameDetectSource.limits() == (2048, 65536)


def _capture(step):
    """Warm-up on a side stream, then ONE capture of step() on one stream -> graph, the captured outputs."""
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    torch.cuda.synchronize()
    return graph, out


def _rewrites():
    """Three states of the detection table and the frame points, written in place between replays."""
    g = _golden()
    prob = np.linspace(0.2, 0.95, 9)
    rev = lambda a: np.ascontiguousarray(np.asarray(a)[::-1])
    moved = g["points"].copy()
    moved[:, 1] += np.float32(0.75)
    return ((g["boxes"], g["box_frame"], TYPES9, prob, g["points"], 9), (rev(g["boxes"]), rev(g["box_frame"]), TYPES9[::-1], rev(prob), moved, 9),
            (g["boxes"], g["box_frame"], TYPES9, prob, moved, 6))


def test_captured_source_step_replays_equal_eager_steps():
    """ONE capture of step(); three replays, the boxes, n_boxes and the frame points overwritten in place between them; every replay
    equals the eager step() of a twin on the same seed and the same data, bit for bit; the draw advances."""
    b = _input_builder(256)
    g = _golden()
    pa, pb = _dev(g["points"]), _dev(g["points"])
    src, twin = _source(b, 6, frame_points=pa, fov=True), _source(b, 6, frame_points=pb, fov=True)
    graph, out = _capture(src.step)
    assert int(src.draws.state.cpu()[0]) == 1                               # capturing runs nothing
    twin.step()
    seen = []
    for r, (boxes, fr, types, prob, points, nb) in enumerate(_rewrites()):
        for s, p in ((src, pa), (twin, pb)):
            s.set_boxes(boxes, fr, types, prob)
            s.n_boxes.fill_(nb)
            p.copy_(_dev(points))
        graph.replay()
        torch.cuda.synchronize()
        got = _host(out)
        want = _host(twin.step())
        torch.cuda.synchronize()
        assert int(src.draws.state.cpu()[0]) == 2 + r == int(twin.draws.state.cpu()[0])
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)
        assert torch.equal(src.fov_off.cpu(), twin.fov_off.cpu()) and torch.equal(src.fov_points.cpu(), twin.fov_points.cpu())
        assert torch.equal(src.points.cpu(), twin.points.cpu()) and int(got["n_kept"][0]) >= 3
        seen.append(got)
    assert not torch.equal(seen[0]["point_cloud"], seen[1]["point_cloud"]) and not torch.equal(seen[1]["slot_box"], seen[2]["slot_box"])
    assert int(src.status.cpu()[0]) == 0 and int(twin.status.cpu()[0]) == 0


# ------------------------------------------------------------------------------------------------ FrameCascade
BOXES = np.asarray([[300.0, 150.0, 520.0, 300.0], [700.0, 160.0, 900.0, 280.0], [600.0, 180.0, 700.0, 183.5],
                    [500.0, 120.0, 760.0, 330.0], [100.0, 150.0, 330.0, 290.0], [640.0, 2.0, 660.0, 9.0]])
BFRAME = np.asarray([0, 0, 0, 1, 1, 1], dtype=np.int32)
TYPES = ["Car", "Pedestrian", "Car", "Car", "Cyclist", "Car"]
PROB = np.asarray([0.9, 0.8, 0.7, 0.6, 0.5, 0.4])
GROUP = np.asarray([0, 1, 0, 2, 3, 2], dtype=np.int32)
BIG = (64, 32, 16, 8)


def _two_stage():
    """The detector and the two dense frames of test_detect_frames_equals_the_hand_composed_sequence (6000 and 5000 rows: S = 2)."""
    from helpers import load_golden
    from test_gpu_model import _model
    from frustum_convnet_amd import cascade, inputs
    g = _golden()
    g1, g2 = load_golden("car_b4_n512"), load_golden("refine_b4_n512")
    m1 = _model(g1).eval()
    ib = inputs.InputBuilder(int(g1["meta_npoint"]))
    m2 = _model(g2).eval()
    rb = inputs.RefineInputBuilder(int(g2["meta_npoint"]))
    rng = np.random.RandomState(9)
    lengths = (6000, 5000)
    xyz = [np.stack([rng.uniform(3, 45, n), rng.uniform(-12, 12, n), rng.uniform(-2.0, 0.5, n), rng.uniform(0, 1, n)], 1) for n in lengths]
    fpts = np.concatenate(xyz, 0).astype(np.float32)
    foff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    return cascade.TwoStageDetector(m1, m2, rb, input_builder=ib), fpts, foff, cal, g["img_wh"]


def _chain(two, fpts, foff, cal, wh, B1, D, B, capacity, lpad, D1=6, capacity1=8000, seed=SEED, boxes=True, **kw):
    fc = two.frame_link(fpts, foff, cal, wh, B1, D1, capacity1, 4, D, B, capacity, lpad, seed, "nms", 0.1, top_k=6, **kw)
    if boxes:
        fc.source.set_boxes(BOXES, BFRAME, TYPES, PROB, GROUP)
    return fc


def test_frame_cascade_equals_detect_frames():
    """A probe chain with room to spare finds the sizes at which nothing is dropped and no slot is empty; the chain at exactly those
    sizes equals TwoStageDetector.detect_frames with the chain's own choice tables as draws / refine_draws, bit for bit.  Then one
    empty first-stage slot: no keep entry of either stage points at a row of an empty slot."""
    from frustum_convnet_amd import cascade
    two, fpts_h, foff, cal, wh = _two_stage()
    fpts = _dev(fpts_h)
    probe = _chain(two, fpts, foff, cal, wh, 4, 32, 32, 40000, BIG)
    assert isinstance(probe, cascade.FrameCascade) and probe.link.frame_off is probe.source.fov_off and probe.link.frames[1] is probe.link.frame_off
    assert probe.source.slot_frame is probe.link.unit_frame and probe.source.slot_group is probe.link.unit_group and probe.link.S == 2
    pr = probe.step()
    torch.cuda.synchronize()
    assert int(probe.source.status.cpu()[0]) == 0 and int(probe.link.status.cpu()[0]) == 0
    n1, n2, ncand = int(pr["n_kept1"].cpu()[0]), int(pr["n_kept"].cpu()[0]), int(pr["n_cand"].cpu()[0])
    assert n1 == 4 and pr["slot_box"].cpu().numpy().tolist() == [0, 1, 3, 4] and 2 <= n2 <= ncand <= 24
    widths = probe.link.pred_size.cpu().numpy()[probe.link.slot_unit.cpu().numpy()[:n2].astype(np.int64), 1]
    lpad = two.refine_builder._lpad(widths)
    total1, total2 = int(probe.source.counts.cpu().numpy().sum()), int(probe.link.counts.cpu().numpy().sum())
    fc = _chain(two, fpts, foff, cal, wh, 4, ncand + 1, n2, total2, lpad, capacity1=total1)
    got = fc.step()
    torch.cuda.synchronize()
    fc.check()                                                              # nothing dropped, no empty slot: no bit
    res = two.detect_frames(fpts, _dev(foff), cal, wh, BOXES, BFRAME, TYPES, PROB, "nms", 0.1, unit_group=GROUP, num_groups=4, top_k=6,
                            draws=(fc.source.t["choice"].clone(),), refine_draws=(fc.link.t["choice"].clone(),))
    torch.cuda.synchronize()
    assert res["kept"].tolist() == got["slot_box"].cpu().numpy().tolist() == [0, 1, 3, 4]
    for k in ("dets", "valid", "keep", "cnt"):
        assert got[k].dtype == res[k].dtype and got[k].shape == res[k].shape and torch.equal(got[k].cpu(), res[k].cpu()), k
    for a, w in zip(got["stage1"], res["stage1"]):
        assert torch.equal(a.cpu(), w.cpu())
    assert np.array_equal(got["stage1_row"].cpu().numpy(), res["stage1_row"]) and int(got["cnt"].sum()) > 0 and int(got["n_kept"].cpu()[0]) == n2
    # ---- an empty first-stage slot (and empty second-stage slots)
    fe = _chain(two, fpts, foff, cal, wh, 5, 24, n2 + 2, 40000, BIG)
    ge = fe.step()
    torch.cuda.synchronize()
    assert int(ge["n_kept1"].cpu()[0]) == 4 and ge["slot_box"].cpu().numpy().tolist() == [0, 1, 3, 4, 6]
    assert fe.link.unit_group.cpu().numpy().tolist() == GROUP[[0, 1, 3, 4]].tolist() + [4]
    L2 = fe.source.builder.L[1]
    k1, c1 = ge["stage1"][2].cpu().numpy(), ge["stage1"][3].cpu().numpy()
    assert k1.shape == (4, 6) and c1.sum() > 0 and all((k1[g, :c1[g]] >= 0).all() and (k1[g, :c1[g]] // L2 < 4).all() for g in range(4))
    assert (fe.link.cand_row.cpu().numpy()[:int(ge["n_cand"].cpu()[0])] // L2 < 4).all()
    n2e = int(ge["n_kept"].cpu()[0])
    k2, c2 = ge["keep"].cpu().numpy(), ge["cnt"].cpu().numpy()
    assert n2e == n2 and c2.sum() > 0 and all((k2[g, :c2[g]] >= 0).all() and (k2[g, :c2[g]] // BIG[1] < n2e).all() for g in range(4))
    assert torch.isfinite(ge["dets"]).all() and all(torch.isfinite(v).all() for v in ge["batch1"].values())
    with pytest.raises(ValueError, match="bit 0") as e:
        fe.check()
    assert not any("bit %d:" % i in str(e.value) for i in (1, 2, 5, 6, 7, 8, 9, 10))
    fe.check()
    with pytest.raises(ValueError):
        cascade.TwoStageDetector(two.stage1, two.stage2, two.refine_builder).frame_link(fpts, foff, cal, wh, 4, 6, 8000, 4, 24, 24, 40000, BIG,
                                                                                        SEED, "nms", 0.1)


def test_captured_frame_cascade_replays_on_new_boxes_equal_to_eager_steps():
    two, fpts_h, foff, cal, wh = _two_stage()
    pa, pb = _dev(fpts_h), _dev(fpts_h)
    src, twin = (_chain(two, p, foff, cal, wh, 5, 24, 24, 40000, BIG) for p in (pa, pb))
    graph, out = _capture(src.step)
    twin.step()
    order = [3, 4, 0, 1, 2, 5]
    moved = fpts_h.copy()
    moved[:, 1] += np.float32(0.5)
    seen = []
    for r, (idx, points, nb) in enumerate((([0, 1, 2, 3, 4, 5], fpts_h, 6), (order, moved, 6), (order, fpts_h, 4))):
        for fc, p in ((src, pa), (twin, pb)):
            fc.source.set_boxes(BOXES[idx], BFRAME[idx], [TYPES[i] for i in idx], PROB[idx], GROUP[idx])
            fc.source.n_boxes.fill_(nb)
            p.copy_(_dev(points))
        graph.replay()
        torch.cuda.synchronize()
        got, gb = _host(out), _host(out["batch"])
        want_out = twin.step()
        torch.cuda.synchronize()
        want, wb = _host(want_out), _host(want_out["batch"])
        for k in ("dets", "valid", "keep", "cnt", "stage1_row", "n_kept", "slot_unit", "cand_row", "n_cand", "slot_box", "n_kept1"):
            assert torch.equal(got[k], want[k]), (r, k)
        for k in wb:
            assert torch.equal(gb[k], wb[k]), (r, k)
        for a, w in zip(out["stage1"], want_out["stage1"]):
            assert torch.equal(a.cpu(), w.cpu()), r
        assert int(got["n_kept1"][0]) >= 2 and int(got["cnt"].sum()) > 0
        seen.append(got)
    assert seen[1]["slot_box"].tolist() != seen[0]["slot_box"].tolist() and not torch.equal(seen[0]["dets"], seen[1]["dets"])
    assert int(src.source.status.cpu()[0]) == 0 and int(src.link.status.cpu()[0]) == 0
