"""-m gpu: capturable SUN-RGBD inference -- fcn_frustum_sunrgbd_detect_count / _plan / _fill (csrc/frustum_sunrgbd_detect_plan.h)
and fcn_det_rows (csrc/det_eval.h) through the C-ABI against the numpy restatement of tests/sunrgbd_detect_plan_ref.py (pinned to the
host path by tests/test_sunrgbd_detect_plan_referee.py) and against the reading selection fcn_frustum_sunrgbd_count / _fill;
SunrgbdInputBuilder.alloc_infer / launch_infer against build_device; frustum.SunrgbdDetectSource against the path it replaces
(sunrgbd_candidates + build_device) and the reference's recorded run of tests/golden/frustum_sunrgbd.npz;
evaluate.SunrgbdFrameChain against SunrgbdDetector.detect_frames; both under a captured graph.  Scenes and helpers are those of
tests/test_gpu_frustum_sunrgbd.py, the model that of tests/test_gpu_sunrgbd_detector.py (hash-initialised five-scale model, N = 512,
C = 10); cap = 64 so that the subsample branch is reached on frames of about 5000 rows (2048 only for the recorded run).
tests/test_emu_sunrgbd_detect_source.py runs the same functions on the host emulation of the kernels (all but the graph captures)."""
import numpy as np
import pytest
import torch

import frustum_sunrgbd_ref as fref
import sunrgbd_detect_plan_ref as R
from test_gpu_frustum import BADARG, _bits, _dev, _p
from test_gpu_frustum_sunrgbd import _builder, _close, _common, _count, _det_sel, _fill, _golden, _scene, _tensors
from test_gpu_refine_plan import _guarded, _intact

pytestmark = pytest.mark.gpu
LIMIT = 10002                      # FCN_E_LIMIT
SEED = 20241021
CAP = 64
BATCH_KEYS = ("point_cloud", "rot_angle", "rgb_prob", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "center_ref5", "one_hot")
SLOT_KEYS = ("slot_box", "slot_frame", "slot_class", "slot_group", "n_kept")


# ------------------------------------------------------------------------------------------------ the plan
PLAN_OUT = (("slot_box", torch.int32, lambda D, S, B: (B,)), ("n_kept", torch.int32, lambda D, S, B: (1,)),
            ("seg_off", torch.int64, lambda D, S, B: (D * S + 1,)), ("off", torch.int64, lambda D, S, B: (B + 1,)),
            ("counts", torch.int64, lambda D, S, B: (B,)), ("cnt32", torch.int32, lambda D, S, B: (B,)),
            ("sub_off", torch.int64, lambda D, S, B: (B + 1,)), ("sub_start", torch.int64, lambda D, S, B: (B,)),
            ("sub_len", torch.int32, lambda D, S, B: (B,)), ("slot_group", torch.int32, lambda D, S, B: (B,)))


def _plan_equals(cnt, frame, cls, nb, thr, cap, B, capacity, F, C):
    """The raw entry on exactly sized, guarded inputs and poisoned, guarded outputs, held to the restatement (every output is
    poisoned first, so equality also says that every output is written) -> the restatement's dict."""
    from frustum_convnet_amd import _native
    cnt = np.asarray(cnt)
    D, S = cnt.shape
    o = {k: _guarded(shape(D, S, B), dt, -7) for k, dt, shape in PLAN_OUT}
    status, sbuf = _guarded((1,), torch.int32, 0)
    ins = []
    for a in (cnt.astype(np.int32), np.asarray(frame, dtype=np.int32).reshape(D), np.asarray(cls, dtype=np.int32).reshape(D),
              np.asarray([nb], dtype=np.int32)):
        v, buf = _guarded(a.shape, torch.int32, -7)
        v.copy_(_dev(a))
        ins.append((v, buf))
    rc = _native.lib().fcn_frustum_sunrgbd_detect_plan(*[_p(v) for v, _ in ins], thr, cap, D, S, B, capacity, F, C,
                                                       *[_p(o[k][0]) for k, _, _ in PLAN_OUT], _p(status), _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and all(_intact(buf, -7) for _, buf in o.values()) and _intact(sbuf, 0) and all(_intact(buf, -7) for _, buf in ins)
    got = {k: v.cpu().numpy() for k, (v, _) in o.items()}
    want = R.plan(cnt, frame, cls, nb, thr, cap, B, capacity, F, C)
    for k, _, _ in PLAN_OUT:
        if k != "n_kept":
            assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])
    assert int(got["n_kept"][0]) == want["n_kept"] and int(status.cpu()[0]) == want["status"]
    return want


def _table(D=12, S=3, F=3, C=10, seed=0):
    """Counts, frames and classes off every knife edge: boxes 1 and 6 without a row, box 3 with 3 rows (under the bar of 5), boxes 2
    and 9 under the cap of 64, the others over it."""
    rs = np.random.RandomState(seed)
    cnt = rs.randint(30, 900, (D, S))
    cnt[[1, 6]] = 0
    cnt[3] = 0
    cnt[3, 0] = 3
    cnt[2], cnt[9] = 0, 0
    cnt[2, S - 1], cnt[9, 0] = 40, 63
    return cnt, rs.randint(0, F, D).astype(np.int32), rs.randint(0, C, D).astype(np.int32)


SURVIVORS = [0, 2, 4, 5, 7, 8, 9, 10, 11]


@pytest.mark.parametrize("case", ["n_boxes_0", "n_boxes_D", "n_boxes_D_plus_1", "n_boxes_negative", "frame_minus_1", "frame_F",
                                  "class_minus_1", "class_C", "exactly_B", "B_plus_1", "no_survivor"])
def test_plan_box_count_ranges_and_slots(case):
    cnt, frame, cls = _table()
    D, big = 12, 1 << 40
    if case.startswith("n_boxes"):
        nb = {"n_boxes_0": 0, "n_boxes_D": D, "n_boxes_D_plus_1": D + 1, "n_boxes_negative": -3}[case]
        p = _plan_equals(cnt, frame, cls, nb, 5, CAP, D, big, 3, 10)
        n = p["n_kept"]
        assert p["status"] == (R.ST_RANGE if nb in (D + 1, -3) else 0) and n == (0 if nb <= 0 else 9)
        assert p["slot_box"][:n].tolist() == SURVIVORS[:n] and (p["slot_box"][n:] == D).all() and (p["slot_group"][n:] == 30).all()
        if n == 0:
            assert not p["seg_off"].any() and p["off"].tolist() == [big] * D + [0] and not p["counts"].any() and not p["sub_off"].any()
        else:
            assert p["sub_len"][:n].tolist() == [CAP, 0, CAP, CAP, CAP, CAP, 0, CAP, CAP]
        assert _plan_equals(cnt, frame, cls, 5, 5, CAP, D, big, 3, 10)["slot_box"][:4].tolist() == [0, 2, 4, D]      # boxes 5.. are not live
        assert _plan_equals(cnt, frame, cls, -2 ** 31, 5, CAP, 3, 100, 3, 10)["status"] == R.ST_RANGE
        assert _plan_equals(cnt, frame, cls, 2 ** 31 - 1, 5, CAP, 3, big, 3, 10)["n_kept"] == 3
    elif case.startswith("frame") or case.startswith("class"):
        bad = (frame if case.startswith("frame") else cls).copy()
        bad[5], bad[1] = {"frame_minus_1": (-1, -2 ** 31), "frame_F": (3, 2 ** 31 - 1), "class_minus_1": (-1, -2 ** 31),
                          "class_C": (10, 2 ** 31 - 1)}[case]                # a survivor and a box without rows
        a = (bad, cls) if case.startswith("frame") else (frame, bad)
        p = _plan_equals(cnt, a[0], a[1], D, 5, CAP, D, big, 3, 10)
        assert p["status"] == R.ST_RANGE and p["slot_box"][:p["n_kept"]].tolist() == [d for d in SURVIVORS if d != 5]
        assert p["seg_off"][5 * 3] == p["seg_off"][6 * 3]                   # an empty slice: the fill stores nothing for it
        assert (p["slot_group"] >= 0).all() and (p["slot_group"] <= 30).all()
        assert _plan_equals(cnt, a[0], a[1], 1, 5, CAP, D, big, 3, 10)["status"] == 0      # beyond n_boxes a table row is nobody's business
    elif case == "exactly_B":
        p = _plan_equals(cnt, frame, cls, D, 5, CAP, 9, big, 3, 10)
        assert p["n_kept"] == 9 and p["status"] == 0 and p["slot_box"].tolist() == SURVIVORS
        assert np.array_equal(p["counts"], cnt[SURVIVORS].sum(1)) and p["off"][9] == cnt[SURVIVORS].sum()
        assert np.array_equal(p["off"][:9], p["seg_off"][np.asarray(SURVIVORS) * 3])
        assert np.array_equal(p["slot_group"], (frame * 10 + cls)[SURVIVORS]) and p["sub_off"][9] == 7 * CAP
        p = _plan_equals(cnt, frame, cls, D, 5, CAP, 11, 1000, 3, 10)       # two empty slots: the spare row and group, no bit for them
        assert p["n_kept"] == 9 and (p["slot_box"][9:] == D).all() and (p["off"][9:11] == 1000).all() and not p["counts"][9:].any()
        assert p["status"] == R.ST_TRUNC and not p["sub_len"][9:].any() and (p["slot_group"][9:] == 30).all()
    elif case == "B_plus_1":
        p = _plan_equals(cnt, frame, cls, D, 5, CAP, 8, big, 3, 10)
        assert p["n_kept"] == 8 and p["status"] == R.ST_MANY and p["slot_box"].tolist() == SURVIVORS[:8]
        assert p["off"][8] == cnt[SURVIVORS[:8]].sum() and p["seg_off"][11 * 3] == p["seg_off"][-1]      # the dropped survivor holds no rows
    else:
        for c, thr in ((cnt * 0, 5), (cnt, 10 ** 6), (np.minimum(cnt, 1), 4)):
            p = _plan_equals(c, frame, cls, D, thr, CAP, 4, 1000, 3, 10)
            assert p["n_kept"] == 0 and p["status"] == 0 and not p["seg_off"].any() and p["off"].tolist() == [1000] * 4 + [0]
            assert (p["slot_box"] == D).all() and not p["sub_off"].any() and (p["slot_group"] == 30).all()


def test_plan_knife_edges():
    one = lambda c, thr=5, cap=CAP, capacity=10000: _plan_equals([[c]], [0], [0], 1, thr, cap, 1, capacity, 1, 1)
    assert one(4)["n_kept"] == 0 and one(5)["n_kept"] == 1                  # point_threshold - 1, point_threshold
    assert one(0, 0)["n_kept"] == 0 and one(1, 0)["n_kept"] == 1 and one(1, -7)["n_kept"] == 1      # the bar is max(1, threshold)
    assert one(CAP)["sub_len"].tolist() == [0] and one(CAP + 1)["sub_len"].tolist() == [CAP]        # cap, cap + 1
    assert one(CAP + 1)["sub_off"].tolist() == [0, CAP] and one(CAP)["sub_off"].tolist() == [0, 0]
    p = one(CAP + 1, capacity=CAP)                                          # the subsample is decided on the STORED rows
    assert p["counts"].tolist() == [CAP] and p["sub_len"].tolist() == [0] and p["status"] == R.ST_TRUNC
    assert one(9, 5, 3)["n_kept"] == 0                                      # min(count, cap) under the bar
    p = _plan_equals([[7, 0, 2]], [1], [3], 1, 5, CAP, 1, 100, 2, 4)        # B = D = 1
    assert p["off"].tolist() == [0, 9] and p["slot_group"].tolist() == [7]
    # the capacity inside a box, exactly at a box end, and at 0 rows of the next
    cnt = np.asarray([[70, 10], [5, 95], [66, 0]])
    for capacity, counts, st in ((130, [80, 50, 0], R.ST_TRUNC), (180, [80, 100, 0], R.ST_TRUNC), (80, [80, 0, 0], R.ST_TRUNC),
                                 (246, [80, 100, 66], 0), (245, [80, 100, 65], R.ST_TRUNC)):
        p = _plan_equals(cnt, [0, 0, 1], [1, 1, 2], 3, 5, CAP, 3, capacity, 2, 3)
        assert p["counts"].tolist() == counts and p["status"] == st and p["n_kept"] == 3 and p["off"][3] == min(capacity, 246)
        assert p["sub_len"].tolist() == [CAP if c > CAP else 0 for c in counts]


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [255, 256, 257])
def test_plans_where_a_threads_run_goes_from_one_box_to_two(D, S):
    """The run-per-thread split is csrc/slot_plan.h's: over 256 threads, 255 and 256 boxes are runs of one (the last thread's empty,
    then not), 257 boxes are runs of two with threads 129.. owning nothing -- and the same for the slots' own run with B = D.  Some
    boxes without a row or under the bar, counts around the cap, a capacity one row short of the total."""
    rs = np.random.RandomState(4 * D + S)
    cnt = rs.randint(0, 70, (D, S)) * (rs.uniform(size=(D, 1)) < 0.8)
    frame, cls = rs.randint(0, 4, D), rs.randint(0, 10, D)
    total = int(R.plan(cnt, frame, cls, D, 5, CAP, D, 1 << 40, 4, 10)["seg_off"][-1])
    p = _plan_equals(cnt, frame, cls, D, 5, CAP, D, total - 1, 4, 10)
    assert 0 < p["n_kept"] < D and p["status"] == R.ST_TRUNC and p["seg_off"][-1] == total - 1 and p["counts"].sum() == total - 1
    assert 0 < (p["sub_len"] > 0).sum() < p["n_kept"]                      # counts on both sides of the cap
    p = _plan_equals(cnt, frame, cls, D - 3, 5, CAP, 100, 1 << 40, 4, 10)
    assert p["status"] == R.ST_MANY and p["n_kept"] == 100


def test_plan_at_its_limits_and_refusals():
    from frustum_convnet_amd import _native, frustum
    L, s = _native.lib(), _native.current_stream()
    max_d, max_segs, max_cap = frustum.SunrgbdDetectSource.limits()
    assert (max_d, max_segs) == (2048, 65536) and max_cap >= 2048
    rs = np.random.RandomState(1)
    for D, S in ((max_d, max_segs // max_d), (777, 5)):                     # the largest plan; more boxes than threads, sums beyond 2^31
        hi = 50 if D == max_d else 2 ** 31 - 1
        cnt = rs.randint(0, hi, (D, S)) * (rs.uniform(size=(D, 1)) < 0.6)
        p = _plan_equals(cnt, rs.randint(0, 9, D), rs.randint(0, 10, D), D, 5, 2048, D, 1 << 50, 9, 10)
        assert 300 < p["n_kept"] < D and p["status"] == 0 and (np.diff(p["slot_box"][:p["n_kept"]]) > 0).all()
        _plan_equals(cnt, rs.randint(-1, 10, D), rs.randint(-1, 11, D), D - 5, 5, 700, 300, 1 << 36 if D == 777 else 9000, 9, 10)
    # ---- refusals: nothing is written
    cnt, frame, cls = _table()
    D, S, B = 12, 3, 4
    po = {k: torch.full(shape(D, S, B), -7, dtype=dt, device="cuda") for k, dt, shape in PLAN_OUT}
    po["status"] = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    pin = (_dev(cnt.astype(np.int32)), _dev(frame), _dev(cls), _dev(np.asarray([D], np.int32)))
    good = [_p(x) for x in pin] + [5, CAP, D, S, B, 10000, 3, 10] + [_p(po[k]) for k, _, _ in PLAN_OUT] + [_p(po["status"]), s]
    assert len(good) == 24
    for i in (0, 1, 2, 3) + tuple(range(12, 23)):
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_sunrgbd_detect_plan(*bad) == BADARG, i
    for i, v, rc in ((5, 0, BADARG), (6, -1, BADARG), (7, 0, BADARG), (8, 0, BADARG), (9, -1, BADARG), (10, -1, BADARG), (11, 0, BADARG),
                     (10, 2 ** 30, BADARG), (6, max_d + 1, LIMIT), (8, max_d + 1, LIMIT), (7, max_segs // D + 1, LIMIT)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_sunrgbd_detect_plan(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in po.values())
    # count and fill: the reading entries' argument refusals, and n_boxes
    sc = _scene(3)
    t = _tensors(sc)
    Db = t["bframe"].numel()
    nb = _dev(np.asarray([Db], np.int32))
    w = {"angle": torch.full((Db,), -7.0, dtype=torch.float64, device="cuda"), "scnt": torch.full((Db, 3), -7, dtype=torch.int32, device="cuda")}
    good = _common(t, 3) + [_p(nb), _p(w["angle"]), _p(w["scnt"]), s]
    for i in (0, 1, 4, 5, 6, 7, 10, 11, 12):
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_sunrgbd_detect_count(*bad) == BADARG, i
    for i, v in ((3, 2), (9, 0), (9, -1), (8, -1), (2, -1), (8, 65536)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_sunrgbd_detect_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in w.values())
    soff = torch.zeros(Db * 3 + 1, dtype=torch.int64, device="cuda")
    out = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda")
    goodf = good[:11] + [_p(soff), _p(out), s]
    for i in (0, 1, 4, 5, 6, 7, 10, 11, 12):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_frustum_sunrgbd_detect_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (9, 0), (8, -1), (8, 65536)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_frustum_sunrgbd_detect_fill(*bad) == BADARG, (i, v)
    assert L.fcn_frustum_sunrgbd_detect_fill(*goodf) == 0                   # (every slice empty: nothing to write)
    zero = list(good)
    zero[2] = 0                                                             # F = 0: the counts are zeroed, nothing else is written
    assert L.fcn_frustum_sunrgbd_detect_count(*zero) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and not w["scnt"].cpu().numpy().any() and (w["angle"].cpu().numpy() == -7.0).all()


# ------------------------------------------------------------------------------------------------ count / fill behind n_boxes
def _dcount(t, S, nb):
    from frustum_convnet_amd import _native
    D = t["bframe"].numel()
    o = {"angle": torch.full((D,), -7.0, dtype=torch.float64, device="cuda"), "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda")}
    nbt, nbuf = _guarded((1,), torch.int32, -7)
    nbt.fill_(nb)
    rc = _native.lib().fcn_frustum_sunrgbd_detect_count(*_common(t, S), _p(nbt), _p(o["angle"]), _p(o["scnt"]), _native.current_stream())
    torch.cuda.synchronize()
    assert _intact(nbuf, -7)
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _dfill(t, S, nb, seg_off, rows, guard=5):
    """The raw fill entry into a poisoned buffer of `rows` rows between `guard` poisoned rows -> rc, the rows, the guards intact."""
    from frustum_convnet_amd import _native
    ps = t["pts"].shape[1]
    buf = torch.full((rows + 2 * guard, ps), -7.0, dtype=torch.float32, device="cuda")
    soff, nbt = _dev(np.asarray(seg_off, dtype=np.int64)), _dev(np.asarray([nb], np.int32))
    rc = _native.lib().fcn_frustum_sunrgbd_detect_fill(*_common(t, S), _p(nbt), _p(soff), _p(buf[guard:]), _native.current_stream())
    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    return rc, h[guard:guard + rows], bool((h[:guard] == -7.0).all() and (h[guard + rows:] == -7.0).all())


@pytest.mark.parametrize("stride", [4, 6])
def test_selection_equals_the_reading_selection_byte_for_byte(stride):
    """The scene of tests/test_gpu_frustum_sunrgbd.py (frames of 0, 1, 63, 64, 65, 255, 4095, 4096, 4097 and 2 * 4096 + 100 rows, two
    boxes each and two more on the longest) with every box live; then with the boxes from 15 on beyond n_boxes and two frames out of
    range: they store nothing.  Stride 4 is the 16-byte path, stride 6 the word-by-word one."""
    sc = _scene(stride)
    S = sc["S"]
    t = _tensors(sc)
    D = len(sc["bframe"])
    rc, want = _count(t, S, label=False)
    assert rc == 0
    want = {k: v.cpu().numpy() for k, v in want.items()}
    rcf, wrows, _, _, wsoff = _fill(t, S, want["scnt"], label=False)
    assert rcf == 0 and len(wrows) > 1000
    rc, got = _dcount(t, S, D)
    assert rc == 0
    for k in ("scnt", "angle"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    assert got["scnt"][14].tolist() == want["scnt"][14].tolist() and want["scnt"][14].sum() > 0 and not want["scnt"][0].any()   # 4096 rows; 0 rows
    rc, rows, intact = _dfill(t, S, D, wsoff, len(wrows))
    assert rc == 0 and intact and np.array_equal(_bits(rows), _bits(wrows))
    # ---- boxes 15.. are not live; box 4 has frame F, box 10 frame -1 (exactly sized tables: nothing beyond them can be read)
    bframe = sc["bframe"].copy()
    bframe[4], bframe[10] = len(sc["lengths"]), -1
    t2 = _tensors(sc, bframe=bframe)
    rc, got = _dcount(t2, S, 15)
    dead = np.asarray([d in (4, 10) or d >= 15 for d in range(D)])
    assert rc == 0 and not got["scnt"][dead].any() and np.array_equal(got["scnt"][~dead], want["scnt"][~dead])
    assert (got["angle"][dead] == -7.0).all() and got["angle"][~dead].tobytes() == want["angle"][~dead].tobytes()
    rc, rows, intact = _dfill(t2, S, 15, wsoff, len(wrows))                 # granted the live run's rows: the dead store none of them
    assert rc == 0 and intact
    for d in range(D):
        a, b = int(wsoff[d * S]), int(wsoff[(d + 1) * S])
        assert (rows[a:b] == -7.0).all() if dead[d] else np.array_equal(_bits(rows[a:b]), _bits(wrows[a:b])), d
    assert want["scnt"][dead].sum() > 1000
    for nb in (0, -5):
        rc, got = _dcount(t, S, nb)
        assert rc == 0 and not got["scnt"].any() and (got["angle"] == -7.0).all()
        rc, rows, intact = _dfill(t, S, nb, wsoff, len(wrows))
        assert rc == 0 and intact and (rows == -7.0).all()


def test_count_plan_fill_on_frames_of_4096_4097_and_0_rows():
    """count -> plan -> fill on frames of exactly seg, seg + 1 and 0 rows (one box wider than the image and one inner box each), the
    capacity exactly met and one row short, into a buffer of exactly capacity + 1 rows between guard rows; equal to
    sunrgbd_candidates' rows of the boxes the existing rule keeps."""
    from frustum_convnet_amd import frustum
    from test_gpu_frustum_sunrgbd import INNER_2D, WHOLE_2D, _back_project, _calib
    seg, lengths = 4096, (4096, 4097, 0)
    rng = np.random.RandomState(5)
    K, Rt = _calib(3)
    frames = [np.concatenate([_back_project(rng, n, K[f], Rt[f]), rng.uniform(0, 1, (n, 3)).astype(np.float32)], 1) for f, n in enumerate(lengths)]
    sc = {"pts": np.concatenate(frames, 0), "off": np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), "K": K, "Rt": Rt,
          "boxes": np.asarray([WHOLE_2D, INNER_2D] * 3, dtype=np.float64), "bframe": np.repeat(np.arange(3), 2).astype(np.int32),
          "gt": np.zeros((6, 7))}
    t = _tensors(sc)
    rc, o = _dcount(t, 2, 6)
    assert rc == 0 and o["scnt"][0, 1] == 0 and o["scnt"][0, 0] > 2000 and 0 < o["scnt"][1].sum() < o["scnt"][0].sum() and not o["scnt"][4:].any()
    sel = frustum.sunrgbd_candidates(t["pts"], t["off"], t["K"], t["Rt"], t["boxes"], t["bframe"], cap=CAP)
    assert np.array_equal(sel["counts"], o["scnt"].sum(1)) and sel["frustum_angle"].cpu().numpy()[:4].tobytes() == o["angle"][:4].tobytes()
    last = sc["pts"][4096 + 4096]                                           # the one row of frame 1's second segment
    u, v, _ = fref.project(last[None, :3], K[1], Rt[1])
    assert o["scnt"][2, 1] == int(fref.box_mask(last[None, :3], u, v, sc["boxes"][2])[0])
    want_rows, woff = sel["points"].cpu().numpy(), sel["off"].cpu().numpy()
    total = int(o["scnt"].sum())
    for cap_rows, bit in ((total, 0), (total - 1, R.ST_TRUNC)):
        p = _plan_equals(o["scnt"], sc["bframe"], [0, 1, 2, 3, 4, 5], 6, 5, CAP, 5, cap_rows, 3, 10)
        assert p["status"] == bit and p["n_kept"] == 4 and p["slot_box"].tolist() == [0, 1, 2, 3, 6] and p["seg_off"][-1] == cap_rows
        rc, rows, intact = _dfill(t, 2, 6, p["seg_off"], cap_rows + 1)
        assert rc == 0 and intact and (rows[cap_rows] == -7.0).all() and np.array_equal(_bits(rows[:cap_rows]), _bits(want_rows[:cap_rows]))
        assert np.array_equal(p["off"][:4], woff[:4]) and p["counts"][:3].tolist() == sel["counts"][:3].tolist()
        assert (p["sub_len"][:4] == CAP).all() and p["slot_group"].tolist() == [0, 1, 12, 13, 30]


# ------------------------------------------------------------------------------------------------ fcn_det_rows
def _rows_equal(keep, cnt, dets, status0=0):
    """The raw entry on exactly sized, guarded buffers, held to the restatement; then fcn_box3d_corners over its rows: NaN exactly
    where the row is -1 or out of range -> the restatement's tuple."""
    from frustum_convnet_amd import _native
    keep, cnt, dets = np.asarray(keep, dtype=np.int32), np.asarray(cnt, dtype=np.int32), np.asarray(dets, dtype=np.float32).reshape(-1, 8)
    G, K = keep.shape
    nd = len(dets)
    ins = []
    for a, dt, fill in ((keep, torch.int32, -7), (cnt, torch.int32, -7), (dets if nd else np.zeros((1, 8), np.float32), torch.float32, -7.0)):
        v, buf = _guarded(a.shape, dt, fill)
        v.copy_(_dev(a))
        ins.append((v, buf, fill))
    o = {"det_off": _guarded((G + 1,), torch.int32, -7), "rows": _guarded((G * K,), torch.int32, -7), "scores": _guarded((G * K,), torch.float32, -7.0),
         "n_rows": _guarded((1,), torch.int32, -7), "corners": _guarded((G * K, 24), torch.float32, -7.0)}
    status, sbuf = _guarded((1,), torch.int32, status0)
    L, s = _native.lib(), _native.current_stream()
    rc = L.fcn_det_rows(_p(ins[0][0]), _p(ins[1][0]), G, K, _p(ins[2][0]) if nd else None, nd, _p(o["det_off"][0]), _p(o["rows"][0]),
                        _p(o["scores"][0]), _p(o["n_rows"][0]), _p(status), s)
    assert rc == 0 and L.fcn_box3d_corners(_p(ins[2][0]) if nd else None, nd, _p(o["rows"][0]), G * K, _p(o["corners"][0]), s) == 0
    torch.cuda.synchronize()
    assert all(_intact(buf, -7) for _, buf in o.values()) and _intact(sbuf, status0) and all(_intact(buf, f) for _, buf, f in ins)
    got = {k: v.cpu().numpy() for k, (v, _) in o.items()}
    det_off, rows, scores, n, st = R.det_rows(keep, cnt, dets)
    assert got["det_off"].tobytes() == det_off.tobytes() and got["rows"].tobytes() == rows.tobytes() and int(got["n_rows"][0]) == n
    assert np.array_equal(_bits(got["scores"]), _bits(scores)) and int(status.cpu()[0]) == (status0 | st)
    nan = R.corners(dets, rows)
    assert np.isnan(got["corners"][nan]).all() and np.isfinite(got["corners"][~nan]).all()
    return det_off, rows, scores, n, st


@pytest.mark.parametrize("G,K", [(1, 6), (255, 3), (256, 3), (257, 3), (40, 1), (7, 300)])
def test_det_rows_equals_the_restatement(G, K):
    """G = 1; a thread's run of groups going from one to two (255 / 256 / 257); top_k = 1; the chain's own top_k.  Counts of 0, top_k,
    beyond top_k and -1; keep entries that are -1, negative, equal to num_dets - 1, equal to num_dets and far beyond."""
    rs = np.random.RandomState(G * 1000 + K)
    nd = 50
    dets = rs.uniform(-3, 3, (nd, 8)).astype(np.float32)
    keep = rs.randint(0, nd, (G, K))
    cnt = rs.randint(0, K + 1, G)
    _, rows, scores, n, st = _rows_equal(keep, cnt, dets)
    assert st == 0 and n == cnt.sum() and not np.isnan(scores[:n]).any() and np.isnan(scores[n:]).all()
    cnt[0], cnt[G // 2], cnt[G - 1] = K, 0, K
    keep[0, 0], keep[G - 1, K - 1] = nd - 1, nd                            # the last row of dets; one past it
    if K > 2:
        keep[0, 1], keep[0, 2] = -1, 2 ** 31 - 1
    det_off, rows, scores, n, st = _rows_equal(keep, cnt, dets)
    assert rows[0] == nd - 1 and scores[0] == dets[nd - 1, 7] and rows[n - 1] == nd and np.isnan(scores[n - 1]) and st == 0
    if G > 2:
        cnt[1], cnt[G - 2] = -1, K + 5                                      # more than 4096 candidates; a count beyond top_k
        det_off, rows, scores, n, st = _rows_equal(keep, cnt, dets, status0=R.ST_TRUNC)
        assert st == R.ST_OVER and det_off[2] == det_off[1] and det_off[G - 1] - det_off[G - 2] == K
    _, rows, _, n, _ = _rows_equal(keep, np.zeros(G, np.int64), dets)
    assert n == 0 and (rows == -1).all()
    _, rows, scores, n, _ = _rows_equal(keep, np.full(G, K), dets[:0])      # no detection at all: every row is out of range
    assert n == G * K and np.isnan(scores).all()


def test_det_rows_refusals():
    from frustum_convnet_amd import _native
    L, s = _native.lib(), _native.current_stream()
    G, K = 5, 4
    i32 = dict(dtype=torch.int32, device="cuda")
    o = [torch.full((G + 1,), -7, **i32), torch.full((G * K,), -7, **i32), torch.full((G * K,), -7.0, dtype=torch.float32, device="cuda"),
         torch.full((1,), -7, **i32), torch.full((1,), -7, **i32)]
    keep, cnt, dets = torch.zeros((G, K), **i32), torch.zeros((G,), **i32), torch.zeros((9, 8), dtype=torch.float32, device="cuda")
    good = [_p(keep), _p(cnt), G, K, _p(dets), 9] + [_p(x) for x in o] + [s]
    for i in (0, 1, 4, 6, 7, 8, 9, 10):
        bad = list(good)
        bad[i] = None
        assert L.fcn_det_rows(*bad) == BADARG, i
    for i, v, rc in ((2, 0, BADARG), (3, 0, BADARG), (5, -1, BADARG), (2, 65537, LIMIT), (3, 4097, LIMIT)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_det_rows(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert all((x.cpu().numpy() == -7).all() for x in o)


# ------------------------------------------------------------------------------------------------ the builder pair
def test_alloc_infer_and_launch_infer_equal_build_device():
    g, dev, sel = _det_sel()
    b = _builder(g, False, False)
    types, prob = [str(x) for x in g["det_types"]], g["det_prob"]
    want = b.build_device(sel, dev["K"], dev["Rtilt"], types, prob, draws=(g["det_draw_choice"],))
    kept = want.pop("kept")
    B = len(kept)
    out = b.alloc_infer(B)
    assert sorted(out.keys()) == sorted(BATCH_KEYS) and not out["rgb_prob"].any() and not out["one_hot"].any()
    assert all(out[k].dtype == want[k].dtype and out[k].shape == want[k].shape for k in BATCH_KEYS)
    idx = _dev(kept)
    choice = g["det_draw_choice"].copy()
    for i, d in enumerate(kept):
        if sel["sub"][d] is not None:
            choice[i] = sel["sub"][d][choice[i]]
    t = {"raw": sel["points"], "off": sel["off"][idx].contiguous(), "choice": _dev(choice.astype(np.int32)),
         "fangle": sel["frustum_angle"][idx].contiguous(), "box2d": sel["box2d"][idx].contiguous(),
         "K": dev["K"].reshape(-1, 9)[sel["box_frame"][idx].long()].contiguous(),
         "R": dev["Rtilt"].reshape(-1, 9)[sel["box_frame"][idx].long()].contiguous(), "B": B, "pt_stride": int(sel["points"].shape[1])}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    got = b.launch_infer(t, out)
    torch.cuda.synchronize()
    assert got is out and {k: v.data_ptr() for k, v in out.items()} == ptrs
    for k in BATCH_KEYS:
        if k not in ("rgb_prob", "one_hot"):
            assert torch.equal(got[k].cpu(), want[k].cpu()), k
    assert not out["rgb_prob"].any() and not out["one_hot"].any()           # the caller's to write
    assert "one_hot" not in type(b)(b.npoints, b.strides, b.max_depth, one_hot=False).alloc_infer(2)


# ------------------------------------------------------------------------------------------------ SunrgbdDetectSource
def _types(g):
    return [str(x) for x in g["det_types"]]


def _source(B, D=7, capacity=14000, seed=SEED, cap=CAP, boxes=True, builder=None, **kw):
    from frustum_convnet_amd import frustum
    g = _golden()
    b = _builder(g, False, False) if builder is None else builder
    a = dict(frame_points=_dev(g["points"]), frame_off=g["off"], K=g["K"], Rtilt=g["Rtilt"])
    a.update(kw)
    src = frustum.SunrgbdDetectSource(a.pop("frame_points"), a.pop("frame_off"), a.pop("K"), a.pop("Rtilt"), b, B, D, capacity, seed,
                                      cap=cap, **a)
    if boxes:
        src.set_boxes(g["det_boxes"], g["det_frame"], _types(g), g["det_prob"])
    return src


def _sub_lists(src, D):
    """The source's per-slot subsample table as sunrgbd_candidates takes it: one entry per box, None without a subsample."""
    sb, so, sl, tab = (x.cpu().numpy() for x in (src.slot_box, src.sub_off, src.sub_len, src.sub))
    sub = [None] * D
    for i, d in enumerate(sb):
        if d < D and sl[i] > 0:
            sub[int(d)] = tab[so[i]:so[i] + sl[i]].astype(np.int64)
    return sub


def _existing(src, boxes=None, bframe=None, types=None, prob=None, points=None, nb=None):
    """The path the source replaces, fed the source's own draws: sunrgbd_candidates(sub=...) + build_device(draws=...) -> sel, batch."""
    from frustum_convnet_amd import frustum
    g = _golden()
    boxes, bframe = (g["det_boxes"] if boxes is None else boxes), (g["det_frame"] if bframe is None else bframe)
    types, prob = (_types(g) if types is None else types), (g["det_prob"] if prob is None else prob)
    nb = len(boxes) if nb is None else nb
    pts, foff, K, Rt = src.frames
    sel = frustum.sunrgbd_candidates(pts if points is None else points, foff, K, Rt, boxes[:nb], bframe[:nb], sub=_sub_lists(src, nb))
    n = int(src.n_kept.cpu()[0])
    return sel, src.builder.build_device(sel, K, Rt, types[:nb], prob[:nb], draws=(src.t["choice"][:n].clone(),),
                                         point_threshold=src.point_threshold)


def _host(x):
    return {k: v.cpu().clone() for k, v in x.items() if isinstance(v, torch.Tensor)}


def test_source_equals_the_existing_path_and_the_recorded_run():
    """B = the survivors, the capacity exactly met, the source's own subsample table and choice table handed to the existing path: the
    batch equals build_device(sunrgbd_candidates(...)) bit for bit in every key -- at the default bar of 5 rows (6 survivors, all
    subsampled at cap = 64) and at a bar of 1 (7 survivors, the 3-row box without a subsample).  Then cap = 2048 with the reference's
    recorded draws (det_sub, det_draw_choice): the batch is the reference loader's, at the bars of
    test_build_device_equals_the_loaders_batch."""
    g = _golden()
    mine = fref.select(g["points"], g["off"], g["K"], g["Rtilt"], g["det_boxes"], g["det_frame"])
    for thr, kept in ((5, g["det_kept"]), (1, np.arange(7))):
        total = int(mine["counts"][kept].sum())
        src = _source(len(kept), capacity=total, point_threshold=thr)
        assert src.S == 2 and src.points.shape == (total + 1, 6) and src.sub.numel() == len(kept) * CAP
        got = src.step()
        torch.cuda.synchronize()
        src.check()                                                         # nothing dropped, no empty slot: no bit
        assert sorted(got.keys()) == sorted(BATCH_KEYS + SLOT_KEYS)
        sel, want = _existing(src)
        assert np.array_equal(want.pop("kept"), kept) and sorted(want.keys()) == sorted(BATCH_KEYS)
        for k in BATCH_KEYS:
            assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and torch.equal(got[k].cpu(), want[k].cpu()), k
        assert got["slot_box"].cpu().numpy().tolist() == kept.tolist() and int(got["n_kept"].cpu()[0]) == len(kept)
        cls = np.asarray([src.builder.classes.index(t) for t in _types(g)])
        assert np.array_equal(got["slot_frame"].cpu().numpy(), g["det_frame"][kept]) and np.array_equal(got["slot_class"].cpu().numpy(), cls[kept])
        assert np.array_equal(got["slot_group"].cpu().numpy(), (g["det_frame"] * 10 + cls)[kept])
        assert np.array_equal(src.counts.cpu().numpy(), mine["counts"][kept]) and np.array_equal(src.seg_cnt.cpu().numpy().sum(1), mine["counts"])
        pts_h, off_h, want_pts, woff = src.points.cpu().numpy(), src.off.cpu().numpy(), sel["points"].cpu().numpy(), sel["off"].cpu().numpy()
        for i, d in enumerate(kept):                                        # the stored rows are sunrgbd_candidates' rows of the box
            assert np.array_equal(_bits(pts_h[off_h[i]:off_h[i] + mine["counts"][d]]), _bits(want_pts[woff[d]:woff[d + 1]])), d
        assert off_h[len(kept)] == total and not pts_h[total].any()
        sl, tab, so = src.sub_len.cpu().numpy(), src.sub.cpu().numpy(), src.sub_off.cpu().numpy()
        assert sl.tolist() == [CAP if mine["counts"][d] > CAP else 0 for d in kept] and (thr == 5 or sl[3] == 0)
        for i, d in enumerate(kept):                                        # a subsample: `cap` distinct rows of the box
            if sl[i]:
                ix = tab[so[i]:so[i] + CAP]
                assert len(set(ix.tolist())) == CAP and ix.min() >= 0 and ix.max() < mine["counts"][d]
        ch = src.t["choice"].cpu().numpy()
        for i, d in enumerate(kept):                                        # every drawn row is one of the record's
            record = set(tab[so[i]:so[i] + CAP].tolist()) if sl[i] else set(range(int(mine["counts"][d])))
            assert set(ch[i].tolist()) <= record, d
    # ---- the recorded run
    kept = g["det_kept"]
    total = int(mine["counts"][kept].sum())
    table = np.zeros((6, 2048), dtype=np.int32)
    table[:2] = g["det_sub"]                                                # the packed per-slot layout: the subsampled slots in order
    src = _source(6, capacity=total, cap=2048, sub=_dev(table.reshape(-1)), choice=_dev(g["det_draw_choice"].astype(np.int32)))
    got = src.step()
    torch.cuda.synchronize()
    src.check()
    assert got["slot_box"].cpu().numpy().tolist() == kept.tolist()
    assert got["slot_box"].cpu().numpy()[src.sub_len.cpu().numpy() > 0].tolist() == g["det_sub_box"].tolist()
    assert torch.equal(got["one_hot"].cpu(), torch.from_numpy(g["det_batch_one_hot"]))
    assert torch.equal(got["rgb_prob"].cpu(), torch.from_numpy(g["det_batch_rgb_prob"]))
    for k in ("point_cloud", "rot_angle", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "center_ref5"):
        _close(got[k].cpu().numpy(), g["det_batch_" + k], k)
    _, _, sel = _det_sel()                                                  # and bit for bit what build_device makes of the same draws
    want = src.builder.build_device(sel, src.frames[2], src.frames[3], _types(g), g["det_prob"], draws=(g["det_draw_choice"],))
    for k in BATCH_KEYS:
        assert torch.equal(got[k].cpu(), want[k].cpu()), k


def test_source_with_empty_slots():
    """B = survivors + 2: the filled slots' rows equal the existing path's, the empty slots hold the spare row's frustum over no rows,
    finite and the same every step; too few slots and too small a buffer are said."""
    g = _golden()
    kept = g["det_kept"]
    n = len(kept)
    src = _source(n + 2, D=9)
    first = _host(src.step())
    torch.cuda.synchronize()
    sel, want = _existing(src)
    for k in BATCH_KEYS:
        assert torch.equal(first[k][:n], want[k].cpu()), k
        assert torch.isfinite(first[k]).all(), k
    assert first["slot_box"].tolist() == kept.tolist() + [9, 9] and first["slot_group"][n:].tolist() == [20, 20]
    assert first["slot_frame"][n:].tolist() == [0, 0] and first["slot_class"][n:].tolist() == [0, 0] and not first["rgb_prob"][n:].any()
    assert first["one_hot"][n:].tolist() == [[1.0] + [0.0] * 9] * 2 and not src.t["choice"][n:].cpu().numpy().any()
    assert src.off.cpu().numpy()[n:n + 2].tolist() == [src.capacity] * 2 and not src.points[src.capacity].cpu().numpy().any()
    assert not src.sub_len.cpu().numpy()[n:].any() and src.counts.cpu().numpy()[n:].tolist() == [0, 0]
    rev = lambda a: np.ascontiguousarray(np.asarray(a)[::-1])
    src.set_boxes(rev(g["det_boxes"]), rev(g["det_frame"]), _types(g)[::-1], rev(g["det_prob"]))
    second = _host(src.step())
    torch.cuda.synchronize()
    assert second["slot_box"].tolist() == sorted((6 - kept).tolist()) + [9, 9]
    assert int(src.draws.state.cpu()[0]) == 2 and int(src.draws_sub.state.cpu()[0]) == 2
    for k in BATCH_KEYS:
        assert torch.equal(first[k][n:], second[k][n:]), k
    with pytest.raises(ValueError, match="bit 0") as e:                     # the draws' own bit: an empty slot has no row either
        src.check()
    assert not any("bit %d:" % i in str(e.value) for i in (1, 2, 4, 8, 10, 11))
    small = _source(n - 1, capacity=100)
    small.step()
    assert small.slot_box.cpu().numpy().tolist() == kept[:n - 1].tolist()
    with pytest.raises(ValueError, match="bit 8") as e:
        small.check()
    assert "bit 2:" in str(e.value) and "bit 10:" not in str(e.value)        # (bit 0 too: the slots behind the cut hold no row)
    assert small.counts.cpu().numpy().sum() == 100 and small.off.cpu().numpy()[-1] == 100
    assert small.sub_len.cpu().numpy().tolist() == [CAP, 0, 0, 0, 0]         # the first box alone stored more than cap rows
    ch, cnts = small.t["choice"].cpu().numpy(), small.counts.cpu().numpy()
    assert ((ch >= 0) & (ch < np.maximum(cnts, 1)[:, None])).all()           # no index points at a row that was not stored


def test_source_check_names_the_bits_and_clears():
    src = _source(4)
    src.check()
    for bit, name in ((R.ST_TRUNC, "bit 2"), (R.ST_MANY, "bit 8"), (R.ST_RANGE, "bit 10")):
        src.status.fill_(bit)
        with pytest.raises(ValueError, match=name) as e:
            src.check()
        assert int(src.status.cpu()[0]) == 0 and sum("bit %d:" % i in str(e.value) for i in (0, 1, 2, 4, 8, 10, 11)) == 1
    for d in (src.draws, src.draws_sub):
        d.status.fill_(1)
        with pytest.raises(ValueError, match="bit 0"):
            src.check()
        assert int(d.status.cpu()[0]) == 0
    src.check()
    # the kernels' own bit 10: a live box whose frame, then class, is out of range, then n_boxes beyond the table; cleared by check()
    for tab, v in ((src.box_frame, 2), (src.box_class, 10)):
        old = int(tab[1].cpu())
        tab[1] = v
        src.step()
        with pytest.raises(ValueError, match="bit 10"):
            src.check()
        assert 1 not in src.slot_box.cpu().numpy().tolist()
        tab[1] = old
    src.n_boxes.fill_(8)
    src.step()
    with pytest.raises(ValueError, match="bit 10"):
        src.check()
    assert src.slot_box.cpu().numpy().tolist() == [0, 1, 2, 4]


def test_source_refusals():
    from frustum_convnet_amd import frustum
    g = _golden()
    pts = _dev(g["points"])
    src = _source(4)
    assert src.frames[0].data_ptr() != pts.data_ptr() and _source(4, frame_points=pts).frames[0].data_ptr() == pts.data_ptr()   # held
    i32 = dict(dtype=torch.int32, device="cuda")
    for kw in (dict(frame_off=[0, 6000, 4862]), dict(frame_off=[0]), dict(frame_off=[0, 4862, 10 ** 6]), dict(frame_points=pts.double()),
               dict(frame_points=pts[:, :2].contiguous()), dict(frame_points=pts[::2]), dict(frame_points=g["points"]),
               dict(B=0), dict(B=8), dict(D=0), dict(D=2049), dict(capacity=0), dict(cap=0), dict(cap=10 ** 6), dict(point_threshold=2 ** 31),
               dict(K=g["K"][:1]), dict(Rtilt=g["Rtilt"][:1]), dict(sub=torch.zeros((4 * CAP - 1,), **i32)),
               dict(sub=torch.zeros((4 * CAP,), dtype=torch.int64, device="cuda")), dict(choice=torch.zeros((4, 511), **i32)),
               dict(choice=np.zeros((4, 512), np.int32))):
        kw = dict(kw)
        with pytest.raises(ValueError):
            _source(kw.pop("B", 4), D=kw.pop("D", 7), capacity=kw.pop("capacity", 4000), cap=kw.pop("cap", CAP), boxes=False, **kw)
    with pytest.raises(ValueError):                                         # D * S beyond the plan's segments
        _source(4, D=2048, boxes=False, frame_points=torch.zeros((4096 * 40, 6), dtype=torch.float32, device="cuda"),
                frame_off=[0, 4096 * 40, 4096 * 40])
    boxes, fr, prob, types = g["det_boxes"], g["det_frame"], g["det_prob"], _types(g)
    for args in ((boxes, fr[:6], types, prob), (boxes, fr, types[:6], prob), (boxes, fr, types, prob[:6]),
                 (np.concatenate([boxes, boxes[:1]]), np.concatenate([fr, fr[:1]]), types + ["bed"], np.concatenate([prob, prob[:1]])),
                 (boxes, np.where(np.arange(7) == 4, 2, fr), types, prob), (boxes, np.where(np.arange(7) == 4, -1, fr), types, prob),
                 (boxes, fr.astype(np.float64), types, prob), (boxes, fr, ["Tram"] + types[1:], prob),
                 (np.where(np.arange(28).reshape(7, 4) == 5, np.nan, boxes), fr, types, prob),
                 (boxes, fr, types, np.where(np.arange(7) == 2, np.inf, prob))):
        with pytest.raises(ValueError):
            src.set_boxes(*args)
    assert int(src.n_boxes.cpu()[0]) == 7 and np.array_equal(src.boxes2d.cpu().numpy()[:7], boxes)      # a refusal writes nothing
    assert src.boxes2d.cpu().numpy()[7].tolist() == [0, 0, 1, 1]
    assert int(src.set_boxes(boxes[:0], fr[:0], [], prob[:0]).n_boxes.cpu()[0]) == 0
    src.step()
    torch.cuda.synchronize()
    assert int(src.n_kept.cpu()[0]) == 0 and (src.slot_box.cpu().numpy() == 7).all() and int(src.status.cpu()[0]) == 0
    assert frustum.SunrgbdDetectSource.limits()[:2] == (2048, 65536)


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
    rev = lambda a: np.ascontiguousarray(np.asarray(a)[::-1])
    moved = g["points"].copy()
    moved[:, 0] += np.float32(0.4)
    first = (g["det_boxes"], g["det_frame"], _types(g), g["det_prob"])
    return (first + (g["points"], 7), (rev(g["det_boxes"]), rev(g["det_frame"]), _types(g)[::-1], rev(g["det_prob"]), moved, 7),
            first + (moved, 4))


def test_captured_source_step_replays_equal_eager_steps():
    """ONE capture of step(); three replays, the boxes, n_boxes and the frame points overwritten in place between them; every replay
    equals the eager step() of a twin on the same seed and the same data, bit for bit; both draws advance."""
    g = _golden()
    pa, pb = _dev(g["points"]), _dev(g["points"])
    src, twin = _source(6, frame_points=pa), _source(6, frame_points=pb)
    graph, out = _capture(src.step)
    assert int(src.draws.state.cpu()[0]) == 1 and int(src.draws_sub.state.cpu()[0]) == 1      # capturing runs nothing
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
        assert int(src.draws.state.cpu()[0]) == 2 + r == int(twin.draws.state.cpu()[0]) == int(src.draws_sub.state.cpu()[0])
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)
        assert torch.equal(src.points.cpu(), twin.points.cpu()) and torch.equal(src.sub.cpu(), twin.sub.cpu()) and int(got["n_kept"][0]) >= 3
        seen.append(got)
    assert not torch.equal(seen[0]["point_cloud"], seen[1]["point_cloud"]) and not torch.equal(seen[1]["slot_box"], seen[2]["slot_box"])
    assert int(src.status.cpu()[0]) == 0 and int(twin.status.cpu()[0]) == 0


# ------------------------------------------------------------------------------------------------ SunrgbdFrameChain
TOP_K = 6
CHAIN_TYPES = ["bed", "bed", "sofa", "desk", "toilet", "toilet", "bookshelf"]      # two (frame, class) groups of two boxes


def _chain(det, points, B, D=7, capacity=14000, seed=SEED, boxes=True, **kw):
    g = _golden()
    ch = det.frame_link(points, g["off"], g["K"], g["Rtilt"], B, D, capacity, seed, "nms", 0.1, top_k=TOP_K, cap=CAP, **kw)
    if boxes:
        ch.source.set_boxes(g["det_boxes"], g["det_frame"], CHAIN_TYPES, g["det_prob"])
    return ch


def _detector():
    from test_gpu_sunrgbd_detector import _setup
    from frustum_convnet_amd import evaluate
    g, b, m, dev, _ = _setup()
    return g, evaluate.SunrgbdDetector(m, b), dev


def test_frame_chain_equals_detect_frames_and_evaluates_alike():
    """Nothing dropped and B = the survivors: per (frame, class) group the kept rows, corners and scores equal detect_frames' bit for
    bit (detect_frames numbers the groups that hold a box, the chain all F * C of them); evaluate gives the same AP.  With two empty
    slots the chain equals model.detect run by hand on the chain's own batch, and no keep entry points at a row of an empty slot."""
    from frustum_convnet_amd import evaluate
    from frustum_convnet_amd.config import reset_cfg
    try:
        g, det, dev = _detector()
        kept = g["det_kept"]
        mine = fref.select(g["points"], g["off"], g["K"], g["Rtilt"], g["det_boxes"], g["det_frame"])
        ch = _chain(det, dev["points"], len(kept), capacity=int(mine["counts"][kept].sum()))
        assert isinstance(ch, evaluate.SunrgbdFrameChain) and ch.G == 20
        out = ch.step()
        torch.cuda.synchronize()
        ch.check()                                                          # nothing dropped, no empty slot: no bit
        assert sorted(out.keys()) == sorted(("dets", "valid", "keep", "cnt", "rows", "n_rows", "det_off", "corners", "scores", "batch",
                                             "slot_box", "n_kept"))
        got = ch.result()
        src = ch.source
        n = len(kept)
        res = det.detect_frames(dev["points"], dev["off"], dev["K"], dev["Rtilt"], g["det_boxes"], g["det_frame"], CHAIN_TYPES, g["det_prob"],
                                "nms", 0.1, top_k=TOP_K, draws=(src.t["choice"][:n].clone(),), sub=_sub_lists(src, 7))
        torch.cuda.synchronize()
        assert np.array_equal(res["kept"], kept) and np.array_equal(got["kept"], kept) and sorted(got.keys()) == sorted(res.keys())
        assert torch.equal(got["dets"].cpu(), res["dets"].cpu()) and torch.equal(got["valid"].cpu(), res["valid"].cpu())
        assert len(res["group_frame"]) == 4 and got["group_frame"].tolist() == [0] * 10 + [1] * 10 and got["group_class"].tolist() == list(range(10)) * 2
        assert got["det_off"].dtype == np.int64 and got["rows"].dtype == np.int64 and len(got["rows"]) == got["det_off"][-1] == len(res["rows"]) > 0
        gc, gs = got["corners"].cpu().numpy(), got["scores"].cpu().numpy()
        rc, rs = res["corners"].cpu().numpy(), res["scores"].cpu().numpy()
        seen = 0
        for q, (f, c) in enumerate(zip(res["group_frame"].tolist(), res["group_class"].tolist())):
            a, b = got["det_off"][f * 10 + c], got["det_off"][f * 10 + c + 1]
            x, y = res["det_off"][q], res["det_off"][q + 1]
            assert b - a == y - x > 0 and np.array_equal(got["rows"][a:b], res["rows"][x:y]), (f, c)
            assert np.array_equal(_bits(gc[a:b]), _bits(rc[x:y])) and np.array_equal(_bits(gs[a:b]), _bits(rs[x:y])), (f, c)
            assert torch.equal(got["keep"][f * 10 + c].cpu(), res["keep"][q].cpu()) and int(got["cnt"][f * 10 + c]) == int(res["cnt"][q])
            seen += b - a
        assert seen == len(got["rows"]) and int(got["cnt"].sum()) == seen    # the other sixteen groups are empty
        assert np.isnan(out["scores"].cpu().numpy()[seen:]).all() and (out["rows"].cpu().numpy()[seen:] == -1).all()
        assert np.isnan(out["corners"].cpu().numpy()[seen:]).all() and int(out["n_rows"].cpu()[0]) == seen
        # ---- the same AP
        classes = det.input_builder.classes
        shrink = lambda c: (c.mean(0, keepdims=True) + 0.9 * (c - c.mean(0, keepdims=True))).astype(np.float32)
        gt = np.stack([shrink(rc[0]), rc[0] + np.float32(40.0), shrink(rc[-1]), shrink(rc[0])])
        gt_frame, gt_class = [0, 0, 1, 1], [classes.index("bed")] * 2 + [classes.index("toilet"), classes.index("chair")]
        ev_c, ev_d = det.evaluate(got, gt, gt_frame, gt_class), det.evaluate(res, gt, gt_frame, gt_class)
        assert ev_c["classes"].tolist() == ev_d["classes"].tolist() and torch.equal(ev_c["ap"].cpu(), ev_d["ap"].cpu())
        assert torch.equal(ev_c["npos"].cpu(), ev_d["npos"].cpu()) and float(ev_c["ap"].sum()) > 0 and int(ev_c["tp"].sum()) == int(ev_d["tp"].sum()) >= 2
        # ---- two empty slots
        ce = _chain(det, dev["points"], n + 2, D=9)
        oe = ce.step()
        torch.cuda.synchronize()
        d, v, k, c = det.model.detect(oe["batch"], unit_group=ce.source.slot_group, num_groups=20, method="nms", thresh=0.1, top_k=TOP_K,
                                      rule="sunrgbd")
        for name, a, w in (("dets", oe["dets"], d), ("valid", oe["valid"], v), ("keep", oe["keep"], k), ("cnt", oe["cnt"], c)):
            assert torch.equal(a.cpu(), w.cpu()), name
        L2 = det.input_builder.L[1]
        k_h, c_h = oe["keep"].cpu().numpy(), oe["cnt"].cpu().numpy()
        assert c_h.sum() > 0 and all((k_h[q, :c_h[q]] >= 0).all() and (k_h[q, :c_h[q]] // L2 < n).all() for q in range(20))
        want = R.det_rows(k_h, c_h, oe["dets"].cpu().numpy())
        assert oe["det_off"].cpu().numpy().tobytes() == want[0].tobytes() and oe["rows"].cpu().numpy().tobytes() == want[1].tobytes()
        assert torch.isfinite(oe["dets"]).all() and all(torch.isfinite(x).all() for x in oe["batch"].values())
        re = ce.result()
        assert re["kept"].tolist() == kept.tolist() and len(re["rows"]) == want[3] and re["corners"].shape == (want[3], 8, 3)
        with pytest.raises(ValueError, match="bit 0") as e:
            ce.check()
        assert not any("bit %d:" % i in str(e.value) for i in (1, 2, 4, 8, 10, 11))
        ce.check()
        ce.status.fill_(R.ST_OVER)
        with pytest.raises(ValueError, match="bit 11"):
            ce.check()
        for kw in (dict(top_k=0), dict(top_k=4097), dict(method="best"), dict(thresh=float("nan"))):
            a = dict(method="nms", thresh=0.1, top_k=TOP_K)
            a.update(kw)
            with pytest.raises(ValueError):
                evaluate.SunrgbdFrameChain(det.model, ce.source, a["method"], a["thresh"], a["top_k"])
    finally:
        reset_cfg()


def test_captured_frame_chain_replays_on_new_boxes_equal_to_eager_steps():
    from frustum_convnet_amd.config import reset_cfg
    try:
        g, det, dev = _detector()
        pa, pb = _dev(g["points"]), _dev(g["points"])
        src, twin = (_chain(det, p, 7) for p in (pa, pb))
        graph, out = _capture(src.step)
        twin.step()
        seen = []
        for r, (boxes, fr, types, prob, points, nb) in enumerate(_rewrites()):
            for ch, p in ((src, pa), (twin, pb)):
                ch.source.set_boxes(boxes, fr, CHAIN_TYPES if r != 1 else CHAIN_TYPES[::-1], prob)
                ch.source.n_boxes.fill_(nb)
                p.copy_(_dev(points))
            graph.replay()
            torch.cuda.synchronize()
            got, gb = _host(out), _host(out["batch"])
            want_out = twin.step()
            torch.cuda.synchronize()
            want, wb = _host(want_out), _host(want_out["batch"])
            for k in ("dets", "valid", "keep", "cnt", "rows", "n_rows", "det_off", "slot_box", "n_kept"):
                assert torch.equal(got[k], want[k]), (r, k)
            for k in ("corners", "scores"):
                assert np.array_equal(_bits(got[k].numpy()), _bits(want[k].numpy())), (r, k)
            for k in wb:
                assert torch.equal(gb[k], wb[k]), (r, k)
            assert int(got["n_kept"][0]) >= 3 and int(got["n_rows"][0]) > 0
            seen.append(got)
        assert seen[1]["slot_box"].tolist() != seen[2]["slot_box"].tolist() and not torch.equal(seen[0]["dets"], seen[1]["dets"])
        assert int(src.source.status.cpu()[0]) == 0 and int(src.status.cpu()[0]) == 0
    finally:
        reset_cfg()
