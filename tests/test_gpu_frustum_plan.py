"""-m gpu: the capturable first-stage training input -- fcn_box2d_perturb, fcn_frustum_train_count / _plan / _fill
(csrc/frustum_plan.h) through the C-ABI against the numpy restatement of tests/frustum_plan_ref.py (pinned to the host path by
tests/test_frustum_plan_referee.py), and frustum.FrameTrainSource against the host path it replaces (perturb_boxes2d's boxes read
back, frustum_training_candidates, InputBuilder.build_device_train), against the reference's recorded run, under a captured
graph, and through one training step.  The scene's generators are those of tests/test_gpu_frustum_label.py / test_gpu_frustum.py;
tests/test_emu_frustum_plan.py runs the same functions on the host emulation of the kernels (all but the graph captures)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import draws_ref
import frustum_label_ref
import frustum_plan_ref as R
import frustum_ref
from test_gpu_frustum import BADARG, _back_project, _bits, _calib, _common, _dev, _p, _seg
from test_gpu_frustum_label import MARGIN, _golden, _inside_box
from test_gpu_frustum_label import _count as _label_count
from test_gpu_frustum_label import _fill as _label_fill

pytestmark = pytest.mark.gpu
LIMIT = 10002                      # FCN_E_LIMIT
LENGTHS = (5000, 9000)             # S = 3: the second frame's rows cross two segment boundaries
# per frame, tx ty tz l w h ry (rect camera, t the bottom centre): three cars, a pedestrian, a cyclist -- they survive; FAR has
# positives but a label box under 25 px; AIR holds no point
LABELS = ((-6.0, 1.6, 15.0, 3.9, 1.6, 1.5, 0.3), (0.0, 1.6, 20.0, 3.9, 1.6, 1.5, -1.2), (5.0, 1.6, 25.0, 3.9, 1.6, 1.5, 1.9),
          (-3.0, 1.7, 30.0, 0.8, 0.6, 1.8, 0.1), (8.0, 1.5, 12.0, 1.8, 0.6, 1.7, -2.5), (2.0, 1.6, 60.0, 3.9, 1.6, 1.5, 0.0),
          (-1.0, 0.2, 8.0, 1.0, 1.0, 1.0, 0.0))
TYPES = ("Car", "Car", "Car", "Pedestrian", "Cyclist", "Car", "Car")
FAR, AIR = 5, 6
SEED = 20240607
KEYS = ("pts", "off", "P", "V2C", "R0", "wh", "boxes", "bframe", "gt")


def _label_box2d(gt, P):
    """The image box of a 3-D label: its eight corners through P."""
    c = frustum_label_ref.corners(gt)
    img = np.concatenate([c, np.ones((8, 1))], 1) @ P.T
    u, v = img[:, 0] / img[:, 2], img[:, 1] / img[:, 2]
    return [u.min(), v.min(), u.max(), v.max()]


@functools.lru_cache(maxsize=None)
def _scene(stride):
    """F = 2 frames of 5 000 and 9 000 rows, G = 14 labels (LABELS in each frame).  Row i of a frame lies inside label i % 16 when
    that is < 6, else it is background outside every 3-D box; every row keeps MARGIN from every face plane."""
    seg = _seg()
    F = len(LENGTHS)
    rng = np.random.RandomState(500 + stride)
    P, V2C, R0, wh = _calib(F)
    gt = np.asarray([b for f in range(F) for b in LABELS], dtype=np.float64)
    bframe = np.repeat(np.arange(F), len(LABELS)).astype(np.int32)
    gt2d = np.asarray([_label_box2d(gt[g], P[bframe[g]].reshape(3, 4)) for g in range(len(gt))], dtype=np.float64)
    frames = []
    for f, n in enumerate(LENGTHS):
        W, H = wh[f]
        owner = np.arange(n) % 16
        xyz = np.zeros((n, 3), dtype=np.float32)
        todo = np.ones(n, dtype=bool)
        for _ in range(100):
            for k in range(AIR):
                m = todo & (owner == k)
                xyz[m] = _inside_box(rng, int(m.sum()), LABELS[k], V2C[f].reshape(3, 4), R0[f].reshape(3, 3))
            m = todo & (owner >= AIR)
            xyz[m] = _back_project(rng, int(m.sum()), P[f].reshape(3, 4), V2C[f].reshape(3, 4), R0[f].reshape(3, 3), W, H, inside=True)
            rect, _, _ = frustum_ref.project(xyz, P[f], V2C[f], R0[f])
            r32 = rect.astype(np.float32)
            todo = np.zeros(n, dtype=bool)
            for k, box in enumerate(LABELS):
                todo |= frustum_label_ref.face_distance(r32, box) < MARGIN
                todo |= frustum_label_ref.in_box(r32, box) != ((owner == k) & (k < AIR))
            if not todo.any():
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (n, stride - 3)).astype(np.float32)], 1))
    pts = np.concatenate(frames, 0)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    hgt = gt2d[:, 3] - gt2d[:, 1]
    assert (hgt[[FAR, FAR + 7]] < 25).all() and (np.delete(hgt, [FAR, FAR + 7]) >= 25).all()
    assert -(-max(LENGTHS) // seg) == 3
    return {"pts": pts, "off": off, "P": P, "V2C": V2C, "R0": R0, "wh": wh, "gt": gt, "gt2d": gt2d, "bframe": bframe,
            "types": [t for f in range(F) for t in TYPES], "S": 3, "seg": seg}


def _builder(N=64, flip=True, shift=True):
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    reset_cfg()
    return inputs.InputBuilder(N, strides=(0.25, 0.5, 1.0, 2.0), max_depth=70.0, random_flip=flip, random_shift=shift)


def _source(sc, B, D=12, seed=SEED, builder=None, capacity=40000, **kw):
    from frustum_convnet_amd import frustum
    cal = {k: _dev(sc[k]) for k in ("P", "V2C", "R0")}
    return frustum.FrameTrainSource(_dev(sc["pts"]), sc["off"], cal, sc["wh"], sc["gt2d"], sc["gt"], sc["bframe"], sc["types"],
                                    builder or _builder(), B, D, capacity, seed, **kw)


def _guarded(shape, dtype, fill, g=4):
    """A tensor of `shape` as a view into a buffer with g poisoned elements on either side -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device="cuda")
    return buf[g:g + n].view(shape), buf


def _intact(buf, fill, g=4):
    h = buf.cpu()
    return bool((h[:g] == fill).all() and (h[-g:] == fill).all())


# ------------------------------------------------------------------------------------------------ perturb
def _perturb(boxes, bframe, wh, r, seed, step, advance):
    """The raw entry on exactly sized, guarded buffers -> rc, out, status, state after."""
    from frustum_convnet_amd import _native
    D, F = len(bframe), len(wh)
    out, obuf = _guarded((D, 4), torch.float64, -7.0)
    status, sbuf = _guarded((1,), torch.int32, 0)
    state = _dev(np.asarray([step], dtype=np.int64))
    ins = (_dev(boxes), _dev(bframe), _dev(wh))                             # exactly sized
    rc = _native.lib().fcn_box2d_perturb(_p(ins[0]), _p(ins[1]), _p(ins[2]), D, F, r, seed, _p(state), advance, _p(out),
                                         _p(status), _native.current_stream())
    torch.cuda.synchronize()
    assert _intact(obuf, -7.0) and _intact(sbuf, 0)
    return rc, out.cpu().numpy(), int(status.cpu()[0]), int(state.cpu()[0])


def _perturb_boxes(D):
    """D boxes over two image sizes: plain ones and, every seventh, one that hangs over an image edge."""
    rs = np.random.RandomState(3)
    wh = np.asarray([[1242.0, 375.0], [1224.0, 370.0]])
    bframe = (np.arange(D) % 2).astype(np.int32)
    x0, y0 = rs.uniform(0, 1000, D), rs.uniform(0, 250, D)
    boxes = np.stack([x0, y0, x0 + rs.uniform(5, 190, D), y0 + rs.uniform(5, 110, D)], 1)
    W = wh[bframe, 0]
    edge = np.arange(D) % 7 == 6
    boxes[edge, 0], boxes[edge, 2] = W[edge] + 1.0, W[edge] + 60.0          # lands rarely: up to a dozen attempts
    return boxes, bframe, wh


# the seed at which the edge box of D = 1 below needs at least two attempts at step 0 (found by search on the restatement)
EDGE_SEED = 1


@pytest.mark.parametrize("step", [0, 1, 2 ** 32 + 5])
@pytest.mark.parametrize("D", [1, 300])
def test_perturb_equals_the_restatement_bit_for_bit(D, step):
    if D == 1:
        boxes, bframe, wh = np.asarray([[1245.5, 100.0, 1302.0, 160.0]]), np.zeros(1, np.int32), np.asarray([[1242.0, 375.0]])
        seed = EDGE_SEED
    else:
        boxes, bframe, wh = _perturb_boxes(D)
        seed = SEED
    want, used, fail = R.perturb(seed, step, boxes, wh[bframe], 0.1)
    assert not fail.any()                                                   # nobody exhausts the cap here
    if D == 1 and step == 0:
        assert used[0] >= 1                                                 # the pinned seed: a second attempt at least
    if D == 300:
        assert used.max() >= 2 and (used == 0).sum() > 200
    for advance in (0, 1):
        rc, got, status, state = _perturb(boxes, bframe, wh, 0.1, seed, step, advance)
        assert rc == 0 and status == 0 and state == step + advance
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (D, step, advance)
    assert not np.array_equal(got, boxes)


def test_perturb_failures_are_flagged_and_copy_the_input():
    """A box wholly beyond the image exhausts the cap; a frame out of range is never looked up: bit 4, the input copied out, the
    other boxes as the restatement has them."""
    boxes, bframe, wh = _perturb_boxes(9)
    boxes[4] = [1300.0, 100.0, 1400.0, 200.0]
    bframe = bframe.copy()
    bframe[7], bframe[2] = 2, -1
    whd = np.concatenate([wh, [[np.nan, np.nan]]], 0)[np.where((bframe < 0) | (bframe > 1), 2, bframe)]
    want, used, fail = R.perturb(SEED, 3, boxes, whd, 0.1)
    assert fail.tolist() == [d in (2, 4, 7) for d in range(9)]
    rc, got, status, state = _perturb(boxes, bframe, wh, 0.1, SEED, 3, 1)
    assert rc == 0 and status == R.ST_PERTURB and state == 4
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.array_equal(got[[2, 4, 7]], boxes[[2, 4, 7]])


# ------------------------------------------------------------------------------------------------ plan
def _plan(cnt, pos, gt2d, min_h, B, capacity):
    from frustum_convnet_amd import _native
    D, S = cnt.shape
    o = {"slot_box": _guarded((B,), torch.int32, -7), "seg_off": _guarded((D * S + 1,), torch.int64, -7),
         "off": _guarded((B + 1,), torch.int64, -7), "n_kept": _guarded((1,), torch.int32, -7), "status": _guarded((1,), torch.int32, 0)}
    ins = (_dev(cnt.astype(np.int32)), _dev(pos.astype(np.int32)), _dev(gt2d))
    rc = _native.lib().fcn_frustum_train_plan(_p(ins[0]), _p(ins[1]), _p(ins[2]), min_h, D, S, B, capacity, _p(o["slot_box"][0]), _p(o["seg_off"][0]), _p(o["off"][0]),
                                              _p(o["n_kept"][0]), _p(o["status"][0]), _native.current_stream())
    torch.cuda.synchronize()
    assert all(_intact(buf, 0 if k == "status" else -7) for k, (_, buf) in o.items())
    return rc, {k: v.cpu().numpy() for k, (v, _) in o.items()}


def _plan_equals(cnt, pos, gt2d, min_h, B, capacity):
    rc, got = _plan(cnt, pos, gt2d, min_h, B, capacity)
    slot_box, seg_off, off, n, st = R.plan(cnt, pos, gt2d, min_h, B, capacity)
    assert rc == 0
    assert np.array_equal(got["slot_box"], slot_box) and np.array_equal(got["seg_off"], seg_off) and np.array_equal(got["off"], off)
    assert int(got["n_kept"][0]) == n and int(got["status"][0]) == st
    return slot_box, seg_off, off, n, st


def _counts(D=12, S=3, seed=0):
    rs = np.random.RandomState(seed)
    cnt = rs.randint(0, 900, (D, S))
    pos = np.minimum(cnt, rs.randint(0, 40, (D, S)))
    pos[[1, 6]] = 0                                                         # no positive: dropped
    cnt[3, 1] = 0
    gt2d = np.stack([np.zeros(D), np.zeros(D), np.full(D, 50.0), rs.uniform(30, 90, D)], 1)
    gt2d[4, 3] = 24.999                                                     # fails the height rule alone
    assert pos[4].sum() > 0
    return cnt, pos, gt2d


@pytest.mark.parametrize("B", [4, 12])
def test_plan_equals_the_restatement(B):
    cnt, pos, gt2d = _counts()
    survivors = [d for d in range(12) if d not in (1, 4, 6)]
    slot_box, seg_off, off, n, st = _plan_equals(cnt, pos, gt2d, 25.0, B, 1 << 40)
    assert slot_box[:n].tolist() == survivors[:B] and n == min(B, 9) and st == (0 if B == 4 else R.ST_FEW)
    total = int(cnt[survivors[:B]].sum())
    assert off[n] == total and (off[n:] == total).all() and (slot_box[n:] == 0).all()
    # the height rule alone decides box 4
    assert 4 in _plan_equals(cnt, pos, gt2d, 24.0, 12, 1 << 40)[0]
    # one row short: bit 2, the last slot one row shorter; far short: several slots empty
    slot_box, seg_off, off, n, st = _plan_equals(cnt, pos, gt2d, 25.0, B, total - 1)
    assert st & R.ST_TRUNC and off[n] == total - 1 and off[n] - off[n - 1] == cnt[slot_box[n - 1]].sum() - 1
    assert not _plan_equals(cnt, pos, gt2d, 25.0, B, total)[4] & R.ST_TRUNC
    small = int(cnt[survivors[0]].sum()) + 5
    slot_box, seg_off, off, n, st = _plan_equals(cnt, pos, gt2d, 25.0, B, small)
    assert st & R.ST_TRUNC and (np.diff(off)[2:n] == 0).all() and off[1] == small - 5 and off[2] == small
    # none at all
    slot_box, seg_off, off, n, st = _plan_equals(cnt, pos * 0, gt2d, 25.0, B, 1 << 40)
    assert n == 0 and st == R.ST_FEW and not seg_off.any() and not off.any() and not slot_box.any()
    _plan_equals(cnt, pos, gt2d, 25.0, B, 0)                                # no room at all


def test_plan_at_its_smallest_and_over_many_boxes():
    one = (np.asarray([[7]]), np.asarray([[2]]), np.asarray([[0.0, 0.0, 10.0, 40.0]]))
    assert _plan_equals(*one, 25.0, 1, 100)[2].tolist() == [0, 7]           # B = D = 1
    assert _plan_equals(one[0], one[1] * 0, one[2], 25.0, 1, 100)[4] == R.ST_FEW
    # more boxes than the workgroup has threads, a box count that is no multiple of it, S = 5, counts whose sum passes 2^31
    rs = np.random.RandomState(1)
    D, S = 777, 5
    cnt = rs.randint(0, 2 ** 31 - 1, (D, S))
    pos = rs.randint(0, 2, (D, S)) * (rs.uniform(size=(D, 1)) < 0.6)
    gt2d = np.stack([np.zeros(D), np.zeros(D), np.full(D, 50.0), rs.uniform(10, 90, D)], 1)
    slot_box, seg_off, off, n, st = _plan_equals(cnt, pos.astype(np.int64), gt2d, 25.0, 300, 1 << 50)
    assert n == 300 and st == 0 and seg_off[-1] > 2 ** 33 and (np.diff(slot_box) > 0).all()
    _plan_equals(cnt, pos.astype(np.int64), gt2d, 25.0, 700, 1 << 36)       # fewer than B and truncated at once
    lim = _plan_limits()
    D = lim[0]                                                              # the largest plan: D boxes of max_segs / D segments
    S = lim[1] // D
    cnt = rs.randint(0, 50, (D, S))
    pos = (rs.uniform(size=(D, S)) < 0.02).astype(np.int64)
    gt2d = np.stack([np.zeros(D), np.zeros(D), np.full(D, 50.0), rs.uniform(10, 90, D)], 1)
    _plan_equals(cnt, pos, gt2d, 25.0, D, 1 << 40)


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [255, 256, 257])
def test_plan_where_a_threads_run_goes_from_one_box_to_two(D, S):
    """The run-per-thread split is csrc/slot_plan.h's, shared by every plan: over 256 threads, 255 and 256 boxes are runs of one
    (the last thread's empty, then not), 257 boxes are runs of two with threads 129.. owning nothing.  B = D, some boxes rejected,
    a capacity one row short of the total."""
    rs = np.random.RandomState(4 * D + S)
    cnt = rs.randint(0, 900, (D, S))
    pos = np.minimum(cnt, rs.randint(0, 40, (D, S))) * (rs.uniform(size=(D, 1)) < 0.7)
    gt2d = np.stack([np.zeros(D), np.zeros(D), np.full(D, 50.0), rs.uniform(10, 90, D)], 1)
    total = int(R.plan(cnt, pos, gt2d, 25.0, D, 1 << 40)[1][-1])
    slot_box, seg_off, off, n, st = _plan_equals(cnt, pos, gt2d, 25.0, D, total - 1)
    assert 0 < n < D and st == R.ST_FEW | R.ST_TRUNC and seg_off[-1] == total - 1 and (np.diff(slot_box[:n]) > 0).all()


def _plan_limits():
    from frustum_convnet_amd import _native
    a, b = ctypes.c_int(0), ctypes.c_int(0)
    assert _native.lib().fcn_frustum_train_plan_limits(ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value, b.value


# ------------------------------------------------------------------------------------------------ the no-read count and fill
def _scene_tensors(sc, boxes=None, bframe=None, gt=None):
    v = dict(sc, boxes=sc["gt2d"] if boxes is None else boxes, bframe=sc["bframe"] if bframe is None else bframe,
             gt=sc["gt"] if gt is None else gt)
    return {k: _dev(v[k]) for k in KEYS}


def _train_count(t, S, into=None):
    from frustum_convnet_amd import _native
    D = t["bframe"].numel()
    f64 = dict(dtype=torch.float64, device="cuda")
    o = into or {"box2d": torch.full((D, 4), -7.0, **f64), "angle": torch.full((D,), -7.0, **f64),
                 "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
                 "spos": torch.full((D, S), -7, dtype=torch.int32, device="cuda"), "corners": torch.full((D, 24), -7.0, **f64)}
    rc = _native.lib().fcn_frustum_train_count(*_common(t, S, False), _p(t["gt"]), _p(o["box2d"]), _p(o["angle"]), _p(o["scnt"]),
                                               _p(o["spos"]), _p(o["corners"]), _native.current_stream())
    return rc, o


def _train_fill(t, S, soff_d, out, oseg):
    from frustum_convnet_amd import _native
    return _native.lib().fcn_frustum_train_fill(*_common(t, S, False), _p(t["gt"]), _p(soff_d), _p(out), _p(oseg),
                                                _native.current_stream())


@pytest.mark.parametrize("stride", [4, 5])
def test_no_read_count_and_fill_equal_the_label_entries_bit_for_bit(stride):
    sc = _scene(stride)
    S = sc["S"]
    bframe = sc["bframe"].copy()
    t = _scene_tensors(sc)
    rc, want = _label_count(t, S)
    assert rc == 0
    rc, got = _train_count(t, S)
    torch.cuda.synchronize()
    assert rc == 0 and all(torch.equal(got[k], want[k]) for k in want)
    scnt = want["scnt"].cpu().numpy()
    spos = want["spos"].cpu().numpy().sum(1)
    assert (scnt[7:12] > 0).all() and (scnt.sum(1) > 0).all() and (spos[[AIR, AIR + 7]] == 0).all() and (np.delete(spos, [AIR, AIR + 7]) > 100).all()
    counts = scnt.copy()
    counts[3] = 0                                                           # a box granted nothing
    counts[9, 1] -= 10                                                      # a segment granted too little
    rc, rows, lab, guard, soff = _label_fill(t, S, counts)
    assert rc == 0
    n = int(soff[-1])
    out = torch.full((n + 5, stride), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((n + 5,), -7, dtype=torch.int64, device="cuda")
    rc = _train_fill(t, S, _dev(soff), out, oseg)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(_bits(out.cpu().numpy()[:n]), _bits(rows)) and np.array_equal(oseg.cpu().numpy()[:n], lab)
    assert (out.cpu().numpy()[n:] == -7.0).all() and (oseg.cpu().numpy()[n:] == -7).all()
    # a frame out of range: the old pair reports it, the new pair skips the box silently -- the same outputs either way
    bframe[5] = 2
    tb = _scene_tensors(sc, bframe=bframe)
    rcw, want = _label_count(tb, S)
    rc, got = _train_count(tb, S)
    torch.cuda.synchronize()
    assert rcw == BADARG and rc == 0 and all(torch.equal(got[k], want[k]) for k in want) and not got["scnt"][5].any()
    # S too small for the longer frame is the caller's duty now: the old pair refuses, the new one searches S segments
    rc, short = _train_count(t, S - 1)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(short["scnt"].cpu().numpy(), scnt[:, :S - 1]) and _label_count(t, S - 1)[0] == BADARG


def test_no_read_count_plan_and_fill_can_be_captured():
    """count -> plan -> fill captured into one graph; the replay's outputs equal the eager label entries' around the restated plan."""
    from frustum_convnet_amd import _native
    sc = _scene(4)
    S, D, B = sc["S"], len(sc["bframe"]), 6
    t = _scene_tensors(sc)
    gt2d = _dev(sc["gt2d"])
    rc, want = _label_count(t, S)
    slot_box, seg_off, off, n, st = R.plan(want["scnt"].cpu().numpy(), want["spos"].cpu().numpy(), sc["gt2d"], 25.0, B, 1 << 40)
    total = int(seg_off[-1])
    rc, rows, lab, _, _ = _label_fill(t, S, np.diff(seg_off).reshape(D, S))
    assert rc == 0 and n == B and total > 0
    _, o = _train_count(t, S)                                               # (also the warm-up)
    plan = {"slot_box": torch.zeros(B, dtype=torch.int32, device="cuda"), "seg_off": torch.zeros(D * S + 1, dtype=torch.int64, device="cuda"),
            "off": torch.zeros(B + 1, dtype=torch.int64, device="cuda"), "n_kept": torch.zeros(1, dtype=torch.int32, device="cuda"),
            "status": torch.zeros(1, dtype=torch.int32, device="cuda")}
    out = torch.full((total + 1, 4), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((total + 1,), -7, dtype=torch.int64, device="cuda")

    def enqueue():
        rc1, _ = _train_count(t, S, into=o)
        rc2 = _native.lib().fcn_frustum_train_plan(_p(o["scnt"]), _p(o["spos"]), _p(gt2d), 25.0, D, S, B, total, _p(plan["slot_box"]),
                                                   _p(plan["seg_off"]), _p(plan["off"]), _p(plan["n_kept"]), _p(plan["status"]),
                                                   _native.current_stream())
        rc3 = _train_fill(t, S, plan["seg_off"], out, oseg)
        return rc1, rc2, rc3
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        assert enqueue() == (0, 0, 0)
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    for k in o:
        o[k].fill_(-7)
    out.fill_(-7.0)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        assert enqueue() == (0, 0, 0)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()                                # capturing runs nothing
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(o[k], want[k]) for k in want)
    assert np.array_equal(plan["seg_off"].cpu().numpy(), seg_off) and np.array_equal(plan["slot_box"].cpu().numpy(), slot_box)
    assert np.array_equal(_bits(out.cpu().numpy()[:total]), _bits(rows)) and np.array_equal(oseg.cpu().numpy()[:total], lab)
    assert (out.cpu().numpy()[total:] == -7.0).all() and int(plan["status"].cpu()[0]) == 0


# ------------------------------------------------------------------------------------------------ FrameTrainSource
def _host_path(sc, src, builder, step, seed):
    """The existing path on the step's perturbed boxes read back: frustum_training_candidates + build_device_train with the
    restated draws of `step` -> (sel, batch)."""
    from frustum_convnet_amd import frustum
    boxes = src.boxes.cpu().numpy()
    lab = src.pick_idx.cpu().numpy().reshape(-1)
    cal = {k: _dev(sc[k]) for k in ("P", "V2C", "R0")}
    sel = frustum.frustum_training_candidates(_dev(sc["pts"]), _dev(sc["off"]), cal, sc["wh"], boxes, sc["bframe"][lab], sc["gt"][lab],
                                              gt_box2d=sc["gt2d"][lab])
    d = draws_ref.draw(seed + 2, step, sel["counts"], builder.npoints, builder.random_flip, builder.random_shift)
    return sel, builder.build_device_train(sel, cal["P"], [sc["types"][g] for g in lab], draws=d[:3]), lab


@pytest.mark.parametrize("B,stride", [(4, 4), (12, 4), (4, 5)])
def test_step_equals_the_existing_path_on_the_same_boxes(B, stride):
    sc = _scene(stride)
    b = _builder()
    src = _source(sc, B, builder=b)
    assert (src.S, src.D, src.G) == (3, 12, 14)
    for step in range(2):
        got = src.step()
        torch.cuda.synchronize()
        lab = src.pick_idx.cpu().numpy().reshape(-1)
        assert np.array_equal(lab, draws_ref.choice_row(SEED, step, 0, 14, 12)) and len(set(lab.tolist())) == 12
        boxes = src.boxes.cpu().numpy()
        want_boxes, _, fail = R.perturb(SEED + 1, step, sc["gt2d"][lab], sc["wh"][sc["bframe"][lab]], 0.1)
        assert not fail.any() and np.array_equal(boxes.view(np.uint64), want_boxes.view(np.uint64))
        sel, want, _ = _host_path(sc, src, b, step, SEED)
        K = len(sel["kept"])
        n = min(K, B)
        slot_box = src.slot_box.cpu().numpy()
        assert 8 <= K <= 10 and int(src.n_kept.cpu()[0]) == n
        assert np.array_equal(slot_box[:n], sel["kept"][:n]) and (slot_box[n:] == 0).all()
        assert sorted(got.keys()) == sorted(want.keys()) and "seg_label" in got and "one_hot" in got
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape[1:] == want[k].shape[1:] and got[k].shape[0] == B, k
            assert torch.equal(got[k][:n].cpu(), want[k][:n].cpu()), (step, k)
        off = src.off.cpu().numpy()
        assert np.array_equal(off[:n + 1], sel["off"].cpu().numpy()[:n + 1]) and (off[n:] == off[n]).all()
        if B == 4:
            src.check()
        else:                                                               # empty slots: flagged by the plan and by the draw
            with pytest.raises(ValueError, match="bit 1") as e:
                src.check()
            assert "bit 0" in str(e.value) and "bit 2" not in str(e.value) and "bit 4" not in str(e.value)
            src.check()                                                     # cleared
            # an empty slot: box 0's labels over the row behind the last one
            assert torch.equal(got["size_class"][n:].cpu(), src.g_class[lab[0]].cpu().expand(B - n, 1))
        assert [int(x.state.cpu()[0]) for x in (src.draws_pick, src.draws_box, src.draws_sample)] == [step + 1] * 3
    assert (got["seg_label"][:n].sum(1) > 0).all()


def test_overflow_is_truncated_flagged_and_stays_in_bounds():
    sc = _scene(4)
    src = _source(sc, 4, capacity=700, pick=False, perturb=False)
    got = src.step()
    torch.cuda.synchronize()
    off = src.off.cpu().numpy()
    assert off[-1] == 700 and int(src.seg_off.cpu()[-1]) == 700 and src.points.shape[0] == 701
    assert not src.points[700].any() and not src.seg[700].any()             # the spare row is never written
    with pytest.raises(ValueError, match="bit 2"):
        src.check()
    assert torch.isfinite(got["point_cloud"]).all()


def test_step_reproduces_the_references_recorded_run():
    """perturb=False, pick=False, B = D = G on the golden fixture's frames, recorded perturbed boxes and labels: the kept boxes, every
    label, row, corner and angle the reference recorded, to the bars of test_training_candidates_equal_the_references_recorded_run."""
    from frustum_convnet_amd import frustum
    from test_gpu_frustum import _check_rows
    g = _golden()
    G = len(g["box_frame"])
    cal = {k: _dev(g[k]) for k in ("P", "V2C", "R0")}
    src = frustum.FrameTrainSource(_dev(g["points"]), g["off"], cal, g["img_wh"], g["gt_box2d"], g["gt_box3d"], g["box_frame"],
                                   [str(x) for x in g["types"]], _builder(192), G, G, 20000, 1, perturb=False, pick=False,
                                   select_box2d=g["ref_boxes"])
    got = src.step()
    torch.cuda.synchronize()
    kept = np.nonzero(~g["ref_reject"])[0]
    K = len(kept)
    counts = g["ref_mask"].sum(1)[kept]
    assert int(src.n_kept.cpu()[0]) == K and np.array_equal(src.slot_box.cpu().numpy()[:K], kept)
    off_h = src.off.cpu().numpy()
    assert np.array_equal(off_h[:K + 1], np.concatenate([[0], np.cumsum(counts)])) and (off_h[K:] == counts.sum()).all()
    assert np.array_equal(src.both[0].sum(1).cpu().numpy()[kept], counts)
    assert np.array_equal(src.both[1].sum(1).cpu().numpy()[kept], g["ref_label"].sum(1)[kept])
    t = src.t
    assert np.array_equal(t["box2d"].cpu().numpy()[:K], g["ref_boxes"][kept])
    assert np.array_equal(t["heading"].cpu().numpy()[:K], g["gt_box3d"][kept, 6])
    assert np.array_equal(t["size"].cpu().numpy()[:K], g["gt_box3d"][kept, 3:6])
    assert np.array_equal(t["P"].cpu().numpy()[:K], g["P"][g["box_frame"][kept]].reshape(K, 12))
    aerr = np.abs(t["fangle"].cpu().numpy()[:K] - g["ref_angle"][kept])
    cerr = np.abs(t["corners"].cpu().numpy()[:K].reshape(K, 8, 3) - g["ref_corners"][kept])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all()
    pts_h, seg_h = src.points.cpu().numpy(), src.seg.cpu().numpy()
    for k, d in enumerate(kept):
        f = g["box_frame"][d]
        n = int(g["off"][f + 1] - g["off"][f])
        m = g["ref_mask"][d, :n]
        fr = slice(int(g["off"][f]), int(g["off"][f + 1]))
        want = np.concatenate([g["ref_rect"][fr][m], g["points"][fr][m, 3:]], 1)
        _check_rows(pts_h[off_h[k]:off_h[k + 1]], want, "box %d" % d)
        assert np.array_equal(seg_h[off_h[k]:off_h[k + 1]], g["ref_label"][d, :n][m].astype(np.int64)), d
    classes = src.builder.classes
    assert got["size_class"].cpu().numpy()[:K, 0].tolist() == [classes.index(str(g["types"][d])) for d in kept]
    with pytest.raises(ValueError, match="bit 1"):                         # K < B: said, not silent
        src.check()
    assert [int(x.state.cpu()[0]) for x in (src.draws_pick, src.draws_box, src.draws_sample)] == [1, 1, 1]


def _snapshot(batch):
    return {k: v.cpu().clone() for k, v in batch.items()}


def test_captured_step_replays_fresh_batches_equal_to_eager_steps():
    sc = _scene(4)
    src, eager = _source(sc, 4), _source(sc, 4)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        src.step()                                                          # warm-up on a side stream: step 0
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.step()
    torch.cuda.synchronize()
    states = lambda s: [int(x.state.cpu()[0]) for x in (s.draws_pick, s.draws_box, s.draws_sample)]
    assert states(src) == [1, 1, 1]                                         # capturing runs nothing
    eager.step()
    seen = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(out)
        want = _snapshot(eager.step())
        assert states(src) == [2 + r] * 3 == states(eager)
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)
        assert torch.equal(src.boxes.cpu(), eager.boxes.cpu()) and torch.equal(src.slot_box.cpu(), eager.slot_box.cpu())
        seen.append(got)
    assert not torch.equal(seen[0]["point_cloud"], seen[1]["point_cloud"]) and not torch.equal(seen[1]["point_cloud"], seen[2]["point_cloud"])
    assert states(src) == [1 + 3] * 3
    src.check()
    eager.check()


def test_one_training_step_on_a_step_batch():
    """The hash-initialised car_b4_n512 model on a step() batch: finite losses, and backward() runs."""
    from helpers import load_golden
    from test_gpu_model import _model
    from frustum_convnet_amd import inputs
    g1 = load_golden("car_b4_n512")
    m = _model(g1).train()
    b = inputs.InputBuilder(int(g1["meta_npoint"]), random_flip=True, random_shift=True)      # (cfg holds the model's strides)
    src = _source(_scene(4), 4, builder=b)
    losses, _ = m(src.step())
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    src.check()
    grads = [p.grad for p in m.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(x).all() for x in grads)
    print({k: float(v.detach()) for k, v in losses.items()})
    assert all(torch.isfinite(v).all() for v in losses.values()) and float(losses["total_loss"].detach()) > 0


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    from frustum_convnet_amd import frustum
    sc = _scene(4)
    mk = lambda **kw: _source(dict(sc, **{k: v for k, v in kw.items() if k in sc}), kw.get("B", 4), D=kw.get("D", 12),
                              capacity=kw.get("capacity", 1000), **{k: v for k, v in kw.items() if k in ("perturb", "shift_ratio", "select_box2d")})
    mk()
    bad2d = sc["gt2d"].copy()
    bad2d[3, 2] = bad2d[3, 0]
    beyond = sc["gt2d"].copy()
    beyond[2] = [1300.0, 100.0, 1400.0, 200.0]
    bf_hi, bf_neg = sc["bframe"].copy(), sc["bframe"].copy()
    bf_hi[0], bf_neg[13] = 2, -1
    for kw in (dict(off=np.asarray([0, 9000, 5000])), dict(off=np.asarray([0, 5000, 14001])), dict(off=np.asarray([0])),
               dict(bframe=bf_hi), dict(bframe=bf_neg), dict(gt2d=bad2d), dict(gt2d=beyond), dict(gt2d=sc["gt2d"][:13]),
               dict(gt=sc["gt"][:13]), dict(types=sc["types"][:13]), dict(types=["Tram"] + sc["types"][1:]),
               dict(D=2049), dict(D=15), dict(B=13), dict(B=0), dict(capacity=0), dict(shift_ratio=1.0), dict(shift_ratio=-0.1),
               dict(select_box2d=sc["gt2d"]), dict(perturb=False, select_box2d=sc["gt2d"][:3])):
        with pytest.raises(ValueError):
            mk(**kw)
    mk(gt2d=beyond, perturb=False)                                          # (an unperturbed box may lie anywhere)
    with pytest.raises(ValueError):                                         # D * S beyond the plan's segments
        frustum.FrameTrainSource(torch.zeros((4096 * 40, 4), dtype=torch.float32, device="cuda"), [0, 4096 * 40],
                                 {k: _dev(sc[k][:1]) for k in ("P", "V2C", "R0")}, sc["wh"][:1], np.tile(sc["gt2d"][:1], (2048, 1)),
                                 np.tile(sc["gt"][:1], (2048, 1)), np.zeros(2048, np.int32), ["Car"] * 2048, _builder(), 4, 2048, 10, 1)
    assert frustum.FrameTrainSource.limits() == (32, 2048, 65536)


def test_entry_refusals_write_nothing():
    from frustum_convnet_amd import _native
    L, s = _native.lib(), _native.current_stream()
    # ---- perturb
    boxes, bframe, wh = _perturb_boxes(5)
    out, obuf = _guarded((5, 4), torch.float64, -7.0)
    status, state = torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    keep = (_dev(boxes), _dev(bframe), _dev(wh))
    good = [_p(keep[0]), _p(keep[1]), _p(keep[2]), 5, 2, 0.1, 9, _p(state), 1, _p(out), _p(status), s]
    for i in (0, 1, 2, 7, 9, 10):
        bad = list(good)
        bad[i] = None
        assert L.fcn_box2d_perturb(*bad) == BADARG, i
    for i, v in ((3, -1), (4, -1), (5, 1.0), (5, -0.01), (5, float("nan"))):
        bad = list(good)
        bad[i] = v
        assert L.fcn_box2d_perturb(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and int(state.cpu()[0]) == 0 and int(status.cpu()[0]) == 0
    assert L.fcn_box2d_perturb(*good) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != -7.0).all() and int(state.cpu()[0]) == 1 and _intact(obuf, -7.0)
    zero = list(good)
    zero[3] = 0                                                             # no box: only the counter moves
    assert L.fcn_box2d_perturb(*zero) == 0
    torch.cuda.synchronize()
    assert int(state.cpu()[0]) == 2
    assert L.fcn_box2d_perturb_limits(None) == BADARG
    # ---- plan
    cnt, pos, gt2d = _counts()
    D, S, B = 12, 3, 4
    o = {"slot_box": torch.full((B,), -7, dtype=torch.int32, device="cuda"), "seg_off": torch.full((D * S + 1,), -7, dtype=torch.int64, device="cuda"),
         "off": torch.full((B + 1,), -7, dtype=torch.int64, device="cuda"), "n_kept": torch.full((1,), -7, dtype=torch.int32, device="cuda"),
         "status": torch.full((1,), -7, dtype=torch.int32, device="cuda")}
    ins = (_dev(cnt.astype(np.int32)), _dev(pos.astype(np.int32)), _dev(gt2d))
    good = [_p(ins[0]), _p(ins[1]), _p(ins[2]), 25.0, D, S, B, 10000] + [_p(o[k]) for k in ("slot_box", "seg_off", "off", "n_kept", "status")] + [s]
    for i in (0, 1, 2, 8, 9, 10, 11, 12):
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_train_plan(*bad) == BADARG, i
    for i, v, rc in ((4, -1, BADARG), (5, 0, BADARG), (6, 0, BADARG), (7, -1, BADARG), (4, 2049, LIMIT), (6, 2049, LIMIT), (5, 5462, LIMIT)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_train_plan(*bad) == rc, (i, v)
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o.values())
    assert L.fcn_frustum_train_plan(*good) == 0 and L.fcn_frustum_train_plan_limits(None, None) == BADARG
    torch.cuda.synchronize()
    assert int(o["n_kept"].cpu()[0]) == 4
    # ---- the no-read count and fill: the label entries' argument refusals
    sc = _scene(4)
    t = _scene_tensors(sc)
    S, D = sc["S"], 14
    f64 = dict(dtype=torch.float64, device="cuda")
    w = {"box2d": torch.full((D, 4), -7.0, **f64), "angle": torch.full((D,), -7.0, **f64),
         "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
         "spos": torch.full((D, S), -7, dtype=torch.int32, device="cuda"), "corners": torch.full((D, 24), -7.0, **f64)}
    good = _common(t, S, False) + [_p(t["gt"]), _p(w["box2d"]), _p(w["angle"]), _p(w["scnt"]), _p(w["spos"]), _p(w["corners"]), s]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17, 18, 19):
        bad = list(good)
        bad[i] = None
        assert L.fcn_frustum_train_count(*bad) == BADARG, i
    for i, v in ((3, 2), (11, 0), (11, -1), (10, -1), (2, -1), (10, 65536)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_frustum_train_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((w[k].cpu().numpy() == -7).all() for k in w)
    soff = torch.zeros(D * S + 1, dtype=torch.int64, device="cuda")
    out = torch.full((4, 4), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((4,), -7, dtype=torch.int64, device="cuda")
    goodf = good[:15] + [_p(soff), _p(out), _p(oseg), s]
    for i in (0, 1, 4, 5, 6, 7, 8, 9, 14, 15, 16, 17):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_frustum_train_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (11, 0), (11, -1), (10, -1), (2, -1), (10, 65536)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_frustum_train_fill(*bad) == BADARG, (i, v)
    assert L.fcn_frustum_train_fill(*goodf) == 0                            # (every slice empty: nothing to write)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (oseg.cpu().numpy() == -7).all()
    del keep


def test_check_raises_names_the_bits_and_clears():
    sc = _scene(4)
    src = _source(sc, 4)
    src.check()
    src.status.fill_(R.ST_PERTURB | R.ST_TRUNC)
    with pytest.raises(ValueError) as e:
        src.check()
    assert "bit 4" in str(e.value) and "bit 2" in str(e.value) and "bit 1" not in str(e.value) and "bit 0" not in str(e.value)
    src.check()
    src.draws_sample.status.fill_(1)
    with pytest.raises(ValueError, match="bit 0"):
        src.check()
    assert int(src.draws_sample.status.cpu()[0]) == 0
    src.check()
