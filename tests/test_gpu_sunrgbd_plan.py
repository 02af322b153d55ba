"""-m gpu: the capturable SUN-RGBD training input -- fcn_box2d_perturb_sunrgbd, fcn_frustum_sunrgbd_train_count / _plan / _fill /
_slots, fcn_frustum_subsample_draw and fcn_draw_batch_sliced (csrc/frustum_sunrgbd_plan.h) through the C-ABI against the numpy
restatement of tests/sunrgbd_plan_ref.py (pinned to the host path by tests/test_sunrgbd_plan_referee.py), and
frustum.SunrgbdTrainSource against the host path it replaces (the step's boxes and subsample table read back,
sunrgbd_training_candidates, SunrgbdInputBuilder.build_device_train), against the reference's recorded run, under a captured graph,
and through one training step.  The scene's generators are those of tests/test_gpu_frustum_sunrgbd.py;
tests/test_emu_sunrgbd_plan.py runs the same functions on the host emulation of the kernels (all but the graph captures)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import draws_ref
import frustum_sunrgbd_ref as ref
import sunrgbd_plan_ref as R
from test_gpu_frustum import BADARG, _bits, _dev, _p, _seg, _seg_counts
from test_gpu_frustum_sunrgbd import (FLOAT_KEYS, MAIN, MARGIN, MARGIN_PX, SECOND, WHOLE_2D, _back_project, _calib, _close, _common,
                                      _fixture_inputs, _frame_rows, _golden, _inside, _same_rows, _tensors)
from test_gpu_frustum_sunrgbd import _builder as _golden_builder
from test_gpu_frustum_sunrgbd import _count as _label_count
from test_gpu_frustum_sunrgbd import _fill as _label_fill

pytestmark = pytest.mark.gpu
LIMIT = 10002                      # FCN_E_LIMIT
LENGTHS = (3000, 9000, 5000)       # S = 3: the second frame's rows cross two segment boundaries
CAP, MIN = 64, 5
SEED = 20240611
# tiny label boxes nearer than any background row and above the others' image rows: their 2-D boxes select EXACTLY the rows put
# there (cx, cy, cz, l, w, h half extents, heading)
TINY = [(x, 0.9, 0.5, 0.06, 0.06, 0.06, 0.0) for x in (-0.5, -0.2, 0.1, 0.4)]
AIR = (0.0, 3.0, 5.0, 0.5, 0.5, 0.3, 2.6)
# (frame, label box, 2-D box or None = the label's image box grown by 10 px, exact rows or None, positives among them, first row)
LABELS = [(0, MAIN, None, None, 0, 0), (0, SECOND, None, None, 0, 0), (1, MAIN, None, None, 0, 0), (1, SECOND, None, None, 0, 0),
          (2, MAIN, None, None, 0, 0), (2, SECOND, None, None, 0, 0),
          (1, TINY[0], "cell", CAP - 1, 9, 4070), (1, TINY[1], "cell", CAP, 12, 8170), (1, TINY[2], "cell", CAP + 1, 6, 100),
          (1, TINY[3], "cell", 60, 3, 300),                                   # FEW: under the bar
          (1, AIR, WHOLE_2D, None, 0, 0),                                     # AIR: many rows, no positive
          (1, MAIN, WHOLE_2D, None, 0, 0),                                    # WIDE: more rows than the draws sort whole
          (2, SECOND, WHOLE_2D, None, 0, 0), (2, TINY[0], "cell", 30, 30, 4085)]
T63, T64, T65, FEW, AIRL, WIDE = 6, 7, 8, 9, 10, 11
GOOD4 = [0, 1, 2, 3]               # four labels that survive any perturbation
SHORT4 = [AIRL, 0, FEW, 1]         # two of four survive


def _image_box(gt, K, Rt, grow):
    c = ref.corners(gt)
    u, v, _ = ref.project(np.stack([c[:, 0], c[:, 2], -c[:, 1]], 1).astype(np.float32), K, Rt)
    return [u.min() - grow, v.min() - grow, u.max() + grow, v.max() + grow]


def _cell_points(rng, n, K, Rt, box):
    """n float32 upright-depth background points from pixels inside `box`, at 1.5 ... 6 m in front of the camera."""
    u, v, z = rng.uniform(box[0] + 1, box[2] - 1, n), rng.uniform(box[1] + 1, box[3] - 1, n), rng.uniform(1.5, 6.0, n)
    c0, c1 = (u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1]
    return (Rt @ np.stack([c0, z, -c1])).T.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _scene(stride):
    """F = 3 frames, G = 14 labels (LABELS).  Row i of a frame lies inside MAIN when i % 7 == 0, inside SECOND when i % 11 == 3,
    else it is background; the rows of a "cell" label are put there by hand -- its positives inside the tiny 3-D box, the others
    behind it -- and no other row projects into a cell; every row keeps the margins of the generators."""
    seg = _seg()
    F, G = len(LENGTHS), len(LABELS)
    rng = np.random.RandomState(700 + stride)
    K, Rt = _calib(F)
    gt = np.asarray([l[1] for l in LABELS], dtype=np.float64)
    bframe = np.asarray([l[0] for l in LABELS], dtype=np.int32)
    boxes = np.asarray([_image_box(l[1], K[l[0]], Rt[l[0]], 10.0 if l[2] is None else 3.0) if not isinstance(l[2], list) else l[2]
                        for l in LABELS], dtype=np.float64)
    frames = []
    for f, n in enumerate(LENGTHS):
        i = np.arange(n)
        owner = np.where(i % 7 == 0, -2, np.where(i % 11 == 3, -3, -1))          # MAIN, SECOND, background
        inside = np.zeros(n, dtype=bool)
        cells = [g for g in range(G) if bframe[g] == f and LABELS[g][2] == "cell"]
        for g in cells:
            _, _, _, rows, pos, first = LABELS[g]
            owner[first:first + rows] = g
            inside[first:first + pos] = True
        mine = np.nonzero(bframe == f)[0]
        xyz = np.zeros((n, 3), dtype=np.float32)
        todo = np.ones(n, dtype=bool)
        for _ in range(200):
            for code, box in ((-2, MAIN), (-3, SECOND)):
                m = todo & (owner == code)
                xyz[m] = _inside(rng, int(m.sum()), box)
            m = todo & (owner == -1)
            xyz[m] = _back_project(rng, int(m.sum()), K[f], Rt[f])
            for g in cells:
                m = todo & (owner == g) & inside
                xyz[m] = _inside(rng, int(m.sum()), LABELS[g][1])
                m = todo & (owner == g) & ~inside
                xyz[m] = _cell_points(rng, int(m.sum()), K[f], Rt[f], boxes[g])
            u, v, _ = ref.project(xyz, K[f], Rt[f])
            todo = np.zeros(n, dtype=bool)
            for d in mine:
                todo |= ref.face_distance(xyz, gt[d]) < MARGIN
                todo |= ref.edge_distance(u, v, boxes[d]) < MARGIN_PX
            for g in cells:
                sel = ref.box_mask(xyz, u, v, boxes[g])
                todo |= sel != (owner == g)                                  # exactly the rows put there
                todo |= (owner == g) & (ref.in_box(xyz, gt[g]) != inside)
            if not todo.any():
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (n, stride - 3)).astype(np.float32)], 1))
    pts = np.concatenate(frames, 0)
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    out = ref.select(pts, off, K, Rt, boxes, bframe, gt)
    S = 3
    assert -(-max(LENGTHS) // seg) == S
    out["seg_cnt"] = _seg_counts(out["index"], S, seg)
    cnt, pos = out["counts"], out["pos"]
    assert cnt[[T63, T64, T65, FEW, 13]].tolist() == [CAP - 1, CAP, CAP + 1, 60, 30] and pos[[T63, T64, T65, FEW, 13]].tolist() == [9, 12, 6, 3, 30]
    assert (out["seg_cnt"][[T63, T64, 13]] > 0).sum(1).tolist() == [2, 2, 2]                       # across a segment boundary
    assert pos[AIRL] == 0 and cnt[AIRL] > seg and (cnt[:6] > 4 * CAP).all() and (pos[:6] > 50).all()
    return {"pts": pts, "off": off, "K": K, "Rt": Rt, "boxes": boxes, "gt2d": boxes, "bframe": bframe, "gt": gt, "ref": out, "S": S,
            "seg": seg, "G": G}


def _types(b, G):
    return [b.classes[g % len(b.classes)] for g in range(G)]


def _builder(N=64, flip=True, shift=True):
    from frustum_convnet_amd.config import reset_cfg
    from frustum_convnet_amd.inputs import SunrgbdInputBuilder
    reset_cfg()
    return SunrgbdInputBuilder(N, (0.1, 0.2, 0.4, 0.8, 1.6), 8.0, random_flip=flip, random_shift=shift)


def _source(sc, B, D=12, seed=SEED, builder=None, capacity=60000, order=None, cap=CAP, **kw):
    from frustum_convnet_amd import frustum
    b = builder or _builder()
    g = np.arange(sc["G"]) if order is None else np.asarray(list(order) + [x for x in range(sc["G"]) if x not in order])
    types = [_types(b, sc["G"])[x] for x in g]
    src = frustum.SunrgbdTrainSource(_dev(sc["pts"]), sc["off"], sc["K"], sc["Rt"], sc["gt2d"][g], sc["gt"][g], sc["bframe"][g], types,
                                     b, B, D, capacity, seed, cap=cap, **kw)
    src.order, src.types = g, types
    return src


def _guarded(shape, dtype, fill, g=4):
    """A tensor of `shape` as a view into a buffer with g poisoned elements on either side -> (view, buffer)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * g,), fill, dtype=dtype, device="cuda")
    return buf[g:g + n].view(shape), buf


def _intact(buf, fill, g=4):
    h = buf.cpu()
    return bool((h[:g] == fill).all() and (h[-g:] == fill).all())


def _states(s):
    return [int(x.state.cpu()[0]) for x in (s.draws_pick, s.draws_box, s.draws_sample, s.draws_sub)]


# ------------------------------------------------------------------------------------------------ perturb
def _perturb(boxes, r, seed, step, advance, D=None):
    from frustum_convnet_amd import _native
    n = len(boxes)
    out, obuf = _guarded((n, 4), torch.float64, -7.0)
    state = _dev(np.asarray([step], dtype=np.int64))
    ins = _dev(boxes)                                                           # exactly sized
    rc = _native.lib().fcn_box2d_perturb_sunrgbd(_p(ins), n if D is None else D, r, seed, _p(state), advance, _p(out),
                                                 _native.current_stream())
    torch.cuda.synchronize()
    assert _intact(obuf, -7.0)
    return rc, out.cpu().numpy(), int(state.cpu()[0])


def _perturb_boxes(D):
    rs = np.random.RandomState(3)
    x0, y0 = rs.uniform(-60, 600, D), rs.uniform(-60, 400, D)
    return np.stack([x0, y0, x0 + rs.uniform(5, 190, D), y0 + rs.uniform(5, 110, D)], 1)


@pytest.mark.parametrize("step", [0, 1, 2 ** 32 + 5])
@pytest.mark.parametrize("D", [1, 300])
def test_perturb_equals_the_restatement_bit_for_bit(D, step):
    boxes = _perturb_boxes(D)
    want = R.perturb(SEED, step, boxes, 0.1)
    for advance in (0, 1):
        rc, got, state = _perturb(boxes, 0.1, SEED, step, advance)
        assert rc == 0 and state == step + advance
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (D, step, advance)
    assert not np.array_equal(got, boxes) and not np.array_equal(want, R.perturb(SEED, step + 1, boxes, 0.1))
    rc, got, state = _perturb(boxes, 0.1, SEED, step, 1, D=0)                   # the pass-through: only the counter moves
    assert rc == 0 and state == step + 1 and (got == -7.0).all()


# ------------------------------------------------------------------------------------------------ count and fill
def _train_count(t, S):
    from frustum_convnet_amd import _native
    D = t["bframe"].numel()
    f64 = dict(dtype=torch.float64, device="cuda")
    o = {"angle": torch.full((D,), -7.0, **f64), "scnt": torch.full((D, S), -7, dtype=torch.int32, device="cuda"),
         "spos": torch.full((D, S), -7, dtype=torch.int32, device="cuda"), "corners": torch.full((D, 24), -7.0, **f64)}
    rc = _native.lib().fcn_frustum_sunrgbd_train_count(*_common(t, S), _p(t["gt"]), _p(o["angle"]), _p(o["scnt"]), _p(o["spos"]),
                                                       _p(o["corners"]), _native.current_stream())
    torch.cuda.synchronize()
    return rc, o


@pytest.mark.parametrize("stride", [3, 6])
def test_no_read_count_and_fill_equal_the_label_entries_bit_for_bit(stride):
    from frustum_convnet_amd import _native
    sc = _scene(stride)
    S = sc["S"]
    t = _tensors(sc)
    rc, want = _label_count(t, S)
    assert rc == 0
    rc, got = _train_count(t, S)
    assert rc == 0 and all(torch.equal(got[k], want[k]) for k in want)
    scnt = want["scnt"].cpu().numpy()
    assert np.array_equal(scnt, sc["ref"]["seg_cnt"]) and np.array_equal(want["spos"].cpu().numpy().sum(1), sc["ref"]["pos"])
    counts = scnt.copy()
    counts[3] = 0                                                           # a box granted nothing
    counts[2, 1] -= 10                                                      # a segment granted too little
    rc, rows, lab, guard, soff = _label_fill(t, S, counts)
    assert rc == 0
    n = int(soff[-1])
    out = torch.full((n + 5, stride), -7.0, dtype=torch.float32, device="cuda")
    oseg = torch.full((n + 5,), -7, dtype=torch.int64, device="cuda")
    soff_d = _dev(soff)
    rc = _native.lib().fcn_frustum_sunrgbd_train_fill(*_common(t, S), _p(t["gt"]), _p(soff_d), _p(out), _p(oseg), _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(_bits(out.cpu().numpy()[:n]), _bits(rows)) and np.array_equal(oseg.cpu().numpy()[:n], lab)
    assert (out.cpu().numpy()[n:] == -7.0).all() and (oseg.cpu().numpy()[n:] == -7).all()
    # a frame out of range: the old pair reports it, the new pair skips the box silently -- the same outputs either way
    bframe = sc["bframe"].copy()
    bframe[5] = 3
    tb = _tensors(sc, bframe=bframe)
    rcw, want = _label_count(tb, S)
    rc, got = _train_count(tb, S)
    assert rcw == BADARG and rc == 0 and all(torch.equal(got[k], want[k]) for k in want) and not got["scnt"][5].any()
    # S too small for the longer frame is the caller's duty now: the old pair refuses, the new one searches S segments
    rc, short = _train_count(t, S - 1)
    assert rc == 0 and np.array_equal(short["scnt"].cpu().numpy(), scnt[:, :S - 1]) and _label_count(t, S - 1)[0] == BADARG


# ------------------------------------------------------------------------------------------------ plan, subsample, slots
def _chain(cnt, pos, labels, B, capacity, cap=CAP, min_pos=MIN, seed=SEED + 3, step=2):
    """plan -> subsample -> fcn_frustum_subset_pos -> slots through the raw entries on guarded, exactly sized buffers, each against
    the restatement.  labels: per box its rows' 0 / 1 labels (the packed seg buffer is what the fill would have stored)."""
    from frustum_convnet_amd import _native
    L, s = _native.lib(), _native.current_stream()
    D, S = cnt.shape
    i32, i64 = torch.int32, torch.int64
    o = {"seg_off": _guarded((D * S + 1,), i64, -7), "row0": _guarded((D,), i64, -7), "stored": _guarded((D,), i32, -7),
         "sub_off": _guarded((D + 1,), i64, -7), "status": _guarded((1,), i32, 0), "sub": _guarded((D * cap,), i32, -7),
         "pos": _guarded((D,), i32, -7), "slot_box": _guarded((B,), i32, -7), "n_kept": _guarded((1,), i32, -7),
         "off": _guarded((B,), i64, -7), "counts": _guarded((B,), i64, -7), "sub_start": _guarded((B,), i64, -7),
         "sub_len": _guarded((B,), i32, -7), "dstatus": _guarded((1,), i32, 0)}
    q = lambda k: _p(o[k][0])
    ins = (_dev(cnt.astype(np.int32)), _dev(pos.astype(np.int32)))
    assert L.fcn_frustum_sunrgbd_train_plan(_p(ins[0]), _p(ins[1]), min_pos, cap, D, S, capacity, q("seg_off"), q("row0"), q("stored"),
                                            q("sub_off"), q("status"), s) == 0
    seg_off, row0, stored, sub_off, st = R.plan(cnt, pos, min_pos, cap, capacity)
    torch.cuda.synchronize()
    h = lambda k: o[k][0].cpu().numpy()
    assert np.array_equal(h("seg_off"), seg_off) and np.array_equal(h("row0"), row0) and np.array_equal(h("stored"), stored)
    assert np.array_equal(h("sub_off"), sub_off) and int(h("status")[0]) == st
    state = _dev(np.asarray([step], dtype=np.int64))
    assert L.fcn_frustum_subsample_draw(q("stored"), q("sub_off"), D, cap, seed, _p(state), 1, q("sub"), q("dstatus"), s) == 0
    torch.cuda.synchronize()
    table = R.subsample(seed, step, stored, sub_off, cap, size=D * cap)
    got = h("sub")
    assert int(state.cpu()[0]) == step + 1 and int(h("dstatus")[0]) == 0
    assert np.array_equal(got[:int(sub_off[-1])], table[:int(sub_off[-1])]) and (got[int(sub_off[-1]):] == -7).all()
    for d in np.nonzero(np.diff(sub_off) > 0)[0]:                           # cap distinct indices into the STORED rows
        mine = got[int(sub_off[d]):int(sub_off[d + 1])]
        assert len(mine) == cap and len(set(mine.tolist())) == cap and mine.min() >= 0 and mine.max() < stored[d], d
    packed = np.concatenate([np.asarray(l, dtype=np.int64) for l, p in zip(labels, pos.sum(1)) if p >= min_pos] +
                            [np.zeros(0, dtype=np.int64)])[:max(capacity, 0)]
    assert len(packed) == seg_off[-1]
    seg_d = _dev(packed if len(packed) else np.zeros(1, dtype=np.int64))    # exactly sized: no row beyond the stored ones is read
    assert L.fcn_frustum_subset_pos(_p(seg_d), q("row0"), q("stored"), q("sub"), q("sub_off"), D, q("pos"), s) == 0
    torch.cuda.synchronize()
    after = R.subset_pos(packed, row0, stored, table, sub_off)
    assert np.array_equal(h("pos"), after)
    assert L.fcn_frustum_sunrgbd_train_slots(_p(ins[1]), q("pos"), q("row0"), q("stored"), q("sub_off"), min_pos, D, S, B, capacity,
                                             q("slot_box"), q("n_kept"), q("off"), q("counts"), q("sub_start"), q("sub_len"),
                                             q("status"), s) == 0
    torch.cuda.synchronize()
    slot_box, n, off, counts, sub_start, sub_len, st2 = R.slots(pos, after, row0, stored, sub_off, min_pos, B, capacity)
    for k, w in (("slot_box", slot_box), ("off", off), ("counts", counts), ("sub_start", sub_start), ("sub_len", sub_len)):
        assert np.array_equal(h(k), w), k
    assert int(h("n_kept")[0]) == n and int(h("status")[0]) == st | st2
    assert all(_intact(buf, 0 if "status" in k else -7) for k, (_, buf) in o.items())
    return {"stored": stored, "sub_off": sub_off, "after": after, "slot_box": slot_box, "n": n, "status": st | st2, "sub": got,
            "seg_off": seg_off}


def _hand_counts(D=12, S=3, seed=0, cap=CAP):
    """Boxes of cap - 1, cap, cap + 1 and many more rows; 1 and 6 under the bar of positives; 4 with exactly the bar among many
    rows (its subsample keeps fewer); 9 without a row."""
    rs = np.random.RandomState(seed)
    n = rs.randint(cap + 2, 12 * cap, D)
    n[[0, 2, 3, 9]] = [cap - 1, cap, cap + 1, 0]
    labels = [(rs.uniform(size=k) < 0.3).astype(np.int64) for k in n]
    for d, k in ((1, 3), (6, 4), (4, 5)):
        labels[d][:] = 0
        labels[d][rs.choice(n[d], k, replace=False)] = 1
    labels[4] = np.zeros(11 * cap, dtype=np.int64)
    labels[4][[5, 100, 300, 500, 700]] = 1
    n[4] = 11 * cap
    cut = [sorted(rs.randint(0, k + 1, S - 1).tolist()) for k in n]
    cnt = np.asarray([np.diff([0] + c + [k]) for c, k in zip(cut, n)], dtype=np.int64)
    pos = np.asarray([[int(l[a:b].sum()) for a, b in zip([0] + c, c + [k])] for l, c, k in zip(labels, cut, n)], dtype=np.int64)
    assert (cnt.sum(1) == n).all() and (pos.sum(1)[[0, 2, 3]] >= MIN).all()
    return cnt, pos, labels


@pytest.mark.parametrize("B", [4, 12])
def test_plan_subsample_and_slots_equal_the_restatement(B):
    cnt, pos, labels = _hand_counts()
    n = cnt.sum(1)
    r = _chain(cnt, pos, labels, B, 1 << 40)
    pre = pos.sum(1) >= MIN
    assert not pre[[1, 6, 9]].any() and pre.sum() == 9
    assert np.array_equal(r["stored"], np.where(pre, n, 0)) and np.array_equal(np.diff(r["sub_off"]) > 0, pre & (n > CAP))
    assert r["after"][4] < MIN <= pos[4].sum()                              # over the bar in all, under it after its subsample
    survivors = [d for d in range(12) if pre[d] and d != 4]
    assert r["slot_box"][:r["n"]].tolist() == survivors[:B] and r["n"] == min(B, 8) and r["status"] == (0 if B == 4 else R.ST_FEW)
    total = int(n[pre].sum())
    assert not _chain(cnt, pos, labels, B, total)["status"] & R.ST_TRUNC
    # one row short: bit 2, the last pre-kept box one row shorter; a capacity that cuts box 3 (cap + 1 rows) to cap: no subsample
    r = _chain(cnt, pos, labels, B, total - 1)
    last = np.nonzero(pre)[0][-1]
    assert r["status"] & R.ST_TRUNC and r["stored"][last] == n[last] - 1
    r = _chain(cnt, pos, labels, B, int(n[[0, 2, 3]].sum()) - 1)
    assert r["stored"][:4].tolist() == [CAP - 1, 0, CAP, CAP] and not r["stored"][4:].any() and r["sub_off"][-1] == 0
    # in the middle of a large box: its subsample comes from the rows that were stored
    r = _chain(cnt, pos, labels, B, int(n[[0, 2, 3]].sum()) + 3 * CAP)
    assert r["stored"][4] == 3 * CAP and np.diff(r["sub_off"]).tolist() == [0, 0, 0, CAP, CAP] + [0] * 7
    _chain(cnt, pos * 0, labels, B, 1 << 40)                                # none at all
    _chain(cnt, pos, labels, B, 0)                                          # no room at all


def test_plan_subsample_and_slots_at_their_smallest_and_over_many_boxes():
    one = (np.asarray([[7]]), np.asarray([[6]]), [np.asarray([1, 1, 1, 0, 1, 1, 1])])
    r = _chain(*one, 1, 100)
    assert (r["n"], r["status"]) == (1, 0) and r["stored"].tolist() == [7]
    assert _chain(one[0], one[1] * 0, one[2], 1, 100)["status"] == R.ST_FEW
    assert _chain(*one, 1, 100, cap=6)["sub_off"].tolist() == [0, 6]        # cap + 1 rows at D = B = S = 1
    assert _chain(*one, 1, 100, cap=1)["after"].tolist() == [1] and _chain(*one, 1, 100, cap=1, min_pos=1)["n"] == 1
    # more boxes than the workgroup has threads: the largest plan, S = 2
    rs = np.random.RandomState(1)
    D, S, cap = 2048, 2, 8
    cnt = rs.randint(0, 3 * cap, (D, S))
    labels = [(rs.uniform(size=k) < 0.5).astype(np.int64) for k in cnt.sum(1)]
    pos = np.asarray([[int(l[:a].sum()), int(l[a:].sum())] for l, a in zip(labels, cnt[:, 0])], dtype=np.int64)
    r = _chain(cnt, pos, labels, 300, 1 << 40, cap=cap)
    assert r["n"] == 300 and r["status"] == 0 and (np.diff(r["slot_box"]) > 0).all() and r["sub_off"][-1] > 500 * cap
    r = _chain(cnt, pos, labels, 2048, int(cnt.sum()) // 3, cap=cap)        # fewer than B and truncated at once
    assert r["status"] == R.ST_FEW | R.ST_TRUNC


@pytest.mark.parametrize("S", [1, 3])
@pytest.mark.parametrize("D", [255, 256, 257])
def test_plan_and_slots_where_a_threads_run_goes_from_one_box_to_two(D, S):
    """The run-per-thread split is csrc/slot_plan.h's, shared by every plan: over 256 threads, 255 and 256 boxes are runs of one
    (the last thread's empty, then not), 257 boxes are runs of two with threads 129.. owning nothing.  B = D, some boxes under
    the bar of positives, a capacity one row short of the total."""
    rs = np.random.RandomState(4 * D + S)
    cap = 8
    cnt = rs.randint(0, 3 * cap, (D, S))
    labels = [(rs.uniform(size=k) < 0.5).astype(np.int64) for k in cnt.sum(1)]
    ends = np.cumsum(cnt, 1)
    pos = np.asarray([[int(l[b - c:b].sum()) for c, b in zip(cs, es)] for l, cs, es in zip(labels, cnt, ends)], dtype=np.int64)
    total = int(R.plan(cnt, pos, MIN, cap, 1 << 40)[0][-1])
    r = _chain(cnt, pos, labels, D, total - 1, cap=cap)
    assert 0 < r["n"] < D and r["status"] == R.ST_FEW | R.ST_TRUNC and r["seg_off"][-1] == total - 1


def test_subsample_of_more_rows_than_the_draws_sort_whole():
    """cap = 2048 and boxes on either side of DeviceDraws.limits()[1]: the whole-row sort and the radix select."""
    from frustum_convnet_amd.inputs import DeviceDraws
    max_n, sort_cap = DeviceDraws.limits()
    rs = np.random.RandomState(2)
    n = np.asarray([sort_cap + 1, 2049, sort_cap, 3 * sort_cap + 77, 2048])
    cnt = n.reshape(-1, 1)
    labels = [(rs.uniform(size=k) < 0.4).astype(np.int64) for k in n]
    pos = np.asarray([[int(l.sum())] for l in labels])
    r = _chain(cnt, pos, labels, 5, 1 << 40, cap=max_n)
    assert max_n == 2048 and np.diff(r["sub_off"]).tolist() == [2048, 2048, 2048, 2048, 0] and r["n"] == 5


# ------------------------------------------------------------------------------------------------ the sliced draw
def _draw(fn_sliced, counts, N, seed, step, sub, a, b):
    """fcn_draw_batch (a = sub_off) or fcn_draw_batch_sliced (a = sub_start, b = sub_len) on guarded buffers."""
    from frustum_convnet_amd import _native
    B = len(counts)
    o = {"choice": _guarded((B, N), torch.int32, -7), "coin": _guarded((B,), torch.float64, -7.0),
         "normal": _guarded((B,), torch.float64, -7.0), "hshift": _guarded((B,), torch.float64, -7.0), "status": _guarded((1,), torch.int32, 0)}
    state = _dev(np.asarray([step], dtype=np.int64))
    keep = [_dev(np.asarray(counts, dtype=np.int64)), _dev(np.asarray(sub, dtype=np.int32)), _dev(np.asarray(a, dtype=np.int64))]
    desc = _native.DrawDesc(B, N, 1, 1)
    outs = [_p(o[k][0]) for k in ("choice", "coin", "normal", "hshift", "status")]
    if fn_sliced:
        keep.append(_dev(np.asarray(b, dtype=np.int32)))
        rc = _native.lib().fcn_draw_batch_sliced(ctypes.byref(desc), _p(keep[0]), _p(keep[1]), _p(keep[2]), _p(keep[3]), seed, _p(state),
                                                 *outs, _native.current_stream())
    else:
        rc = _native.lib().fcn_draw_batch(ctypes.byref(desc), _p(keep[0]), _p(keep[1]), _p(keep[2]), seed, _p(state), *outs,
                                          _native.current_stream())
    torch.cuda.synchronize()
    assert rc == 0 and int(state.cpu()[0]) == step + 1
    assert all(_intact(buf, 0 if k == "status" else -7) for k, (_, buf) in o.items())
    return {k: v.cpu().numpy() for k, (v, _) in o.items()}


def test_sliced_draw_equals_the_packed_draw_and_reads_the_right_slice():
    N, seed, step = 64, SEED + 2, 2 ** 32 + 1
    rs = np.random.RandomState(4)
    counts = [500, 40, 9000, 0, 300, 64]                                    # with a slice: 0, 2, 4; row 3 has nothing to draw from
    lens = [100, 0, 64, 0, 30, 0]
    slices = [rs.choice(c, k, replace=False).astype(np.int32) if k else np.zeros(0, np.int32) for c, k in zip(counts, lens)]
    sub_off = np.concatenate([[0], np.cumsum(lens)])
    packed = np.concatenate(slices)
    want = _draw(False, counts, N, seed, step, packed, sub_off, None)
    got = _draw(True, counts, N, seed, step, packed, sub_off[:-1], lens)
    assert all(np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)) for k in want) and got["status"][0] == 1
    ref_choice = draws_ref.draw(seed, step, counts, N, True, True, packed, sub_off)[0]
    assert np.array_equal(want["choice"], ref_choice)
    # the slices anywhere in the table, in another order, with poison between them
    table = np.full(400, -10 ** 6, dtype=np.int32)
    starts = [250, 7, 100, 3, 10, 399]
    for st, sl in zip(starts, slices):
        table[st:st + len(sl)] = sl
    got = _draw(True, counts, N, seed, step, table, starts, lens)
    assert all(np.array_equal(got[k].view(np.uint8), want[k].view(np.uint8)) for k in want)
    assert got["choice"].min() >= 0


# ------------------------------------------------------------------------------------------------ SunrgbdTrainSource
def _sub_list(src):
    off, table = src.sub_off.cpu().numpy(), src.sub.cpu().numpy()
    return [table[off[d]:off[d + 1]].copy() if off[d + 1] > off[d] else None for d in range(src.D)]


def _host_path(sc, src, rows=None):
    """The existing path on the step's boxes and subsample table read back, over the boxes `rows` (default: all D)."""
    from frustum_convnet_amd import frustum
    boxes = src.boxes.cpu().numpy()
    lab = src.order[src.pick_idx.cpu().numpy().reshape(-1)]
    sub = _sub_list(src)
    rows = np.arange(src.D) if rows is None else np.asarray(rows)
    return frustum.sunrgbd_training_candidates(_dev(sc["pts"]), _dev(sc["off"]), sc["K"], sc["Rt"], boxes[rows], sc["bframe"][lab[rows]],
                                               sc["gt"][lab[rows]], sub=[sub[d] for d in rows], cap=src.cap, min_positives=src.min_positives)


@pytest.mark.parametrize("D,stride,order,full", [(12, 3, None, True), (12, 6, None, True), (4, 6, GOOD4, True), (4, 3, SHORT4, False)],
                         ids=["D12-s3", "D12-s6", "D4-full", "D4-short"])
def test_step_equals_the_existing_path_on_the_same_boxes(D, stride, order, full):
    sc = _scene(stride)
    b = _builder()
    B = 4
    src = _source(sc, B, D=D, builder=b, order=order, pick=order is None)
    assert (src.S, src.D, src.G) == (3, D, 14)
    for step in range(2):
        got = src.step()
        torch.cuda.synchronize()
        pick = src.pick_idx.cpu().numpy().reshape(-1)
        if order is None:
            assert np.array_equal(pick, draws_ref.choice_row(SEED, step, 0, 14, D)) and len(set(pick.tolist())) == D
        else:
            assert pick.tolist() == list(range(D))
        lab = src.order[pick]
        boxes = src.boxes.cpu().numpy()
        assert np.array_equal(boxes.view(np.uint64), R.perturb(SEED + 1, step, sc["gt2d"][lab], 0.1).view(np.uint64))
        stored = src.cnt_stored.cpu().numpy()
        table = R.subsample(SEED + 3, step, stored, src.sub_off.cpu().numpy(), CAP, size=D * CAP)
        used = int(src.sub_off.cpu()[-1])
        assert used > 0 and np.array_equal(src.sub.cpu().numpy()[:used], table[:used])
        whole = _host_path(sc, src)                                         # every box: the kept list
        n = int(src.n_kept.cpu()[0])
        slot_box = src.slot_box.cpu().numpy()
        assert n == min(B, len(whole["kept"])) and np.array_equal(slot_box[:n], whole["kept"][:n]) and (slot_box[n:] == 0).all()
        assert n == B if full else n == 2                                   # (never a comparison of zero rows)
        sel = _host_path(sc, src, slot_box[:n])                             # the slots' boxes: their batch
        assert len(sel["kept"]) == n
        draws = tuple(src.t[k][:n].contiguous() for k in ("choice", "coin", "normal", "hshift"))
        want = b.build_device_train(sel, _dev(sc["K"]), _dev(sc["Rt"]), [src.types[g] for g in pick[slot_box[:n]]], draws=draws)
        torch.cuda.synchronize()
        assert sorted(got.keys()) == sorted(want.keys()) and "seg_label" in got and "one_hot" in got
        for k in want:
            assert got[k].dtype == want[k].dtype and got[k].shape[1:] == want[k].shape[1:] and got[k].shape[0] == B, k
            assert torch.equal(got[k][:n].cpu(), want[k].cpu()), (step, k)
        assert np.array_equal(src.counts.cpu().numpy()[:n], sel["counts"]) and np.array_equal(src.pos.cpu().numpy()[slot_box[:n]], sel["pos"].cpu().numpy())
        # the choice table is the restated draw through the step's slices
        lens = src.sub_len.cpu().numpy()
        for i in range(n):
            row = draws_ref.choice_row(SEED + 2, step, i, lens[i] if lens[i] else int(src.counts.cpu()[i]), b.npoints)
            sl = _sub_list(src)[slot_box[i]]
            assert np.array_equal(src.t["choice"][i].cpu().numpy(), row if sl is None else sl[row]), i
        if full:
            src.check()
        else:                                                               # empty slots: flagged by the slots and by the draw
            with pytest.raises(ValueError, match="bit 1") as e:
                src.check()
            assert "bit 0" in str(e.value) and "bit 2" not in str(e.value) and "bit 4" not in str(e.value)
            src.check()                                                     # cleared
            # an empty slot: box 0's labels over the spare row
            assert torch.equal(got["size_class"][n:].cpu(), src.g_class[pick[0]].cpu().expand(B - n, 1))
            assert (src.off.cpu().numpy()[n:] == src.capacity).all() and not got["point_cloud"][n:].isnan().any()
        assert _states(src) == [step + 1] * 4
    assert (got["seg_label"][:n].sum(1) > 0).all()


def test_exact_cells_are_subsampled_on_either_side_of_cap():
    """pick=False, perturb=False over all labels: the boxes of cap - 1 and cap rows have no subsample, cap + 1 and the large ones do;
    AIR and FEW never reach a slot."""
    sc = _scene(6)
    src = _source(sc, 12, D=14, pick=False, perturb=False)
    src.step()
    torch.cuda.synchronize()
    has = np.diff(src.sub_off.cpu().numpy()) > 0
    cnt = sc["ref"]["counts"]
    assert np.array_equal(src.cnt_stored.cpu().numpy(), np.where(sc["ref"]["pos"] >= MIN, cnt, 0))
    assert has[[T63, T64, T65, WIDE]].tolist() == [False, False, True, True] and not has[[AIRL, FEW]].any()
    whole = _host_path(sc, src)
    n = int(src.n_kept.cpu()[0])
    assert n == len(whole["kept"]) == 12 and np.array_equal(src.slot_box.cpu().numpy(), whole["kept"])
    assert AIRL not in whole["kept"] and FEW not in whole["kept"]
    src.check()


def test_large_cap_takes_the_radix_select_inside_a_step():
    from frustum_convnet_amd.inputs import DeviceDraws
    sc = _scene(3)
    src = _source(sc, 4, D=14, pick=False, perturb=False, cap=2048)
    got = src.step()
    torch.cuda.synchronize()
    stored, off = src.cnt_stored.cpu().numpy(), src.sub_off.cpu().numpy()
    assert stored[WIDE] > DeviceDraws.limits()[1] and off[WIDE + 1] - off[WIDE] == 2048
    mine = src.sub.cpu().numpy()[off[WIDE]:off[WIDE + 1]]
    assert np.array_equal(mine, draws_ref.choice_row(SEED + 3, 0, WIDE, stored[WIDE], 2048)) and len(set(mine.tolist())) == 2048
    assert int(src.n_kept.cpu()[0]) == 4 and torch.isfinite(got["point_cloud"]).all()
    src.check()


def test_overflow_is_truncated_flagged_and_stays_in_bounds():
    sc = _scene(6)
    total = int(sc["ref"]["counts"][sc["ref"]["pos"] >= MIN].sum())
    capacity = int(sc["ref"]["counts"][:3].sum()) + 3 * CAP + 7                 # in the middle of box 3
    src = _source(sc, 4, D=14, pick=False, perturb=False, capacity=capacity)
    # poisoned guards around points / seg / sub: the source's own buffers re-seated in guarded ones
    pts, pbuf = _guarded((capacity + 1, 6), torch.float32, -7.0, g=12)
    seg, sbuf = _guarded((capacity + 1,), torch.int64, -7)
    sub, ubuf = _guarded((14 * CAP,), torch.int32, -7)
    pts.zero_(), seg.zero_()
    src.points, src.seg, src.sub = pts, seg, sub
    src.t["raw"], src.t["seg"] = pts, seg
    got = src.step()
    torch.cuda.synchronize()
    stored, off = src.cnt_stored.cpu().numpy(), src.sub_off.cpu().numpy()
    assert total > capacity and int(src.seg_off.cpu()[-1]) == capacity and stored[3] == 3 * CAP + 7 and not stored[4:].any()
    assert stored.sum() == capacity and _intact(pbuf, -7.0, 12) and _intact(sbuf, -7) and _intact(ubuf, -7)
    assert not pts[capacity].any() and not seg[capacity].any()              # the spare row is never written
    table = sub.cpu().numpy()
    for d in np.nonzero(np.diff(off) > 0)[0]:                               # no index beyond the stored rows
        assert table[off[d]:off[d + 1]].max() < stored[d] and table[off[d]:off[d + 1]].min() >= 0
    assert (table[off[-1]:] == -7).all() and np.diff(off)[3] == CAP
    n = int(src.n_kept.cpu()[0])
    choice, cnts = src.t["choice"].cpu().numpy(), src.counts.cpu().numpy()
    assert n == 4 and all(choice[i].max() < cnts[i] for i in range(n)) and choice.min() >= 0
    with pytest.raises(ValueError, match="bit 2"):
        src.check()
    assert torch.isfinite(got["point_cloud"]).all()


def test_step_reproduces_the_references_recorded_run():
    """perturb=False, pick=False, B = D = G on the golden fixture's frames, recorded perturbed boxes, labels and subsample draws: the
    kept boxes, every row, label, the float32 box2d, corners and angles the reference recorded, and -- with the recorded draws written
    over the step's -- the reference loader's batch, to the bars of tests/test_gpu_frustum_sunrgbd.py."""
    from frustum_convnet_amd import frustum
    g = _golden()
    dev, boxes, bframe, gt = _fixture_inputs(g, "train")
    G = len(bframe)
    b = _golden_builder(g, True, True)
    types = [str(x) for x in g["train_types"]]
    src = frustum.SunrgbdTrainSource(dev["points"], g["off"], g["K"], g["Rtilt"], boxes, gt, bframe, types, b, G, G, 40000, 1,
                                     perturb=False, pick=False, select_box2d=boxes, sub=ref.fixture_sub(g, "train"),
                                     cap=int(g["meta_cap"]))
    got = src.step()
    torch.cuda.synchronize()
    kept = g["train_kept"]
    K = len(kept)
    assert int(src.n_kept.cpu()[0]) == K < G and np.array_equal(src.slot_box.cpu().numpy()[:K], kept)
    off_h, cnt_h = src.off.cpu().numpy(), src.counts.cpu().numpy()
    pts_h, seg_h = src.points.cpu().numpy(), src.seg.cpu().numpy()
    sub = _sub_list(src)
    pos_h = src.pos.cpu().numpy()
    for k, (d, index, label) in enumerate(ref.fixture_records(g, "train")):
        rows, lab = pts_h[off_h[k]:off_h[k] + cnt_h[k]], seg_h[off_h[k]:off_h[k] + cnt_h[k]]
        pick = slice(None) if sub[d] is None else sub[d]
        _same_rows(rows[pick], _frame_rows(g, int(g["train_box_frame"][d]), index), "box %d" % d)
        assert np.array_equal(lab[pick], label) and pos_h[d] == label.sum(), d
        assert (sub[d] is None) == (cnt_h[k] <= int(g["meta_cap"]))
    t = src.t
    assert np.array_equal(t["box2d"].cpu().numpy()[:K], g["train_box2d"].astype(np.float64))
    assert np.array_equal(t["heading"].cpu().numpy()[:K], g["train_heading"]) and np.array_equal(t["size"].cpu().numpy()[:K], g["train_size"])
    aerr = np.abs(t["fangle"].cpu().numpy()[:K] - g["train_angle"])
    cerr = np.abs(t["corners"].cpu().numpy()[:K].reshape(K, 8, 3) - g["train_box3d"])
    print("angle worst abs err %.3e, corners worst abs err %.3e" % (aerr.max(), cerr.max()))
    assert (aerr <= 1e-12).all() and (cerr <= 1e-12).all()
    with pytest.raises(ValueError, match="bit 1"):                         # K < B: said, not silent
        src.check()
    assert _states(src) == [1, 1, 1, 1]
    # the recorded draws in place of the step's: the reference loader's batch
    choice = g["train_draw_choice"].astype(np.int32).copy()
    for k, d in enumerate(kept):
        if sub[d] is not None:
            choice[k] = sub[d][choice[k]]
    t["choice"][:K].copy_(_dev(choice))
    for key, name in (("coin", "train_draw_coin"), ("normal", "train_draw_normal"), ("hshift", "train_draw_hshift")):
        t[key][:K].copy_(_dev(g[name]))
    got = b.launch(t, src.out)
    torch.cuda.synchronize()
    for k in ("cls_label", "seg_label", "size_class", "one_hot"):
        assert torch.equal(got[k][:K].cpu(), torch.from_numpy(g["train_batch_" + k])), k
    for k in FLOAT_KEYS:
        _close(got[k][:K].cpu().numpy(), g["train_batch_" + k], k)


def _snapshot(batch):
    return {k: v.cpu().clone() for k, v in batch.items()}


def test_captured_step_replays_fresh_batches_equal_to_eager_steps():
    sc = _scene(6)
    src, eager = _source(sc, 4), _source(sc, 4)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        first = src.step()                                                  # warm-up on a side stream: step 0
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in first.items()}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        before = torch.cuda.memory_stats()["allocation.all.allocated"]      # (behind the capture's own set-up)
        out = src.step()
        inside = torch.cuda.memory_stats()["allocation.all.allocated"]
    torch.cuda.synchronize()
    assert inside == before                                                 # step() allocates nothing in the captured region
    assert {k: v.data_ptr() for k, v in out.items()} == ptrs
    assert _states(src) == [1] * 4                                          # capturing runs nothing
    eager.step()
    seen = []
    for r in range(3):
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(out)
        want = _snapshot(eager.step())
        assert _states(src) == [2 + r] * 4 == _states(eager)
        for k in want:
            assert torch.equal(got[k], want[k]), (r, k)
        assert torch.equal(src.boxes.cpu(), eager.boxes.cpu()) and torch.equal(src.slot_box.cpu(), eager.slot_box.cpu())
        assert torch.equal(src.sub.cpu(), eager.sub.cpu())
        seen.append((got, src.boxes.cpu().clone()))
    assert not torch.equal(seen[0][0]["point_cloud"], seen[1][0]["point_cloud"]) and not torch.equal(seen[1][1], seen[2][1])
    # the four state words written back (the first replay read 1 and left 2): the same batch again
    for s in (src.draws_pick, src.draws_box, src.draws_sample, src.draws_sub):
        s.state.fill_(1)
    graph.replay()
    torch.cuda.synchronize()
    again = _snapshot(out)
    assert all(torch.equal(again[k], seen[0][0][k]) for k in again) and _states(src) == [2] * 4
    assert torch.equal(src.boxes.cpu(), seen[0][1])
    src.check()
    eager.check()


def test_one_training_step_on_a_step_batch():
    """The five-scale model with hash-initialised weights on a step() batch of the golden fixture's frames: finite losses, and
    backward() runs."""
    from frustum_convnet_amd.config import cfg, reset_cfg
    from frustum_convnet_amd import det_base_sunrgbd, frustum, synth
    g = _golden()
    dev, boxes, bframe, gt = _fixture_inputs(g, "train")
    b = _golden_builder(g, True, True)
    cfg.DATA.HEIGHT_HALF = tuple(float(x) for x in g["meta_strides"])
    cfg.DATA.STRIDE = cfg.DATA.HEIGHT_HALF
    cfg.DATA.DATASET_NAME = "SUNRGBD"
    cfg.DATA.MAX_DEPTH = float(g["meta_max_depth"])
    try:
        src = frustum.SunrgbdTrainSource(dev["points"], g["off"], g["K"], g["Rtilt"], boxes, gt, bframe, [str(x) for x in g["train_types"]],
                                         b, 3, 12, 40000, 5, cap=int(g["meta_cap"]))
        m = det_base_sunrgbd.PointNetDet(3, num_vec=10, num_classes=2)
        synth.fill_state_dict(m.state_dict(), seed=7)
        m = m.cuda().train()
        losses, _ = m(src.step())
        losses["total_loss"].backward()
        torch.cuda.synchronize()
        src.check()
        assert int(src.n_kept.cpu()[0]) == 3
        grads = [p.grad for p in m.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(x).all() for x in grads)
        print({k: float(v.detach()) for k, v in losses.items()})
        assert all(torch.isfinite(v).all() for v in losses.values()) and float(losses["total_loss"].detach()) > 0
    finally:
        reset_cfg()


# ------------------------------------------------------------------------------------------------ refusals
def test_constructor_refusals():
    from frustum_convnet_amd import frustum
    sc = _scene(3)
    b = _builder()
    base = dict(off=sc["off"], K=sc["K"], Rt=sc["Rt"], gt2d=sc["gt2d"], gt=sc["gt"], bframe=sc["bframe"], types=_types(b, 14), B=4, D=12,
                capacity=1000, seed=1)
    pts = _dev(sc["pts"])

    def mk(**kw):
        a = dict(base, **{k: v for k, v in kw.items() if k in base})
        opt = {k: v for k, v in kw.items() if k not in base}
        return frustum.SunrgbdTrainSource(pts, a["off"], a["K"], a["Rt"], a["gt2d"], a["gt"], a["bframe"], a["types"], b, a["B"], a["D"],
                                          a["capacity"], a["seed"], **opt)
    mk()
    bf_hi, bf_neg = sc["bframe"].copy(), sc["bframe"].copy()
    bf_hi[0], bf_neg[13] = 3, -1
    none12 = [None] * 12
    far = list(none12)
    far[2] = np.asarray([0, 10 ** 6])
    fixed = dict(perturb=False, pick=False, capacity=60000)
    for kw in (dict(off=np.asarray([0, 9000, 5000, 17000])), dict(off=np.asarray([0, 3000, 12000, 17001])), dict(off=np.asarray([0])),
               dict(K=sc["K"][:2]), dict(Rt=sc["Rt"][:2]), dict(bframe=bf_hi), dict(bframe=bf_neg), dict(gt2d=sc["gt2d"][:13]),
               dict(gt=sc["gt"][:13]), dict(types=_types(b, 13)), dict(types=["tram"] + _types(b, 14)[1:]),
               dict(D=2049), dict(D=15), dict(B=13), dict(B=0), dict(capacity=0), dict(shift_ratio=1.0), dict(shift_ratio=-0.1),
               dict(cap=0), dict(cap=2049), dict(select_box2d=sc["gt2d"]), dict(perturb=False, select_box2d=sc["gt2d"][:3]),
               dict(sub=none12), dict(perturb=False, sub=none12), dict(pick=False, sub=none12), dict(sub=none12[:11], **fixed),
               dict(sub=far, **fixed), dict(sub=none12, perturb=False, pick=False, capacity=1000)):
        with pytest.raises(ValueError):
            mk(**kw)
    mk(sub=none12, **fixed)
    with pytest.raises(ValueError):                                         # D * S beyond the plan's segments
        frustum.SunrgbdTrainSource(torch.zeros((4096 * 40, 3), dtype=torch.float32, device="cuda"), [0, 4096 * 40], sc["K"][:1], sc["Rt"][:1],
                                   np.tile(sc["gt2d"][:1], (2048, 1)), np.tile(sc["gt"][:1], (2048, 1)), np.zeros(2048, np.int32),
                                   [b.classes[0]] * 2048, b, 4, 2048, 10, 1)
    with pytest.raises(ValueError):
        frustum.SunrgbdTrainSource(torch.zeros((10, 2), dtype=torch.float32, device="cuda"), [0, 10], sc["K"][:1], sc["Rt"][:1], sc["gt2d"],
                                   sc["gt"], np.zeros(14, np.int32), _types(b, 14), b, 4, 12, 10, 1)
    assert frustum.SunrgbdTrainSource.limits() == (2048, 65536, 2048)


def test_entry_refusals_write_nothing():
    from frustum_convnet_amd import _native
    L, s = _native.lib(), _native.current_stream()
    i32, i64 = torch.int32, torch.int64
    full = lambda shape, dtype: torch.full(shape, -7, dtype=dtype, device="cuda")
    state = torch.zeros(1, dtype=i64, device="cuda")

    def refuse(fn, good, nulls, values, outs):
        for i in nulls:
            bad = list(good)
            bad[i] = None
            assert fn(*bad) == BADARG, (fn.__name__, i)
        for i, v, rc in values:
            bad = list(good)
            bad[i] = v
            assert fn(*bad) == rc, (fn.__name__, i, v)
        torch.cuda.synchronize()
        assert all((o.cpu().numpy() == -7).all() for o in outs) and int(state.cpu()[0]) == 0
    # ---- perturb
    boxes = _dev(_perturb_boxes(5))
    out = torch.full((5, 4), -7.0, dtype=torch.float64, device="cuda")
    good = [_p(boxes), 5, 0.1, 9, _p(state), 1, _p(out), s]
    refuse(L.fcn_box2d_perturb_sunrgbd, good, (0, 4, 6), ((1, -1, BADARG), (2, 1.0, BADARG), (2, -0.01, BADARG), (2, float("nan"), BADARG)), [out])
    assert L.fcn_box2d_perturb_sunrgbd(*good) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() != -7.0).all() and int(state.cpu()[0]) == 1
    state.zero_()
    # ---- plan
    cnt, pos, labels = _hand_counts()
    D, S, B = 12, 3, 4
    ins = (_dev(cnt.astype(np.int32)), _dev(pos.astype(np.int32)))
    o = {"seg_off": full((D * S + 1,), i64), "row0": full((D,), i64), "stored": full((D,), i32), "sub_off": full((D + 1,), i64), "status": full((1,), i32)}
    good = [_p(ins[0]), _p(ins[1]), MIN, CAP, D, S, 10000] + [_p(o[k]) for k in ("seg_off", "row0", "stored", "sub_off", "status")] + [s]
    refuse(L.fcn_frustum_sunrgbd_train_plan, good, (0, 1, 7, 8, 9, 10, 11),
           ((4, -1, BADARG), (5, 0, BADARG), (3, 0, BADARG), (6, -1, BADARG), (4, 2049, LIMIT), (5, 5462, LIMIT)), o.values())
    # ---- subsample
    stored, sub_off = _dev(np.asarray([100, 3], dtype=np.int32)), _dev(np.asarray([0, 64, 64], dtype=np.int64))
    sub, status = full((64,), i32), full((1,), i32)
    good = [_p(stored), _p(sub_off), 2, 64, 9, _p(state), 1, _p(sub), _p(status), s]
    refuse(L.fcn_frustum_subsample_draw, good, (0, 1, 5, 7, 8), ((2, -1, BADARG), (3, 0, BADARG), (3, 2049, LIMIT)), [sub, status])
    zero = list(good)
    zero[2] = 0                                                             # no box: only the counter moves
    assert L.fcn_frustum_subsample_draw(*zero) == 0
    torch.cuda.synchronize()
    assert int(state.cpu()[0]) == 1 and (sub.cpu().numpy() == -7).all()
    state.zero_()
    # ---- slots
    row0 = torch.zeros(D, dtype=i64, device="cuda")
    o2 = {"slot_box": full((B,), i32), "n_kept": full((1,), i32), "off": full((B,), i64), "counts": full((B,), i64),
          "sub_start": full((B,), i64), "sub_len": full((B,), i32), "status": full((1,), i32)}
    zs, zo = torch.zeros(D, dtype=i32, device="cuda"), torch.zeros(D + 1, dtype=i64, device="cuda")
    good = [_p(ins[1]), _p(zs), _p(row0), _p(zs), _p(zo), MIN, D, S, B, 10000] + [_p(v) for v in o2.values()] + [s]
    refuse(L.fcn_frustum_sunrgbd_train_slots, good, (0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 15, 16),
           ((6, -1, BADARG), (7, 0, BADARG), (8, 0, BADARG), (9, -1, BADARG), (6, 2049, LIMIT), (8, 2049, LIMIT), (7, 5462, LIMIT)), o2.values())
    # ---- the sliced draw
    counts = _dev(np.asarray([10, 20], dtype=np.int64))
    tab, st, ln = _dev(np.zeros(4, np.int32)), _dev(np.zeros(2, np.int64)), _dev(np.zeros(2, np.int32))
    o3 = {"choice": full((2, 8), i32), "coin": torch.full((2,), -7.0, dtype=torch.float64, device="cuda"),
          "normal": torch.full((2,), -7.0, dtype=torch.float64, device="cuda"), "status": full((1,), i32)}
    desc = _native.DrawDesc(2, 8, 1, 1)
    good = [ctypes.byref(desc), _p(counts), _p(tab), _p(st), _p(ln), 9, _p(state), _p(o3["choice"]), _p(o3["coin"]), _p(o3["normal"]), None,
            _p(o3["status"]), s]
    refuse(L.fcn_draw_batch_sliced, good, (0, 1, 2, 3, 4, 6, 7, 8, 9, 11), (), o3.values())
    for B_, N_, rc in ((0, 8, BADARG), (2, 0, BADARG), (2, 2049, LIMIT)):
        bad = list(good)
        bad[0] = ctypes.byref(_native.DrawDesc(B_, N_, 1, 1))
        assert L.fcn_draw_batch_sliced(*bad) == rc
    torch.cuda.synchronize()
    assert all((v.cpu().numpy() == -7).all() for v in o3.values()) and int(state.cpu()[0]) == 0
    assert L.fcn_draw_batch_sliced(*good) == 0                              # (hshift may be NULL)
    torch.cuda.synchronize()
    assert int(state.cpu()[0]) == 1 and (o3["choice"].cpu().numpy() >= 0).all()
    state.zero_()
    # ---- the no-read count and fill: the label entries' argument refusals
    sc = _scene(3)
    t = _tensors(sc)
    S, D = sc["S"], 14
    f64 = dict(dtype=torch.float64, device="cuda")
    w = {"angle": torch.full((D,), -7.0, **f64), "scnt": full((D, S), i32), "spos": full((D, S), i32), "corners": torch.full((D, 24), -7.0, **f64)}
    sizes = ((3, 2, BADARG), (9, 0, BADARG), (9, -1, BADARG), (8, -1, BADARG), (2, -1, BADARG), (8, 65536, BADARG))
    good = _common(t, S) + [_p(t["gt"]), _p(w["angle"]), _p(w["scnt"]), _p(w["spos"]), _p(w["corners"]), s]
    refuse(L.fcn_frustum_sunrgbd_train_count, good, (0, 1, 4, 5, 6, 7, 10, 11, 12, 13, 14), sizes, w.values())
    soff = torch.zeros(D * S + 1, dtype=i64, device="cuda")
    out, oseg = torch.full((4, 3), -7.0, dtype=torch.float32, device="cuda"), full((4,), i64)
    goodf = _common(t, S) + [_p(t["gt"]), _p(soff), _p(out), _p(oseg), s]
    refuse(L.fcn_frustum_sunrgbd_train_fill, goodf, (0, 1, 4, 5, 6, 7, 10, 11, 12, 13), sizes, [out, oseg])
    assert L.fcn_frustum_sunrgbd_train_fill(*goodf) == 0                    # (every slice empty: nothing to write)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all() and (oseg.cpu().numpy() == -7).all()


def test_check_raises_names_the_bits_and_clears():
    sc = _scene(3)
    src = _source(sc, 4)
    src.check()
    src.status.fill_(R.ST_FEW | R.ST_TRUNC)
    with pytest.raises(ValueError) as e:
        src.check()
    assert "bit 1" in str(e.value) and "bit 2" in str(e.value) and "bit 4" not in str(e.value) and "bit 0" not in str(e.value)
    src.check()
    for d in (src.draws_sample, src.draws_sub):
        d.status.fill_(1)
        with pytest.raises(ValueError, match="bit 0"):
            src.check()
        assert int(d.status.cpu()[0]) == 0
    src.check()
