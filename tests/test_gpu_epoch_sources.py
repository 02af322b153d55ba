"""GPU: the three capturable training sources with pick="epoch" (frustum.FrameTrainSource, frustum.SunrgbdTrainSource,
cascade.RefineTrainSource; inputs.EpochSampler, csrc/epoch_pick.h).  The scenes, builders and host-path helpers are those of
tests/test_gpu_frustum_plan.py, test_gpu_sunrgbd_plan.py and test_gpu_refine_plan.py, imported.  The referee of the label rows is
draws_ref.choice_row(seed, e, 0, G, G) and its windows; the referee of a batch is the SAME source class with pick=False over the
labels reordered by that window, its generators set to the same step: bit for bit in every key.  pick=True and pick=False keep what
they gave: one comparison each through the modules' own host-path helpers."""
import functools

import numpy as np
import pytest
import torch

import draws_ref

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _perm(seed, e, G):
    p = draws_ref.choice_row(seed, e, 0, G, G)
    p.setflags(write=False)
    return p


class _Kitti:
    """G = 14 labels, D = 4 per step: T = 3 turns and a tail of 2."""
    G, D, B = 14, 4, 2

    def __init__(self):
        import test_gpu_frustum_plan as TP
        self.TP, self.SEED, self.sc = TP, TP.SEED, TP._scene(4)

    def make(self, order=None, **kw):
        sc = self.sc
        if order is not None:
            g = np.asarray(list(order) + [x for x in range(self.G) if x not in order])
            sc = dict(sc, gt2d=sc["gt2d"][g], gt=sc["gt"][g], bframe=sc["bframe"][g], types=[sc["types"][x] for x in g])
        return self.TP._source(sc, self.B, D=self.D, builder=self.TP._builder(), **kw)

    idx = staticmethod(lambda s: s.pick_idx)
    gens = staticmethod(lambda s: (s.draws_pick, s.draws_box, s.draws_sample))
    kept = staticmethod(lambda s: (s.boxes, s.slot_box, s.n_kept, s.off))


class _Sunrgbd:
    G, D, B = 14, 4, 4

    def __init__(self):
        import test_gpu_sunrgbd_plan as TS
        self.TS, self.SEED, self.sc = TS, TS.SEED, TS._scene(6)

    def make(self, order=None, **kw):
        return self.TS._source(self.sc, self.B, D=self.D, builder=self.TS._builder(), order=None if order is None else list(order), **kw)

    idx = staticmethod(lambda s: s.pick_idx)
    gens = staticmethod(lambda s: (s.draws_pick, s.draws_box, s.draws_sample, s.draws_sub))
    kept = staticmethod(lambda s: (s.boxes, s.slot_box, s.n_kept, s.off, s.counts))


class _Refine:
    """R = 8 detections, D = 3 per step: T = 2 turns and a tail of 2; A = 3 jittered copies each."""
    G, D, B = 8, 3, 4

    def __init__(self):
        import test_gpu_refine_plan as TR
        self.TR, self.SEED, self.sc = TR, TR.SEED, TR._scene(4)

    def make(self, order=None, **kw):
        TR = self.TR
        if order is not None:
            dets, dframe, types = TR._table(self.sc)
            g = np.asarray(list(order) + [x for x in range(self.G) if x not in order])
            kw = dict(kw, dets=TR._dev(np.ascontiguousarray(dets[g])), det_frame=dframe[g], det_types=[types[x] for x in g])
        return TR._source(self.sc, self.B, D=self.D, builder=TR._builder(64, random_flip=True, random_shift=True), **kw)

    idx = staticmethod(lambda s: s.cand_row)
    gens = staticmethod(lambda s: (s.draws_pick, s.draws_jitter, s.draws_sample))
    kept = staticmethod(lambda s: (s.jitter, s.slot_unit, s.n_kept, s.off, s.gt_idx))


KINDS = {"kitti": _Kitti, "sunrgbd": _Sunrgbd, "refine": _Refine}


@functools.lru_cache(maxsize=None)
def _kind(name):
    return KINDS[name]()


def _states(k, s):
    return [int(x.state.cpu()[0]) for x in k.gens(s)]


def _epoch_state(s):
    return tuple(int(v) for v in s.sampler.state.cpu().tolist())


def _snapshot(batch):
    return {key: v.cpu().clone() for key, v in batch.items()}


def _same(got, want, what):
    assert sorted(got.keys()) == sorted(want.keys())
    for key in want:
        assert got[key].dtype == want[key].dtype and got[key].shape == want[key].shape, (what, key)
        assert torch.equal(got[key], want[key]), (what, key)


@pytest.mark.parametrize("name", list(KINDS))
def test_one_epoch_visits_distinct_labels_in_the_referees_windows(name):
    from frustum_convnet_amd import inputs
    k = _kind(name)
    G, D, T = k.G, k.D, k.G // k.D
    src = k.make(pick="epoch")
    assert isinstance(src.sampler, inputs.EpochSampler) and src.pick == "epoch" and src.sampler.seed == k.SEED
    assert src.sampler.steps_per_epoch(G, D) == T >= 2 and G % D != 0
    rows = []
    for t in range(T + 1):
        src.step()
        rows.append(k.idx(src).clone())
    torch.cuda.synchronize()
    rows = torch.stack(rows).cpu().numpy().reshape(T + 1, D)
    epoch = rows[:T].reshape(-1)
    assert np.array_equal(epoch, _perm(k.SEED, 0, G)[:T * D]) and len(np.unique(epoch)) == T * D
    assert np.array_equal(rows[T], _perm(k.SEED, 1, G)[:D])             # the tail is dropped: the next epoch's first window
    assert _epoch_state(src) == (1, 1) and _states(k, src) == [T + 1] * len(k.gens(src))
    try:
        src.check()
    except ValueError as err:                                            # (a scene's empty slots are the plans' to flag)
        assert "bit 12" not in str(err)


@pytest.mark.parametrize("name", list(KINDS))
def test_a_turns_batch_equals_a_pick_false_source_on_the_reordered_labels(name):
    k = _kind(name)
    G, D = k.G, k.D
    e, t, step = 2, 1, 5
    window = _perm(k.SEED, e, G)[t * D:(t + 1) * D]
    src = k.make(pick="epoch")
    ref = k.make(order=[int(x) for x in window], pick=False)
    assert ref.sampler is None and ref.pick is False
    src.sampler.state.copy_(torch.tensor([e, t], dtype=torch.int64))
    for a, b in zip(k.gens(src), k.gens(ref)):
        a.state.fill_(step)
        b.state.fill_(step)
    got = _snapshot(src.step())
    want = _snapshot(ref.step())
    torch.cuda.synchronize()
    assert np.array_equal(k.idx(src).cpu().numpy().reshape(-1), window)
    assert k.idx(ref).cpu().numpy().reshape(-1).tolist() == list(range(D))
    _same(got, want, name)
    for a, b in zip(k.kept(src), k.kept(ref)):
        assert torch.equal(a.cpu(), b.cpu())
    assert int(src.n_kept.cpu()[0]) >= 1                                 # (never a comparison of empty batches)
    assert _states(k, src) == _states(k, ref) == [step + 1] * len(k.gens(src))
    assert _epoch_state(src) == ((e, t + 1) if t + 1 < G // D else (e + 1, 0))


@pytest.mark.parametrize("name", list(KINDS))
def test_captured_step_replays_across_an_epoch_boundary_equal_to_eager_steps(name):
    k = _kind(name)
    T = k.G // k.D
    src, eager = k.make(pick="epoch"), k.make(pick="epoch")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        src.step()                                                      # warm-up on a side stream: turn 0
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = src.step()
    torch.cuda.synchronize()
    assert _epoch_state(src) == (0, 1) and _states(k, src) == [1] * len(k.gens(src))      # capturing runs nothing
    eager.step()
    seen = []
    for r in range(T + 1):                                              # turns 1 .. T - 1 of epoch 0, then epoch 1
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(out)
        want = _snapshot(eager.step())
        _same(got, want, (name, r))
        assert torch.equal(k.idx(src).cpu(), k.idx(eager).cpu())
        for a, b in zip(k.kept(src), k.kept(eager)):
            assert torch.equal(a.cpu(), b.cpu())
        turn = 2 + r
        assert _epoch_state(src) == _epoch_state(eager) == (turn // T, turn % T)
        seen.append(k.idx(src).cpu().numpy().reshape(-1).copy())
    seen = np.concatenate(seen)
    want_rows = np.concatenate([_perm(k.SEED, 0, k.G)[k.D:T * k.D], _perm(k.SEED, 1, k.G)[:2 * k.D]])
    assert np.array_equal(seen, want_rows)


@pytest.mark.parametrize("name", list(KINDS))
def test_check_names_the_samplers_bit(name):
    k = _kind(name)
    T = k.G // k.D
    src = k.make(pick="epoch")
    src.sampler.state.copy_(torch.tensor([0, T], dtype=torch.int64))   # a turn outside the epoch, written by hand
    src.step()
    torch.cuda.synchronize()
    assert (k.idx(src).cpu().numpy() == 0).all() and _epoch_state(src) == (0, T) and int(src.sampler.status.cpu()[0]) == 1
    with pytest.raises(ValueError, match="bit 12"):
        src.check()
    assert int(src.sampler.status.cpu()[0]) == 0
    src.check()                                                         # cleared by the raise
    fine = k.make(pick=True)
    fine.step()
    try:
        fine.check()
    except ValueError as err:
        assert "bit 12" not in str(err)


@pytest.mark.parametrize("name", list(KINDS))
def test_constructor_refusals_and_ranks(name):
    k = _kind(name)
    G, D = k.G, k.D
    assert 2 * D <= G < 5 * D
    for kw in (dict(pick="epoch", world=5), dict(pick="epoch", world=0), dict(pick="epoch", rank=2, world=2),
               dict(pick="epoch", rank=-1, world=2), dict(pick="epoch", rank=1), dict(pick="random"), dict(pick=True, rank=0),
               dict(pick=True, world=1), dict(pick=False, rank=0, world=1), dict(pick=False, world=2)):
        with pytest.raises(ValueError):
            k.make(**kw)
    both = [k.make(pick="epoch", rank=r, world=2) for r in range(2)]
    for s in both:
        s.step()
    torch.cuda.synchronize()
    rows = np.concatenate([k.idx(s).cpu().numpy().reshape(-1) for s in both])
    assert np.array_equal(rows, _perm(k.SEED, 0, G)[:2 * D])
    T2 = G // (2 * D)
    assert all(_epoch_state(s) == ((0, 1) if T2 > 1 else (1, 0)) for s in both)


# ------------------------------------------------------------------------------------------------ pick=True / pick=False as before
@pytest.mark.parametrize("pick", [True, False])
def test_kitti_source_keeps_its_behaviour(pick):
    k = _kind("kitti")
    TP, sc = k.TP, k.sc
    b = TP._builder()
    src = TP._source(sc, 4, builder=b, pick=pick)
    assert src.sampler is None and src.pick is pick
    got = src.step()
    torch.cuda.synchronize()
    lab = src.pick_idx.cpu().numpy().reshape(-1)
    assert np.array_equal(lab, draws_ref.choice_row(TP.SEED, 0, 0, 14, 12) if pick else np.arange(12))
    sel, want, _ = TP._host_path(sc, src, b, 0, TP.SEED)
    n = min(len(sel["kept"]), 4)
    assert n == 4 == int(src.n_kept.cpu()[0]) and np.array_equal(src.slot_box.cpu().numpy(), sel["kept"][:n])
    assert sorted(got.keys()) == sorted(want.keys())
    for key in want:
        assert torch.equal(got[key][:n].cpu(), want[key][:n].cpu()), key
    assert _states(k, src) == [1, 1, 1]
    src.check()


@pytest.mark.parametrize("pick", [True, False])
def test_sunrgbd_source_keeps_its_behaviour(pick):
    k = _kind("sunrgbd")
    TS, sc = k.TS, k.sc
    b = TS._builder()
    B, D = 4, 12 if pick else 4
    src = TS._source(sc, B, D=D, builder=b, order=None if pick else TS.GOOD4, pick=pick)
    assert src.sampler is None and src.pick is pick
    got = src.step()
    torch.cuda.synchronize()
    idx = src.pick_idx.cpu().numpy().reshape(-1)
    assert np.array_equal(idx, draws_ref.choice_row(TS.SEED, 0, 0, 14, D) if pick else np.arange(D))
    whole = TS._host_path(sc, src)
    n = int(src.n_kept.cpu()[0])
    slot_box = src.slot_box.cpu().numpy()
    assert n == B and np.array_equal(slot_box, whole["kept"][:n])
    sel = TS._host_path(sc, src, slot_box)
    draws = tuple(src.t[key][:n].contiguous() for key in ("choice", "coin", "normal", "hshift"))
    want = b.build_device_train(sel, TS._dev(sc["K"]), TS._dev(sc["Rt"]), [src.types[g] for g in idx[slot_box]], draws=draws)
    torch.cuda.synchronize()
    assert sorted(got.keys()) == sorted(want.keys())
    for key in want:
        assert torch.equal(got[key].cpu(), want[key].cpu()), key
    for i in range(n):                                                  # the choice table is the restated draw through the step's slices
        ln = int(src.sub_len.cpu()[i])
        row = draws_ref.choice_row(TS.SEED + 2, 0, i, ln if ln else int(src.counts.cpu()[i]), b.npoints)
        sl = TS._sub_list(src)[slot_box[i]]
        assert np.array_equal(src.t["choice"][i].cpu().numpy(), row if sl is None else sl[row]), i
    assert _states(k, src) == [1, 1, 1, 1]
    src.check()


@pytest.mark.parametrize("pick", [True, False])
def test_refine_source_keeps_its_behaviour(pick):
    k = _kind("refine")
    TR, sc = k.TR, k.sc
    b = TR._builder(64, random_flip=True, random_shift=True)
    probe = TR._source(sc, 4, builder=b, pick=pick)                     # (generous window counts: reads the step's picks and jitter)
    probe.step()
    torch.cuda.synchronize()
    _, _, sel, _ = TR._host_path(sc, probe, b, 0, TR.SEED)
    K = len(sel["kept"])
    lpad = b._lpad(sel["pred_size"][:, 1].cpu().numpy())
    src = TR._source(sc, K, lpad=lpad, builder=b, pick=pick)
    assert src.sampler is None and src.pick is pick
    got = src.step()
    torch.cuda.synchronize()
    crow = src.cand_row.cpu().numpy().reshape(-1)
    assert np.array_equal(crow, draws_ref.choice_row(TR.SEED, 0, 0, 8, 8) if pick else np.arange(8))
    gidx, best, sel, want = TR._host_path(sc, src, b, 0, TR.SEED)
    assert torch.equal(src.gt_idx.cpu(), gidx.cpu()) and torch.equal(src.best_iou.cpu(), best.cpu())
    assert len(sel["kept"]) == K >= 4 and int(src.n_kept.cpu()[0]) == K and np.array_equal(src.slot_unit.cpu().numpy(), sel["kept"])
    assert sorted(got.keys()) == sorted(want.keys())
    for key in want:
        assert torch.equal(got[key].cpu(), want[key].cpu()), key
    assert _states(k, src) == [1, 1, 1]
    src.check()
