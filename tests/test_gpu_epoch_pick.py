"""GPU: the epoch sampler (C-ABI fcn_epoch_pick / fcn_epoch_pick_limits, csrc/epoch_pick.h; inputs.EpochSampler) against the numpy
restatement of the draws' contract: the permutation of epoch e over G labels is draws_ref.choice_row(seed, e, 0, G, G), a step's
pick the window (t * world + rank) * D ... + D of it.  Everything is integers: bit for bit.  Every pick is written between poisoned
guard words, which are checked afterwards.  tests/test_emu_epoch_pick.py runs the kernel-level cases on the CPU; the graph capture
runs here only, the three training sources in tests/test_gpu_epoch_sources.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import draws_ref as R

pytestmark = pytest.mark.gpu

SEED = 0x0123456789ABCDEF
POISON = 0x5A5A5A5A
BADARG, LIMIT = 10001, 10002


@functools.lru_cache(maxsize=None)
def _perm(e, G, seed=SEED):
    """perm_e over G labels: computed once per (epoch, G), shared, never written."""
    p = R.choice_row(seed, e, 0, G, G)
    p.setflags(write=False)
    return p


def _sampler(e=0, t=0, seed=SEED, rank=0, world=1):
    from frustum_convnet_amd import inputs
    s = inputs.EpochSampler(seed, rank=rank, world=world)
    _set(s, e, t)
    return s


def _set(s, e, t):
    s.state.copy_(torch.tensor([e, t], dtype=torch.int64))


def _state(s):
    return tuple(int(v) for v in s.state.cpu().tolist())


def _count(G):
    return torch.tensor([int(G)], dtype=torch.int64, device="cuda")


class _Rows:
    """n pick rows of D int32, each between g poisoned words on either side."""

    def __init__(self, n, D, g=16):
        self.n, self.D, self.g = n, D, g
        self.buf = torch.full((n * (D + 2 * g),), POISON, dtype=torch.int32, device="cuda")

    def row(self, i):
        o = i * (self.D + 2 * self.g) + self.g
        return self.buf[o:o + self.D]

    def host(self):
        """(n, D) picks; the guards are checked."""
        h = self.buf.cpu().numpy().reshape(self.n, self.D + 2 * self.g)
        assert (h[:, :self.g] == POISON).all() and (h[:, self.g + self.D:] == POISON).all(), "pick guard words overwritten"
        return h[:, self.g:self.g + self.D]


def _walk(s, G, D, n, g=16):
    """n consecutive picks of s -> (n, D)."""
    rows, cd = _Rows(n, D, g), _count(G)
    for i in range(n):
        out = s.pick(cd, D, out=rows.row(i))
        assert out.data_ptr() == rows.row(i).data_ptr()
    torch.cuda.synchronize()
    return rows.host()


def _at(G, D, e, t, rank=0, world=1, g=16, seed=SEED):
    """The pick at state (e, t) -> ((D,) pick, the state left behind)."""
    s = _sampler(e, t, seed, rank, world)
    got = _walk(s, G, D, 1, g)[0]
    assert int(s.status.cpu()[0]) == 0
    return got, _state(s)


WHOLE = [(1, 1), (2, 1), (5, 2), (256, 256), (257, 16), (4095, 48), (4096, 48), (4096, 2048), (4097, 48), (5000, 7)]
TURNS = [(20000, 48), (70000, 2048), (70000, 1)]


def test_limits_and_the_case_table():
    from frustum_convnet_amd import inputs
    max_d, cap = inputs.EpochSampler.limits()
    assert (max_d, cap) == (2048, 4096) and inputs.DeviceDraws.limits() == (max_d, cap)
    gs = [g for g, _ in WHOLE + TURNS]
    assert any(g < cap for g in gs) and cap in gs and cap + 1 in gs and cap - 1 in gs       # both paths and the edge between them
    assert any(g % d == 0 and g > d for g, d in WHOLE) and any(g == d for g, d in WHOLE)
    s = inputs.EpochSampler(SEED, rank=1, world=3)
    assert s.steps_per_epoch(5000, 48) == 5000 // 144 and _sampler().steps_per_epoch(4096, 2048) == 2


@pytest.mark.parametrize("G,D", WHOLE)
def test_whole_epoch_and_the_first_turn_of_the_next(G, D):
    e, T = 3, G // D
    s = _sampler(e)
    got = _walk(s, G, D, T + 1, g=16 if D != 7 else 3)                 # (g = 3: rows that are not 16-byte aligned)
    epoch = got[:T].reshape(-1)
    assert np.array_equal(epoch, _perm(e, G)[:T * D])
    assert len(np.unique(epoch)) == T * D                              # no label twice; the tail G - T * D is what is missing
    assert np.array_equal(got[T], _perm(e + 1, G)[:D])
    assert _state(s) == ((e + 1, 1) if T > 1 else (e + 2, 0)) and int(s.status.cpu()[0]) == 0
    s2 = _sampler(e)                                                    # the state right behind the epoch
    _walk(s2, G, D, T)
    assert _state(s2) == (e + 1, 0)


@pytest.mark.parametrize("G,D", TURNS)
def test_chosen_turns_of_a_large_epoch(G, D):
    e, T = 7, G // D
    for t in (0, 1, T // 2, T - 1):
        got, after = _at(G, D, e, t)
        assert np.array_equal(got, _perm(e, G)[t * D:(t + 1) * D]), t
        assert after == ((e, t + 1) if t + 1 < T else (e + 1, 0))


@pytest.mark.parametrize("G,D", [(5, 2), (257, 16), (4096, 2048), (4097, 48), (70000, 2048), (70000, 1)])
def test_turn_zero_equals_the_draw_kernels_choice_row(G, D):
    """Turn 0 of epoch e = the choice row of fcn_draw_batch at B = 1, N = D, counts = G, state = e: both on the device."""
    from frustum_convnet_amd import inputs
    e = 11
    dd = inputs.DeviceDraws(SEED)
    dd.state.fill_(e)
    choice = dd.draw(_count(G), D, False, False)[0]
    got, _ = _at(G, D, e, 0)
    torch.cuda.synchronize()
    assert np.array_equal(got, choice.cpu().numpy().reshape(-1))


@pytest.mark.parametrize("e", [2 ** 32 - 1, 2 ** 32, 2 ** 40 + 5])
def test_epochs_at_and_above_two_to_the_32(e):
    for G, D in ((50, 8), (5001, 8)):
        T = G // D
        got, _ = _at(G, D, e, 2)
        assert np.array_equal(got, _perm(e, G)[2 * D:3 * D])
        s = _sampler(e, T - 1)                                          # across the epoch boundary: the carry into the high word
        two = _walk(s, G, D, 2)
        assert np.array_equal(two[0], _perm(e, G)[(T - 1) * D:T * D]) and np.array_equal(two[1], _perm(e + 1, G)[:D])
        assert _state(s) == (e + 1, 1)


# draws_ref finds, at G = 70 000 under SEED, two rows of epoch 6 with one 32-bit key; the index breaks the tie
TIE_EPOCH, TIE_ROWS, TIE_RANK = 6, (58559, 59591), 3170


def test_a_key_tie_inside_a_window_and_across_a_window_boundary():
    G, e, r = 70000, TIE_EPOCH, TIE_RANK
    k = R._words(SEED, e, 0, 0, G)
    perm = _perm(e, G)
    assert k[TIE_ROWS[0]] == k[TIE_ROWS[1]] and (int(perm[r]), int(perm[r + 1])) == TIE_ROWS
    D = 48                                                              # one window holds both ranks
    assert r // D == (r + 1) // D
    got, _ = _at(G, D, e, r // D)
    assert np.array_equal(got, perm[(r // D) * D:(r // D + 1) * D]) and TIE_ROWS[0] in got and TIE_ROWS[1] in got
    D = 151                                                             # D divides r + 1: a boundary falls between them
    assert (r + 1) % D == 0
    t = (r + 1) // D
    last, _ = _at(G, D, e, t - 1)
    first, _ = _at(G, D, e, t)
    assert np.array_equal(last, perm[(t - 1) * D:t * D]) and np.array_equal(first, perm[t * D:(t + 1) * D])
    assert int(last[-1]) == TIE_ROWS[0] and int(first[0]) == TIE_ROWS[1]


@pytest.mark.parametrize("G,D,world", [(1000, 16, 3), (5000, 48, 2), (4100, 2048, 2)])
def test_ranks_take_disjoint_windows_of_one_epoch(G, D, world):
    e, T = 2, G // (D * world)
    assert T >= 1
    ranks = [_sampler(e, 0, rank=r, world=world) for r in range(world)]
    got = np.stack([_walk(s, G, D, T) for s in ranks])                  # (world, T, D)
    seen = got.reshape(-1)
    assert len(np.unique(seen)) == world * T * D                        # disjoint
    assert np.array_equal(got.transpose(1, 0, 2).reshape(-1), _perm(e, G)[:T * D * world])
    assert all(_state(s) == (e + 1, 0) for s in ranks)
    nxt = np.stack([_walk(s, G, D, 1)[0] for s in ranks]).reshape(-1)
    assert np.array_equal(nxt, _perm(e + 1, G)[:D * world])


def test_state_restores_and_advance_zero_keeps_it():
    from frustum_convnet_amd import inputs
    G, D = 4500, 32
    cd = _count(G)
    s = _sampler(40, 9)
    a = s.pick(cd, D).cpu().numpy()
    assert _state(s) == (40, 10) and a.dtype == np.int32 and a.shape == (D,)
    b = s.pick(cd, D).cpu().numpy()
    assert _state(s) == (40, 11) and not np.array_equal(a, b)
    _set(s, 40, 9)
    assert np.array_equal(s.pick(cd, D).cpu().numpy(), a) and _state(s) == (40, 10)
    c = s.pick(cd, D, advance=False).cpu().numpy()
    assert np.array_equal(c, b) and _state(s) == (40, 10)
    assert np.array_equal(a, _perm(40, G)[9 * D:10 * D]) and np.array_equal(b, _perm(40, G)[10 * D:11 * D])
    s.check()
    assert isinstance(s, inputs.EpochSampler) and s.state.shape == (2,) and s.status.shape == (1,)


FAILURES = [("count 0", 0, 8, 1, 0, 0), ("count 2^31", 2 ** 31, 8, 1, 0, 0), ("D * world > G", 15, 8, 2, 0, 0),
            ("t = T", 100, 8, 2, 3, 6), ("t < 0", 100, 8, 2, 3, -1), ("e < 0", 100, 8, 2, -1, 0), ("t = T above the cap", 5000, 8, 2, 3, 312),
            ("negative count", -4, 8, 1, 0, 0)]


@pytest.mark.parametrize("name,G,D,world,e,t", FAILURES, ids=[f[0].replace(" ", "_") for f in FAILURES])
def test_defined_failures_give_zeros_the_bit_and_the_state_as_it_was(name, G, D, world, e, t):
    s = _sampler(e, t, rank=world - 1, world=world)
    got = _walk(s, G, D, 1)[0]
    assert (got == 0).all() and int(s.status.cpu()[0]) == 1 and _state(s) == (e, t)
    with pytest.raises(ValueError):
        s.check()
    s.check()                                                           # cleared by the raise


def test_refusals_of_the_entry_and_of_the_wrapper():
    from frustum_convnet_amd import _native, inputs
    L = _native.lib()
    mx, cap = ctypes.c_int(0), ctypes.c_int(0)
    assert L.fcn_epoch_pick_limits(None, ctypes.byref(cap)) == BADARG and L.fcn_epoch_pick_limits(ctypes.byref(mx), None) == BADARG
    assert L.fcn_epoch_pick_limits(ctypes.byref(mx), ctypes.byref(cap)) == 0 and (mx.value, cap.value) == inputs.EpochSampler.limits()
    D = 8
    s = _sampler(3, 4)
    cd = _count(100)
    rows = _Rows(1, D)
    p = lambda t: None if t is None else t.data_ptr()
    st = _native.current_stream()

    def call(count=cd, D=D, rank=0, world=1, state=s.state, pick=rows.row(0), status=s.status):
        return L.fcn_epoch_pick(p(count), D, rank, world, SEED, p(state), 1, p(pick), p(status), st)

    for k in ("count", "state", "pick", "status"):
        assert call(**{k: None}) == BADARG, k
    assert call(D=0) == BADARG and call(D=-3) == BADARG and call(world=0) == BADARG and call(world=-1) == BADARG
    assert call(rank=-1) == BADARG and call(rank=1) == BADARG and call(rank=2, world=2) == BADARG
    assert call(D=mx.value + 1) == LIMIT
    torch.cuda.synchronize()
    assert (rows.host() == POISON).all() and _state(s) == (3, 4) and int(s.status.cpu()[0]) == 0    # a refused call writes nothing
    assert call() == 0
    torch.cuda.synchronize()
    assert _state(s) == (3, 5) and np.array_equal(rows.host()[0], _perm(3, 100)[4 * D:5 * D])
    # the wrapper
    bad = [lambda: s.pick(cd.to(torch.int32), D), lambda: s.pick(torch.cat([cd, cd]), D), lambda: s.pick(cd, 0),
           lambda: s.pick(cd, D, out=torch.zeros((D + 1,), dtype=torch.int32, device="cuda")),
           lambda: s.pick(cd, D, out=torch.zeros((D,), dtype=torch.int64, device="cuda")),
           lambda: s.pick(cd, D, out=torch.zeros((D, 2), dtype=torch.int32, device="cuda")[:, 0]),
           lambda: inputs.EpochSampler(SEED, rank=1, world=1), lambda: inputs.EpochSampler(SEED, rank=-1, world=2),
           lambda: inputs.EpochSampler(SEED, rank=0, world=0)]
    for f in bad:
        with pytest.raises(ValueError):
            f()
    with pytest.raises(_native.NativeError):
        s.pick(cd, mx.value + 1)
    assert _state(s) == (3, 5)
    cpu = torch.tensor([100], dtype=torch.int64)
    if not cpu.is_cuda:                                                 # (the emulation's shim reports every tensor as a device one)
        with pytest.raises(ValueError):
            s.pick(cpu, D)
        with pytest.raises(ValueError):
            s.pick(cd, D, out=torch.zeros((D,), dtype=torch.int32))
        with pytest.raises(RuntimeError):
            inputs.EpochSampler(SEED, device="cpu")


# ------------------------------------------------------------------------------------------------ GPU only
def test_graph_of_a_pick_replays_across_an_epoch_boundary():
    """One single-stream capture of sampler.pick(out=...), replayed T + 2 times from turn 0: the picks are the eager sampler's and
    the restated windows, across the epoch boundary."""
    G, D, e = 5000, 1024, 5
    T = G // D
    assert T == 4
    cd = _count(G)
    s = _sampler(e, 0)
    rows = _Rows(1, D)
    out = rows.row(0)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        s.pick(cd, D, out=out)                                          # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    torch.cuda.synchronize()
    _set(s, e, 0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s.pick(cd, D, out=out)
    torch.cuda.synchronize()
    assert _state(s) == (e, 0)                                          # capturing runs nothing
    eager = _sampler(e, 0)
    for r in range(T + 2):
        graph.replay()
        torch.cuda.synchronize()
        ep, t = e + r // T, r % T
        got = rows.host()[0]
        assert np.array_equal(got, eager.pick(cd, D).cpu().numpy()), r
        assert np.array_equal(got, _perm(ep, G)[t * D:(t + 1) * D]), r
        assert _state(s) == _state(eager) == (e + (r + 1) // T, (r + 1) % T)
    s.check()
