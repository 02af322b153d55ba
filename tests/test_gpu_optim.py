"""-m gpu: the optimiser kernels of csrc/optim.hip (C-ABI fcn_adam_step_f32 / fcn_sgd_step_f32) and train_state.FlatTrainState on
a toy module, ONE step at a time from the device's own state against the fp64 restatement of tests/optim_ref.py -- every
elementwise comparison uses that module's a-priori bound (safety factor 2), nothing is tuned to the kernels' output.  Gradients
are supplied, not computed: no model forward runs here.  tests/test_optim_referee.py shows what a pass excludes."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

import optim_ref as R

pytestmark = pytest.mark.gpu

FCN_E_BADARG = 10001            # include/fcn_hip.h
POISON = 0x7FC12345             # a NaN pattern no kernel produces
SLOT_POISON = -77
WORST = {}                      # entry -> worst error / bound seen by this process (printed; EXPERIMENTS.md records it)


def _lib():
    from frustum_convnet_amd import _native
    return _native.lib(), _native.current_stream()


def _guarded(values, pre, post=8):
    """A 16-byte aligned float32 view at a non-zero offset inside a larger poisoned allocation."""
    n = len(values)
    big = torch.empty(pre + n + post, dtype=torch.float32, device="cuda")
    big.view(torch.int32).fill_(POISON)
    view = big[pre:pre + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)))
    assert pre > 0 and pre % 4 == 0 and view.data_ptr() % 16 == 0
    return big, view, pre


def _guards_intact(big, view, pre):
    bits = big.view(torch.int32).cpu()
    return bool((bits[:pre] == POISON).all()) and bool((bits[pre + view.numel():] == POISON).all())


def _np(t):
    return t.detach().cpu().numpy().copy()


def _bits(a):
    return np.asarray(a, dtype=np.float32).view(np.int32)


def _inside(entry, got, want, bound, what):
    err = np.abs(got.astype(np.float64) - want)
    assert np.all(np.isfinite(got)), what
    r = float((err / bound).max())
    WORST[entry] = max(WORST.get(entry, 0.0), r)
    i = int(np.argmax(err / bound))
    assert r <= 1.0, (what, "element %d: got %r want %r bound %.3e ratio %.3f" % (i, got[i], want[i], bound[i], r))


@pytest.mark.parametrize("n", R.SIZES)
def test_adam_entry_one_step_at_a_time(n):
    L, stream = _lib()
    nslots = int(L.fcn_adam_step_slots(ctypes.c_int64(n)))
    assert nslots == R.adam_blocks(n)
    p0, g0, m0, v0 = R.make_inputs(n, 0)
    P, G, M, V = _guarded(p0, 4), _guarded(g0, 8), _guarded(m0, 12), _guarded(v0, 16)
    slots_big = torch.full((nslots + 4,), SLOT_POISON, dtype=torch.int64, device="cuda")
    slots = slots_big[2:2 + nslots]
    slots.copy_(torch.from_numpy(R.slot_init(n)))
    hyper = torch.tensor(R.ADAM_HYPER[0], dtype=torch.float32, device="cuda")
    el = R.element_slots(n)
    for k, h in enumerate(R.ADAM_HYPER):
        if k:           # new values in the SAME device memory: nothing is re-created between steps
            hyper.copy_(torch.tensor(h, dtype=torch.float32))
            G[1].copy_(torch.from_numpy(R.gradients(np.random.default_rng([7, n, k]), n)[0]))
        p, g, m, v, s, h32 = _np(P[1]), _np(G[1]), _np(M[1]), _np(V[1]), _np(slots), _np(hyper)
        assert R.normal_range_ok(p, g, h32)
        rc = L.fcn_adam_step_f32(P[1].data_ptr(), G[1].data_ptr(), M[1].data_ptr(), V[1].data_ptr(), ctypes.c_int64(n),
                                 hyper.data_ptr(), slots.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0
        (wp, wm, wv), (bp, bm, bv) = R.adam_step(p, g, m, v, h32, s[el])       # every element with ITS workgroup's count
        _inside("fcn_adam_step_f32", _np(P[1]), wp, bp, ("p", n, k))
        _inside("fcn_adam_step_f32", _np(M[1]), wm, bm, ("m", n, k))
        _inside("fcn_adam_step_f32", _np(V[1]), wv, bv, ("v", n, k))
        assert np.array_equal(_np(slots), s + 1), (n, k)                       # each slot advanced by exactly 1
        sb = _np(slots_big)
        assert (sb[:2] == SLOT_POISON).all() and (sb[2 + nslots:] == SLOT_POISON).all(), (n, k)
        assert np.array_equal(_bits(_np(G[1])), _bits(g)), (n, k)              # grad unchanged bit for bit
        assert np.array_equal(_bits(_np(hyper)), _bits(h32))
        for buf in (P, G, M, V):
            assert _guards_intact(*buf), (n, k)
        if h[0] == 0.0:                                                        # lr = 0: p bit-identical, moments and slots moved
            assert np.array_equal(_bits(_np(P[1])), _bits(p)), (n, k)
            assert not np.array_equal(_bits(_np(M[1])), _bits(m)) and not np.array_equal(_bits(_np(V[1])), _bits(v))
    print("fcn_adam_step_f32 n=%d: worst error / bound so far %.3f" % (n, WORST["fcn_adam_step_f32"]))


@pytest.mark.parametrize("n", R.SIZES)
def test_sgd_entry_one_step_at_a_time(n):
    L, stream = _lib()
    p0, g0, b0, _ = R.make_inputs(n, 0)
    P, G, B = _guarded(p0, 4), _guarded(g0, 8), _guarded(b0, 12)
    hyper = torch.tensor(R.SGD_HYPER[0], dtype=torch.float32, device="cuda")
    for k, h in enumerate(R.SGD_HYPER):          # momentum 0.9, 0 and 0.9 again; weight decay 1e-4 and 0
        if k:
            hyper.copy_(torch.tensor(h, dtype=torch.float32))
            G[1].copy_(torch.from_numpy(R.gradients(np.random.default_rng([7, n, k]), n)[0]))
        p, g, b, h32 = _np(P[1]), _np(G[1]), _np(B[1]), _np(hyper)
        assert R.normal_range_ok(p, g, h32, adam=False)
        rc = L.fcn_sgd_step_f32(P[1].data_ptr(), G[1].data_ptr(), B[1].data_ptr(), ctypes.c_int64(n), hyper.data_ptr(), stream)
        torch.cuda.synchronize()
        assert rc == 0
        (wp, wb), (bp, bb) = R.sgd_step(p, g, b, h32)
        _inside("fcn_sgd_step_f32", _np(P[1]), wp, bp, ("p", n, k))
        _inside("fcn_sgd_step_f32", _np(B[1]), wb, bb, ("buf", n, k))
        assert np.array_equal(_bits(_np(G[1])), _bits(g)), (n, k)
        assert np.array_equal(_bits(_np(hyper)), _bits(h32))
        for buf in (P, G, B):
            assert _guards_intact(*buf), (n, k)
    print("fcn_sgd_step_f32 n=%d: worst error / bound so far %.3f" % (n, WORST["fcn_sgd_step_f32"]))


def _refusal_buffers(n, count):
    bufs = [_guarded(a, 4 * (i + 1)) for i, a in enumerate(R.make_inputs(n, 1)[:count])]
    slots = torch.full((R.adam_blocks(n) + 4,), SLOT_POISON, dtype=torch.int64, device="cuda")
    slots[2:2 + R.adam_blocks(n)] = 5
    return bufs, slots


def test_adam_entry_refusals_touch_nothing():
    L, stream = _lib()
    n = 2052
    bufs, slots = _refusal_buffers(n, 4)
    hyper = torch.tensor(R.ADAM_HYPER[0], dtype=torch.float32, device="cuda")
    before = [b[0].view(torch.int32).clone() for b in bufs] + [slots.clone(), hyper.clone()]
    good = [b[1].data_ptr() for b in bufs] + [n, hyper.data_ptr(), slots.data_ptr() + 16]

    def call(a):
        return L.fcn_adam_step_f32(a[0], a[1], a[2], a[3], ctypes.c_int64(a[4]), a[5], a[6], stream)

    for i in (0, 1, 2, 3, 5, 6):                      # each null pointer
        a = list(good)
        a[i] = None
        assert call(a) == FCN_E_BADARG, ("null", i)
    for bad_n in (0, 3, -1):
        a = list(good)
        a[4] = bad_n
        assert call(a) == FCN_E_BADARG, ("n", bad_n)
    for i in range(4):                                # each array 4 bytes off a 16-byte boundary, one at a time
        a = list(good)
        a[i] += 4
        assert call(a) == FCN_E_BADARG, ("misaligned", i)
    torch.cuda.synchronize()
    after = [b[0].view(torch.int32) for b in bufs] + [slots, hyper]
    assert all(torch.equal(x, y) for x, y in zip(before, after))


def test_sgd_entry_refusals_touch_nothing():
    L, stream = _lib()
    n = 2052
    bufs, _ = _refusal_buffers(n, 3)
    hyper = torch.tensor(R.SGD_HYPER[0], dtype=torch.float32, device="cuda")
    before = [b[0].view(torch.int32).clone() for b in bufs] + [hyper.clone()]
    good = [b[1].data_ptr() for b in bufs] + [n, hyper.data_ptr()]

    def call(a):
        return L.fcn_sgd_step_f32(a[0], a[1], a[2], ctypes.c_int64(a[3]), a[4], stream)

    for i in (0, 1, 2, 4):
        a = list(good)
        a[i] = None
        assert call(a) == FCN_E_BADARG, ("null", i)
    for bad_n in (0, 3, -1):
        a = list(good)
        a[3] = bad_n
        assert call(a) == FCN_E_BADARG, ("n", bad_n)
    for i in range(3):
        a = list(good)
        a[i] += 4
        assert call(a) == FCN_E_BADARG, ("misaligned", i)
    torch.cuda.synchronize()
    after = [b[0].view(torch.int32) for b in bufs] + [hyper]
    assert all(torch.equal(x, y) for x, y in zip(before, after))


# ------------------------------------------------------------------------------------------------
# FlatTrainState on a toy module whose parameter names follow the real model's

class _Bag(nn.Module):
    def __init__(self, shapes):
        super().__init__()
        for i, s in enumerate(shapes):
            self.register_parameter("w%d" % i, nn.Parameter(torch.randn(*s)))


def _toy(extra=False):
    """16 812 flat elements, 9 step slots; the scales span 2, 1 and 3 workgroup tiles, the bucket cut is at 12 288.  Tensor sizes
    that are no multiple of 4 and that cross a tile (2049, 4100, 4097).  reg_out is registered before cls_out, as in the real
    model: the flat order (heads last, cls before reg) differs from model.parameters() order."""
    torch.manual_seed(5)
    m = nn.Module()
    m.feat_net = nn.Module()
    m.feat_net.pointnet1 = _Bag([(5,), (2049,)])
    m.feat_net.pointnet2 = _Bag([(3,), (7, 11)])
    m.feat_net.pointnet3 = _Bag([(4100,)])
    if extra:
        m.feat_net.extra = _Bag([(10,)])             # (a sub-module: registered behind pointnet3)
    m.conv_net = _Bag([(4097,), (6,)])
    m.reg_out = nn.Conv1d(9, 39, 1)
    m.cls_out = nn.Conv1d(9, 2, 1)
    return m.cuda()


def _state(model, **kw):
    from frustum_convnet_amd.train_state import FlatTrainState
    import emu_shim
    st = FlatTrainState(model, **kw)
    if torch.cuda.device is emu_shim._Inert:          # under the host emulation the tensors live on the CPU: let the step through
        st.device = torch.device("cuda")
    return st


def _used(st):
    used = np.zeros(st.numel, dtype=bool)
    for p, o in zip(st.params, st.offsets):
        assert not used[o:o + p.numel()].any(), "parameters overlap"
        used[o:o + p.numel()] = True
    return used


def _toy_grad(st, k):
    """Gradient k of the shared stream: the distribution of optim_ref.gradients on the parameters, zero in the padding."""
    g = np.zeros(st.numel, dtype=np.float32)
    used = _used(st)
    g[used] = R.gradients(np.random.default_rng([11, k]), int(used.sum()))[0]
    return torch.from_numpy(g)


def _padding_is_zero(st):
    pad = torch.from_numpy(~_used(st))
    bufs = (st.flat, st.grad, st.exp_avg, st.exp_avg_sq)
    return all(bool((b.cpu()[pad] == 0).all()) for b in bufs)


def _step_inside_bound(st, step_fn, t, entry):
    """One step of `st` against the restatement applied to its own state before the step."""
    p, g, m, v, h = _np(st.flat), _np(st.grad), _np(st.exp_avg), _np(st.exp_avg_sq), _np(st.hyper)
    step_fn()
    torch.cuda.synchronize()
    if st.optimizer == "sgd":
        (wp, wm), (bp, bm) = R.sgd_step(p, g, m, h[:4])
    else:
        (wp, wm, wv), (bp, bm, bv) = R.adam_step(p, g, m, v, h, t)
        _inside(entry, _np(st.exp_avg_sq), wv, bv, ("v", t))
    _inside(entry, _np(st.flat), wp, bp, ("p", t))
    _inside(entry, _np(st.exp_avg), wm, bm, ("m", t))


def test_toy_layout():
    from frustum_convnet_amd.train_state import STEP_SPAN
    assert STEP_SPAN == R.STEP_SPAN
    st = _state(_toy())
    off = dict(zip(st.names, st.offsets))
    num = {n: p.numel() for n, p in zip(st.names, st.params)}
    for n, o in off.items():
        if n.startswith("reg_out."):                  # directly behind cls_out.*: one GEMM operand
            c = n.replace("reg_out.", "cls_out.")
            assert o == off[c] + num[c], n
        else:
            assert o % 4 == 0, (n, o)
    _used(st)                                         # no two parameters overlap
    assert st.numel == 16812 and st._step_slots.numel() == 9
    assert st.buckets == [("fcn+heads", 12288, 16812), ("pointnet", 0, 12288)]
    assert all(lo % STEP_SPAN == 0 for lo, _ in st.scale_ranges.values()) and st.buckets[0][1] % STEP_SPAN == 0
    tiles = {k: (hi + STEP_SPAN - 1) // STEP_SPAN - lo // STEP_SPAN for k, (lo, hi) in st.scale_ranges.items()}
    assert tiles == {0: 2, 1: 1, 2: 3}
    # model.parameters() order has reg_out before cls_out, the flat order the reverse: param_index is not the identity
    assert st.param_index != list(range(len(st.params))) and sorted(st.param_index) == list(range(len(st.params)))


def test_parameter_in_a_scale_tile_is_refused():
    """A feat_net parameter placed directly behind the last scale would sit in that scale's last tile: adam_step_scale would advance
    its step counter without stepping it."""
    with pytest.raises(ValueError, match="feat_net.extra.w0.*shares an optimiser tile"):
        _state(_toy(extra=True))


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_toy_twins_whole_bucket_and_scale_steps(optimizer):
    kw = dict(lr=1e-3, weight_decay=1e-4, optimizer=optimizer)
    a, b, c = (_state(_toy(), **kw) for _ in range(3))
    entry = "FlatTrainState/" + optimizer
    for k in range(5):
        g = _toy_grad(a, k)
        for st in (a, b, c):
            st.grad.copy_(g)
        _step_inside_bound(a, a.adam_step, k, entry)
        b.adam_step_bucket(1)
        b.adam_step_bucket(0)
        c.adam_step_bucket(0)
        for s in (2, 0, 1):
            c.adam_step_scale(s)
        torch.cuda.synchronize()
        for st in (b, c):
            for x, y in ((a.flat, st.flat), (a.exp_avg, st.exp_avg), (a.exp_avg_sq, st.exp_avg_sq), (a._step_slots, st._step_slots)):
                assert torch.equal(x, y), k
        if optimizer == "adam":
            assert bool((a._step_slots == k + 1).all()), (k, a._step_slots)
        assert int(a.step_count) == k + 1
        assert _padding_is_zero(a) and _padding_is_zero(c), k
    print("%s: worst error / bound %.3f" % (entry, WORST[entry]))


def test_toy_world_of_eight_applies_one_eighth():
    st = _state(_toy(), lr=1e-3, weight_decay=1e-4, world=8)
    assert float(st.hyper[5]) == 0.125
    for k in range(2):
        st.grad.copy_(_toy_grad(st, k))
        _step_inside_bound(st, st.adam_step, k, "FlatTrainState/adam")        # no collective: the kernel's grad_scale alone
        assert _padding_is_zero(st)
    st = _state(_toy(), lr=1e-2, weight_decay=1e-4, world=8, optimizer="sgd")
    assert float(st.hyper[3]) == 0.125
    st.grad.copy_(_toy_grad(st, 0))
    _step_inside_bound(st, st.adam_step, 0, "FlatTrainState/sgd")
    assert _padding_is_zero(st)


def _set_torch_grads(model, st, g):
    named = dict(model.named_parameters())
    for n, p, o in zip(st.names, st.params, st.offsets):
        named[n].grad = g[o:o + p.numel()].view(p.shape).to(named[n].device).clone()


def _same(a, b):
    return all(torch.equal(x, y) for x, y in ((a.flat, b.flat), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq),
                                              (a._step_slots, b._step_slots)))


@pytest.mark.parametrize("optimizer", ["adam", "sgd"])
def test_toy_state_transfer(optimizer):
    lr, wd = 1e-3, 1e-4
    kw = dict(lr=lr, weight_decay=wd, optimizer=optimizer)
    ma = _toy()
    a = _state(ma, **kw)
    mt = _toy()                                       # the float32 torch optimiser over a twin, same gradients
    opt = (torch.optim.Adam(mt.parameters(), lr=lr, weight_decay=wd) if optimizer == "adam" else
           torch.optim.SGD(mt.parameters(), lr=lr, momentum=0.9, weight_decay=wd))
    for k in range(3):
        g = _toy_grad(a, k)
        a.grad.copy_(g)
        a.adam_step()
        _set_torch_grads(mt, a, g)
        opt.step()
    torch.cuda.synchronize()
    # 1. this object's state_dict into a fresh state over a twin that holds the same parameters: two more steps, bit-identical
    mc = _toy()
    mc.load_state_dict(ma.state_dict())
    c = _state(mc, **kw)
    c.load_state_dict(a.state_dict())
    assert _same(a, c)
    for k in range(3, 5):
        g = _toy_grad(a, k)
        for st in (a, c):
            st.grad.copy_(g)
            st.adam_step()
    torch.cuda.synchronize()
    assert _same(a, c) and int(c.step_count) == 5
    # 2. torch's state_dict (model.parameters() order) into a fresh state: one more step against the restatement applied to the
    # state as torch holds it, looked up BY NAME, with t = 3 in every slot
    md = _toy()
    md.load_state_dict(mt.state_dict())
    d = _state(md, **kw)
    d.load_state_dict(opt.state_dict())
    named_t = dict(mt.named_parameters())
    p0, m0, v0 = (np.zeros(d.numel, dtype=np.float32) for _ in range(3))
    for n, p, o in zip(d.names, d.params, d.offsets):
        s = opt.state[named_t[n]]
        p0[o:o + p.numel()] = _np(named_t[n]).reshape(-1)
        m0[o:o + p.numel()] = _np(s["momentum_buffer" if optimizer == "sgd" else "exp_avg"]).reshape(-1)
        if optimizer == "adam":
            v0[o:o + p.numel()] = _np(s["exp_avg_sq"]).reshape(-1)
            assert float(s["step"]) == 3.0
    if optimizer == "adam":
        assert bool((d._step_slots == 3).all())
    g = _toy_grad(d, 3)
    d.grad.copy_(g)
    h = _np(d.hyper)
    d.adam_step()
    torch.cuda.synchronize()
    entry = "FlatTrainState/" + optimizer
    if optimizer == "adam":
        (wp, wm, wv), (bp, bm, bv) = R.adam_step(p0, g.numpy(), m0, v0, h, 3)
        _inside(entry, _np(d.exp_avg_sq), wv, bv, "loaded v")
        assert bool((d._step_slots == 4).all())
    else:
        (wp, wm), (bp, bm) = R.sgd_step(p0, g.numpy(), m0, h[:4])
    _inside(entry, _np(d.flat), wp, bp, "loaded p")
    _inside(entry, _np(d.exp_avg), wm, bm, "loaded m")
    # 3. this object's state_dict into torch's optimiser over the model: model.parameters() order, step 3 on every entry
    # (a has moved on to step 5: take a state that stands at step 3)
    me = _toy()
    e = _state(me, **kw)
    for k in range(3):
        e.grad.copy_(_toy_grad(e, k))
        e.adam_step()
    torch.cuda.synchronize()
    sd = e.state_dict()
    opt2 = (torch.optim.Adam(me.parameters(), lr=1.0) if optimizer == "adam" else torch.optim.SGD(me.parameters(), lr=1.0, momentum=0.5))
    opt2.load_state_dict({"state": sd["state"], "param_groups": sd["param_groups"]})
    off = dict(zip(e.names, e.offsets))
    for n, p in me.named_parameters():
        s = opt2.state[p]
        o = off[n]
        if optimizer == "adam":
            assert float(s["step"]) == 3.0, n
            assert torch.equal(s["exp_avg"].reshape(-1), e.exp_avg[o:o + p.numel()]), n
            assert torch.equal(s["exp_avg_sq"].reshape(-1), e.exp_avg_sq[o:o + p.numel()]), n
        else:
            assert torch.equal(s["momentum_buffer"].reshape(-1), e.exp_avg[o:o + p.numel()]), n
    assert opt2.param_groups[0]["lr"] == float(np.float32(lr))
    if optimizer == "sgd":
        assert sd["step"] == 3


def test_toy_step_in_one_captured_graph():
    """One captured graph holds one adam_step() (a single kernel, no parallel branch), replayed 20 times with a fresh gradient copied
    in before each replay and the learning rate changed on the device half-way: bit-identical to an eager twin."""
    kw = dict(lr=1e-3, weight_decay=1e-4)
    warm, a, b = (_state(_toy(), **kw) for _ in range(3))
    grads = torch.stack([_toy_grad(a, k) for k in range(20)]).cuda()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        warm.adam_step()                              # the kernel's first launch (code load) stays outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.adam_step()
    torch.cuda.synchronize()
    assert int(a.step_count) == 0                     # captured, not run
    for k in range(20):
        if k == 10:
            a.set_lr(2.5e-4)
            b.set_lr(2.5e-4)
        a.grad.copy_(grads[k])
        graph.replay()
        b.grad.copy_(grads[k])
        b.adam_step()
    torch.cuda.synchronize()
    assert int(a.step_count) == 20 and bool((a._step_slots == 20).all())
    assert _same(a, b)
    assert float(a.hyper[0]) == float(np.float32(2.5e-4))
