"""The ConvFeatNet kernels (csrc/fcn_net.hip) layer by layer, off the fixture shapes, through the C-ABI against the fp64 module path
(tests/fcn_ref.py; the reference's own conditions are held by tests/test_fcn_ref_referee.py).  The whole-model tests reach these
kernels at the fixture shapes only and judge one maximum; here every layer's pre-BatchNorm output, published BatchNorm row, running
statistics and every gradient tensor is judged on its own, at shapes that put rows at tile, split and frustum boundaries, at every
head and one-hot width class, in the three BatchNorm modes.  Every case is registered in tests/test_emu_gpu_subset.py and runs on
the host emulation in the default suite.  Measured figures: EXPERIMENTS.md, "The ConvFeatNet kernels layer by layer".
Each case takes well under a second on an MI355X (the reference on the CPU included)."""
import ctypes

import pytest
import torch

import fcn_ref as F
from frustum_convnet_amd import _native as N

pytestmark = pytest.mark.gpu

PRECS = (F.SPLIT, F.F32)
DEV = "cuda"


def _check(name, prec):
    ref = F.reference(F.BY_NAME[name])
    res = F.compare(ref, F.run(N.lib(), ref, prec, DEV), prec)
    print("%s %s: logits %.1e, worst per-layer error / bar %.2f (%s), worst gradient %.1e (%s)" % ((name, F.PREC_NAME[prec]) + F.worst(res)))
    bad = F.failures(res)
    assert not bad, {k: "%.3e > %.3e" % v for k, v in bad.items()}
    return res


@pytest.mark.parametrize("prec", PRECS, ids=[F.PREC_NAME[p] for p in PRECS])
@pytest.mark.parametrize("name", [c.name for c in F.TRAIN_CASES])
def test_train_case(name, prec):
    """BN_TRAIN forward + backward: y, mean, rstd, scale, shift, running statistics per layer; dfeats per level; dW, dgamma, dbeta per
    layer; dWh, dbias; the logits and their zero padding."""
    _check(name, prec)


@pytest.mark.parametrize("prec", PRECS, ids=[F.PREC_NAME[p] for p in PRECS])
@pytest.mark.parametrize("name", [c.name for c in F.SENTINEL_CASES])
def test_sentinel_rows(name, prec):
    """dlogits zero except on the first row, both sides of the first tile boundary, both sides of every boundary between two of the heads'
    weight-gradient splits, rows 511 / 512 where the grid has them and the last row of the L2 grid: dWh and dbias are sums over exactly
    those rows, so a dropped or doubled boundary row is an O(1) error."""
    _check(name, prec)


@pytest.mark.parametrize("prec", PRECS, ids=[F.PREC_NAME[p] for p in PRECS])
@pytest.mark.parametrize("name", [c.name for c in F.WIDTH_CASES])
def test_widths(name, prec):
    """nvec 0 (no one-hot pointer), 1, 10 (hot columns 9, 0, 5, 4) and 64 (hot columns 63, 0, 32, 31: both K chunks of the OH_PAD
    segment) and reg_out 1, 39, 62 (fills ld = 64), 63 (first ld = 128), 67,
    126 (fills ld = 128): logits, padding columns, dWh, dbias and everything else of the case (nvec = 3 is reg39)."""
    _check(name, prec)


@pytest.mark.parametrize("prec", PRECS, ids=[F.PREC_NAME[p] for p in PRECS])
@pytest.mark.parametrize("name", [c.name for c in F.MODE_CASES])
def test_modes(name, prec):
    """BN_RUNNING (forward) and BN_FROZEN (forward + backward: dfeats, every dW, the heads) with non-trivial running statistics, which
    must come back bit-identical with their counters at 0."""
    _check(name, prec)


def _bits(t):
    return t.detach().to(device="cpu").contiguous().view(torch.int32)


GRAD_KEYS = ("dfeats", "dW", "dgamma", "dbeta", "dWh", "dbias")


@pytest.mark.parametrize("name", ["plain_3x33", "base3_57x9"])
def test_second_run_on_the_same_workspace_is_bit_identical(name):
    """The arenas are re-zeroed by the packing launch and the split reduce runs in a fixed order: forward + backward twice on one
    workspace give the same bits in the logits and in every gradient."""
    r = F.Runner(N.lib(), F.reference(F.BY_NAME[name]), F.SPLIT, DEV)
    outs = []
    for _ in range(2):
        assert r.forward() == 0 and r.backward() == 0
        outs.append(r.collect())
    for k in outs[0]:
        if k == "logits" or k.split("/")[0] in GRAD_KEYS:
            assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), k
    assert all(int(outs[1]["nbt/" + n]) == 2 for n in r.names)


@pytest.mark.parametrize("name", ["plain_3x33", "frozen_base3_57x9"])
def test_prepacked_forward_is_bit_identical_to_the_inline_pack(name):
    ref = F.reference(F.BY_NAME[name])
    a = F.Runner(N.lib(), ref, F.SPLIT, DEV)
    assert a.forward() == 0
    b = F.Runner(N.lib(), ref, F.SPLIT, DEV)
    assert b.pack() == 0 and b.forward(prepacked=True, two=True) == 0
    A, B = a.collect(), b.collect()
    for k in A:
        if k == "logits" or k.split("/")[0] in ("y", "scale", "shift", "mean", "rstd"):
            assert torch.equal(_bits(A[k]), _bits(B[k])), k
    a.sync()
    assert torch.equal(_bits(a.a["wp"]), _bits(b.a["wp"])) and torch.equal(_bits(a.a["oh64"]), _bits(b.a["oh64"]))


@pytest.mark.parametrize("prec", PRECS, ids=[F.PREC_NAME[p] for p in PRECS])
def test_running_logits_do_not_depend_on_the_rest_of_the_batch(prec):
    """BN_RUNNING: a frustum's logits inside the B = 57 batch, alone (B = 1) and inside a permuted batch agree to 1e-4, the bar of
    test_eval_outputs_are_independent_of_the_rest_of_the_batch, at other tile shapes: the frustum sits at other rows of other tiles."""
    ref = F.reference(F.BY_NAME["running_base3_57x9"])
    c = ref.case
    L2 = c.Ls[1]

    def logits_of(order):
        cc = c._replace(B=len(order), nbase=0)
        r = ref._replace(case=cc, feats=[f[order] for f in ref.feats], one_hot=ref.one_hot[order], G=ref.G[:len(order) * L2])
        rn = F.Runner(N.lib(), r, prec, DEV)
        assert rn.forward() == 0
        return rn.collect()["logits"].reshape(len(order), L2, -1)

    full = logits_of(torch.arange(c.B))
    perm = torch.randperm(c.B, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(c.B))
    mixed = logits_of(perm)
    assert float((mixed - full[perm]).abs().max()) <= 1e-4
    for b in (0, 6, 31, 56):                     # (rows 0.., 30..34 over the first tile boundary, 155.., the last five)
        alone = logits_of(torch.tensor([b]))
        assert float((alone[0] - full[b]).abs().max()) <= 1e-4, b


def _desc(**kw):
    base = dict(B=2, Ls=(9, 5, 3, 2), nvec=3, reg_out=39, mode=N.BN_TRAIN, prepacked=0, precision=0, nlev=4, c1=128)
    base.update(kw)
    Ls = tuple(base["Ls"]) + (0,) * (N.CN_MAXLEV - len(base["Ls"]))
    return N.CnDesc(base["B"], (ctypes.c_int32 * N.CN_MAXLEV)(*Ls), base["nvec"], base["reg_out"], base["mode"], 1e-5, 0.1,
                    base["prepacked"], base["precision"], base["nlev"], base["c1"])


def test_refusals_return_their_code_and_write_nothing():
    """Host-side refusals of fcn_convnet_sizes / _pack / _forward / _backward: the documented code comes back and the logits, every
    gradient buffer and the arenas keep their sentinel fill (nothing was launched)."""
    lib = N.lib()
    ref = F.reference(F.BY_NAME["plain_2x9"])
    r = F.Runner(lib, ref, F.SPLIT, DEV)
    r.logits.fill_(7.0)
    outs = [r.logits, r.dbh] + r.dfeats + r.dW + r.dg + r.db + [r.a[k] for k in ("y", "dz", "wp", "bn", "coef", "partial", "oh64")]
    before = [_bits(t).clone() for t in outs]
    fe, oh, st = F._arr(r.feats, N.CN_MAXLEV), r.oh.data_ptr(), r._stream()

    def fwd(d, ws=None, one_hot=oh):
        return lib.fcn_convnet_forward(ctypes.byref(d), ctypes.byref(r.params), ctypes.byref(ws or r.ws), fe, one_hot, r.logits.data_ptr(), st)

    def pack(d, ws=None, one_hot=oh):
        return lib.fcn_convnet_pack(ctypes.byref(d), ctypes.byref(r.params), ctypes.byref(ws or r.ws), one_hot, st)

    def bwd(d, ws=None):
        return lib.fcn_convnet_backward(ctypes.byref(d), ctypes.byref(r.params), ctypes.byref(ws or r.ws), fe, oh, r.dlog.data_ptr(),
                                        F._arr(r.dfeats, N.CN_MAXLEV), F._arr(r.dW, N.CN_MAXLAYER), F._arr(r.dg, N.CN_MAXLAYER),
                                        F._arr(r.db, N.CN_MAXLAYER), r.dbh.data_ptr(), st, None, None)

    shape = [(_desc(nlev=3, Ls=(9, 5, 3)), F.E_BADARG), (_desc(nlev=6), F.E_BADARG), (_desc(c1=96), F.E_BADARG),
             (_desc(Ls=(9, 4, 2, 1)), F.E_BADARG), (_desc(Ls=(9, 5, 3, 1)), F.E_BADARG), (_desc(Ls=(10, 5, 2, 1)), F.E_BADARG),
             (_desc(reg_out=0), F.E_LIMIT), (_desc(reg_out=127), F.E_LIMIT)]
    for d, code in shape:
        assert F.sizes(lib, d)[0] == code and pack(d) == code and fwd(d) == code and bwd(d) == code, (list(d.L), d.nlev, d.c1, d.reg_out)
    assert lib.fcn_convnet_logits_ld(ctypes.byref(_desc(reg_out=0))) == -1 and lib.fcn_convnet_logits_ld(ctypes.byref(_desc(reg_out=127))) == -1
    # the one-hot segment: 64 is the widest (test_widths runs it), 65 is refused; nvec > 0 needs the pointer
    assert fwd(_desc(nvec=65)) == F.E_LIMIT and pack(_desc(nvec=65)) == F.E_LIMIT
    assert fwd(_desc(), one_hot=None) == F.E_BADARG and pack(_desc(), one_hot=None) == F.E_BADARG
    for p in (-1, 4):
        assert fwd(_desc(precision=p)) == F.E_BADARG and bwd(_desc(precision=p)) == F.E_BADARG, p
    assert fwd(_desc(mode=3)) == F.E_BADARG and pack(_desc(mode=3)) == F.E_BADARG
    assert bwd(_desc(mode=N.BN_RUNNING)) == F.E_BADARG and bwd(_desc(mode=3)) == F.E_BADARG
    # null arenas
    fields = [f for f, _ in N.CnWs._fields_]

    def without(name):
        vals = {f: getattr(r.ws, f) for f in fields}
        vals[name] = None
        return N.CnWs(*[vals[f] for f in fields])

    for name in ("y", "wp", "bn", "stat", "partial", "oh64"):
        assert fwd(_desc(), ws=without(name)) == F.E_BADARG, name
    for name in ("y", "dz", "wp", "bn", "bstat", "coef", "partial"):
        assert bwd(_desc(), ws=without(name)) == F.E_BADARG, name
    for name in ("wp", "oh64"):
        assert pack(_desc(), ws=without(name)) == F.E_BADARG, name
    # size limits, by return code alone (no allocation).  Rows are divided through a float reciprocal (exact below 2^23) and every
    # arena is addressed with 32-bit byte offsets (rows * channels < 2^30 elements per layer).  The element limit binds first: the
    # heads read 768 channels on the L2 grid, so B * L2 = floor((2^30 - 1) / 768) = 1 398 101 rows is the largest accepted batch and
    # one more row is FCN_E_LIMIT -- as are B * L1 = 2^23 - 1 and 2^23, which the row limit alone would have told apart.
    def chain(L1):
        Ls = [L1]
        while len(Ls) < 4:
            Ls.append((Ls[-1] + 1) // 2)
        return tuple(Ls)

    top = ((1 << 30) - 1) // 768
    assert top == 1398101
    for B, L1, code in ((1, 2 * top, 0), (2, top - 1, 0), (1, 2 * top + 1, F.E_LIMIT), (2, top, F.E_LIMIT), (1, (1 << 23) - 1, F.E_LIMIT),
                        (1, 1 << 23, F.E_LIMIT), (1 << 23, 1, F.E_LIMIT), (2048, 4096, F.E_LIMIT)):
        assert (B * chain(L1)[1] <= top) == (code == 0)
        rc, sz = F.sizes(lib, _desc(B=B, Ls=chain(L1)))
        assert rc == code, (B, L1, rc)
        if code == 0:
            assert sz == F.plan(B, chain(L1), 128, 39)[1]
    r.sync()
    for t, b in zip(outs, before):
        assert torch.equal(_bits(t), b)
