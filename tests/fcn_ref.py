"""TEST INFRASTRUCTURE ONLY: the ConvFeatNet kernels (csrc/fcn_net.hip) layer by layer, off the fixture shapes, against the project's own
ConvFeatNet module + two Conv1d heads in fp64.  One harness for both backends: every entry goes through the C-ABI (fcn_convnet_sizes /
_pack / _forward / _backward) with caller-owned arenas, so the same code drives the host emulation with CPU tensors and
_native.lib() with CUDA tensors, and reads the pre-BatchNorm outputs and the published BatchNorm rows straight out of the workspace.

What a case is (Case): B, the lengths per level, block1's width, nvec, reg_out, the BatchNorm mode, nbase, a seed and an optional list
of dlogits rows that alone are nonzero.  nbase > 0 builds the batch from nbase distinct base frustums (features of every level + the
one-hot row) spread over the B slots by a fixed pseudo-random map: rows, tiles and weight-gradient splits are as many as wanted while
the batch statistics stay those of a small well-conditioned set and the distinct activations stay few enough for a draw that keeps
every BatchNorm output KINK_MIN away from zero; dlogits is random per row, so a wrong row always shows.

Units of the reported errors: logits absolute; every gradient tensor and the running statistics in units of the fp64 tensor's maximum;
the per-layer y and mean in units of max(1, the fp64 tensor's maximum) -- absolute for the O(1) tensors the logits bar was written for,
relative where a layer's values are larger; rstd, scale and shift per channel as the ACTIVATION error that explains them: with
rstd = (var + eps)^-1/2 and d var ~ 2 dy / rstd, d rstd ~ rstd^2 dy, so |d rstd| and |d scale| are divided by max(1, rstd^2) and
|d shift| (which carries mean * d scale) by max(1, rstd^2 * max(1, |mean|)) before the maximum over channels is taken.  (Judged
against the tensor maximum instead, one low-variance channel -- four distinct rows at the top of the small cases -- amplifies a 1e-6
activation error a hundredfold in the kernels and in the fp32 module alike, and the ratio of two such maxima says nothing.)  Bars (bars()): the project's own (tests/test_emu_fcn.py) per tensor; in the
exact-fp32 mode a gradient tensor gets max(1e-4, 4 x the error of the fp32 evaluation of the same module on the same inputs), a
per-layer forward tensor max(the mode's logits bar, 4 x that fp32 error) -- the kernels are an fp32 evaluation in another summation order.
tests/test_fcn_ref_referee.py holds the reference itself to the conditions that make those bars meaningful."""
import collections
import copy
import ctypes
import functools
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from frustum_convnet_amd import _native as N                                   # noqa: E402
from frustum_convnet_amd.fcn_fused import layer_names                          # noqa: E402

E_BADARG, E_LIMIT = 10001, 10002          # FCN_E_BADARG, FCN_E_LIMIT
SPLIT, F32 = 0, 1                         # FCN_PREC_SPLIT, FCN_PREC_F32
PREC_NAME = {SPLIT: "split", F32: "f32"}
KINK_MIN, MAX_DRAWS = 3e-5, 20
MIN_BN_ROWS = 4                           # distinct rows a BN_TRAIN layer must see (fewer: ill-conditioned, no tolerance rescues it)
CAP_GRAD, CAP_LOGITS = 5e-5, 1e-5         # what the fp32 module itself may be off fp64 (half the exact-fp32 gradient bar; the logits bar)
# constants of csrc/fcn_net.hip restated (plan() is checked against fcn_convnet_sizes)
OH_PAD, CG_REP, KC, WG_TARGET, WG_MINROWS = 64, 4, 32, 512, 256

Case = collections.namedtuple("Case", "name B Ls c1 nvec reg_out mode nbase seed rows hot")


def case(name, B, Ls, nbase=0, c1=None, nvec=3, reg_out=None, mode=N.BN_TRAIN, seed=0, rows=None, hot=None):
    """hot: the one-hot column of every slot (None: base index modulo nvec)."""
    nlev = len(Ls)
    return Case(name, B, tuple(Ls), c1 or (128 if nlev == 4 else 64), nvec, reg_out or (39 if nlev == 4 else 67), mode, nbase, seed,
                None if rows is None else tuple(rows), None if hot is None else tuple(hot))


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases (shared by the CPU referee, tests/test_gpu_fcn_layers.py and its registration in tests/test_emu_gpu_subset.py)
# ---------------------------------------------------------------------------------------------------------------------------------
# Seeds: 0 unless the reference itself asks for another one (tests/test_fcn_ref_referee.py): base3_40x33 has no kink-free draw in 20 with
# seed 0; plain_2x9, the reg_out cases on it and plain_2x21_5lev_c128 sit at or over the fp32-module cap with seed 0 (4.4e-5, 5.0e-5,
# 8.9e-5 against 5e-5) and well inside it with seed 1.
# Sentinel rows of the L2 grid (-1: the last row): the first row, both sides of the first 32-row tile boundary, both sides of every
# boundary between two weight-gradient splits of the heads (160 rows each at B = 57, 256 at B = 40: heads_split_starts, checked by the
# referee), rows 511 / 512 where the grid has them, the last row.

TRAIN_CASES = [
    case("plain_2x9", 2, (9, 5, 3, 2), seed=1),                  # every layer under one 32-row tile
    case("plain_3x11", 3, (11, 6, 3, 2)),                       # 33 rows: one over a tile
    case("plain_1x64", 1, (64, 32, 16, 8)),                     # B = 1, exact tile multiples, 8 rows at the top
    case("plain_3x33", 3, (33, 17, 9, 5)),                      # all lengths odd; deconvolution outputs 18 and 20 cropped to 17
    case("plain_8x5", 8, (5, 3, 2, 1)),                         # a level of one position: both k=3 neighbours are padding
    case("plain_16x3", 16, (3, 2, 1, 1)),                       # two such levels
    case("plain_2x21_5lev", 2, (21, 11, 6, 3, 2)),              # 5 levels, cropped
    case("base3_57x9", 57, (9, 5, 3, 2), nbase=3),              # 513 rows: one over a weight-gradient split
    case("base3_58x9", 58, (9, 5, 3, 2), nbase=3),              # 522 rows
    case("base3_40x33", 40, (33, 17, 9, 5), nbase=3, seed=1),        # 1320 rows: several splits, tiles crossing frustum ends
    case("base4_103x5", 103, (5, 3, 2, 1), nbase=4),            # 515 rows with a one-position level
    case("base2_47x21_5lev", 47, (21, 11, 6, 3, 2), nbase=2),   # 5 levels, 987 rows at level 1 and 517 on the L2 grid
    case("plain_2x9_c64", 2, (9, 5, 3, 2), c1=64),              # (4 levels, c1 = 64): accepted by the plan, no product class
    case("plain_2x21_5lev_c128", 2, (21, 11, 6, 3, 2), c1=128, seed=1),  # (5 levels, c1 = 128): the same
]
SENTINEL_CASES = [
    case("base3_57x9_rows", 57, (9, 5, 3, 2), nbase=3, rows=(0, 31, 32, 159, 160, -1)),
    case("base3_40x33_rows", 40, (33, 17, 9, 5), nbase=3, seed=1, rows=(0, 31, 32, 255, 256, 511, 512, -1)),
]
NVECS = (0, 1, 3, 10, 64)
REG_OUTS = (1, 39, 62, 63, 67, 126)       # 62 fills ld = 64 exactly, 63 is the first that takes ld = 128
_WIDTH_SEED = {"nvec10": 2, "reg1": 2, "reg39": 1, "reg62": 1, "reg63": 1, "reg126": 1}     # (as above: the cap)
# the hot columns of the nvec cases span the segment: the last column (nvec - 1), the first, and both sides of its middle -- at nvec = 64
# both 32-wide K chunks of the OH_PAD segment and column 63; four frustums carry them
_HOT = {10: (9, 0, 5, 4), 64: (63, 0, 32, 31)}
WIDTH_CASES = ([case("nvec%d" % v, 4 if v in _HOT else 2, (9, 5, 3, 2), nvec=v, seed=_WIDTH_SEED.get("nvec%d" % v, 0), hot=_HOT.get(v))
                for v in NVECS if v != 3] +
               [case("reg%d" % r, 2, (9, 5, 3, 2), reg_out=r, seed=_WIDTH_SEED.get("reg%d" % r, 0)) for r in REG_OUTS])
MODE_CASES = [case("%s_%s" % (mname, nm), B, Ls, nbase=nb, mode=mode)
              for mname, mode in (("running", N.BN_RUNNING), ("frozen", N.BN_FROZEN))
              for nm, B, Ls, nb in (("1x9", 1, (9, 5, 3, 2), 0), ("base3_57x9", 57, (9, 5, 3, 2), 3))]
ALL_CASES = TRAIN_CASES + SENTINEL_CASES + WIDTH_CASES + MODE_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


# ---------------------------------------------------------------------------------------------------------------------------------
# cn_make_plan / cn_offsets restated: layer order, widths, lengths and the arena totals
# ---------------------------------------------------------------------------------------------------------------------------------
def logits_ld(reg_out):
    return 64 if 2 + reg_out <= 64 else 128


def wgrad_split_rows(R, Nn, Kt):
    """rows per weight-gradient split of a layer of R rows, Nn outputs and reduction length Kt (pick_wrows / cn_wgrad_split)."""
    ns = max(1, min(WG_TARGET // max((Nn // 64) * (Kt // 64), 1), (R + WG_MINROWS - 1) // WG_MINROWS))
    return max(((R + ns - 1) // ns + 31) // 32 * 32, 2 * KC)


def heads_split_starts(c):
    """first rows of the heads' weight-gradient splits on the L2 grid (dWh is the fixed-order sum of one partial per split)."""
    R = c.B * c.Ls[1]
    rows = wgrad_split_rows(R, logits_ld(c.reg_out), 256 * (len(c.Ls) - 1))
    return list(range(0, R, rows))


def plan(B, Ls, c1, reg_out):
    """[(name, Lout, N, Cs, Ktot, dk)] in the C-ABI's layer order + the six totals of fcn_convnet_sizes."""
    n = len(Ls)
    bw = (0, c1, 128, 256, 512, 512)              # block widths by level
    fc = (0, 128, 128, 256, 512, 512)             # pooled feature widths by level
    lay = [("block1_conv1", Ls[0], c1, c1, 3 * (fc[1] + OH_PAD), 0)]
    for j in range(2, n + 1):
        lay.append(("block%d_conv1" % j, Ls[j - 1], bw[j], bw[j], 3 * bw[j - 1], 0))
        lay.append(("block%d_conv2" % j, Ls[j - 1], bw[j], bw[j], 3 * bw[j], 0))
        lay.append(("block%d_merge" % j, Ls[j - 1], bw[j], bw[j], bw[j] + fc[j] + OH_PAD, 0))
    for j in range(2, n + 1):
        k = 1 << (j - 2)
        lay.append(("block%d_deconv" % j, Ls[j - 1], k * 256, 256, bw[j], k))
    ld = logits_ld(reg_out)
    lay.append(("heads", Ls[1], ld, ld, 256 * (n - 1), 0))
    assert tuple(l[0] for l in lay[:-1]) == layer_names(n)
    ny = sum(B * Lo * Nn for _, Lo, Nn, _, _, _ in lay)
    nwp = sum(Nn * Kt for _, _, Nn, _, Kt, _ in lay)
    ncs = sum(Cs for _, _, _, Cs, _, _ in lay)
    pmax = 0
    for _, Lo, Nn, _, Kt, _ in lay:
        rows = wgrad_split_rows(B * Lo, Nn, Kt)
        pmax = max(pmax, ((B * Lo + rows - 1) // rows) * Nn * Kt)
    return lay, (ny, 3 * nwp, 4 * ncs, CG_REP * 2 * ncs, 5 * ncs, 4 * pmax)


def make_desc(c, precision=SPLIT, prepacked=0):
    return N.CnDesc(c.B, (ctypes.c_int32 * N.CN_MAXLEV)(*c.Ls), c.nvec, c.reg_out, c.mode, 1e-5, 0.1, prepacked, precision, len(c.Ls), c.c1)


def sizes(lib, desc):
    out = (ctypes.c_int64 * 6)()
    rc = lib.fcn_convnet_sizes(ctypes.byref(desc), ctypes.byref(out))
    return rc, tuple(int(v) for v in out)


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference: the module in fp64 (and the same module in fp32, for the bars and the referee's cap)
# ---------------------------------------------------------------------------------------------------------------------------------
def net_class(nlev, c1):
    from frustum_convnet_amd import det_base, det_base_sunrgbd
    base = det_base.ConvFeatNet if nlev == 4 else det_base_sunrgbd.ConvFeatNet
    if base.WIDTHS[0] == c1:
        return base

    class _OtherBlock1(base):          # a width pair the plan accepts and no product class uses: only WIDTHS differs
        WIDTHS = (c1,) + tuple(base.WIDTHS[1:])
    return _OtherBlock1


def slot_map(c):
    """base index of every slot of the batch: fixed per case, pseudo-random, every base present."""
    if not c.nbase:
        return torch.arange(c.B)
    g = torch.Generator().manual_seed(977 + c.seed)
    m = torch.randint(c.nbase, (c.B,), generator=g)
    m[torch.randperm(c.B, generator=g)[:c.nbase]] = torch.arange(c.nbase)
    return m


def sentinel_rows(c):
    R = c.B * c.Ls[1]
    return sorted({r % R for r in c.rows if -R <= r < R})


def _evaluate(c, net, cls_out, reg, feats, one_hot, G):
    """One forward (+ backward unless BN_RUNNING) of the module path; every tensor the kernels are compared on, by name, in the
    kernels' layouts (rows = (frustum, position))."""
    names = layer_names(len(c.Ls))
    dt = feats[0].dtype
    feats = [f.detach().clone().requires_grad_(True) for f in feats]
    xs = [f.permute(0, 2, 1) if one_hot is None else torch.cat([f.permute(0, 2, 1), one_hot[:, :, None].expand(-1, -1, f.shape[1])], 1)
          for f in feats]
    convs, kink = {}, [float("inf")]
    hooks = []
    for n in names:
        seq = getattr(net, n)
        hooks.append(seq[0].register_forward_hook(lambda m, i, o, n=n: convs.__setitem__(n, o.detach())))
        hooks.append(seq[1].register_forward_hook(lambda m, i, o: kink.__setitem__(0, min(kink[0], float(o.detach().abs().min())))))
    before = {n: (getattr(net, n)[1].running_mean.clone(), getattr(net, n)[1].running_var.clone()) for n in names}
    out = net(*xs)
    for h in hooks:
        h.remove()
    logits = torch.cat([cls_out(out), reg(out)], 1)                         # (B, ncol, L2)
    ncol = 2 + c.reg_out
    T = {"logits": logits.detach().permute(0, 2, 1).reshape(c.B * c.Ls[1], ncol)}
    for n in names:
        bn = getattr(net, n)[1]
        y = convs[n].permute(0, 2, 1).reshape(-1, convs[n].shape[1])         # a deconvolution: the uncropped (B * L * k, 256) rows
        if c.mode == N.BN_TRAIN:
            mean, var = y.mean(0), y.var(0, unbiased=False)
        else:
            mean, var = before[n]
        rstd = 1.0 / torch.sqrt(var + bn.eps)
        scale = bn.weight.detach() * rstd
        T["y/" + n], T["mean/" + n], T["rstd/" + n], T["scale/" + n] = y, mean, rstd, scale
        T["shift/" + n] = bn.bias.detach() - mean * scale
        T["rmean/" + n], T["rvar/" + n] = bn.running_mean.clone(), bn.running_var.clone()
        T["nbt/" + n] = bn.num_batches_tracked.clone()
    if c.mode != N.BN_RUNNING:
        (logits * G.to(dt).reshape(c.B, c.Ls[1], ncol).permute(0, 2, 1)).sum().backward()
        for s, f in enumerate(feats):
            T["dfeats/%d" % s] = f.grad
        for n in names:
            seq = getattr(net, n)
            T["dW/" + n], T["dgamma/" + n], T["dbeta/" + n] = seq[0].weight.grad, seq[1].weight.grad, seq[1].bias.grad
        T["dWh"] = torch.cat([cls_out.weight.grad, reg.weight.grad], 0)
        T["dbias"] = torch.cat([cls_out.bias.grad, reg.bias.grad], 0)
    return {k: v.detach() for k, v in T.items()}, kink[0]


def _draw(c, attempt):
    torch.manual_seed(c.seed + 1000 * attempt)
    nlev = len(c.Ls)
    net = net_class(nlev, c.c1)(128, c.nvec).double()
    names = layer_names(nlev)
    cls_out = torch.nn.Conv1d(256 * (nlev - 1), 2, 1).double()
    reg = torch.nn.Conv1d(256 * (nlev - 1), c.reg_out, 1).double()
    with torch.no_grad():
        for n in names:
            bn = getattr(net, n)[1]
            bn.weight.uniform_(0.5, 1.5)
            bn.bias.uniform_(-0.3, 0.3)
            bn.running_mean.normal_(0.0, 0.3)          # non-trivial running statistics in every mode: the update of BN_TRAIN must
            bn.running_var.uniform_(0.5, 2.0)          # blend them, BN_RUNNING / BN_FROZEN normalise with them
        cls_out.bias.uniform_(-0.1, 0.1)
        reg.bias.uniform_(-0.1, 0.1)
    net.train(c.mode == N.BN_TRAIN)
    widths = net.WIDTHS
    nsrc = c.nbase or c.B
    m = slot_map(c)
    feats = [torch.randn(nsrc, c.Ls[s], widths[s] if s else 128, dtype=torch.float64).abs()[m] for s in range(nlev)]
    one_hot = None
    if c.nvec:
        one_hot = torch.zeros(c.B, c.nvec, dtype=torch.float64)
        one_hot[torch.arange(c.B), m % c.nvec if c.hot is None else torch.tensor(c.hot)] = 1.0
    R, ncol = c.B * c.Ls[1], 2 + c.reg_out
    G = torch.randn(R, ncol, dtype=torch.float64)
    if c.rows is not None:
        keep = torch.zeros(R, 1, dtype=torch.float64)
        keep[sentinel_rows(c)] = 1.0
        G = G * keep
    return net, cls_out, reg, feats, one_hot, G


Reference = collections.namedtuple("Reference", "case net cls_out reg feats one_hot G init T T32 e32 kink draws")


def err_of(name, a, b, T):
    """error of tensor `name` (a) against the fp64 tensor b = T[name], in the unit of its kind (module docstring)."""
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    d = (a - b).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf")             # NaN anywhere: as wrong as can be
    kind = name.split("/")[0]
    if kind == "logits":
        return float(d.max())
    if kind in ("y", "mean"):
        return float(d.max()) / max(1.0, float(b.abs().max()))
    if kind in ("rstd", "scale", "shift"):
        r2 = T["rstd/" + name.split("/")[1]].double() ** 2
        if kind == "shift":
            r2 = r2 * T["mean/" + name.split("/")[1]].double().abs().clamp(min=1.0)
        return float((d / r2.clamp(min=1.0)).max())
    return float(d.max()) / max(float(b.abs().max()), 1e-30)


@functools.lru_cache(maxsize=None)
def reference(c):
    """The kink-free draw of a case: fp64 module tensors (T), the fp32 module's (T32) and its errors (e32).  Cached and never modified:
    the split, exact-fp32 and exact-property tests of a case share it."""
    for attempt in range(MAX_DRAWS):
        net, cls_out, reg, feats, one_hot, G = _draw(c, attempt)
        init = {n: (getattr(net, n)[1].running_mean.clone(), getattr(net, n)[1].running_var.clone()) for n in layer_names(len(c.Ls))}
        twin = [copy.deepcopy(m).float() for m in (net, cls_out, reg)]
        T, kink = _evaluate(c, net, cls_out, reg, feats, one_hot, G)
        if kink >= KINK_MIN:
            break
    else:
        raise RuntimeError("%s: no kink-free draw in %d" % (c.name, MAX_DRAWS))
    T32, _ = _evaluate(c, twin[0], twin[1], twin[2], [f.float() for f in feats], None if one_hot is None else one_hot.float(), G)
    e32 = {k: err_of(k, T32[k], T[k], T) for k in T if not k.startswith("nbt/")}
    return Reference(c, net, cls_out, reg, feats, one_hot, G, init, T, T32, e32, kink, attempt + 1)


def bars(ref, precision):
    """bar of every compared tensor of a case in an operand mode (module docstring)."""
    c = ref.case
    logit_bar = 1e-4 if precision == SPLIT else 1e-5
    out = {}
    for k in ref.T:
        kind = k.split("/")[0]
        if kind == "nbt":
            continue
        if kind == "logits":
            out[k] = logit_bar
        elif kind in ("rmean", "rvar"):
            out[k] = 1e-5 if c.mode == N.BN_TRAIN else 0.0           # not BN_TRAIN: bit-identical to what went in
        elif kind in ("y", "mean", "rstd", "scale", "shift"):
            out[k] = max(logit_bar, 4.0 * ref.e32[k])
        elif c.mode == N.BN_FROZEN and kind in ("dgamma", "dbeta"):
            continue                                                 # (test_c_abi_bn_modes / test_gpu_frozen_bn.py hold that contract)
        else:
            out[k] = 1e-3 if precision == SPLIT else max(1e-4, 4.0 * ref.e32[k])
    return out


def distinct_bn_rows(ref):
    """fewest distinct rows any BatchNorm of the case takes its statistics over."""
    return min(int(torch.unique(ref.T["y/" + n], dim=0).shape[0]) for n in layer_names(len(ref.case.Ls)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernels through the C-ABI
# ---------------------------------------------------------------------------------------------------------------------------------
def load_emu():
    """the host emulation of the kernels (tests/host_harness) with the argument types of the entries used here: takes CPU tensors."""
    import emu_fcn
    L = emu_fcn.load_emu()
    L.fcn_convnet_forward2.argtypes = list(L.fcn_convnet_forward.argtypes) + [ctypes.POINTER(N.c_fp)]
    return L


def _arr(ts, n):
    return (N.c_fp * n)(*([None if t is None else t.data_ptr() for t in ts] + [None] * (n - len(ts))))


class Runner:
    """Arenas, parameters and outputs of one case on `device`, and the C-ABI calls on them.  Arenas the kernels are to write are
    pre-filled with NaN (the product allocates them uninitialised)."""

    def __init__(self, lib, ref, precision, device):
        c = self.case = ref.case
        self.lib, self.ref, self.dev = lib, ref, device
        self.names = layer_names(len(c.Ls))
        f32 = torch.float32
        put = lambda t, dt=f32: t.detach().to(dt).clone().contiguous().to(device=device)
        self.desc = make_desc(c, precision)
        rc, sz = sizes(lib, self.desc)
        assert rc == 0, rc
        self.layers, totals = plan(c.B, c.Ls, c.c1, c.reg_out)
        assert sz == totals, (sz, totals)
        ny, nwp, nbn, nst, ncoef, npart = sz
        nan = lambda n: torch.full((max(n, 1),), float("nan"), dtype=f32, device=device)
        self.a = dict(y=nan(ny), dz=nan(ny), wp=nan(nwp), bn=nan(nbn), stat=torch.zeros(nst, dtype=torch.float64, device=device),
                      bstat=torch.zeros(nst, dtype=torch.float64, device=device), coef=nan(ncoef), partial=nan(npart),
                      oh64=torch.zeros(c.B * OH_PAD, dtype=f32, device=device), flags=torch.zeros(1, dtype=torch.int32, device=device))
        self.ws = N.CnWs(*[self.a[k].data_ptr() for k in ("y", "dz", "wp", "bn", "stat", "bstat", "coef", "partial", "oh64", "flags")])
        seqs = [getattr(ref.net, n) for n in self.names]
        self.Ws = [put(s[0].weight) for s in seqs]
        self.gs = [put(s[1].weight) for s in seqs]
        self.bs = [put(s[1].bias) for s in seqs]
        self.Wh = put(torch.cat([ref.cls_out.weight, ref.reg.weight], 0))
        self.bh = put(torch.cat([ref.cls_out.bias, ref.reg.bias], 0))
        self.rm = [put(ref.init[n][0]) for n in self.names]
        self.rv = [put(ref.init[n][1]) for n in self.names]
        self.nbt = [torch.zeros(1, dtype=torch.int64, device=device) for _ in self.names]
        self.params = N.CnParams(_arr(self.Ws + [self.Wh], N.CN_MAXLAYER), _arr(self.gs, N.CN_MAXLAYER), _arr(self.bs, N.CN_MAXLAYER),
                                 _arr(self.rm, N.CN_MAXLAYER), _arr(self.rv, N.CN_MAXLAYER), _arr(self.nbt, N.CN_MAXLAYER),
                                 self.bh.data_ptr())
        self.feats = [put(f) for f in ref.feats]
        self.oh = None if ref.one_hot is None else put(ref.one_hot)
        self.ld = lib.fcn_convnet_logits_ld(ctypes.byref(self.desc))
        assert self.ld == logits_ld(c.reg_out)
        R, ncol = c.B * c.Ls[1], 2 + c.reg_out
        self.logits = torch.full((R, self.ld), float("nan"), dtype=f32, device=device)
        dlog = torch.zeros(R, self.ld, dtype=f32)
        dlog[:, :ncol] = ref.G.to(f32)
        self.dlog = dlog.to(device=device)
        like = lambda t: torch.full_like(t, float("nan"))
        self.dfeats = [like(f) for f in self.feats]
        self.dW = [like(w) for w in self.Ws] + [like(self.Wh)]
        self.dg = [like(g) for g in self.gs]
        self.db = [like(b) for b in self.bs]
        self.dbh = like(self.bh)

    def _stream(self):
        return N.current_stream(self.dev) if str(self.dev).startswith("cuda") else None

    def sync(self):
        if str(self.dev).startswith("cuda"):
            torch.cuda.synchronize()

    def _oh(self):
        return None if self.oh is None else self.oh.data_ptr()

    def pack(self):
        return self.lib.fcn_convnet_pack(ctypes.byref(self.desc), ctypes.byref(self.params), ctypes.byref(self.ws), self._oh(), self._stream())

    def forward(self, prepacked=False, two=False):
        self.desc.prepacked = 1 if prepacked else 0
        args = (ctypes.byref(self.desc), ctypes.byref(self.params), ctypes.byref(self.ws), _arr(self.feats, N.CN_MAXLEV), self._oh(),
                self.logits.data_ptr(), self._stream())
        rc = self.lib.fcn_convnet_forward2(*args, None) if two else self.lib.fcn_convnet_forward(*args)
        self.desc.prepacked = 0
        return rc

    def backward(self):
        return self.lib.fcn_convnet_backward(ctypes.byref(self.desc), ctypes.byref(self.params), ctypes.byref(self.ws),
                                             _arr(self.feats, N.CN_MAXLEV), self._oh(), self.dlog.data_ptr(), _arr(self.dfeats, N.CN_MAXLEV),
                                             _arr(self.dW, N.CN_MAXLAYER), _arr(self.dg, N.CN_MAXLAYER), _arr(self.db, N.CN_MAXLAYER),
                                             self.dbh.data_ptr(), self._stream(), None, None)

    def collect(self):
        """every compared tensor by the names of _evaluate, on the CPU (+ 'pad': the logits' padding columns, 'flags')."""
        self.sync()
        c = self.case
        cpu = lambda t: t.detach().to(device="cpu").clone()
        ncol = 2 + c.reg_out
        lg = cpu(self.logits)
        T = {"logits": lg[:, :ncol], "pad": lg[:, ncol:], "flags": cpu(self.a["flags"])}
        y, bn = cpu(self.a["y"]), cpu(self.a["bn"])
        yo = bo = 0
        for i, n in enumerate(self.names):
            _, Lo, Nn, Cs, _, dk = self.layers[i]
            T["y/" + n] = y[yo:yo + c.B * Lo * Nn].reshape(c.B * Lo * max(dk, 1), Cs)
            for q, kind in enumerate(("scale", "shift", "mean", "rstd")):
                T[kind + "/" + n] = bn[bo + q * Cs:bo + (q + 1) * Cs]
            yo += c.B * Lo * Nn
            bo += 4 * Cs
            T["rmean/" + n], T["rvar/" + n], T["nbt/" + n] = cpu(self.rm[i]), cpu(self.rv[i]), cpu(self.nbt[i])
            T["dW/" + n], T["dgamma/" + n], T["dbeta/" + n] = cpu(self.dW[i]), cpu(self.dg[i]), cpu(self.db[i])
        for s in range(len(c.Ls)):
            T["dfeats/%d" % s] = cpu(self.dfeats[s])
        T["dWh"], T["dbias"] = cpu(self.dW[len(self.names)]), cpu(self.dbh)
        return T


def run(lib, ref, precision, device):
    """forward (+ backward unless BN_RUNNING) of a case through the C-ABI; returns the collected tensors."""
    r = Runner(lib, ref, precision, device)
    rc = r.forward()
    assert rc == 0, ("fcn_convnet_forward", rc)
    if ref.case.mode != N.BN_RUNNING:
        rc = r.backward()
        assert rc == 0, ("fcn_convnet_backward", rc)
    return r.collect()


def compare(ref, got, precision):
    """{tensor: (error, bar)} of every compared tensor + the exact conditions (padding columns, counters, flags) as errors 0 / inf."""
    c = ref.case
    res = {}
    for k, bar in bars(ref, precision).items():
        if bar == 0.0:
            res[k] = (0.0 if torch.equal(got[k].float(), ref.T[k].float()) else float("inf"), 0.0)
        else:
            res[k] = (err_of(k, got[k], ref.T[k], ref.T), bar)
    res["logits_pad"] = (float(got["pad"].abs().max()) if got["pad"].numel() else 0.0, 0.0)
    want = 1 if c.mode == N.BN_TRAIN else 0
    res["num_batches_tracked"] = (0.0 if all(int(got["nbt/" + n]) == want for n in layer_names(len(c.Ls))) else float("inf"), 0.0)
    res["flags"] = (float(int(got["flags"])), 0.0)
    return res


def failures(res):
    return {k: v for k, v in res.items() if not v[0] <= v[1]}


def worst(res):
    """(logits error, worst per-layer forward ratio error / bar, its tensor, worst gradient error, its tensor) for the tables of EXPERIMENTS.md."""
    f = [(v[0] / v[1], k) for k, v in res.items() if k.split("/")[0] in ("y", "mean", "rstd", "scale", "shift")]
    fw = max(f) if f else (0.0, "-")
    g = [(v[0], k) for k, v in res.items() if k.split("/")[0] in ("dfeats", "dW", "dgamma", "dbeta", "dWh", "dbias")]
    gw = max(g) if g else (0.0, "-")
    return res["logits"][0], fw[0], fw[1], gw[0], gw[1]
