"""-m gpu: frozen BatchNorm (freeze_bn, FCN_BN_FROZEN at the C-ABI) -- BatchNorm normalises with its running statistics, never
changes them, and the step differentiates through them: the reference's model.eval() fine-tune (models/det_base.py:62-103,
163-224 return differentiable tensors in eval mode).  The referee is the fp64 oracle run with training=False, whose _bn then
differentiates through the running statistics.

The fixtures' running statistics sit at their init values (0 / 1), where a kernel that ignores them could pass by accident, so
every parity test first installs seeded, clearly non-trivial running statistics (means of the order of the batch means,
variances in [0.3, 3]) and checks that the frozen result is at least 100 x its bar away from the train()-mode result of the same
model: a kernel that still normalised with batch statistics could not pass.

Bars.  The oracle parity holds the frozen step, in the default split-operand mode and in the exact-fp32 one, to the bars of
test_gradients_vs_fp64_oracle (8e-5 of each tensor's max + 2e-6 of the largest gradient).  The running statistics are kept off the
ReLU kinks first (_clear_kinks): with running statistics an activation error reaches the ReLU unnormalised, and a mask that flips
against fp64 at an output 1e-6 from zero moves a whole gradient tensor -- the comparison would measure the data, not the kernels."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import load_golden, golden_inputs, golden_state_dict
from frustum_convnet_amd import synth
from test_gpu_model import _model

pytestmark = pytest.mark.gpu
GUARD = 100.0          # the frozen result must be at least GUARD x its bar away from the train()-mode result
TIGHT_REL = 8e-5       # gradient bar relative to each tensor's max, as test_gradients_vs_fp64_oracle holds the training step


@pytest.fixture
def exact_f32():
    """The exact-fp32 operand mode for the whole test (the tight oracle bars, see the module docstring)."""
    from frustum_convnet_amd import precision
    with precision.precision("f32"):
        yield


KINK_MIN = 2e-4         # every pre-ReLU BatchNorm output of a frozen unit is kept at least this far from zero (see _clear_kinks)


def _frozen_pre_relu(g, sd):
    """{BatchNorm prefix: pre-ReLU output} of the fp64 oracle's running-statistics forward (training=False everywhere)."""
    from oracle import det_ref
    d64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in synth.to_torch(golden_inputs(g)).items()}
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    zs, orig = {}, det_ref._bn

    def bn(x, sd_, prefix, training, rec=None):
        z = orig(x, sd_, prefix, training, rec)
        zs[prefix] = z
        return z
    det_ref._bn = bn
    try:
        with torch.no_grad():
            det_ref.forward(sd64, d64, tuple(g["meta_strides"]), training=False, with_loss=False)
    finally:
        det_ref._bn = orig
    return zs


def _clear_kinks(g, sd, passes=16, span=0.05):
    """Moves each channel's running mean by at most span / (gamma * rstd) so that no pre-ReLU output of the fp64 oracle lies within
    KINK_MIN of zero.  Under running statistics an activation error of the fp32 path reaches the ReLU unnormalised: the default
    split-operand mode carries ~1e-6 absolute error in a pre-activation (fp16 operand parts of small weights lose bits to
    subnormals), enough to flip the mask of an output the fp64 oracle puts at 1.8e-6 -- one such position of car_b4_n512 with
    running statistics equal to the batch statistics moves conv_net.block4_conv1's gradients by 0.19 of their max, the whole
    difference being that position's dL/dz.  A test that compares against fp64 has to keep its data off the kinks (the FCN's host
    emulation test draws until it is, tests/emu_fcn.py); the shift per channel is a constant, chosen as the largest gap of the
    channel's values around zero, and repeated pass by pass down the network (a channel's shift moves every later layer)."""
    eps = 1e-5
    for _ in range(passes):
        zs = _frozen_pre_relu(g, sd)
        moved = False
        for prefix, z in zs.items():
            v = z.transpose(0, 1).reshape(z.shape[1], -1)
            near = v.abs().min(dim=1).values < KINK_MIN
            if not bool(near.any()):
                continue
            gam = sd[prefix + ".weight"].double()
            rstd = torch.rsqrt(sd[prefix + ".running_var"].double() + eps)
            rm = sd[prefix + ".running_mean"].double().clone()
            for c in torch.nonzero(near).flatten().tolist():
                w = v[c][(v[c] > -2 * span) & (v[c] < 2 * span)].sort().values
                cand = torch.cat([torch.tensor([-span, span], dtype=torch.float64), -(w[1:] + w[:-1]) / 2])
                cand = cand[cand.abs() <= span]
                dist = (w.view(1, -1) + cand.view(-1, 1)).abs().min(dim=1).values if w.numel() else torch.full_like(cand, 1.0)
                sft = float(cand[int(dist.argmax())])
                if float(gam[c]) != 0.0:
                    rm[c] -= sft / (float(gam[c]) * float(rstd[c]))
                    moved = True
            sd[prefix + ".running_mean"] = rm.float()
        if not moved:
            return sd
    return sd


_STATS_CACHE = {}


def _running_stats(g, seed=11, spread=1.0):
    key = tuple(str(np.asarray(g[k]).tolist()) for k in ("meta_batch", "meta_npoint", "meta_strides", "meta_variant", "meta_seed")) + (
        seed, spread)
    if key not in _STATS_CACHE:
        _STATS_CACHE[key] = _make_running_stats(g, seed, spread)
    return {k: v.clone() for k, v in _STATS_CACHE[key].items()}


def _make_running_stats(g, seed, spread):
    """Golden state dict with seeded running statistics: mean = batch mean + 0.5 spread batch std * N(0,1), var = batch var *
    e^(0.5 spread N(0,1)) clipped to [0.3, 3] where the batch variance lies in that range (spread = 0: the batch statistics
    themselves), the batch statistics taken from one fp64 oracle training forward on the fixture's batch, then moved off the ReLU
    kinks (_clear_kinks).  (The layer-1 batch variances of the PointNet scales reach ~460 on these fixtures: pinning those to 3
    inflates every later activation ~12x.)"""
    from oracle import det_ref
    sd = {k: v.clone() for k, v in golden_state_dict(g).items()}
    data_np = golden_inputs(g)
    rec = det_ref.BNState()
    with torch.no_grad():
        d64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in synth.to_torch(data_np).items()}
        sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
        det_ref.forward(sd64, d64, tuple(g["meta_strides"]), training=True, rec=rec, with_loss=False)
    gen = torch.Generator().manual_seed(seed)
    for prefix, (mean, var, _n) in sorted(rec.stats.items()):
        mean, var = mean.float(), var.float()
        rm = mean + 0.5 * spread * var.clamp(min=0).sqrt() * torch.randn(mean.shape, generator=gen)
        rv = var * torch.exp(0.5 * spread * torch.randn(var.shape, generator=gen))
        if spread > 0:
            inside = (var >= 0.3) & (var <= 3.0)
            rv = torch.where(inside, rv.clamp(0.3, 3.0), rv)
        sd[prefix + ".running_mean"] = rm
        sd[prefix + ".running_var"] = rv
    return _clear_kinks(g, sd)


def _load(g, sd, freeze=None, train=True):
    m = _model(g)
    m.load_state_dict(sd, strict=True)
    m.train(train)
    if freeze == "all":
        m.freeze_bn()
    elif freeze == "feat":
        m.feat_net.freeze_bn()
    elif freeze == "conv":
        m.conv_net.freeze_bn()
    return m


def _bn_buffers(m):
    return {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k or "tracked" in k}


def _run(m, data, backward=True):
    losses, _ = m(data)
    if backward:
        losses["total_loss"].backward()
    torch.cuda.synchronize()
    cls, reg = m.last_logits
    grads = {k: (None if p.grad is None else p.grad.detach().cpu().clone()) for k, p in m.named_parameters()}
    return {k: float(v) for k, v in losses.items()}, cls.detach().cpu().clone(), reg.detach().cpu().clone(), grads


def _oracle(g, sd, feat_training=False, conv_training=False, frozen_affine=False):
    """fp64 oracle of the composed model: the PointNet part and the FCN each with batch (training) or running statistics."""
    from oracle import det_ref
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    for k, v in sd64.items():
        if v.dtype.is_floating_point and "running" not in k:
            affine = (".1.weight" in k or ".1.bias" in k)
            if not (frozen_affine and affine):
                v.requires_grad_(True)
    data_np = golden_inputs(g)
    d64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in synth.to_torch(data_np).items()}
    rec = det_ref.BNState()
    pc = d64["point_cloud"][:, :3, :].contiguous()
    refs = [d64["center_ref%d" % i] for i in range(1, 6) if ("center_ref%d" % i) in d64]
    feats = det_ref.pointnet_feat(pc, refs, d64.get("one_hot"), sd64, tuple(g["meta_strides"]), feat_training, rec)
    x = det_ref.conv_feat_net(*feats, sd=sd64, training=conv_training, rec=rec)
    cls, reg = det_ref.heads(x, sd64)
    lo = det_ref.loss_tail(cls, reg, d64)
    lo["total_loss"].backward()
    grads = {k: v.grad for k, v in sd64.items() if v.grad is not None}
    return ({k: float(v) for k, v in lo.items()}, cls.detach(), reg.detach(), grads,
            det_ref.updated_running_stats(sd, rec) if rec.stats else {})


def _check_vs_oracle(got, ref, tag, guard=None, rel=TIGHT_REL):
    """Losses, logits and every gradient of `got` against the oracle `ref` at the bars of test_gradients_vs_fp64_oracle; with
    `guard` (the train()-mode result of the same model) the logits and every gradient tensor of the BatchNorm units (feat_net.*,
    conv_net.*) must also lie at least GUARD x their bar away from it.  (The heads' own parameters see the statistics only through
    the logits: refine_b4_n512's cls_out.bias gradient moves by 5 x its bar -- it is not a witness of the mode.)"""
    lo, cls, reg, grads = got
    rlo, rcls, rreg, rgrads = ref[:4]
    for k, v in rlo.items():
        assert abs(lo[k] - v) <= 1e-4 * max(1.0, abs(v)), (tag, k, lo[k], v)
    lbar = 1e-4 * max(1.0, float(rcls.abs().max()), float(rreg.abs().max()))
    dl = max(float((cls.double() - rcls).abs().max()), float((reg.double() - rreg).abs().max()))
    assert dl <= lbar, (tag, "logits", dl, lbar)
    gscale = max(float(v.abs().max()) for v in rgrads.values())
    worst, sep = 0.0, 0.0
    for k, r in rgrads.items():
        assert grads[k] is not None, (tag, k)
        bar = rel * float(r.abs().max()) + 2e-6 * gscale
        d = float((grads[k].double().view(r.shape) - r).abs().max())
        worst = max(worst, d / bar)
        assert d <= bar, (tag, k, d, bar)
        if guard is not None and guard[3][k] is not None and k.startswith(("feat_net.", "conv_net.")):
            gap = float((guard[3][k].double().view(r.shape) - grads[k].double().view(r.shape)).abs().max()) / bar
            assert gap >= GUARD, (tag, k, "frozen gradient too close to the batch-statistics one", gap)
            sep = gap if sep == 0.0 else min(sep, gap)
    print(tag, "worst gradient vs fp64 oracle: %.3f of its bar (relative bar %.0e)" % (worst, rel))
    if guard is not None:
        gl = max(float((guard[1] - cls).abs().max()), float((guard[2] - reg).abs().max()))
        print(tag, "train()-mode distance: logits %.1f x their bar, every gradient tensor at least %.1f x" % (gl / lbar, sep))
        assert gl >= GUARD * lbar, (tag, "frozen logits too close to the batch-statistics ones", gl, lbar)


@pytest.mark.parametrize("case", ["car_b4_n512", "people_b2_n512", "refine_b4_n512", "sunrgbd_b4_n1024"])
def test_frozen_model_matches_oracle(case):
    """The whole model frozen in train(): all losses, both logit tensors and every parameter gradient against the fp64 oracle with
    running statistics; running_mean / running_var / num_batches_tracked bit-unchanged by forward + backward."""
    from frustum_convnet_amd import precision
    g = load_golden(case)
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")
    ref = _oracle(g, sd)
    for prec in ("f32", "split"):
        with precision.precision(prec):
            m = _load(g, sd, "all", train=True)
            before = _bn_buffers(m)
            got = _run(m, data)
            after = _bn_buffers(m)
            for k, v in before.items():
                assert torch.equal(v, after[k]), ("a frozen forward wrote a running statistic", k)
            guard = _run(_load(g, sd, None, train=True), data)
            _check_vs_oracle(got, ref, case + " " + prec, guard)


@pytest.mark.parametrize("part", ["feat", "conv"])
def test_mixed_frozen_and_training_parts(part, exact_f32):
    """Frozen PointNet with a training ConvFeatNet and the reverse: gradients against the composed oracle, the training part's
    running statistics against det_ref.updated_running_stats, the frozen part's bit-unchanged."""
    g = load_golden("car_b4_n512")
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")
    m = _load(g, sd, part, train=True)
    before = _bn_buffers(m)
    got = _run(m, data)
    after = _bn_buffers(m)
    ref = _oracle(g, sd, feat_training=(part == "conv"), conv_training=(part == "feat"))
    upd = ref[4]
    frozen_prefix = "feat_net." if part == "feat" else "conv_net."
    nupd = 0
    for k, v in before.items():
        if k.startswith(frozen_prefix):
            assert torch.equal(v, after[k]), ("frozen part's statistic changed", k)
        elif "tracked" in k:
            assert int(after[k]) == int(v) + 1, k
        else:
            want = upd[k].float()
            assert torch.allclose(after[k].cpu(), want, rtol=1e-4, atol=1e-5), (k, float((after[k].cpu() - want).abs().max()))
            nupd += 1
    assert nupd > 10
    guard = _run(_load(g, sd, None, train=True), data)
    _check_vs_oracle(got, ref, "mixed-" + part, guard)


def test_frozen_modes_agree():
    """Frozen in eval() and in train() give bit-identical losses and gradients; a frozen forward under no_grad gives the eval
    inference logits bit for bit; a frozen forward with grad agrees with those to 1e-5 absolute (the same fold of the same running
    statistics: expected bit-identical -- the eval path may take the max-pool from keys where the graph-carrying one pools rows,
    which compares the same fp32 values)."""
    g = load_golden("car_b4_n512")
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")
    tr = _run(_load(g, sd, "all", train=True), data)
    ev = _run(_load(g, sd, "all", train=False), data)
    assert tr[0] == ev[0]
    for k, v in tr[3].items():
        assert v is not None and torch.equal(v, ev[3][k]), k
    plain = _load(g, sd, None, train=False)
    with torch.no_grad():
        inf = _run(plain, data, backward=False)
        fz = _run(_load(g, sd, "all", train=True), data, backward=False)
    assert torch.equal(fz[1], inf[1]) and torch.equal(fz[2], inf[2])
    d = max(float((tr[1] - inf[1]).abs().max()), float((tr[2] - inf[2]).abs().max()))
    print("frozen forward with grad vs eval inference logits: max abs %.3e (%s)" % (d, "bit-identical" if d == 0 else "not bit-identical"))
    assert d <= 1e-5, d


def test_frozen_backward_launch_structures_bit_identical():
    """Frozen gradients are bit-identical across every backward structure the training tests cover: one-, two- and three-stream
    weight gradients, partial_both 0 / 1 / 2, the rebuilt dy3, the shared backward stream on and off and the split backward."""
    g = load_golden("car_b4_n512")
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")
    settings = {
        "default": ({}, None, False, None, False),
        "one stream, 8 launches": ({"FCN_PN_MID": "0", "FCN_PN_TAIL": "0"}, (), False, None, False),
        "one stream, merged mid": ({"FCN_PN_MID": "1"}, (), False, None, False),
        "one stream, tail launch": ({"FCN_PN_MID": "0", "FCN_PN_TAIL": "1"}, (), False, None, False),
        "three streams": ({}, None, True, None, False),       # (not under the host emulation: its stream handles are NULL)
        "rebuilt dy3": ({"FCN_STORE_DY3": "0"}, None, False, None, False),
        "no shared backward stream": ({}, None, False, "off", False),
        "split backward": ({}, None, False, None, True),
    }
    keys = ("FCN_PN_MID", "FCN_PN_TAIL", "FCN_STORE_DY3")
    saved = {k: os.environ.get(k) for k in keys}
    grads = {}
    if os.environ.get("FCN_EMULATE", "0") == "1":
        settings.pop("three streams")
    try:
        for name, (env, side, three, share, split) in settings.items():
            for k in keys:
                os.environ.pop(k, None)
            os.environ.update(env)
            m = _load(g, sd, "all", train=True)
            fn = m.feat_net
            fn.set_wgrad_streams((fn.num_scales - 1,) if side is None else side, three=three)
            if share == "off":
                fn.bwd_share.clear()
            m.split_backward = split
            losses, _ = m(data)
            if split:
                m.backward_split(losses["total_loss"])
            else:
                m.backward(losses["total_loss"])
            torch.cuda.synchronize()
            grads[name] = {k: p.grad.detach().cpu().clone() for k, p in m.named_parameters() if p.grad is not None}
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    ref = grads["default"]
    assert len(ref) > 70
    for name, gr in grads.items():
        assert gr.keys() == ref.keys(), name
        for k in ref:
            assert torch.isfinite(gr[k]).all(), (name, k)
            assert torch.equal(gr[k], ref[k]), (name, k)


def test_frozen_key_pool_backward_with_zero_and_negative_gamma(exact_f32):
    """One scale in FCN_BN_FROZEN with seeded running statistics, BN3 with one channel at gamma = 0 (beta > 0: every row of a window
    ties, the first wins) and one at gamma < 0: the backward behind the key-pooled forward against the one behind the row pooling
    (every gradient to 1e-5 of its max), both against the fp64 oracle's running-statistics autograd of the pooled scale."""
    import gpu_stage_check as gsc
    from oracle import det_ref
    from frustum_convnet_amd import _native, pointnet_fused as pf

    B, N, stride, K, mlp, dist = gsc.CASES[4]
    dev = torch.device("cuda:0")
    pc, ref, sd, _ = gsc.make_case(B, N, stride, K, mlp, dist)
    sd["m.conv3.1.weight"][1] = -0.7
    sd["m.conv3.1.weight"][2] = 0.0
    sd["m.conv3.1.bias"][2] = 0.5
    gen = torch.Generator().manual_seed(3)
    rec = det_ref.BNState()
    with torch.no_grad():
        det_ref.pointnet_module(pc.double(), ref.double(), {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()},
                                "m", dist, K, True, rec)
    for prefix, (mean, var, _n) in rec.stats.items():
        sd[prefix + ".running_mean"] = (mean + 0.5 * var.sqrt() * torch.randn(mean.shape, generator=gen, dtype=torch.float64)).float()
        sd[prefix + ".running_var"] = (var * torch.exp(0.5 * torch.randn(var.shape, generator=gen, dtype=torch.float64))).clamp(0.3, 3.0).float()
    L = ref.shape[2]
    dfeat = torch.from_numpy(synth.normalish(3, 1, (B, L, mlp[2])).astype(np.float32)).contiguous()       # position-major
    names = ["dW1", "dg1", "db1", "dW2", "dg2", "db2", "dW3", "dg3", "db3"]
    out = {}
    old = os.environ.get("FCN_POOL_KEYS")
    try:
        for keys in ("1", "0"):
            os.environ["FCN_POOL_KEYS"] = keys
            sdg = {k: v.clone().to(dev) for k, v in sd.items()}
            plist = []
            for j in (1, 2, 3):
                plist += [sdg["m.conv%d.0.weight" % j], sdg["m.conv%d.1.weight" % j], sdg["m.conv%d.1.bias" % j]]
            bufs = ([sdg["m.conv%d.1.running_mean" % j] for j in (1, 2, 3)], [sdg["m.conv%d.1.running_var" % j] for j in (1, 2, 3)],
                    [sdg["m.conv%d.1.num_batches_tracked" % j] for j in (1, 2, 3)])
            before = [t.clone() for b in bufs for t in b]
            pool = pf.WorkspacePool()
            cfgt = (float(dist), int(K), _native.BN_FROZEN, 1e-5, 0.1, True, True)          # (.., need_grad, nlc)
            feat, idx, cnt, ws, desc, keep = pf._forward_impl(pool, cfgt, pc.to(dev), ref.to(dev), None, bufs, plist, True)
            assert (ws.pkey is not None) == (keys == "1")
            Wc, gs, bs = keep[0], keep[1], keep[2]
            dW = [torch.empty_like(w) for w in Wc]
            dg = [torch.empty_like(t) for t in gs]
            db = [torch.empty_like(t) for t in bs]
            params = pf._params_struct(Wc, gs, bs, [None] * 3, [None] * 3, [None] * 3)
            arr = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
            dfd = dfeat.to(dev)          # (kept alive across the call)
            rc = _native.lib().fcn_pn_backward(ctypes.byref(desc), ctypes.byref(params), dfd.data_ptr(), ctypes.byref(ws.c),
                                               arr(dW), arr(dg), arr(db), _native.current_stream(dev))
            assert rc == 0, rc
            torch.cuda.synchronize()
            for a, b in zip(before, [t for b in bufs for t in b]):
                assert torch.equal(a, b)
            out[keys] = ([t.detach().cpu().clone() for i in range(3) for t in (dW[i], dg[i], db[i])], feat.detach().cpu().clone())
    finally:
        if old is None:
            os.environ.pop("FCN_POOL_KEYS", None)
        else:
            os.environ["FCN_POOL_KEYS"] = old
    # fp64 oracle: the pooled scale with running statistics, position-major gradient
    sd64 = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
    leaves = []
    for j in (1, 2, 3):
        for nm in ("m.conv%d.0.weight", "m.conv%d.1.weight", "m.conv%d.1.bias"):
            sd64[nm % j].requires_grad_(True)
            leaves.append(sd64[nm % j])
    gd, _, _ = det_ref.pointnet_module(pc.double(), ref.double(), sd64, "m", dist, K, False)
    f = gd.max(dim=-1)[0]                                     # (B, C3, L)
    assert float((out["1"][1].double().permute(0, 2, 1) - f.detach()).abs().max()) <= 1e-4 * float(f.abs().max())
    (f * dfeat.double().permute(0, 2, 1)).sum().backward()
    errs = []
    for n, a, b, r in zip(names, out["1"][0], out["0"][0], leaves):
        assert torch.isfinite(a).all()
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-9, (n, float((a - b).abs().max()))
        rg = r.grad.view(-1)
        d = float((a.double().view(-1) - rg).abs().max())
        print("%s vs fp64 oracle: %.2e of its max" % (n, d / float(rg.abs().max())))
        errs.append((n, d, float(rg.abs().max())))
    for n, d, mx in errs:
        assert d <= 1e-4 * mx + 1e-7, (n, d, mx)
    assert abs(float(out["0"][0][7][2])) > 0                   # the gamma = 0 channel really has a d gamma


@pytest.mark.parametrize("scale,dist,K", [(3, 1.0, 64), (1, 0.25, 32)])
def test_frozen_dense_module_api_matches_oracle(scale, dist, K):
    """PointNetModule.freeze_bn() then .eval(): the reference-shaped (B, C3, L, nsample) forward carries its graph; output and all 9
    gradients against the oracle's pointnet_module(..., training=False) autograd at the bar of
    test_dense_module_api_matches_oracle, for a wide scale and a narrow one; the running statistics are not written."""
    from oracle import det_ref
    g = load_golden("car_b4_n512")
    data_np = golden_inputs(g)
    sd = _running_stats(g)
    m = _load(g, sd, None, train=False)
    net = getattr(m.feat_net, "pointnet%d" % scale).freeze_bn()
    assert net.bn_frozen and "bn_frozen" not in str(list(net.state_dict().keys()))
    pc = torch.from_numpy(data_np["point_cloud"][:, :3, :].copy()).cuda().contiguous()
    ref = torch.from_numpy(data_np["center_ref%d" % scale]).cuda()
    before = _bn_buffers(m)
    out = net(pc, None, ref)
    assert out.grad_fn is not None
    with torch.no_grad():
        out0 = net(pc, None, ref)
    assert out0.grad_fn is None and torch.equal(out.detach(), out0)
    prefix = "feat_net.pointnet%d" % scale
    sdg = {k: (v.double().requires_grad_(True) if k.startswith(prefix) and v.dtype.is_floating_point and "running" not in k
               else (v.double() if v.dtype.is_floating_point else v)) for k, v in sd.items()}
    exp, _, _ = det_ref.pointnet_module(torch.from_numpy(data_np["point_cloud"][:, :3, :].copy()).double(),
                                        torch.from_numpy(data_np["center_ref%d" % scale]).double(), sdg, prefix, dist, K, False)
    assert out.shape == exp.shape
    assert float((out.detach().cpu().double() - exp.detach()).abs().max()) < 2e-4
    gen = torch.Generator().manual_seed(17)
    dout = torch.randn(exp.shape, generator=gen, dtype=torch.float64) * (torch.rand(exp.shape, generator=gen) < 0.5).double()
    (exp * dout).sum().backward()
    (out * dout.float().cuda()).sum().backward()
    torch.cuda.synchronize()
    for j in (1, 2, 3):
        conv = getattr(net, "conv%d" % j)
        for name, got in (("%s.conv%d.0.weight" % (prefix, j), conv[0].weight.grad), ("%s.conv%d.1.weight" % (prefix, j), conv[1].weight.grad),
                          ("%s.conv%d.1.bias" % (prefix, j), conv[1].bias.grad)):
            want = sdg[name].grad
            err = float((got.cpu().double().view(want.shape) - want).abs().max())
            assert err <= 1e-3 * float(want.abs().max()) + 1e-6, (name, err, float(want.abs().max()))
    after = _bn_buffers(m)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    # the default keeps refusing eval() + grad without freeze_bn
    net.freeze_bn(False)
    with pytest.raises(NotImplementedError, match="eval mode"):
        net(pc, None, ref)


def test_frozen_affine_parameters_get_no_gradient(exact_f32):
    """torchvision's FrozenBatchNorm: gamma / beta with requires_grad=False under freeze_bn.  The conv weights (and heads) get the
    oracle's gradients, the affine parameters get None, the running statistics stay."""
    g = load_golden("car_b4_n512")
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")
    m = _load(g, sd, "all", train=True)
    affine = [k for k, _ in m.named_parameters() if ".1.weight" in k or ".1.bias" in k]
    assert len(affine) > 40
    for k, p in m.named_parameters():
        if k in affine:
            p.requires_grad_(False)
    before = _bn_buffers(m)
    got = _run(m, data)
    for k in affine:
        assert got[3][k] is None, k
    after = _bn_buffers(m)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    ref = _oracle(g, sd, frozen_affine=True)
    assert not any(k in ref[3] for k in affine)
    guard = _run(_load(g, sd, None, train=True), data)
    _check_vs_oracle(got, ref, "frozen-affine", guard)


def test_frozen_step_loop_eager_equals_one_hipgraph():
    """FlatTrainState + Adam in frozen mode: three steps eager and the same three steps captured in one torch.cuda.graph (warm-up
    forward outside): the parameters agree bit for bit -- frozen statistics never move, so the warm-up changes nothing -- and the
    running statistics are untouched."""
    from frustum_convnet_amd.train_state import FlatTrainState
    g = load_golden("car_b4_n512")
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")

    def make():
        m = _load(g, sd, "all", train=True)
        return m, FlatTrainState(m, lr=1e-4, weight_decay=1e-4)

    m1, s1 = make()
    eager = []
    for _ in range(3):
        lo, _ = m1(data)
        eager.append(float(lo["total_loss"]))
        lo["total_loss"].backward()
        s1.step()
    m2, s2 = make()
    before = _bn_buffers(m2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lo, _ = m2(data)
        lo["total_loss"].backward()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lo, _ = m2(data)
        lo["total_loss"].backward()
        s2.adam_step()
    losses = []
    for _ in range(3):
        graph.replay()
        losses.append(float(lo["total_loss"]))
    torch.cuda.synchronize()
    assert int(s2.step_count) == 3
    assert losses == eager, (losses, eager)
    assert torch.equal(s1.flat, s2.flat)
    after = _bn_buffers(m2)
    for k, v in before.items():
        assert torch.equal(v, after[k]), k
    # the loss trajectory against the fp64 oracle stepped by torch.optim.Adam on its own running-statistics gradients (rel 1e-3,
    # as test_gpu_train_state.test_two_step_trajectory_vs_cpu_oracle holds the training loop at this learning rate)
    from oracle import det_ref
    f64 = lambda v: v.double() if v.dtype.is_floating_point else v
    sd64 = {k: f64(v.clone()) for k, v in sd.items()}
    leaves = [v.requires_grad_(True) for k, v in sd64.items() if v.dtype.is_floating_point and "running" not in k]
    opt = torch.optim.Adam(leaves, lr=1e-4, weight_decay=1e-4)
    d64 = {k: f64(v) for k, v in synth.to_torch(golden_inputs(g)).items()}
    ref = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        _, _, lo = det_ref.forward(sd64, d64, tuple(g["meta_strides"]), training=False)
        ref.append(float(lo["total_loss"]))
        lo["total_loss"].backward()
        opt.step()
    print("frozen trajectory: fp64 oracle", ref, "hip", eager)
    for r, h in zip(ref, eager):
        assert abs(r - h) <= 1e-3 * abs(r), (ref, eager)


def test_frozen_full_size_step():
    """The bench shape (car_b32_n1024: the max-pool keys are picked by size, not forced): a frozen forward with grad gives the eval
    inference logits (1e-5 absolute), forward + backward write no running statistic, and the gradients agree with those of the
    row-pooled forward (FCN_POOL_KEYS=0) to 1e-5 of each tensor's max."""
    g = load_golden("car_b32_n1024")
    data = synth.to_torch(golden_inputs(g), "cuda")
    sd = golden_state_dict(g)
    gen = torch.Generator().manual_seed(5)
    for k in list(sd):
        if k.endswith("running_var"):
            sd[k] = (0.3 + 2.7 * torch.rand(sd[k].shape, generator=gen)).float()
        elif k.endswith("running_mean"):
            sd[k] = (0.5 * torch.randn(sd[k].shape, generator=gen)).float()
    with torch.no_grad():
        inf = _run(_load(g, sd, None, train=False), data, backward=False)
    res = {}
    old = os.environ.get("FCN_POOL_KEYS")
    try:
        for keys in (None, "0"):
            os.environ.pop("FCN_POOL_KEYS", None)
            if keys is not None:
                os.environ["FCN_POOL_KEYS"] = keys
            m = _load(g, sd, "all", train=True)
            before = _bn_buffers(m)
            res[keys] = _run(m, data)
            after = _bn_buffers(m)
            for k, v in before.items():
                assert torch.equal(v, after[k]), k
    finally:
        os.environ.pop("FCN_POOL_KEYS", None)
        if old is not None:
            os.environ["FCN_POOL_KEYS"] = old
    d = max(float((res[None][1] - inf[1]).abs().max()), float((res[None][2] - inf[2]).abs().max()))
    assert d <= 1e-5, d
    for k, a in res[None][3].items():
        b = res["0"][3][k]
        assert torch.isfinite(a).all(), k
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-9, (k, float((a - b).abs().max()))


def test_frozen_with_batch_statistics_matches_oracle():
    """Running statistics equal to the batch statistics of the fixture's batch (kept off the ReLU kinks, _clear_kinks): the frozen
    forward is then the training forward up to those shifts, and the frozen gradients -- without the batch-mean terms -- are held to
    the fp64 oracle at the tight bars in both operand modes, every gradient tensor at least GUARD x its bar away from the training
    step's."""
    from frustum_convnet_amd import precision
    g = load_golden("car_b4_n512")
    sd = _running_stats(g, spread=0.0)
    data = synth.to_torch(golden_inputs(g), "cuda")
    ref = _oracle(g, sd)
    for prec in ("split", "f32"):
        with precision.precision(prec):
            got = _run(_load(g, sd, "all", train=True), data)
            tr = _run(_load(g, sd, None, train=True), data)
            _check_vs_oracle(got, ref, "batch-statistics " + prec)
            for k, r in ref[3].items():
                if not k.startswith(("feat_net.", "conv_net.")):
                    continue
                gscale = max(float(v.abs().max()) for v in ref[3].values())
                bar = TIGHT_REL * float(r.abs().max()) + 2e-6 * gscale
                gap = float((tr[3][k].double().view(r.shape) - got[3][k].double().view(r.shape)).abs().max()) / bar
                assert gap >= GUARD, (prec, k, gap)


def test_c_abi_bn_modes():
    """FCN_BN_FROZEN (2) is accepted by every forward and backward entry and writes no running statistic; FCN_BN_RUNNING (0) still
    makes every backward return FCN_E_BADARG; an unknown mode (3) is FCN_E_BADARG at the forward entries."""
    from frustum_convnet_amd import _native, pointnet_fused as pf, fcn_fused
    E_BADARG = 10001                  # FCN_E_BADARG
    g = load_golden("car_b4_n512")
    sd = _running_stats(g)
    data = synth.to_torch(golden_inputs(g), "cuda")
    m = _load(g, sd, "all", train=True)
    lib = _native.lib()
    net = m.feat_net.pointnet2
    params, bufs = net._param_pack()
    pc = data["point_cloud"][:, :3, :].contiguous()
    ref = data["center_ref2"]
    before = [t.clone() for b in bufs for t in b]
    # PointNet scale: the fused front + forward + every backward entry in FCN_BN_FROZEN
    entries = ("fcn_pn_backward", "fcn_pn_backward2", "fcn_pn_backward3")
    if os.environ.get("FCN_EMULATE", "0") == "1":
        entries = entries[:2]          # (fcn_pn_backward3 needs real streams: the host emulation's handles are NULL)
    for entry in entries:
        h = pf.prepare_pooled(net._pool, net.dist, net.nsample, _native.BN_FROZEN, 1e-5, 0.1, pc, ref, None, bufs, params, nlc=True)
        assert h["desc"].training == _native.BN_FROZEN
        pf.group_compact([h], pc)
        feat, _, cnt, ws, desc, keep = pf._run_forward(h, h["ws"].cnt, pf._empty_idx(pc.device))
        Wc, gs, bs = keep[0], keep[1], keep[2]
        dW = [torch.empty_like(w) for w in Wc]
        dg = [torch.empty_like(t) for t in gs]
        db = [torch.empty_like(t) for t in bs]
        P = pf._params_struct(Wc, gs, bs, [None] * 3, [None] * 3, [None] * 3)
        arr = lambda ts: (ctypes.c_void_p * 3)(*[t.data_ptr() for t in ts])
        dfeat = torch.ones_like(feat)
        st = _native.current_stream(pc.device)
        if entry == "fcn_pn_backward":
            rc = lib.fcn_pn_backward(ctypes.byref(desc), ctypes.byref(P), dfeat.data_ptr(), ctypes.byref(ws.c), arr(dW), arr(dg), arr(db), st)
        elif entry == "fcn_pn_backward2":
            rc = lib.fcn_pn_backward2(ctypes.byref(desc), ctypes.byref(P), dfeat.data_ptr(), ctypes.byref(ws.c), arr(dW), arr(dg), arr(db),
                                      st, None, None)
        else:
            side, _evs, evarr, side3 = net._pool.side_stream(pc.device)
            rc = lib.fcn_pn_backward3(ctypes.byref(desc), ctypes.byref(P), dfeat.data_ptr(), ctypes.byref(ws.c), arr(dW), arr(dg), arr(db),
                                      st, ctypes.c_void_p(side.cuda_stream), ctypes.c_void_p(side3.cuda_stream), evarr)
        assert rc == 0, (entry, rc)
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in dW + dg + db), entry
        # the same descriptor in FCN_BN_RUNNING / an unknown mode: refused before anything is launched
        for bad in (_native.BN_RUNNING, 3):
            desc.training = bad
            rc = lib.fcn_pn_backward(ctypes.byref(desc), ctypes.byref(P), dfeat.data_ptr(), ctypes.byref(ws.c), arr(dW), arr(dg), arr(db), st)
            assert rc == E_BADARG, (bad, rc)
        desc.training = 3
        rc = lib.fcn_pn_forward(ctypes.byref(desc), ctypes.byref(h["params"]), ws.cnt.data_ptr(), None, ctypes.byref(ws.c),
                                feat.data_ptr(), st)
        assert rc == E_BADARG, rc
        net._pool.release(ws)
    h = pf.prepare_pooled(net._pool, net.dist, net.nsample, _native.BN_FROZEN, 1e-5, 0.1, pc, ref, None, bufs, params, nlc=True)
    h["desc"].training = 3
    with pytest.raises(_native.NativeError):
        pf.group_compact([h], pc)
    net._pool.release(h["ws"])
    torch.cuda.synchronize()
    for a, b in zip(before, [t for b in bufs for t in b]):
        assert torch.equal(a, b)
    # ConvFeatNet: fcn_convnet_pack / _forward / _backward in FCN_BN_FROZEN through the model; mode 0 / 3 refused
    cbefore = {k: v.clone() for k, v in m.conv_net.state_dict().items() if "running" in k or "tracked" in k}
    lo, _ = m(data)
    lo["total_loss"].backward()
    torch.cuda.synchronize()
    for k, v in m.conv_net.state_dict().items():
        if k in cbefore:
            assert torch.equal(cbefore[k], v), k
    pt, cbufs, bn0 = fcn_fused._gather(m.conv_net, m.cls_out, m.reg_out)
    Ls = [data["center_ref%d" % i].shape[2] for i in range(1, 5)]
    pre = fcn_fused._prepare(m._cn_pool, (3, 1e-5, 0.1, True), cbufs, data["one_hot"], pc.shape[0], Ls, pc.device, pt)
    assert pre["desc"].training == 3
    rc = lib.fcn_convnet_pack(ctypes.byref(pre["desc"]), ctypes.byref(pre["params"]), ctypes.byref(pre["ws"].c),
                              data["one_hot"].data_ptr(), _native.current_stream(pc.device))
    assert rc == E_BADARG, rc
    feats = [torch.zeros((pc.shape[0], Ls[s], c), device=pc.device) for s, c in enumerate((128, 128, 256, 512))]
    fp = fcn_fused._arr(feats, _native.CN_MAXLEV)
    logits = torch.empty((pc.shape[0] * Ls[1], 64), device=pc.device)
    rc = lib.fcn_convnet_forward(ctypes.byref(pre["desc"]), ctypes.byref(pre["params"]), ctypes.byref(pre["ws"].c), fp,
                                 data["one_hot"].data_ptr(), logits.data_ptr(), _native.current_stream(pc.device))
    assert rc == E_BADARG, rc
    z = lambda: fcn_fused._arr([], _native.CN_MAXLAYER)
    for bad in (_native.BN_RUNNING, 3):
        pre["desc"].training = bad
        rc = lib.fcn_convnet_backward(ctypes.byref(pre["desc"]), ctypes.byref(pre["params"]), ctypes.byref(pre["ws"].c), fp,
                                      data["one_hot"].data_ptr(), logits.data_ptr(), fcn_fused._arr(feats, _native.CN_MAXLEV),
                                      z(), z(), z(), logits.data_ptr(), _native.current_stream(pc.device), None, None)
        assert rc == E_BADARG, (bad, rc)
    m._cn_pool.release(pre["ws"])


def test_feat_scales_must_agree_on_freeze():
    """PointNetFeat refuses scales that disagree on freeze_bn (the fused front takes one mode for all of them); the flag is module
    state, not part of the state_dict, and freeze_bn returns the module like .train() does."""
    g = load_golden("car_b4_n512")
    m = _model(g)
    assert m.freeze_bn() is m and m.feat_net.bn_frozen and m.conv_net.bn_frozen
    assert list(m.state_dict().keys()) == list(golden_state_dict(g).keys())
    assert m.freeze_bn(False) is m and not m.feat_net.bn_frozen and not m.conv_net.bn_frozen
    m.feat_net.pointnet2.freeze_bn()
    data = synth.to_torch(golden_inputs(g), "cuda")
    with pytest.raises(ValueError, match="disagree"):
        m(data)
