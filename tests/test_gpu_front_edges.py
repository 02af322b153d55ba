"""-m gpu: the fused PointNet front (fcn_pn_group_compact2: gc_hits_kernel, gc_entries_kernel, gc_fold_kernel) OFF the workload
shapes and AT its limits: the global-memory z row (N > 8192), more than one window per thread in the offset scan (L > 1024),
the tile-list loop carried over several rounds (B > 1024), per-frustum moments that do / do not fit the dead LDS area, 16-bit
hit indices above 32767, one and eight scales, K = 1 / 1024, L = 1, N < 64, windows all empty / all saturated, a frustum whose
row count is an exact multiple of the tile rows, BN1 from the running statistics, the phased front, the largest L the launch
admits -- and every refusal of the host check.

Inputs are built here (not by synth.make_batch); the reference is the ORACLE's grouping (oracle/grouping.py) -> the entry-space
restatement (tests/entry_ref.compact) -> moments and BN1 fold in extended / double precision numpy.  Nothing of the reference is
derived from the code under test.  Every case asserts ON THE REFERENCE that the regime it is named after is really present, so a
changed seed cannot turn it into a fixture-like case.  The cases also run on the host emulation (tests/test_emu_gpu_subset.py);
the arrival counter, the write-through stores and the "last frustum finalises" section only exist on the hardware."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import entry_ref
from gpu_stage_check import check as stage_check
from oracle import grouping

pytestmark = pytest.mark.gpu

SENT = -1515870811                  # 0xA5A5A5A5 as int32: no count, offset, window id or tile id is negative
MLP = (64, 64, 128)
EPS, MOMENTUM = 1e-5, 0.1
BN_RUNNING, BN_TRAIN, BN_FROZEN = 0, 1, 2
FCN_E_BADARG, FCN_E_LIMIT = 10001, 10002
# static __shared__ of gc_entries_kernel (csrc/group_compact.hip): wsum[16] ints, red[16][10] doubles, last_s, carry_s
GE_STATIC_LDS = 1360               # 16 * 4 + 16 * 10 * 8 + 2 * 4 = 1352 bytes of objects; 1360 (.group_segment_fixed_size) with alignment
GC_WPB, GE_T, GC_LDS_MAX_PTS = 16, 1024, 8192


# ---------------------------------------------------------------------------------------------------------------- inputs
def _cloud(rng, B, N, span):
    pc = np.empty((B, 3, N), np.float32)
    pc[:, :2] = rng.uniform(-1.0, 1.0, (B, 2, N))
    pc[:, 2] = rng.uniform(0.0, span, (B, N))
    return pc


def _centres(rng, B, L, span):
    """z on a linspace over the span plus a small per-frustum offset; x, y small."""
    ref = np.empty((B, 3, L), np.float32)
    ref[:, :2] = rng.uniform(-0.2, 0.2, (B, 2, L))
    ref[:, 2] = np.linspace(0.0, span, L, dtype=np.float64)[None, :] + rng.uniform(-0.05, 0.05, (B, 1))
    return ref


def _random_case(seed, B, N, span, scales):
    rng = np.random.default_rng(seed)
    pc = _cloud(rng, B, N, span)
    return pc, [_centres(rng, B, L, span) for (L, K, dis) in scales]


def _fits(B, L):
    """gc_entries_kernel: the B x 12 per-frustum moments fit the dead LDS area of (20 L + 4) bytes"""
    return 12 * B <= (20 * L + 4) // 8


# Every case: dict(B, N, scales [(L, K, dis_z)], pc, refs, mlp, mode, feat (scale indices whose pooled features are compared),
# claims (per scale: regimes the reference must show: "empty", "partial", "saturated", "all_empty", "all_saturated"),
# extra(case, refs_out) further assertions on the reference)
def _case_nolds():
    scales = [(20, 16, 0.3), (5, 64, 1.0)]
    pc, refs = _random_case(101, 1, GC_LDS_MAX_PTS + 1, 300.0, scales)
    # the LAST points of the row are the only hits of the last window of scale 0 (centre outside the span)
    refs[0][0, 2, -1] = 400.0
    pc[0, 2, [GC_LDS_MAX_PTS - 2, GC_LDS_MAX_PTS]] = (400.1, 399.9)

    def extra(case, out):
        assert case["N"] > GC_LDS_MAX_PTS
        assert out[0]["idx"][0, -1, :2].tolist() == [GC_LDS_MAX_PTS - 2, GC_LDS_MAX_PTS] and int(out[0]["cnt"][0, -1]) == 2
    return dict(B=1, N=GC_LDS_MAX_PTS + 1, scales=scales, pc=pc, refs=refs, feat=(0, 1), extra=extra,
                claims=[("partial", "saturated"), ("partial",)])


def _case_lds_edge():
    scales = [(20, 16, 0.3)]
    pc, refs = _random_case(102, 1, GC_LDS_MAX_PTS, 300.0, scales)
    refs[0][0, 2, -1] = 400.0
    pc[0, 2, [GC_LDS_MAX_PTS - 3, GC_LDS_MAX_PTS - 1]] = (400.1, 399.9)

    def extra(case, out):
        assert case["N"] == GC_LDS_MAX_PTS
        assert out[0]["idx"][0, -1, :2].tolist() == [GC_LDS_MAX_PTS - 3, GC_LDS_MAX_PTS - 1] and int(out[0]["cnt"][0, -1]) == 2
    return dict(B=1, N=GC_LDS_MAX_PTS, scales=scales, pc=pc, refs=refs, extra=extra, claims=[("partial", "saturated")])


def _case_big_l():
    scales = [(1500, 4, 0.02), (1025, 2, 0.001), (2049, 1, 0.01)]
    pc, refs = _random_case(103, 1, 300, 10.0, scales)
    refs[1][0, 2, 1024] = pc[0, 2, 7]                               # the one window of scale 1 past the first 1024 is live

    def extra(case, out):
        assert [-(-L // GE_T) for (L, K, dis) in case["scales"]] == [2, 2, 3]        # windows per thread of the offset scan
        for o, (L, K, dis) in zip(out, case["scales"]):
            assert int((o["cnt"] == 0).sum()) > L // 4                                # many empty windows
            assert int((o["cnt"][0, GE_T:] > 0).sum()) > 0                            # and live ones past the first 1024
    return dict(B=1, N=300, scales=scales, pc=pc, refs=refs, feat=(0,), extra=extra,
                claims=[("empty", "partial", "saturated"), ("empty", "partial"), ("empty", "saturated")])


def _case_big_b():
    scales = [(3, 4, 2.0), (7, 2, 0.5)]
    pc, refs = _random_case(104, 1030, 40, 20.0, scales)

    def extra(case, out):
        assert case["B"] > GE_T and case["N"] < 64
        assert all(not _fits(case["B"], L) for (L, K, dis) in case["scales"])
    return dict(B=1030, N=40, scales=scales, pc=pc, refs=refs, extra=extra,
                claims=[("partial", "saturated"), ("empty", "partial", "saturated")])


def _case_fits():
    # (64, 2, 0.3) fits; for B = 2 the smallest L that fits is 10 (24 doubles <= (20 L + 4) / 8) and L = 9 does not
    scales = [(64, 2, 0.3), (10, 2, 0.3), (9, 2, 0.3)]
    pc, refs = _random_case(105, 2, 64, 10.0, scales)

    def extra(case, out):
        assert [_fits(2, L) for (L, K, dis) in case["scales"]] == [True, True, False]
    return dict(B=2, N=64, scales=scales, pc=pc, refs=refs, extra=extra, claims=[("empty", "partial", "saturated"), (), ()])


def _case_idx16():
    N, dis = 65535, 1.0
    rng = np.random.default_rng(106)
    pc = _cloud(rng, 1, N, 1.0)
    pc[0, 2] += 500.0                                               # nobody near a window ...
    ref = _centres(rng, 1, 4, 1.0)
    ref[0, 2] = (10.0, 20.0, 30.0, 40.0)
    w0 = [5, 100, 32767, 32768, 40000, 65533, 65534]                # ... but these: 7 < K hits, all kept
    pc[0, 2, w0] = 10.0 + rng.uniform(-0.5, 0.5, len(w0))
    w2 = list(range(60000, 60020))                                  # saturated: the first 8 of 20, all above 32767
    pc[0, 2, w2] = 30.0 + rng.uniform(-0.5, 0.5, len(w2))
    w3 = [1, 65532]
    pc[0, 2, w3] = (40.25, 39.75)

    def extra(case, out):
        idx, cnt = out[0]["idx"], out[0]["cnt"]
        assert cnt[0].tolist() == [7, 0, 8, 2]
        assert idx[0, 0, :7].tolist() == w0 and idx[0, 2].tolist() == w2[:8] and idx[0, 3, :2].tolist() == w3
    return dict(B=1, N=N, scales=[(4, 8, dis)], pc=pc.astype(np.float32), refs=[ref], extra=extra,
                claims=[("empty", "partial", "saturated")])


def _case_one_a():
    pc, refs = _random_case(107, 1, 1, 1.0, [(1, 1, 0.5)])
    refs[0][0, 2, 0] = pc[0, 2, 0] + np.float32(0.1)
    return dict(B=1, N=1, scales=[(1, 1, 0.5)], pc=pc, refs=refs, claims=[("all_saturated",)])


def _case_one_b():
    pc, refs = _random_case(108, 2, 1, 1.0, [(1, 2, 100.0)])

    def extra(case, out):
        assert out[0]["c"]["ent"][:, 0, 3].tolist() == [2.0, 2.0]            # one hit, padding weight K
    return dict(B=2, N=1, scales=[(1, 2, 100.0)], pc=pc, refs=refs, extra=extra, claims=[("partial",)])


def _case_k_max():
    scales = [(2, 1024, 100.0), (17, 1, 0.2)]
    pc, refs = _random_case(109, 1, 1500, 10.0, scales)
    return dict(B=1, N=1500, scales=scales, pc=pc, refs=refs, claims=[("all_saturated",), ("all_saturated",)])


def _case_eight():
    scales = [(5 + i, 4 + i, 0.3 + 0.1 * i) for i in range(8)]
    pc, refs = _random_case(110, 2, 100, 20.0, scales)

    def extra(case, out):
        assert all(L % GC_WPB for (L, K, dis) in case["scales"])
        cnt = np.concatenate([(o["cnt"] - K).ravel() for o, (L, K, dis) in zip(out, case["scales"])])
        assert (cnt < 0).any() and (cnt == 0).any()                           # partial and saturated windows among the scales
    return dict(B=2, N=100, scales=scales, pc=pc, refs=refs, feat=(0, 7), extra=extra, claims=[()] * 8)


def _case_single():
    scales = [(33, 8, 0.4)]
    pc, refs = _random_case(111, 3, 129, 10.0, scales)
    return dict(B=3, N=129, scales=scales, pc=pc, refs=refs, mlp=(128, 128, 256), claims=[("partial", "saturated")])


def _case_all_empty():
    scales = [(9, 4, 1e-6)]
    pc, refs = _random_case(112, 2, 70, 10.0, scales)
    refs[0][:, 2] += 110.0                                          # far from every point

    def extra(case, out):
        c = out[0]["c"]
        assert c["nent"].tolist() == [9, 9] and bool((c["ent"][:, :9, 3] == 4.0).all())      # point 0, weight K
    return dict(B=2, N=70, scales=scales, pc=pc, refs=refs, extra=extra, claims=[("all_empty",)])


def _case_tile_edge():
    """Clusters of known size: 16 windows with rows / 16 points each (scale 0: nent == rows exactly, one live tile of two) and one
    more point that only the wider dis_z of scale 1 catches (nent == rows + 1: two live tiles)."""
    rows = _rows()
    assert rows % 16 == 0 and rows + 1 <= 256
    per, N, L = rows // 16, 256, 16
    rng = np.random.default_rng(113)
    pc = _cloud(rng, 1, N, 1.0)
    pc[0, 2] += 1000.0
    order = rng.permutation(N)
    for l in range(L):
        pc[0, 2, order[l * per:(l + 1) * per]] = 10.0 * l + rng.uniform(-0.1, 0.1, per)
    pc[0, 2, order[rows]] = 0.5
    refs = []
    for s in range(2):
        ref = _centres(rng, 1, L, 1.0)
        ref[0, 2] = 10.0 * np.arange(L)
        refs.append(ref)
    K = 2 * per

    def extra(case, out):
        assert [int(o["c"]["nent"][0]) for o in out] == [rows, rows + 1]
        assert -(-L * K // rows) == 2                                         # tile slots per frustum
    return dict(B=1, N=N, scales=[(L, K, 0.3), (L, K, 0.8)], pc=pc.astype(np.float32), refs=refs, extra=extra,
                claims=[("partial",), ("partial",)])


def _case_running(mode):
    scales = [(35, 8, 0.5)]
    pc, refs = _random_case(114, 2, 130, 10.0, scales)
    return dict(B=2, N=130, scales=scales, pc=pc, refs=refs, mode=mode, claims=[("partial", "saturated")])


def _case_max_l(L):
    scales = [(L, 1, 0.002)]
    pc, refs = _random_case(115, 1, 64, 10.0, scales)
    return dict(B=1, N=64, scales=scales, pc=pc, refs=refs, claims=[("empty", "saturated")])


CASES = {
    "nolds": _case_nolds, "lds_edge": _case_lds_edge, "big_l": _case_big_l, "big_b": _case_big_b, "fits": _case_fits,
    "idx16": _case_idx16, "one_a": _case_one_a, "one_b": _case_one_b, "k_max": _case_k_max, "eight": _case_eight,
    "single": _case_single, "all_empty": _case_all_empty, "tile_edge": _case_tile_edge,
    "running": lambda: _case_running(BN_RUNNING), "frozen": lambda: _case_running(BN_FROZEN),
}


# ------------------------------------------------------------------------------------------------------------- reference
def _rows():
    from frustum_convnet_amd import _native
    return int(_native.lib().fcn_pn_wgrad_rows())


def _moments(c):
    """The 10 weighted input moments of the reference entries (sum w, w u [3], w u u^T [6]) in extended precision, the sum of
    the terms' magnitudes and the entry count.  (u, w are fp32: every product is exact in a 64-bit significand.)"""
    e = entry_ref._flat(c, c["ent"]).numpy().astype(np.longdouble)
    w, x, y, z = e[:, 3], e[:, 0], e[:, 1], e[:, 2]
    terms = np.stack([w, w * x, w * y, w * z, w * x * x, w * x * y, w * x * z, w * y * y, w * y * z, w * z * z], 1)
    return terms.sum(0), np.abs(terms).sum(0), e.shape[0]


def _fold(mean, var, gamma, beta):
    rstd = 1.0 / np.sqrt(var + EPS)
    sc = gamma.astype(np.float64) * rstd
    return np.concatenate([sc, beta.astype(np.float64) - mean * sc, mean, rstd])


def _batch_mean_var(mom, M, W1):
    mo = mom.astype(np.float64) / M
    mu = mo[1:4]
    m2 = np.array([[mo[4], mo[5], mo[6]], [mo[5], mo[7], mo[8]], [mo[6], mo[8], mo[9]]])
    cov = m2 - mu[:, None] * mu[None, :]
    W = W1.astype(np.float64)
    return W @ mu, np.maximum(((W @ cov) * W).sum(1), 0.0)


def _reference(case):
    out = []
    pc_t = torch.from_numpy(case["pc"])
    for (L, K, dis), ref in zip(case["scales"], case["refs"]):
        assert ref.shape == (case["B"], 3, L) and case["pc"].shape == (case["B"], 3, case["N"])
        idx, cnt = grouping.query_depth_point(float(np.float32(dis)), K, case["pc"], ref)
        c = entry_ref.compact(torch.from_numpy(idx), torch.from_numpy(cnt), pc_t, torch.from_numpy(ref), K)
        out.append(dict(idx=idx, cnt=cnt, c=c))
    return out


def _assert_claims(case, out):
    for s, ((L, K, dis), o, claims) in enumerate(zip(case["scales"], out, case["claims"])):
        cnt = o["cnt"]
        have = {"empty": (cnt == 0).any(), "partial": ((cnt > 0) & (cnt < K)).any(), "saturated": (cnt == K).any(),
                "all_empty": (cnt == 0).all(), "all_saturated": (cnt == K).all()}
        for name in claims:
            assert have[name], (s, name, np.bincount(cnt.ravel(), minlength=K + 1).tolist())
    if case.get("extra"):
        case["extra"](case, out)


@functools.lru_cache(maxsize=None)
def _built(name):
    """A case and its reference, computed once and shared (read-only) by the tests that use it."""
    case = CASES[name]() if name in CASES else _case_max_l(int(name[6:]))
    out = _reference(case)
    _assert_claims(case, out)
    return case, out


# ---------------------------------------------------------------------------------------------------------------- device
def _params(C, seed, mode):
    g = torch.Generator().manual_seed(seed)
    W = [torch.randn(C[0], 3, generator=g) * 0.5, torch.randn(C[1], C[0], generator=g) * 0.1, torch.randn(C[2], C[1], generator=g) * 0.1]
    gam = [torch.rand(c, generator=g) + 0.5 for c in C]
    bet = [torch.randn(c, generator=g) * 0.1 for c in C]
    if mode == BN_TRAIN:
        rm, rv = [torch.zeros(c) for c in C], [torch.ones(c) for c in C]
    else:                                                           # non-trivial running statistics
        rm, rv = [torch.randn(c, generator=g) * 0.3 for c in C], [torch.rand(c, generator=g) + 0.25 for c in C]
    host = dict(W=W, gamma=gam, beta=bet, rmean=rm, rvar=rv)
    plist = []
    for i in range(3):
        plist += [W[i].cuda(), gam[i].cuda(), bet[i].cuda()]
    bufs = ([t.cuda() for t in rm], [t.cuda() for t in rv], [torch.zeros((), dtype=torch.int64).cuda() for c in C])
    return plist, bufs, host


def _poison(ws):
    for t in (ws.cnt, ws.woff, ws.ewin):
        t.fill_(SENT)
    ws.ent.fill_(float("nan"))
    ws.tiles[4:].fill_(SENT)


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else (t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t)


def _snapshot(ws, C1):
    return [_bits(t).cpu().clone() for t in (ws.cnt, ws.woff, ws.ent, ws.ewin, ws.tiles, ws.stat[:10], ws.bn[:4 * C1], ws.gmom)]


def _acquire_all(pf, case, pc, seed0):
    mode, mlp = case.get("mode", BN_TRAIN), case.get("mlp", MLP)
    handles, hosts = [], []
    for s, ((L, K, dis), ref) in enumerate(zip(case["scales"], case["refs"])):
        plist, bufs, host = _params(mlp, seed0 + s, mode)
        cfgt = (float(dis), K, mode, EPS, MOMENTUM, False, True)
        handles.append(pf._acquire(pf.WorkspacePool(), cfgt, pc, torch.from_numpy(ref).cuda(), None, bufs, plist, False))
        hosts.append((plist, bufs, host))
    return handles, hosts


def _run_front_case(name):
    from frustum_convnet_amd import pointnet_fused as pf
    case, out = _built(name)
    B, mode, mlp = case["B"], case.get("mode", BN_TRAIN), case.get("mlp", MLP)
    C1 = mlp[0]
    rows = _rows()
    pc = torch.from_numpy(case["pc"]).cuda()
    handles, hosts = _acquire_all(pf, case, pc, 300)
    for h in handles:
        _poison(h["ws"])
    pf.group_compact(handles, pc)
    torch.cuda.synchronize()
    first = [_snapshot(h["ws"], C1) for h in handles]
    assert all(int(h["ws"].tiles[1]) == 0 for h in handles)
    pf.group_compact(handles, pc)                       # twice: the arrival counter is left at zero, the results are identical
    torch.cuda.synchronize()
    for s, ((L, K, dis), o, h) in enumerate(zip(case["scales"], out, handles)):
        ws, c = h["ws"], o["c"]
        for a, b in zip(first[s], _snapshot(ws, C1)):
            assert torch.equal(a, b), (s, "second launch differs")
        nent = [int(n) for n in c["nent"]]
        # 2. exact: counts, offsets, entry rows, window ids
        assert torch.equal(ws.cnt.cpu(), torch.from_numpy(o["cnt"])), s
        assert torch.equal(ws.woff.cpu(), c["woff"]), s
        ent, ewin = ws.ent.cpu(), ws.ewin.cpu()
        live = torch.arange(L * K)[None, :] < torch.tensor(nent)[:, None]
        assert torch.equal(ent[live], c["ent"][live]), s
        assert torch.equal(ewin[live], c["ewin"][live]), s
        # 1. nothing written past what the kernel owns
        assert bool(torch.isnan(ent[~live]).all()) and bool((ewin[~live] == SENT).all()), s
        # 3. tiles
        tps = -(-L * K // rows)
        want = torch.tensor([b * tps + t for b in range(B) for t in range(-(-nent[b] // rows))], dtype=torch.int32)
        tiles = ws.tiles.cpu()
        assert tiles.numel() == 4 + B * tps
        assert int(tiles[0]) == want.numel() and int(tiles[1]) == 0, (s, int(tiles[0]), want.numel(), int(tiles[1]))
        assert torch.equal(tiles[4:4 + want.numel()], want), s
        assert bool((tiles[4 + want.numel():] == SENT).all()), s
        assert float(ws.gmom.view(B, 12)[:, 10:].abs().max()) == 0.0
        # 4. moments: any fp64 summation order of E terms is within E 2^-53 sum|term| of the exact sum; slack 4
        mom, mabs, E = _moments(c)
        M = B * L * K
        got = ws.stat[:10].cpu().numpy()
        assert got[0] == float(M) and float(mom[0]) == float(M), (s, got[0], M)
        err = np.abs(got.astype(np.longdouble) - mom)
        bound = 4.0 * E * 2.0 ** -53 * mabs
        print("%s scale %d: E %d  moments |got-ref| / bound %s" % (name, s, E, np.array2string((err / np.maximum(bound, 1e-300)).astype(np.float64), precision=3)))
        assert (err <= bound).all(), (s, err, bound)
        # 5. BN1 block and running statistics against the fp64 fold of the REFERENCE moments
        plist, bufs, host = hosts[s]
        g1, b1 = host["gamma"][0].numpy(), host["beta"][0].numpy()
        res = {}

        def rec(key, got_t, exp):
            g = got_t.detach().cpu().numpy().astype(np.float64)
            res[key] = (float(np.abs(g - exp).max()), float(np.abs(exp).max()))
        if mode == BN_TRAIN:
            mean, var = _batch_mean_var(mom, float(M), host["W"][0].numpy())
            rec("rmean1", bufs[0][0], 0.19 * mean)                  # from zero: 0.1 m, then 0.9 * 0.1 m + 0.1 m
            if M > 1:
                rec("rvar1", bufs[1][0], 0.81 + 0.19 * var * (M / (M - 1.0)))         # from one, two steps
            # (M = B L K = 1: the unbiased factor M / (M - 1) is undefined -- torch's BatchNorm refuses a single value per
            # channel in training mode -- so the running variance is not compared there)
            assert int(bufs[2][0]) == 2, s
        else:
            mean, var = host["rmean"][0].numpy().astype(np.float64), host["rvar"][0].numpy().astype(np.float64)
            assert torch.equal(bufs[0][0].cpu(), host["rmean"][0]) and torch.equal(bufs[1][0].cpu(), host["rvar"][0]), s
            assert int(bufs[2][0]) == 0, s
        exp = _fold(mean, var, g1, b1)
        bn = ws.bn[:4 * C1]
        for q, key in enumerate(("bn1.scale", "bn1.shift", "bn1.mean", "bn1.rstd")):
            rec(key, bn[q * C1:(q + 1) * C1], exp[q * C1:(q + 1) * C1])
        bad = stage_check(res)
        assert not bad, (s, bad)
    # 6. pooled features of the forward on the grouped workspace: a wrong tile list or offsets that are still self-consistent
    for s in case.get("feat", ()):
        h, c = handles[s], out[s]["c"]
        host = hosts[s][2]
        feat = pf._run_forward(h, h["ws"].cnt, pf._empty_idx(pc.device))[0]
        torch.cuda.synchronize()
        f = entry_ref.forward(c, host["W"][0], host["gamma"][0], host["beta"][0], host["W"][1], host["gamma"][1], host["beta"][1],
                              host["W"][2], host["gamma"][2], host["beta"][2])["feat"]
        assert feat.shape == (B, case["scales"][s][0], mlp[2])                # (B, L, C3): the handle asks for the NLC layout
        d = float((feat.cpu().double().transpose(1, 2) - f.double()).abs().max())
        bad = stage_check({"feat": (d, float(f.abs().max()))})
        assert not bad, (s, bad)


@pytest.mark.parametrize("name", list(CASES))
def test_front_edge_case(name):
    _run_front_case(name)


@pytest.mark.parametrize("name", ["big_b", "eight"])
def test_phased_front_edge_case(name):
    """Phase 1, the same in-place weight change on both parameter sets, phase 2: bit-identical to the fused phase 3 where the
    finalising section sees the most workgroups (1030 arrivals per scale; eight scales)."""
    from frustum_convnet_amd import pointnet_fused as pf
    case, out = _built(name)
    C1 = case.get("mlp", MLP)[0]
    pc = torch.from_numpy(case["pc"]).cuda()
    fused, pf_hosts = _acquire_all(pf, case, pc, 400)
    phased, pp_hosts = _acquire_all(pf, case, pc, 400)
    pf.group_compact(phased, pc, phase=1)
    torch.cuda.synchronize()
    assert all(h["desc"].grouped == 0 for h in phased)
    for (pa, ba, _), (pb, bb, _) in zip(pf_hosts, pp_hosts):
        for ta, tb in zip(pa, pb):
            ta.mul_(1.25).add_(0.01)
            tb.mul_(1.25).add_(0.01)
    pf.group_compact(phased, pc, phase=2)
    pf.group_compact(fused, pc)
    torch.cuda.synchronize()
    assert all(h["desc"].grouped == 1 for h in phased)
    for s, o in enumerate(out):
        wf, wp = fused[s]["ws"], phased[s]["ws"]
        for nm in ("cnt", "woff", "tiles", "stat", "gmom", "wenc", "bn"):
            a, b = getattr(wf, nm), getattr(wp, nm)
            if nm == "bn":
                a, b = a[:4 * C1], b[:4 * C1]
            assert torch.equal(_bits(a), _bits(b)), (s, nm)
        assert torch.equal(wf.cnt.cpu(), torch.from_numpy(o["cnt"])) and torch.equal(wf.woff.cpu(), o["c"]["woff"]), s
        (pa, ba, _), (pb, bb, _) = pf_hosts[s], pp_hosts[s]
        assert torch.equal(ba[0][0], bb[0][0]) and torch.equal(ba[1][0], bb[1][0]) and int(ba[2][0]) == int(bb[2][0]) == 1, s


def _lds_limit():
    """Bytes of LDS one workgroup may use on the device (hipDeviceAttributeMaxSharedMemoryPerBlock, as torch reports it); None
    on the host emulation, which has no such limit."""
    if not torch.cuda.is_available():
        return None
    return int(torch.cuda.get_device_properties(torch.cuda.current_device()).shared_memory_per_block)


MAX_L = 3276        # the host check admits 20 L + 4 <= 65536 bytes of dynamic LDS


def test_largest_accepted_window_count():
    """L = 3276 is the largest window count the host check admits: 20 L + 4 = 65 524 bytes of dynamic LDS, and gc_entries_kernel
    holds GE_STATIC_LDS = 1 360 bytes of static __shared__ on top: 66 884 bytes in all.  It FITS: the MI355X
    reports 163 840 bytes of LDS per workgroup (hipDeviceAttributeMaxSharedMemoryPerBlock), so the host check's 64 KiB cap on the
    dynamic part is the binding limit and needs no correction for the static part.
    The sum is checked against the device's limit BEFORE the launch; then the case goes through every comparison of the other
    cases (per = 4 windows per thread in the offset scan, K = 1)."""
    limit = _lds_limit()
    need = GE_STATIC_LDS + 20 * MAX_L + 4
    print("gc_entries_kernel at L = %d: %d static + %d dynamic = %d bytes of LDS; device limit %s" %
          (MAX_L, GE_STATIC_LDS, 20 * MAX_L + 4, need, limit))
    assert 20 * MAX_L + 4 <= 65536 < 20 * (MAX_L + 1) + 4
    assert limit is None or need <= limit, (need, limit)
    _run_front_case("max_l_%d" % MAX_L)


# ------------------------------------------------------------------------------------------------------------- refusals
def _raw_call(L, descs, params, pc, refs, dz, wss, cnts, nscale, phase):
    from frustum_convnet_amd import _native
    n = len(descs)
    arr = lambda vals: (ctypes.c_void_p * n)(*vals)
    return L.fcn_pn_group_compact2(nscale, arr([ctypes.addressof(d) if d is not None else None for d in descs]),
                                   arr([ctypes.addressof(p) for p in params]), pc.data_ptr(), arr(refs),
                                   (ctypes.c_float * n)(*dz), arr([ctypes.addressof(w) if w is not None else None for w in wss]),
                                   arr(cnts), phase, _native.current_stream(pc.device))


def _desc_copy(d, **kw):
    from frustum_convnet_amd._native import PnDesc
    c = PnDesc.from_buffer_copy(d)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_refusals_return_their_code_and_launch_nothing():
    """Every refusal goes through the raw C entry, returns its code and leaves the poisoned workspaces as they were.  The
    descriptors that exceed a limit (N, L, K, B, the dynamic LDS) describe buffers far larger than the ones behind them: the
    buffers are never dereferenced, because the call returns before any launch -- B = 65536 included, whose real workspace would
    be needlessly large."""
    from frustum_convnet_amd import pointnet_fused as pf, _native
    lib = _native.lib()
    case, out = _built("fits")
    pc = torch.from_numpy(case["pc"]).cuda()
    handles, hosts = _acquire_all(pf, case, pc, 500)
    handles = handles[:2]
    for h in handles:
        _poison(h["ws"])
        h["ws"].stat.fill_(-7.0)
        h["ws"].bn.fill_(float("nan"))
    before = [[_bits(t).cpu().clone() for t in (h["ws"].cnt, h["ws"].woff, h["ws"].ent, h["ws"].ewin, h["ws"].tiles, h["ws"].stat,
                                                h["ws"].bn)] for h in handles]
    d = [h["desc"] for h in handles]
    p = [h["params"] for h in handles]
    refs = [h["ref"].data_ptr() for h in handles]
    wss = [h["ws"].c for h in handles]
    cnts = [h["ws"].cnt.data_ptr() for h in handles]
    dz = [h["dist"] for h in handles]

    def call(nscale=1, phase=3, descs=None, refs_=None, wss_=None, cnts_=None):
        descs = descs or d
        n = len(descs)
        return _raw_call(lib, descs, p[:n], pc, (refs_ or refs)[:n], dz[:n], (wss_ or wss)[:n], (cnts_ or cnts)[:n], nscale, phase)

    limit = {"N=65536": dict(N=65536), "L=8193": dict(L=8193), "K=1025": dict(K=1025), "B=65536": dict(B=65536),
             "L=3277 (20 L + 4 = 65544 bytes of dynamic LDS)": dict(L=3277)}
    for what, kw in limit.items():
        assert call(descs=[_desc_copy(d[0], **kw)]) == FCN_E_LIMIT, what
    assert call(phase=0) == FCN_E_BADARG and call(phase=4) == FCN_E_BADARG
    assert call(nscale=0) == FCN_E_BADARG and call(nscale=9) == FCN_E_BADARG
    assert call(descs=[_desc_copy(d[0], C1=96)]) == FCN_E_BADARG
    for what, kw in {"B": dict(B=3), "N": dict(N=63), "eps": dict(eps=2e-5), "momentum": dict(momentum=0.2),
                     "mode": dict(training=BN_FROZEN)}.items():
        assert call(nscale=2, descs=[d[0], _desc_copy(d[1], **kw)]) == FCN_E_BADARG, what
    assert call(nscale=2, wss_=[wss[0], None]) == FCN_E_BADARG
    assert call(nscale=2, refs_=[refs[0], None]) == FCN_E_BADARG
    assert call(nscale=2, cnts_=[cnts[0], None]) == FCN_E_BADARG
    assert call(wss_=[None]) == FCN_E_BADARG and call(refs_=[None]) == FCN_E_BADARG and call(cnts_=[None]) == FCN_E_BADARG
    torch.cuda.synchronize()
    for h, b4 in zip(handles, before):
        ws = h["ws"]
        for a, t in zip(b4, (ws.cnt, ws.woff, ws.ent, ws.ewin, ws.tiles, ws.stat, ws.bn)):
            assert torch.equal(a, _bits(t).cpu()), "a refused call wrote to a workspace"
        assert all(int(b) == 0 for b in h["bufs"][2])
