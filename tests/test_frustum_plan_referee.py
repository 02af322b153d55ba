"""CPU: the numpy restatement of the capturable training input (tests/frustum_plan_ref.py) against the host path it replaces --
its perturbation, fed uniforms from a seeded np.random, against frustum.perturb_boxes2d bit for bit; its plan against the kept
list and offsets frustum.frustum_training_candidates computes from the same segment counts (the counts and the offsets are read
off the host emulation's count and fill calls) -- plus the known properties of the counter layout (tag 3 collides with no stream
of fcn_draw_batch)."""
import ctypes
import os
import shutil

import numpy as np
import pytest

import draws_ref
import frustum_plan_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_label.npz")
CLANG = os.environ.get("FCN_HOST_CLANG", "/opt/rocm/lib/llvm/bin/clang++")
W, H = 1242.0, 375.0


def _boxes():
    """Plain boxes, boxes at every image edge (attempts fail there), a box almost beyond the image (many attempts)."""
    rs = np.random.RandomState(11)
    x0, y0 = rs.uniform(0, W - 200, 40), rs.uniform(0, H - 120, 40)
    plain = np.stack([x0, y0, x0 + rs.uniform(5, 190, 40), y0 + rs.uniform(5, 110, 40)], 1)
    edge = np.asarray([[W - 1.5, 100.0, W + 60.0, 180.0], [-80.0, 50.0, 0.7, 120.0], [300.0, H - 1.2, 380.0, H + 90.0],
                       [500.0, -70.0, 560.0, 0.4], [W + 4.0, 100.0, W + 60.0, 160.0], [200.0, H + 2.5, 260.0, H + 30.0]])
    return np.concatenate([plain, edge], 0)


def test_perturb_with_injected_uniforms_equals_perturb_boxes2d_bit_for_bit():
    from frustum_convnet_amd import frustum
    boxes = _boxes()
    for r in (0.1, 0.3, 0.0):
        if r == 0.0:
            boxes = boxes[:40]                                                  # (no shift: an edge box beyond the image never lands)
        want = frustum.perturb_boxes2d(boxes, [W, H], r, rng=np.random.RandomState(5))
        rs = np.random.RandomState(5)
        got, used, fail = ref.perturb(0, 0, boxes, [W, H], r, T=100000, draw=lambda d, t: [rs.random_sample() for _ in range(4)])
        assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), r
        assert not fail.any() and (used >= 0).all()
        if r > 0:
            assert used.max() >= 2 and (used == 0).sum() >= 40                  # retries happened, in the reference's order
    # per-image sizes, as the kernel reads them through box_frame
    wh = np.where(np.arange(len(boxes))[:, None] % 2 == 0, [[W, H]], [[1224.0, 370.0]])
    want = frustum.perturb_boxes2d(boxes, wh, 0.1, rng=np.random.RandomState(6))
    rs = np.random.RandomState(6)
    got, _, _ = ref.perturb(0, 0, boxes, wh, 0.1, T=100000, draw=lambda d, t: [rs.random_sample() for _ in range(4)])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_perturb_contract_stream_cap_and_failures():
    # tag 3: the words of an attempt are blocks 2t, 2t + 1 of row d; no stream of fcn_draw_batch (tags 0, 1, 2) shares a counter
    u = ref.uniforms(1234, (1 << 32) + 5, 7, 3)
    w = draws_ref._words(1234, (1 << 32) + 5, 7, 3, 32)[24:32]
    assert u == [draws_ref._u53(w[2 * i], w[2 * i + 1]) * 2.0 ** -53 for i in range(4)] and all(0.0 <= x < 1.0 for x in u)
    assert u != ref.uniforms(1234, 5, 7, 3) and u != ref.uniforms(1234, (1 << 32) + 5, 7, 2)
    for tag in (0, 1, 2):
        assert not np.array_equal(draws_ref._words(1234, 5, 7, tag, 8), draws_ref._words(1234, 5, 7, 3, 8))
    boxes = _boxes()[:40]
    a, used, fail = ref.perturb(9, 0, boxes, [W, H], 0.1)
    b, _, _ = ref.perturb(9, 1, boxes, [W, H], 0.1)
    assert not fail.any() and (used == 0).all() and not np.array_equal(a, b)       # plain boxes land at once; steps differ
    assert (np.abs(a - boxes) <= 0.1 * 190 * 1.5 + 1e-9).all()
    # beyond the image: every attempt fails, the input is kept and flagged; an out-of-range frame (NaN size) likewise
    beyond = np.asarray([[1300.0, 100.0, 1400.0, 200.0], [100.0, 100.0, 200.0, 200.0]])
    out, used, fail = ref.perturb(9, 0, beyond, [[W, H], [np.nan, np.nan]], 0.1)
    assert fail.tolist() == [True, True] and used.tolist() == [-1, -1] and np.array_equal(out, beyond)
    assert ref.ATTEMPTS == 32


def test_plan_cases_by_hand():
    cnt = np.asarray([[5, 0, 2], [3, 3, 3], [0, 0, 0], [4, 1, 0], [7, 7, 7]])
    pos = np.asarray([[1, 0, 0], [0, 0, 0], [0, 0, 0], [0, 1, 0], [2, 0, 0]])
    gt = np.asarray([[0, 0, 10, 30.0], [0, 0, 10, 30.0], [0, 0, 10, 30.0], [0, 0, 10, 30.0], [0, 10, 10, 34.9]])
    sb, so, off, n, st = ref.plan(cnt, pos, gt, 25.0, 3, 100)                   # boxes 0, 3 survive (4 fails the height rule)
    assert sb.tolist() == [0, 3, 0] and n == 2 and st == ref.ST_FEW
    assert so.tolist() == [0, 5, 5, 7, 7, 7, 7, 7, 7, 7, 11, 12, 12, 12, 12, 12] and off.tolist() == [0, 7, 12, 12]
    sb, so, off, n, st = ref.plan(cnt, pos, gt, 20.0, 2, 11)                    # 0, 3, 4 survive, two slots, one row short
    assert sb.tolist() == [0, 3] and n == 2 and st == ref.ST_TRUNC and off.tolist() == [0, 7, 11] and so[-1] == 11 and so[11] == 11
    sb, so, off, n, st = ref.plan(cnt, pos * 0, gt, 20.0, 2, 11)                # none
    assert sb.tolist() == [0, 0] and n == 0 and st == ref.ST_FEW and not so.any() and not off.any()
    assert sb.dtype == np.int32 and so.dtype == np.int64 and off.dtype == np.int64


@pytest.mark.skipif(not (os.path.exists(CLANG) or shutil.which(CLANG)), reason="host clang++ not available")
@pytest.mark.parametrize("min_h", [25.0, 10.0, 1000.0])
def test_plan_equals_what_frustum_training_candidates_computes_from_the_same_counts(min_h):
    """B >= survivors and capacity >= total: the regime in which the host path and the plan describe the same packed buffers."""
    import torch
    from emu_shim import emulated_gpu
    from frustum_convnet_amd import frustum
    g = dict(np.load(GOLDEN))
    D = len(g["box_frame"])
    seen = {}
    with emulated_gpu() as L:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
        cal = {k: dev(g[k]) for k in ("P", "V2C", "R0")}
        real_count, real_fill = L.fcn_frustum_label_count, L.fcn_frustum_label_fill
        rd = lambda ptr, n, ct, dt: np.frombuffer((ct * n).from_address(ptr), dtype=dt).copy()

        def count(*a):
            rc = real_count(*a)
            seen["S"] = a[11]
            seen["cnt"] = rd(a[17], D * a[11], ctypes.c_int32, np.int32).reshape(D, a[11])
            seen["pos"] = rd(a[18], D * a[11], ctypes.c_int32, np.int32).reshape(D, a[11])
            return rc

        def fill(*a):
            seen["seg_off"] = rd(a[15], D * a[11] + 1, ctypes.c_int64, np.int64)
            return real_fill(*a)
        try:
            L.fcn_frustum_label_count, L.fcn_frustum_label_fill = count, fill
            sel = frustum.frustum_training_candidates(dev(g["points"]), dev(g["off"]), cal, g["img_wh"], g["ref_boxes"], g["box_frame"],
                                                      g["gt_box3d"], gt_box2d=g["gt_box2d"], min_box_height=min_h)
        finally:
            L.fcn_frustum_label_count, L.fcn_frustum_label_fill = real_count, real_fill
        off = sel["off"].numpy().copy() if "off" in sel else None
    S = seen["S"]
    slot_box, seg_off, poff, n, st = ref.plan(seen["cnt"], seen["pos"], g["gt_box2d"], min_h, D, 1 << 40)
    kept = sel["kept"]
    assert n == len(kept) and np.array_equal(slot_box[:n], kept) and (slot_box[n:] == 0).all()
    assert st == (ref.ST_FEW if n < D else 0)
    if min_h == 1000.0:
        assert n == 0 and not seg_off.any() and not poff.any() and "seg_off" not in seen      # (no fill without a survivor)
        return
    assert 0 < n < D
    assert np.array_equal(seg_off, seen["seg_off"])
    assert np.array_equal(poff[:n + 1], off) and (poff[n:] == off[-1]).all()
    assert len(seg_off) == D * S + 1
