"""-m gpu: the cascade link -- fcn_refine_select_count / _fill (csrc/refine_select.h) through the C-ABI, RefineInputBuilder.
build_device against build() on host records, and TwoStageDetector against the hand-composed sequence of the same calls.
The referee is the fp64 numpy restatement of tests/cascade_ref.py (pinned to the reference by tests/test_cascade_referee.py).
tests/test_emu_cascade.py runs the same functions on the host emulation of the kernels."""
import functools

import numpy as np
import pytest
import torch

import cascade_ref

pytestmark = pytest.mark.gpu
BADARG = 10001                     # FCN_E_BADARG
NAN_PAYLOAD = 0x7fc12345           # a quiet NaN with a payload: a copy through float arithmetic could lose it
COUNTS = (1000, 77, 0)
CAND_ROW = (7, 2, 9, 0, 4, 5, 1)
CAND_FRAME = (0, 0, 0, 1, 2, 0, 1)


@functools.lru_cache(maxsize=None)
def _scene(stride):
    """F = 3 frames of 1000, 77 and 0 points; D = 7 candidates over R = 10 rows (see the comments); referee's answer."""
    rng = np.random.RandomState(77 + stride)
    n = sum(COUNTS)
    pts = np.zeros((n, stride), dtype=np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-8, 8, n), rng.uniform(0, 2, n), rng.uniform(5, 25, n)
    if stride > 3:
        pts[:, 3:] = rng.uniform(0, 1, (n, stride - 3))
    pts[500] = [0.5, 1.0, 15.0] + [0.25] * (stride - 3)          # in the middle of candidates 0, 1 and 5 ...
    pts[500, 0] = np.nan                                         # ... but for its NaN x: never selected
    pts[501, :3], pts[502, :3] = [0.5, np.inf, 15.0], [0.5, 1.0, -np.inf]
    pts[503, :3] = [0.25, 1.0, 14.5]                             # selected by 0, 1 and 5
    if stride > 3:
        pts[503:504, 3].view(np.uint32)[0] = NAN_PAYLOAD         # carried along bit for bit
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    dets = rng.uniform(-1, 1, (10, 8)).astype(np.float32)        # rows no candidate points at: noise

    def row(centre, lwh, ry):                                    # label format: ty is the box BOTTOM
        return [centre[0], centre[1] + lwh[2] / 2.0, centre[2], lwh[0], lwh[1], lwh[2], ry, rng.rand()]
    dets[7] = row((0, 1, 12), (6, 5, 1.5), 0.0)                  # 0: frame 0
    dets[2] = row((1, 1, 13), (6, 4, 1.8), np.pi / 2)            # 1: frame 0, overlaps candidate 0
    dets[9] = row((100, 1, 100), (2, 2, 2), -np.pi / 2)          # 2: frame 0, holds no point
    dets[0] = row((0, 1, 15), (40, 40, 10), 2.5)                 # 3: frame 1, holds every point of it
    dets[4] = row((0, 1, 15), (4, 2, 2), -3.1)                   # 4: the empty frame
    dets[5] = row((0, 1, 15), (12, 14, 3), 2.5)                  # 5: frame 0, most of it: hits in every 256-point chunk
    dets[1] = row((2, 1, 10), (8, 6, 2), -3.1)                   # 6: frame 1, part of it
    crow, cframe = np.asarray(CAND_ROW, dtype=np.int32), np.asarray(CAND_FRAME, dtype=np.int32)
    ref = cascade_ref.select(pts, off, dets, crow, cframe, 1.2)
    c = ref["counts"]
    assert c[2] == 0 and c[3] == 77 and c[4] == 0 and 0 < c[0] < 1000 and 0 < c[1] < 1000 and 0 < c[6] < 77
    assert len(np.intersect1d(ref["index"][0], ref["index"][1])) > 0                     # two overlapping boxes in one frame
    assert c[5] % 64 != 0 and all(((ref["index"][5] // 256) == q).sum() > 64 for q in range(4))
    assert 500 not in ref["index"][5] and 503 in ref["index"][5] and 503 in ref["index"][0] and 503 in ref["index"][1]
    return {"pts": pts, "off": off, "dets": dets, "crow": crow, "cframe": cframe, "ref": ref}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def _count(t, ratio=1.2):
    """The raw count entry point on device tensors t (pts, off, dets, crow, cframe) -> rc, outputs (sentinel-filled first)."""
    from frustum_convnet_amd import _native
    D = t["crow"].numel()
    o = {"pred_box3d": torch.full((D, 8, 3), -7.0, dtype=torch.float64, device="cuda"),
         "pred_angle": torch.full((D,), -7.0, dtype=torch.float64, device="cuda"),
         "pred_size": torch.full((D, 3), -7.0, dtype=torch.float64, device="cuda"),
         "cnt": torch.full((D,), -7, dtype=torch.int32, device="cuda")}
    rc = _native.lib().fcn_refine_select_count(
        _p(t["pts"]), _p(t["off"]), t["off"].numel() - 1, t["pts"].shape[1], _p(t["dets"]), t["dets"].shape[0], _p(t["crow"]),
        _p(t["cframe"]), D, ratio, _p(o["pred_box3d"]), _p(o["pred_angle"]), _p(o["pred_size"]), _p(o["cnt"]),
        _native.current_stream())
    torch.cuda.synchronize()
    return rc, o


def _fill(t, counts, ratio=1.2, guard=5):
    """The raw fill entry point -> rc, out rows (total, stride) and the `guard` sentinel rows behind them."""
    from frustum_convnet_amd import _native
    D, ps = t["crow"].numel(), t["pts"].shape[1]
    ooff = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = torch.full((int(ooff[-1]) + guard, ps), -7.0, dtype=torch.float32, device="cuda")
    ooff_d = _dev(ooff)
    rc = _native.lib().fcn_refine_select_fill(
        _p(t["pts"]), _p(t["off"]), t["off"].numel() - 1, ps, _p(t["dets"]), t["dets"].shape[0], _p(t["crow"]), _p(t["cframe"]),
        D, ratio, _p(ooff_d), _p(out), _native.current_stream())
    torch.cuda.synchronize()
    return rc, out[:int(ooff[-1])].cpu().numpy(), out[int(ooff[-1]):].cpu().numpy(), ooff


def _tensors(sc, **over):
    t = {k: _dev(over.get(k, sc[k])) for k in ("pts", "off", "dets", "crow", "cframe")}
    return t


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expected_rows(sc):
    ref = sc["ref"]
    return np.concatenate([sc["pts"][int(sc["off"][f]):][idx] for idx, f in zip(ref["index"], sc["cframe"])], 0)


@pytest.mark.parametrize("stride", [3, 4])
def test_select_entry_points_match_the_referee(stride):
    sc = _scene(stride)
    ref = sc["ref"]
    t = _tensors(sc)
    rc, o = _count(t)
    assert rc == 0
    cnt = o["cnt"].cpu().numpy()
    print("cnt", cnt.tolist(), "referee", ref["counts"].tolist())
    assert np.array_equal(cnt, ref["counts"])
    # fp64 arithmetic on the same fp32 inputs: 1e-12 relative, element by element (cascade_ref.within).  A corner coordinate is
    # centre + rotated half edge and may cancel to nearly zero, so its floor is the box's largest edge; heading and size have none.
    for d in range(len(cnt)):
        got, want, ext = o["pred_box3d"][d].cpu().numpy(), ref["pred_box3d"][d], ref["pred_size"][d].max()
        print("candidate %d: corners worst rel err %.2e" % (d, cascade_ref.worst(got, want, ext)))
        assert cascade_ref.within(got, want, extent=ext), (d, cascade_ref.worst(got, want, ext))
    for k in ("pred_angle", "pred_size"):
        got, want = o[k].cpu().numpy(), ref[k]
        assert cascade_ref.within(got, want), (k, cascade_ref.worst(got, want))
    rc, rows, guard, _ = _fill(t, cnt)
    assert rc == 0
    want = _expected_rows(sc)
    assert rows.shape == want.shape
    assert np.array_equal(_bits(rows), _bits(want))                      # bit-identical and in order, NaN payload included
    assert (guard == -7.0).all()
    if stride == 4:
        assert (_bits(rows)[:, 3] == NAN_PAYLOAD).sum() == 3            # point 503, once per candidate that holds it
    assert not np.isnan(rows[:, :3]).any() and np.isfinite(rows[:, :3]).all()
    rc2, rows2, _, _ = _fill(t, cnt)
    assert rc2 == 0 and np.array_equal(_bits(rows2), _bits(rows))        # identical over two runs


def test_select_rows_that_are_not_16_byte_aligned():
    """pt_stride 4 takes 16-byte loads only when the buffers allow it: a view that starts 4 bytes into an allocation must give
    the same rows through the scalar path."""
    sc = _scene(4)
    t = _tensors(sc)
    flat = torch.zeros(sc["pts"].size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = t["pts"].reshape(-1)
    t["pts"] = flat[1:].view(-1, 4)
    assert t["pts"].data_ptr() % 16 == 4
    rc, o = _count(t)
    assert rc == 0 and np.array_equal(o["cnt"].cpu().numpy(), sc["ref"]["counts"])
    rc, rows, guard, _ = _fill(t, sc["ref"]["counts"])
    assert rc == 0 and np.array_equal(_bits(rows), _bits(_expected_rows(sc))) and (guard == -7.0).all()


def test_select_nothing_to_do_and_bad_arguments():
    from frustum_convnet_amd import _native
    sc = _scene(3)
    t = _tensors(sc)
    L = _native.lib()
    # D = 0: empty candidate lists (and empty outputs: their pointers may be NULL)
    t0 = dict(t, crow=_dev(np.zeros(0, np.int32)), cframe=_dev(np.zeros(0, np.int32)))
    rc, o = _count(t0)
    assert rc == 0 and o["cnt"].numel() == 0
    rc, rows, guard, _ = _fill(t0, np.zeros(0, np.int64))
    assert rc == 0 and rows.shape == (0, 3) and (guard == -7.0).all()
    # F = 0: no frame to search
    tf = dict(t, off=_dev(np.zeros(1, np.int64)))
    rc, o = _count(tf)
    assert rc == 0 and (o["cnt"].cpu().numpy() == 0).all() and (o["pred_size"].cpu().numpy() == -7.0).all()
    # pt_stride < 3 and NULL pointers: refused before anything is launched
    s = _native.current_stream()
    D, R = t["crow"].numel(), t["dets"].shape[0]
    rc, o = _count(t)
    good = [_p(t["pts"]), _p(t["off"]), 3, 3, _p(t["dets"]), R, _p(t["crow"]), _p(t["cframe"]), D, 1.2,
            _p(o["pred_box3d"]), _p(o["pred_angle"]), _p(o["pred_size"]), _p(o["cnt"]), s]
    assert L.fcn_refine_select_count(*good) == 0
    torch.cuda.synchronize()
    for i in (0, 1, 4, 6, 7, 10, 11, 12, 13):
        bad = list(good)
        bad[i] = None
        assert L.fcn_refine_select_count(*bad) == BADARG, i
    bad = list(good)
    bad[3] = 2
    assert L.fcn_refine_select_count(*bad) == BADARG
    ooff = _dev(np.concatenate([[0], np.cumsum(sc["ref"]["counts"])]).astype(np.int64))
    out = torch.zeros((int(sc["ref"]["counts"].sum()), 3), dtype=torch.float32, device="cuda")
    goodf = good[:10] + [_p(ooff), _p(out), s]
    assert L.fcn_refine_select_fill(*goodf) == 0
    torch.cuda.synchronize()
    for i in (0, 1, 4, 6, 7, 10, 11):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_refine_select_fill(*bad) == BADARG, i


@pytest.mark.parametrize("what", ["frame_high", "frame_negative", "row_high", "row_negative"])
def test_out_of_range_candidate_is_reported_and_never_dereferenced(what):
    from frustum_convnet_amd import cascade, _native
    sc = _scene(4)
    crow, cframe = sc["crow"].copy(), sc["cframe"].copy()
    if what.startswith("frame"):
        cframe[1] = 3 if what == "frame_high" else -1            # F = 3
    else:
        crow[1] = 10 if what == "row_high" else -(2 ** 31)       # R = 10
    t = _tensors(sc, crow=crow, cframe=cframe)
    rc, o = _count(t)
    assert rc == BADARG
    cnt = o["cnt"].cpu().numpy()
    want = sc["ref"]["counts"].copy()
    want[1] = 0
    assert np.array_equal(cnt, want)                             # its cnt is 0, every other candidate is processed
    for k in ("pred_box3d", "pred_angle", "pred_size"):
        got = o[k].cpu().numpy()
        assert (got[1] == -7.0).all(), k                         # nothing beyond its own cnt is touched
        for d in range(len(cnt)):
            if d != 1:
                ext = sc["ref"]["pred_size"][d].max() if k == "pred_box3d" else 0.0
                assert cascade_ref.within(got[d], sc["ref"][k][d], extent=ext), (k, d)
    rc, rows, guard, _ = _fill(t, cnt)
    assert rc == BADARG and (guard == -7.0).all()
    ref = sc["ref"]
    exp = np.concatenate([sc["pts"][int(sc["off"][f]):][idx] for d, (idx, f) in enumerate(zip(ref["index"], sc["cframe"]))
                          if d != 1], 0)
    assert np.array_equal(_bits(rows), _bits(exp))
    with pytest.raises(_native.NativeError):
        cascade.refine_candidates(t["pts"], t["off"], t["dets"], t["crow"], t["cframe"])


def test_fill_never_writes_past_a_candidates_slice():
    """out_off bounds the writes: with offsets that grant candidate 5 fewer rows than it selects, the surplus is dropped and
    the neighbours' rows and the rows behind the buffer stay as they were."""
    sc = _scene(4)
    t = _tensors(sc)
    counts = sc["ref"]["counts"].copy()
    counts[5] -= 100
    rc, rows, guard, ooff = _fill(t, counts)
    assert rc == 0 and (guard == -7.0).all()
    ref = sc["ref"]
    for d, (idx, f) in enumerate(zip(ref["index"], sc["cframe"])):
        exp = sc["pts"][int(sc["off"][f]):][idx][:counts[d]]
        assert np.array_equal(_bits(rows[ooff[d]:ooff[d + 1]]), _bits(exp)), d


@functools.lru_cache(maxsize=None)
def _edge_scene(stride):
    """The frame lengths the shared scan-and-compact skeleton's paths turn on (csrc/seg_compact.h; seg = fcn_frustum_select_seg()),
    one frame each, and one candidate per frame that holds most of it.  The link scans a whole frame as ONE segment: these are
    its empty, partial, one-iteration and many-iteration quarters."""
    from frustum_convnet_amd import _native
    seg = int(_native.lib().fcn_frustum_select_seg())
    lengths = (0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1, 2 * seg + 100)
    rng = np.random.RandomState(177 + stride)
    n = sum(lengths)
    pts = np.zeros((n, stride), dtype=np.float32)
    pts[:, 0], pts[:, 1], pts[:, 2] = rng.uniform(-8, 8, n), rng.uniform(0, 2, n), rng.uniform(5, 25, n)
    pts[:, 3:] = rng.uniform(0, 1, (n, stride - 3))
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    dets = np.tile(np.asarray([0.0, 1.0 + 1.5, 15.0, 12.0, 14.0, 3.0, 2.5, 0.5], dtype=np.float32), (len(lengths), 1))
    dets[:, 6] += np.linspace(0.0, 0.5, len(lengths)).astype(np.float32)         # (a box of its own per frame)
    crow = cframe = np.arange(len(lengths), dtype=np.int32)
    ref = cascade_ref.select(pts, off, dets, crow, cframe, 1.2)
    c = ref["counts"]
    assert c[0] == 0 and (c[2:] > 0).all() and (c[2:] < np.asarray(lengths[2:])).all() and (c[6:] % 64 != 0).any()
    return {"pts": pts, "off": off, "dets": dets, "crow": crow, "cframe": cframe, "ref": ref}


@pytest.mark.parametrize("stride", [3, 4, 5])
def test_select_over_the_frame_lengths_the_scan_turns_on(stride):
    """Frames of 0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1 and 2 * seg + 100 rows at strides 3, 4 and 5: counts and rows equal the
    referee's, bit for bit and in order; at stride 4 a buffer that starts 4 bytes into an allocation (the scalar path) gives the
    rows of the aligned run; offsets that grant nothing store nothing."""
    sc = _edge_scene(stride)
    ref = sc["ref"]
    t = _tensors(sc)
    rc, o = _count(t)
    assert rc == 0 and np.array_equal(o["cnt"].cpu().numpy(), ref["counts"])
    rc, rows, guard, _ = _fill(t, ref["counts"])
    assert rc == 0 and (guard == -7.0).all()
    assert np.array_equal(_bits(rows), _bits(_expected_rows(sc)))
    if stride == 4:
        flat = torch.zeros(sc["pts"].size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = t["pts"].reshape(-1)
        tu = dict(t, pts=flat[1:].view(-1, 4))
        assert tu["pts"].data_ptr() % 16 == 4
        rc, ou = _count(tu)
        assert rc == 0 and torch.equal(ou["cnt"].cpu(), o["cnt"].cpu())
        rc, rows_u, guard, _ = _fill(tu, ref["counts"])
        assert rc == 0 and np.array_equal(_bits(rows_u), _bits(rows)) and (guard == -7.0).all()
    rc, rows, guard, _ = _fill(t, np.zeros_like(ref["counts"]))          # the empty grant
    assert rc == 0 and rows.shape == (0, stride) and (guard == -7.0).all()


def _builder(npoints):
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    reset_cfg()
    return inputs.RefineInputBuilder(npoints, strides=(0.1, 0.2, 0.4, 0.8))


def test_build_device_equals_build_on_host_records():
    """RefineInputBuilder.build_device on the device selection against build(records, with_labels=False) on the referee's
    selection of the same frames with the same draws: bit-identical batch; candidates without a point are absent."""
    from frustum_convnet_amd import cascade, inputs
    sc = _scene(4)
    ref = sc["ref"]
    t = _tensors(sc)
    b = _builder(256)
    cands = cascade.refine_candidates(t["pts"], t["off"], t["dets"], t["crow"], t["cframe"], ratio=1.2)
    assert np.array_equal(cands["counts"], ref["counts"]) and cands["counts"].dtype == np.int64
    assert np.array_equal(cands["off"].cpu().numpy(), np.concatenate([[0], np.cumsum(ref["counts"])]))
    assert np.array_equal(_bits(cands["points"].cpu().numpy()), _bits(_expected_rows(sc)))
    types = ["Car", "Pedestrian", "Cyclist", "Car", "Car", "Cyclist", "Pedestrian"]
    kept = np.nonzero(ref["counts"] > 0)[0]
    assert kept.tolist() == [0, 1, 3, 5, 6]
    draws = inputs.draw_refine(ref["counts"][kept], 256, False, False, rng=np.random.RandomState(3))
    assert (draws[0].max(1) < ref["counts"][kept]).all() and draws[0][3].max() >= 256        # 77 and > 256 points: both resample modes
    got = b.build_device(cands, types, draws=draws)
    score = sc["dets"][sc["crow"], 7]
    recs = [{"points": sc["pts"][int(sc["off"][sc["cframe"][d]]):][ref["index"][d]], "pred_box3d": ref["pred_box3d"][d],
             "pred_angle": ref["pred_angle"][d], "pred_size": ref["pred_size"][d], "type": types[d], "prob": score[d]}
            for d in kept]
    want = b.build(recs, draws=draws, with_labels=False)
    torch.cuda.synchronize()
    assert np.array_equal(got["kept"], kept)
    for k in ("point_cloud", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "rot_angle", "ref_center", "lens",
              "rgb_prob", "one_hot"):
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    assert "cls_label" not in got and got["point_cloud"].shape == (5, 3, 256)
    # rgb_prob handed in instead of the first-stage score; every candidate kept: no gather
    prob = np.linspace(0.1, 0.7, 7)
    got2 = b.build_device(cands, types, prob=prob, draws=draws)
    assert np.array_equal(got2["rgb_prob"].cpu().numpy().ravel(), prob.astype(np.float32)[kept])
    sub = [0, 1, 5]
    c3 = cascade.refine_candidates(t["pts"], t["off"], t["dets"], sc["crow"][sub], sc["cframe"][sub])
    d3 = (draws[0][[0, 1, 3]], draws[1][[0, 1, 3]], draws[2][[0, 1, 3]])
    got3 = b.build_device(c3, [types[i] for i in sub], draws=d3)
    assert got3["kept"].tolist() == [0, 1, 2]
    assert torch.equal(got3["point_cloud"].cpu(), want["point_cloud"][[0, 1, 3]].cpu())
    # nobody survives: 'kept' alone
    c0 = cascade.refine_candidates(t["pts"], t["off"], t["dets"], sc["crow"][[2, 4]], sc["cframe"][[2, 4]])
    assert c0["points"].shape == (0, 4) and list(b.build_device(c0, ["Car", "Car"]).keys()) == ["kept"]


def test_two_stage_detector_equals_the_hand_composed_sequence():
    """A car first stage (B = 4, N = 512) and a refine second stage (N = 512, strides 0.1 .. 0.8), both hash-initialised:
    TwoStageDetector.detect == stage1.detect, keep lists, refine_candidates, build_device, stage2.detect by hand, bit for bit."""
    from helpers import load_golden, golden_inputs
    from test_gpu_model import _model
    from frustum_convnet_amd import cascade, inputs, synth
    g1, g2 = load_golden("car_b4_n512"), load_golden("refine_b4_n512")
    m1 = _model(g1).eval()
    data = synth.to_torch(golden_inputs(g1), "cuda")
    m2 = _model(g2).eval()                                       # (cfg now holds the refine strides: the builder reads them)
    builder = inputs.RefineInputBuilder(int(g2["meta_npoint"]))
    assert builder.strides == tuple(float(s) for s in g2["meta_strides"])
    B, L2 = data["center_ref2"].shape[0], data["center_ref2"].shape[2]
    dd = {k: data[k] for k in ("point_cloud", "one_hot", "center_ref1", "center_ref2", "center_ref3", "center_ref4")}
    ug = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
    frustum_frame, types = [0, 0, 1, 1], ["Car", "Car", "Pedestrian", "Cyclist"]
    kw = dict(unit_group=ug, num_groups=2, method="nms", thresh=0.1, top_k=6)
    # ---- by hand
    dets1, valid1, keep1, cnt1 = m1.detect(dd, **kw)
    rows = np.concatenate([keep1[g, :int(cnt1[g])].cpu().numpy() for g in range(2)]).astype(np.int64)
    assert len(rows) > 0
    unit = rows // L2
    # the frames: each frustum's own points + a cloud around every kept first-stage box, so that the boxes hold points
    rng = np.random.RandomState(9)
    d1 = dets1.cpu().numpy().astype(np.float64)
    frames = []
    for f in range(2):
        own = [data["point_cloud"][u].t().cpu().numpy() for u in range(B) if frustum_frame[u] == f]
        near = [np.array([d1[r, 0], d1[r, 1] - d1[r, 5] / 2.0, d1[r, 2]]) + rng.uniform(-2.5, 2.5, (150, 3))
                for r, u in zip(rows, unit) if frustum_frame[u] == f]
        xyz = np.concatenate(own + near, 0)
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1))], 1).astype(np.float32))
    fpts = _dev(np.concatenate(frames, 0))
    foff = _dev(np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64))
    cframe = np.asarray(frustum_frame)[unit]
    cands = cascade.refine_candidates(fpts, foff, dets1, rows.astype(np.int32), cframe.astype(np.int32), 1.2)
    print("first stage kept rows", rows.tolist(), "points per enlarged box", cands["counts"].tolist())
    assert (cands["counts"] > 0).any()
    np.random.seed(11)
    batch = builder.build_device(cands, [types[u] for u in unit])
    kept = batch.pop("kept")
    batch.pop("lens")
    ug2 = torch.from_numpy(ug.numpy()[unit[kept]].astype(np.int32)).to("cuda")
    want = m2.detect(batch, unit_group=ug2, num_groups=2, method="nms", thresh=0.1, top_k=6)
    # ---- the driver
    np.random.seed(11)
    two = cascade.TwoStageDetector(m1, m2, builder)
    res = two.detect(dd, fpts, foff, frustum_frame, types, "nms", 0.1, unit_group=ug, num_groups=2, top_k=6)
    torch.cuda.synchronize()
    for k, w in zip(("dets", "valid", "keep", "cnt"), want):
        assert torch.equal(res[k].cpu(), w.cpu()), k
    for a, w in zip(res["stage1"], (dets1, valid1, keep1, cnt1)):
        assert torch.equal(a.cpu(), w.cpu())
    assert np.array_equal(res["stage1_row"], rows[kept]) and res["stage1_row"].dtype == np.int64
    assert set(res["stage1_row"].tolist()) <= set(rows.tolist())           # every returned row is one stage 1 kept
    assert res["dets"].shape == (len(kept) * batch["center_ref2"].shape[2], 8)
    assert int(res["cnt"].sum()) > 0 and torch.isfinite(res["dets"]).all()
