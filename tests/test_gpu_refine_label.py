"""-m gpu: the refinement stage's training link -- fcn_refine_match, fcn_refine_label_count / _fill (csrc/refine_label.h) through
the C-ABI, cascade.match_detections / draw_box3d_jitter / refine_training_candidates against the reference's recorded run
(tests/golden/refine_label.npz), RefineInputBuilder.build_device_train against build() on host records, and one training step on
its batch.  The referee is the fp64 numpy restatement of tests/refine_label_ref.py, pinned to the reference by
tests/test_refine_label_referee.py, whose cached fixture and referee answer are shared here.  tests/test_emu_refine_label.py runs
the same functions on the host emulation of the kernels."""
import functools

import numpy as np
import pytest
import torch

import cascade_ref
import refine_label_ref as rr
from test_gpu_cascade import BADARG, NAN_PAYLOAD, _bits, _dev, _p
from test_gpu_cascade import _count as _select_count
from test_gpu_cascade import _fill as _select_fill
from test_refine_label_referee import BELOW, NO_LABEL, NO_POINT, NO_POSITIVE, TIE, golden, referee

pytestmark = pytest.mark.gpu
A = 3                              # the fixture's augmentX
SEG = 4096                         # fcn_frustum_select_seg(), asserted in _scene
IOU_BAR = 5e-5                     # the suite's bar for the float32 IoU core against fp64
KEYS = ("pts", "off", "dets", "crow", "cframe", "cgt", "gt", "goff", "jit")
PAYLOAD_ROW = 3                    # (frame 0) a row candidate 0 selects: its column 3 carries a NaN payload when there is one


def _seg_counts(index, S):
    """Per unit the number of its (frame-relative) rows in each of S segments."""
    return np.stack([np.bincount(np.asarray(ix, dtype=np.int64) // SEG, minlength=S)[:S] for ix in index]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def _scene(stride):
    """The fixture's scene with rows of `stride` floats; the referee's answer (shared, computed once) with per-segment counts."""
    from frustum_convnet_amd import _native
    assert _native.lib().fcn_frustum_select_seg() == SEG
    g, ref = golden(), dict(referee())
    pts = g["points"]
    if stride == 3:
        pts = np.ascontiguousarray(pts[:, :3])
    elif stride == 5:
        pts = np.concatenate([pts, np.random.RandomState(5).uniform(0, 1, (len(pts), 1)).astype(np.float32)], 1)
    else:
        pts = pts.copy()
    if stride > 3:
        i = int(ref["index"][0][PAYLOAD_ROW])
        pts[i:i + 1, 3].view(np.uint32)[0] = NAN_PAYLOAD
    S = 3
    ref["seg_cnt"] = _seg_counts(ref["index"], S)
    ref["seg_pos"] = _seg_counts([ix[p] for ix, p in zip(ref["index"], ref["positive"])], S)
    assert (ref["seg_cnt"][4 * A:5 * A] > 0).all() and (ref["seg_cnt"][4 * A:5 * A] % 64 != 0).all()      # every segment of frame 2
    return {"pts": pts, "off": g["off"], "dets": g["dets"], "crow": g["cand_row"], "cframe": g["cand_frame"],
            "cgt": g["ref_gt_idx"].astype(np.int32), "gt": g["gt_box3d"], "goff": g["gt_off"], "jit": g["jitter"], "ref": ref,
            "S": S, "g": g}


def _tensors(sc, **over):
    return {k: _dev(over.get(k, sc[k])) for k in KEYS}


def _rows(sc, units=None, caps=None):
    """The rows the fill must write for `units` (default all), unit after unit, optionally the first caps[u] of each."""
    ref, out = sc["ref"], []
    for u in (range(len(ref["index"])) if units is None else units):
        f = sc["cframe"][u // (len(ref["index"]) // len(sc["crow"]))]
        rows = sc["pts"][int(sc["off"][f]):][ref["index"][u]]
        out.append(rows if caps is None else rows[:caps[u]])
    return np.concatenate(out, 0) if out else np.zeros((0, sc["pts"].shape[1]), dtype=np.float32)


def _match(t, thresh=0.5):
    from frustum_convnet_amd import _native
    D = t["crow"].numel()
    gidx = torch.full((D,), -7, dtype=torch.int32, device="cuda")
    best = torch.full((D,), -7.0, dtype=torch.float32, device="cuda")
    rc = _native.lib().fcn_refine_match(_p(t["dets"]), t["dets"].shape[0], _p(t["crow"]), _p(t["cframe"]), D, _p(t["gt"]),
                                        t["gt"].shape[0], _p(t["goff"]), t["goff"].numel() - 1, thresh, _p(gidx), _p(best),
                                        _native.current_stream())
    torch.cuda.synchronize()
    return rc, gidx.cpu().numpy(), best.cpu().numpy()


def _common(t, S, jitter=True, ratio=1.2, shift=0.05):
    a = t["jit"].shape[1] if jitter else 1
    return [_p(t["pts"]), _p(t["off"]), t["off"].numel() - 1, t["pts"].shape[1], _p(t["dets"]), t["dets"].shape[0], _p(t["crow"]),
            _p(t["cframe"]), t["crow"].numel(), ratio, _p(t["cgt"]), _p(t["gt"]), t["gt"].shape[0], a,
            _p(t["jit"]) if jitter else None, shift, S]


def _outputs(U, S):
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    return {"scnt": torch.full((U, S), -7, **i32), "spos": torch.full((U, S), -7, **i32),
            "pred_box3d": torch.full((U, 8, 3), -7.0, **f64), "pred_angle": torch.full((U,), -7.0, **f64),
            "pred_size": torch.full((U, 3), -7.0, **f64), "box3d": torch.full((U, 8, 3), -7.0, **f64),
            "heading": torch.full((U,), -7.0, **f64), "size": torch.full((U, 3), -7.0, **f64)}


OUT_ORDER = ("scnt", "spos", "pred_box3d", "pred_angle", "pred_size", "box3d", "heading", "size")


def _count(t, S, jitter=True, ratio=1.2):
    """The raw labelled count on device tensors -> rc, outputs as numpy (sentinel-filled first)."""
    from frustum_convnet_amd import _native
    c = _common(t, S, jitter, ratio)
    o = _outputs(c[8] * c[13], S)
    rc = _native.lib().fcn_refine_label_count(*c, *[_p(o[k]) for k in OUT_ORDER], _native.current_stream())
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in o.items()}


def _fill(t, S, seg_counts, jitter=True, ratio=1.2, front=0, guard=5):
    """The raw labelled fill with slices of seg_counts rows behind `front` poisoned rows -> rc, the whole buffer (front + rows +
    guard), seg_off."""
    from frustum_convnet_amd import _native
    ps = t["pts"].shape[1]
    soff = (front + np.concatenate([[0], np.cumsum(np.asarray(seg_counts).reshape(-1))])).astype(np.int64)
    out = torch.full((int(soff[-1]) + guard, ps), -7.0, dtype=torch.float32, device="cuda")
    soff_d = _dev(soff)
    rc = _native.lib().fcn_refine_label_fill(*_common(t, S, jitter, ratio), _p(soff_d), _p(out), _native.current_stream())
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), soff


def _check_boxes(o, ref, g, units):
    """Jittered size and angle bit for bit, corners at cascade_ref.within's 1e-12 bar, label heading / size exact."""
    for u in units:
        d, a = divmod(u, A)
        assert np.array_equal(o["pred_size"][u], g["ref_box"][d, a, 3:6]), (u, o["pred_size"][u], g["ref_box"][d, a, 3:6])
        assert o["pred_angle"][u] == g["ref_box"][d, a, 6], (u, o["pred_angle"][u], g["ref_box"][d, a, 6])
        j = g["ref_gt_idx"][d]
        ext_p, ext_g = g["ref_box"][d, a, 3:6].max(), g["gt_box3d"][j, 3:6].max()
        for got, want, ext in ((o["pred_box3d"][u], g["ref_pred_corners"][u], ext_p), (o["box3d"][u], g["ref_gt_corners"][j], ext_g),
                               (o["pred_box3d"][u], ref["pred_box3d"][u], ext_p), (o["box3d"][u], ref["box3d"][u], ext_g)):
            assert cascade_ref.within(got, want, extent=ext), (u, cascade_ref.worst(got, want, ext))
        assert o["heading"][u] == g["gt_box3d"][j, 6] and np.array_equal(o["size"][u], g["gt_box3d"][j, 3:6])


@pytest.mark.parametrize("stride", [3, 4, 5, "unaligned4"])
def test_entry_points_match_the_referee(stride):
    sc = _scene(4 if stride == "unaligned4" else stride)
    ref, S, g = sc["ref"], sc["S"], sc["g"]
    t = _tensors(sc)
    if stride == "unaligned4":
        flat = torch.zeros(sc["pts"].size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = t["pts"].reshape(-1)
        t["pts"] = flat[1:].view(-1, 4)
        assert t["pts"].data_ptr() % 16 == 4
    # ---- match
    rc, gidx, best = _match(t, float(g["meta_thresh"]))
    assert rc == 0
    want_best = np.nan_to_num(np.nanmax(np.where(np.isnan(g["ref_iou"]), -1.0, g["ref_iou"]), 1).clip(0.0))
    print("gt_idx", gidx.tolist(), "best_iou worst abs err %.3e" % np.abs(best - want_best).max())
    assert np.array_equal(gidx, g["ref_gt_idx"]) and gidx[TIE] == 2 and gidx[BELOW] == -1 and gidx[NO_LABEL] == -1
    assert (np.abs(best - want_best) <= IOU_BAR).all() and best[NO_LABEL] == 0.0
    # ---- count
    rc, o = _count(t, S)
    assert rc == 0
    print("cnt", o["scnt"].sum(1).tolist(), "pos", o["spos"].sum(1).tolist())
    assert np.array_equal(o["scnt"], ref["seg_cnt"]) and np.array_equal(o["spos"], ref["seg_pos"])       # per segment
    matched = [u for u in range(len(sc["crow"]) * A) if sc["cgt"][u // A] >= 0]
    _check_boxes(o, ref, g, matched)
    for u in set(range(len(sc["crow"]) * A)) - set(matched):        # an unmatched candidate's units: counts 0, nothing else written
        assert all((o[k][u] == -7.0).all() for k in OUT_ORDER[2:]), u
    # ---- fill
    rc, buf, soff = _fill(t, S, o["scnt"], front=4)
    assert rc == 0
    want = _rows(sc)
    rows = buf[4:4 + len(want)]
    assert np.array_equal(_bits(rows), _bits(want))                  # bit-identical and in frame order, NaN payload included
    assert (buf[:4] == -7.0).all() and (buf[4 + len(want):] == -7.0).all() and len(buf) == 4 + len(want) + 5
    if sc["pts"].shape[1] > 3:
        assert (_bits(rows)[:, 3] == NAN_PAYLOAD).sum() >= 1
    assert np.isfinite(rows[:, :3]).all()
    assert np.array_equal(soff[::S] - 4, np.concatenate([[0], np.cumsum(ref["counts"])]))
    rc2, buf2, _ = _fill(t, S, o["scnt"], front=4)
    rc3, o3 = _count(t, S)
    assert rc2 == 0 and np.array_equal(_bits(buf2), _bits(buf))      # identical over two runs
    assert rc3 == 0 and all(np.array_equal(o3[k], o[k]) for k in o)
    # more segments than any frame needs: the surplus ones count 0
    rc, o5 = _count(t, S + 2)
    assert rc == 0 and np.array_equal(o5["scnt"][:, :S], ref["seg_cnt"]) and (o5["scnt"][:, S:] == 0).all()
    assert np.array_equal(o5["spos"][:, :S], ref["seg_pos"]) and (o5["spos"][:, S:] == 0).all()


@pytest.mark.parametrize("stride", [3, 4, 5])
def test_count_and_fill_over_the_frame_lengths_the_scan_turns_on(stride):
    """The cascade link's edge scene (frames of 0, 1, 63, 64, 65, 255, seg - 1, seg, seg + 1, 2 * seg + 100 rows, one candidate per
    frame) with every candidate's own row as its label box, one un-jittered copy: per-segment counts and positives equal the
    referee's, rows bit for bit and in order; at stride 4 a buffer that starts 4 bytes into an allocation (the word-by-word path)
    gives the aligned run's answer; offsets that grant nothing store nothing."""
    from test_gpu_cascade import _edge_scene
    es = _edge_scene(stride)
    D, S = len(es["crow"]), 3
    cgt, gt = np.arange(D, dtype=np.int32), es["dets"][:, :7].astype(np.float64)
    ref = rr.select_labeled(es["pts"], es["off"], es["dets"], es["crow"], es["cframe"], cgt, gt, None)
    want_cnt = _seg_counts(ref["index"], S)
    want_pos = _seg_counts([ix[p] for ix, p in zip(ref["index"], ref["positive"])], S)
    assert (want_cnt[-1] > 0).all() and 0 < want_pos.sum() < want_cnt.sum()
    want = np.concatenate([es["pts"][int(es["off"][f]):][ix] for f, ix in enumerate(ref["index"])], 0)
    t = {k: _dev(v) for k, v in dict(es, cgt=cgt, gt=gt).items() if k != "ref"}
    rc, o = _count(t, S, jitter=False)
    assert rc == 0 and np.array_equal(o["scnt"], want_cnt) and np.array_equal(o["spos"], want_pos)
    rc, buf, _ = _fill(t, S, o["scnt"], jitter=False)
    assert rc == 0 and np.array_equal(_bits(buf[:len(want)]), _bits(want)) and (buf[len(want):] == -7.0).all()
    if stride == 4:
        flat = torch.zeros(es["pts"].size + 1, dtype=torch.float32, device="cuda")
        flat[1:] = t["pts"].reshape(-1)
        tu = dict(t, pts=flat[1:].view(-1, 4))
        assert tu["pts"].data_ptr() % 16 == 4
        rc, ou = _count(tu, S, jitter=False)
        assert rc == 0 and all(np.array_equal(ou[k], o[k]) for k in o)
        rc, buf_u, _ = _fill(tu, S, ou["scnt"], jitter=False)
        assert rc == 0 and np.array_equal(_bits(buf_u), _bits(buf))
    rc, buf, _ = _fill(t, S, np.zeros_like(want_cnt), jitter=False)      # the empty grant
    assert rc == 0 and (buf == -7.0).all()


def test_one_copy_without_jitter_equals_the_unlabelled_selection():
    """A = 1 and jitter = NULL on the fixture's candidates against fcn_refine_select_count / _fill on the same candidates:
    counts, rows and pred_* bit-identical.  Every candidate is given a label row, so every unit selects."""
    sc = _scene(4)
    S = sc["S"]
    cgt = np.where(sc["cgt"] >= 0, sc["cgt"], 0).astype(np.int32)
    t = _tensors(sc, cgt=cgt)
    rc, o = _count(t, S, jitter=False)
    assert rc == 0
    rc, so = _select_count({"pts": t["pts"], "off": t["off"], "dets": t["dets"], "crow": t["crow"], "cframe": t["cframe"]})
    assert rc == 0
    cnt = so["cnt"].cpu().numpy()
    assert np.array_equal(o["scnt"].sum(1), cnt) and cnt.sum() > 500 and (cnt > 0).sum() >= 6
    for k in ("pred_box3d", "pred_angle", "pred_size"):
        assert np.array_equal(o[k], so[k].cpu().numpy()), k
    rc, buf, soff = _fill(t, S, o["scnt"], jitter=False, guard=5)
    assert rc == 0
    rc, rows, guard, _ = _select_fill({"pts": t["pts"], "off": t["off"], "dets": t["dets"], "crow": t["crow"], "cframe": t["cframe"]}, cnt)
    assert rc == 0 and np.array_equal(_bits(buf[:len(rows)]), _bits(rows)) and (buf[len(rows):] == -7.0).all()
    # positives: the un-enlarged label box, a subset of the selection
    ref1 = rr.select_labeled(sc["pts"], sc["off"], sc["dets"], sc["crow"], sc["cframe"], cgt, sc["gt"], None)
    assert np.array_equal(o["spos"].sum(1), ref1["pos"]) and np.array_equal(o["scnt"].sum(1), ref1["counts"])
    assert (o["spos"] <= o["scnt"]).all() and 0 < o["spos"].sum() < o["scnt"].sum()


def test_copies_chain_as_the_references_do():
    """Copy a of the device is the recorded reference chain (each copy perturbs the one before), not an independent perturbation
    of the un-jittered box: sizes and angles bit for bit against ref_box, and the independent variant differs."""
    sc = _scene(4)
    g = sc["g"]
    rc, o = _count(_tensors(sc), sc["S"])
    assert rc == 0
    differs = 0
    for d in np.nonzero(sc["cgt"] >= 0)[0]:
        for a in range(A):
            u = d * A + a
            assert np.array_equal(o["pred_size"][u], g["ref_box"][d, a, 3:6]) and o["pred_angle"][u] == g["ref_box"][d, a, 6], u
            if a:
                alone = rr.enlarged_chain(sc["dets"][sc["crow"][d]], sc["jit"][d][a:a + 1])[0]
                differs += int(not np.array_equal(alone[3:6], o["pred_size"][u]))
    assert differs == 12
    # copy 0 alone (A = 1 with the first draw of every candidate) equals copy 0 of the chain
    t1 = _tensors(sc, jit=np.ascontiguousarray(sc["jit"][:, :1]))
    rc, o1 = _count(t1, sc["S"])
    assert rc == 0 and np.array_equal(o1["pred_size"], o["pred_size"][::A]) and np.array_equal(o1["scnt"], o["scnt"][::A])


def test_points_exactly_on_a_face_are_inside_and_one_step_out_is_outside():
    """Axis-aligned boxes (ry = 0) with dyadic centres and sizes and ratio = 2: the enlarged box is x in [3, 5], y in [0.625, 1.125],
    z in [15.5, 16.5], the label box x in [3.5, 4.5], y in [0.75, 1], z in [15.75, 16.25].  Per face of each: one float32 step
    inside, exactly on it, one step outside."""
    dets = np.asarray([[4.0, 1.0, 16.0, 1.0, 0.5, 0.25, 0.0, 0.9]], dtype=np.float32)
    gt = np.asarray([[4.0, 1.0, 16.0, 1.0, 0.5, 0.25, 0.0]])
    centre = np.asarray([4.0, 0.875, 16.0], dtype=np.float32)
    rows, sel, pos = [], [], []
    for label, faces in ((False, ((3.0, 5.0), (0.625, 1.125), (15.5, 16.5))), (True, ((3.5, 4.5), (0.75, 1.0), (15.75, 16.25)))):
        for axis, (lo, hi) in enumerate(faces):
            for face, outward in ((lo, -np.inf), (hi, np.inf)):
                f32 = np.float32(face)
                assert float(f32) == face
                for val, inside in ((np.nextafter(f32, np.float32(-outward)), 1), (f32, 1), (np.nextafter(f32, np.float32(outward)), 0)):
                    p = centre.copy()
                    p[axis] = val
                    rows.append(p)
                    sel.append(1 if label else inside)               # a row at a label face is well inside the enlarged box
                    pos.append(inside if label else 0)               # a row at an enlarged face is outside the label box
    pts = np.concatenate([np.asarray(rows, dtype=np.float32), np.full((len(rows), 1), 0.5, dtype=np.float32)], 1)
    sel, pos = np.asarray(sel, dtype=bool), np.asarray(pos, dtype=bool)
    assert len(pts) == 36 and sel.sum() == 30 and pos.sum() == 12
    sc = {"pts": pts, "off": np.asarray([0, 36], dtype=np.int64), "dets": dets, "crow": np.zeros(1, np.int32),
          "cframe": np.zeros(1, np.int32), "cgt": np.zeros(1, np.int32), "gt": gt, "goff": np.asarray([0, 1], dtype=np.int64),
          "jit": np.zeros((1, 1, 7))}
    ref = rr.select_labeled(pts, sc["off"], dets, sc["crow"], sc["cframe"], sc["cgt"], gt, None, ratio=2.0)
    assert np.array_equal(ref["index"][0], np.nonzero(sel)[0]) and np.array_equal(ref["positive"][0], pos[sel])      # (the referee agrees)
    t = _tensors(sc)
    rc, o = _count(t, 1, jitter=False, ratio=2.0)
    assert rc == 0 and o["scnt"].tolist() == [[30]] and o["spos"].tolist() == [[12]]
    rc, buf, _ = _fill(t, 1, [[30]], jitter=False, ratio=2.0)
    assert rc == 0 and np.array_equal(_bits(buf[:30]), _bits(pts[sel])) and (buf[30:] == -7.0).all()
    assert np.array_equal(o["pred_box3d"][0], ref["pred_box3d"][0]) and np.array_equal(o["box3d"][0], ref["box3d"][0])   # cos 0, sin 0: exact
    assert o["pred_size"].tolist() == [[2.0, 1.0, 0.5]] and o["size"].tolist() == [[1.0, 0.5, 0.25]]


def test_slices_bound_the_stores():
    """seg_off bounds the writes: every slice is granted three rows fewer than its segment selects (valid calls: the surplus is
    dropped), behind 6 poisoned rows and before 5: each slice holds the first rows of its segment, its neighbours and both guards
    are untouched.  Then no slice is granted anything: nothing is written at all."""
    sc = _scene(4)
    S, ref = sc["S"], sc["ref"]
    t = _tensors(sc)
    caps = np.maximum(ref["seg_cnt"] - 3, 0)
    assert (ref["seg_cnt"] > 3).sum() > 20 and ((ref["seg_cnt"] > 0) & (ref["seg_cnt"] <= 3)).sum() >= 0
    rc, buf, soff = _fill(t, S, caps, front=6)
    assert rc == 0 and (buf[:6] == -7.0).all() and (buf[soff[-1]:] == -7.0).all() and len(buf) == soff[-1] + 5
    for u in range(len(caps)):
        f = sc["cframe"][u // A]
        for s in range(S):
            i = u * S + s
            idx = ref["index"][u][(ref["index"][u] // SEG) == s][:caps[u, s]]
            want = sc["pts"][int(sc["off"][f]):][idx]
            assert np.array_equal(_bits(buf[soff[i]:soff[i + 1]]), _bits(want)), (u, s)
    rc, buf, soff = _fill(t, S, np.zeros_like(caps), front=6)
    assert rc == 0 and soff[-1] == 6 and (buf == -7.0).all()


def _train_sel(sc=None, **kw):
    from frustum_convnet_amd import cascade
    sc = sc or _scene(4)
    t = _tensors(sc)
    return t, cascade.refine_training_candidates(t["pts"], t["off"], t["dets"], t["crow"], t["cframe"], t["cgt"], t["gt"],
                                                 jitter=kw.pop("jitter", t["jit"]), **kw)


def test_rejected_units_take_no_room():
    sc = _scene(4)
    ref, g = sc["ref"], sc["g"]
    t, sel = _train_sel(sc)
    kept = np.nonzero(ref["pos"] > 0)[0]
    assert np.array_equal(kept, np.nonzero(~g["ref_reject"])[0]) and len(kept) == 12
    assert np.array_equal(sel["kept"], kept) and sel["kept"].dtype == np.int64
    assert np.array_equal(sel["unit_cand"], kept // A) and sel["unit_cand"].dtype == np.int64
    assert not set(sel["unit_cand"].tolist()) & {BELOW, NO_LABEL, NO_POSITIVE, NO_POINT}
    counts = ref["counts"][kept]
    assert np.array_equal(sel["counts"], counts) and sel["counts"].dtype == np.int64
    assert np.array_equal(sel["cnt"].cpu().numpy(), counts) and sel["cnt"].dtype == torch.int32
    assert np.array_equal(sel["pos"].cpu().numpy(), ref["pos"][kept]) and sel["pos"].dtype == torch.int32
    off_h = sel["off"].cpu().numpy()
    assert np.array_equal(off_h, np.concatenate([[0], np.cumsum(counts)])) and sel["off"].dtype == torch.int64
    pts_h = sel["points"].cpu().numpy()
    assert sel["points"].dtype == torch.float32 and len(pts_h) == counts.sum()
    assert np.array_equal(_bits(pts_h), _bits(_rows(sc, kept)))      # the rejected units' rows are nowhere
    o = {k: sel[k].cpu().numpy() for k in ("pred_box3d", "pred_angle", "pred_size", "box3d", "heading", "size")}
    for k, u in enumerate(kept):
        d, a = divmod(int(u), A)
        assert np.array_equal(o["pred_size"][k], g["ref_box"][d, a, 3:6]) and o["pred_angle"][k] == g["ref_box"][d, a, 6]
        assert cascade_ref.within(o["pred_box3d"][k], g["ref_pred_corners"][u], extent=g["ref_box"][d, a, 3:6].max())
        j = g["ref_gt_idx"][d]
        assert cascade_ref.within(o["box3d"][k], g["ref_gt_corners"][j], extent=g["gt_box3d"][j, 3:6].max())
        assert o["heading"][k] == g["gt_box3d"][j, 6] and np.array_equal(o["size"][k], g["gt_box3d"][j, 3:6])
    for k in o:
        assert sel[k].dtype == torch.float64 and sel[k].is_cuda, k
    assert sorted(sel.keys()) == sorted(["points", "off", "pred_box3d", "pred_angle", "pred_size", "box3d", "heading", "size", "cnt",
                                         "pos", "kept", "unit_cand", "counts"])
    # the documented loop: the device's match feeds the selection
    from frustum_convnet_amd import cascade
    gidx, best = cascade.match_detections(t["dets"], t["crow"], t["cframe"], t["gt"], t["goff"], 0.5)
    assert gidx.dtype == torch.int32 and best.dtype == torch.float32 and np.array_equal(gidx.cpu().numpy(), sc["cgt"])
    sel2 = cascade.refine_training_candidates(t["pts"], t["off"], t["dets"], t["crow"], t["cframe"], gidx, t["gt"], jitter=sc["jit"])
    assert np.array_equal(sel2["kept"], kept) and np.array_equal(_bits(sel2["points"].cpu().numpy()), _bits(pts_h))


@pytest.mark.parametrize("what", ["row_high", "row_negative", "frame_high", "frame_negative", "gt_high"])
def test_out_of_range_candidate_is_reported_and_never_dereferenced(what):
    from frustum_convnet_amd import cascade, _native
    sc = _scene(4)
    S, ref, g = sc["S"], sc["ref"], sc["g"]
    crow, cframe, cgt = sc["crow"].copy(), sc["cframe"].copy(), sc["cgt"].copy()
    bad = 4                                                          # the candidate with rows in every segment
    if what.startswith("row"):
        crow[bad] = 10 if what == "row_high" else -(2 ** 31)         # R = 10
    elif what.startswith("frame"):
        cframe[bad] = 3 if what == "frame_high" else -1              # F = 3
    else:
        cgt[bad] = 7                                                 # G = 7
    t = _tensors(sc, crow=crow, cframe=cframe, cgt=cgt)              # exactly sized buffers: nothing beyond them can be read
    if what != "gt_high":
        rc, gidx, best = _match(t)
        want = g["ref_gt_idx"].copy()
        want[bad] = -1
        assert rc == BADARG and np.array_equal(gidx, want) and best[bad] == 0.0
        with pytest.raises(_native.NativeError):
            cascade.match_detections(t["dets"], t["crow"], t["cframe"], t["gt"], t["goff"], 0.5)
    rc, o = _count(t, S)
    assert rc == BADARG
    units = np.arange(bad * A, (bad + 1) * A)
    want_c, want_p = ref["seg_cnt"].copy(), ref["seg_pos"].copy()
    want_c[units], want_p[units] = 0, 0
    assert np.array_equal(o["scnt"], want_c) and np.array_equal(o["spos"], want_p)       # its counts are 0, the others are processed
    for k in OUT_ORDER[2:]:
        assert (o[k][units] == -7.0).all(), k                        # nothing else of it is written
    others = [u for u in range(len(crow) * A) if sc["cgt"][u // A] >= 0 and u // A != bad]
    _check_boxes(o, ref, g, others)
    rc, buf, soff = _fill(t, S, o["scnt"])
    assert rc == BADARG and (buf[soff[-1]:] == -7.0).all()
    keep = [u for u in range(len(crow) * A) if u // A != bad]
    assert np.array_equal(_bits(buf[:soff[-1]]), _bits(_rows(sc, keep)))
    with pytest.raises(_native.NativeError):
        cascade.refine_training_candidates(t["pts"], t["off"], t["dets"], t["crow"], t["cframe"], t["cgt"], t["gt"], jitter=t["jit"])


def test_bad_arguments_are_refused_with_nothing_written():
    from frustum_convnet_amd import _native
    sc = _scene(3)
    S = sc["S"]
    t = _tensors(sc)
    L, s = _native.lib(), _native.current_stream()
    U = t["crow"].numel() * A
    rc, o = _count(t, S)
    assert rc == 0
    w = _outputs(U, S)
    good = _common(t, S) + [_p(w[k]) for k in OUT_ORDER] + [s]
    # arguments: 0 pts 1 off 2 F 3 stride 4 dets 5 R 6 crow 7 cframe 8 D 9 ratio 10 cgt 11 gt 12 G 13 A 14 jitter 15 shift 16 S
    for i in (0, 1, 4, 6, 7, 10, 11, 14, 17, 18, 19, 20, 21, 22, 23, 24):       # NULL pointers (NULL jitter with A = 3 among them)
        bad = list(good)
        bad[i] = None
        assert L.fcn_refine_label_count(*bad) == BADARG, i
    # pt_stride 2, S < 1, S too small for the longest frame, A out of range, negative sizes, more than 65535 units
    for i, v in ((3, 2), (16, 0), (16, -1), (16, S - 1), (13, 0), (13, 65), (13, -1), (8, -1), (2, -1), (5, -1), (12, -1), (8, 21846)):
        bad = list(good)
        bad[i] = v
        assert L.fcn_refine_label_count(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert all((w[k].cpu().numpy() == -7).all() for k in w)          # nothing written by any of them
    assert L.fcn_refine_label_count(*good) == 0                      # (the same list is accepted when nothing is wrong)
    torch.cuda.synchronize()
    assert all(np.array_equal(w[k].cpu().numpy(), o[k]) for k in o)
    soff = _dev(np.concatenate([[0], np.cumsum(o["scnt"].reshape(-1))]).astype(np.int64))
    out = torch.full((int(o["scnt"].sum()), 3), -7.0, dtype=torch.float32, device="cuda")
    goodf = good[:17] + [_p(soff), _p(out), s]
    for i in (0, 1, 4, 6, 7, 10, 11, 14, 17, 18):
        bad = list(goodf)
        bad[i] = None
        assert L.fcn_refine_label_fill(*bad) == BADARG, i
    for i, v in ((3, 2), (16, 0), (16, S - 1), (13, 0), (13, 65), (8, -1), (2, -1), (8, 21846)):
        bad = list(goodf)
        bad[i] = v
        assert L.fcn_refine_label_fill(*bad) == BADARG, (i, v)
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()
    assert L.fcn_refine_label_fill(*goodf) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(_rows(sc)))
    # the match
    gidx = torch.full((8,), -7, dtype=torch.int32, device="cuda")
    best = torch.full((8,), -7.0, dtype=torch.float32, device="cuda")
    goodm = [_p(t["dets"]), 10, _p(t["crow"]), _p(t["cframe"]), 8, _p(t["gt"]), 7, _p(t["goff"]), 3, 0.5, _p(gidx), _p(best), s]
    for i in (0, 2, 3, 5, 7, 10, 11):
        bad = list(goodm)
        bad[i] = None
        assert L.fcn_refine_match(*bad) == BADARG, i
    for i in (1, 4, 6, 8):
        bad = list(goodm)
        bad[i] = -1
        assert L.fcn_refine_match(*bad) == BADARG, i
    torch.cuda.synchronize()
    assert (gidx.cpu().numpy() == -7).all() and (best.cpu().numpy() == -7.0).all()
    # a NaN threshold matches nothing
    rc, gi, _ = _match(t, float("nan"))
    assert rc == 0 and (gi == -1).all()


def test_empty_results_launch_nothing_behind_them():
    from frustum_convnet_amd import cascade, _native
    sc = _scene(4)
    t = _tensors(sc)
    S = sc["S"]
    L = _native.lib()
    calls = []
    real = L.fcn_refine_label_fill
    none = [NO_POSITIVE, NO_POINT]
    try:
        L.fcn_refine_label_fill = lambda *a: calls.append(a) or real(*a)
        run = lambda **kw: cascade.refine_training_candidates(
            kw.get("pts", t["pts"]), kw.get("off", t["off"]), t["dets"], kw.get("crow", t["crow"]), kw.get("cframe", t["cframe"]),
            kw.get("cgt", t["cgt"]), t["gt"], jitter=kw.get("jit", t["jit"]))
        # only units the reject rule drops
        sel = run(crow=sc["crow"][none], cframe=sc["cframe"][none], cgt=sc["cgt"][none], jit=sc["jit"][none])
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and sel["kept"].dtype == np.int64 and calls == []
        # only unmatched candidates
        sel = run(cgt=np.full(8, -1, np.int32))
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and calls == []
        # D = 0
        sel = run(crow=np.zeros(0, np.int32), cframe=np.zeros(0, np.int32), cgt=np.zeros(0, np.int32), jit=np.zeros((0, A, 7)))
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and calls == []
        # F = 0: no frame to search
        sel = run(pts=torch.zeros((0, 4), dtype=torch.float32, device="cuda"), off=np.zeros(1, np.int64))
        assert list(sel.keys()) == ["kept"] and len(sel["kept"]) == 0 and calls == []
        ok = run()
        assert len(calls) == 1 and len(ok["kept"]) == 12             # (the spy sees the launch when there is one)
    finally:
        L.fcn_refine_label_fill = real
    assert list(_builder(64).build_device_train(sel, []).keys()) == ["kept"]
    gi, bi = cascade.match_detections(t["dets"], np.zeros(0, np.int32), np.zeros(0, np.int32), t["gt"], t["goff"], 0.5)
    assert gi.numel() == 0 and bi.numel() == 0
    # the entry points themselves: D = 0 touches nothing, F = 0 zeroes both counts (match: -1 and 0)
    t0 = dict(t, crow=_dev(np.zeros(0, np.int32)), cframe=_dev(np.zeros(0, np.int32)), cgt=_dev(np.zeros(0, np.int32)),
              jit=_dev(np.zeros((0, A, 7))))
    rc, o = _count(t0, S)
    assert rc == 0 and o["scnt"].size == 0
    rc, buf, _ = _fill(t0, S, np.zeros((0, S), np.int64))
    assert rc == 0 and (buf == -7.0).all()
    tf = dict(t, off=_dev(np.zeros(1, np.int64)), goff=_dev(np.zeros(1, np.int64)))
    rc, o = _count(tf, S)
    assert rc == 0 and (o["scnt"] == 0).all() and (o["spos"] == 0).all() and (o["pred_size"] == -7.0).all() and (o["box3d"] == -7.0).all()
    rc, buf, _ = _fill(tf, S, np.zeros((8 * A, S), np.int64))
    assert rc == 0 and (buf == -7.0).all()
    rc, gi, bi = _match(tf)
    assert rc == 0 and (gi == -1).all() and (bi == 0.0).all()


def test_label_boxes_as_their_own_candidates():
    """extract_frustum_data (:239-403): every label box is its own candidate, no matching -- the label rows as dets rows (their
    float32 casts), cand_gt = arange.  Against the referee, with jitter (A = 2)."""
    from frustum_convnet_amd import cascade
    sc = _scene(4)
    g = sc["g"]
    gt = g["gt_box3d"].astype(np.float32).astype(np.float64)         # float32-representable labels: dets and gt are the same boxes
    G = len(gt)
    dets = np.concatenate([gt, np.ones((G, 1))], 1).astype(np.float32)
    cframe = (np.searchsorted(g["gt_off"], np.arange(G), side="right") - 1).astype(np.int32)
    crow = cgt = np.arange(G, dtype=np.int32)
    jit = np.random.RandomState(8).random_sample((G, 2, 7))
    ref = rr.select_labeled(sc["pts"], sc["off"], dets, crow, cframe, cgt, gt, jit)
    sel = cascade.refine_training_candidates(_dev(sc["pts"]), _dev(sc["off"]), _dev(dets), crow, cframe, cgt, gt, jitter=jit)
    kept = np.nonzero(ref["pos"] > 0)[0]
    assert len(kept) >= 6 and np.array_equal(sel["kept"], kept) and np.array_equal(sel["unit_cand"], kept // 2)
    assert np.array_equal(sel["counts"], ref["counts"][kept]) and np.array_equal(sel["pos"].cpu().numpy(), ref["pos"][kept])
    want = np.concatenate([sc["pts"][int(sc["off"][cframe[u // 2]]):][ref["index"][u]] for u in kept], 0)
    assert np.array_equal(_bits(sel["points"].cpu().numpy()), _bits(want))
    assert np.array_equal(sel["pred_size"].cpu().numpy(), ref["pred_size"][kept])
    assert np.array_equal(sel["pred_angle"].cpu().numpy(), ref["pred_angle"][kept])
    assert np.array_equal(sel["size"].cpu().numpy(), gt[kept // 2, 3:6]) and np.array_equal(sel["heading"].cpu().numpy(), gt[kept // 2, 6])
    for k, u in enumerate(kept):
        assert cascade_ref.within(sel["pred_box3d"][k].cpu().numpy(), ref["pred_box3d"][u], extent=ref["pred_size"][u].max())
        assert cascade_ref.within(sel["box3d"][k].cpu().numpy(), ref["box3d"][u], extent=ref["size"][u].max())
    # un-jittered, every label box holds its own points: positives == the rows inside the box
    sel1 = cascade.refine_training_candidates(_dev(sc["pts"]), _dev(sc["off"]), _dev(dets), crow, cframe, cgt, gt)
    ref1 = rr.select_labeled(sc["pts"], sc["off"], dets, crow, cframe, cgt, gt, None)
    assert np.array_equal(sel1["kept"], np.nonzero(ref1["pos"] > 0)[0]) and np.array_equal(sel1["pos"].cpu().numpy(), ref1["pos"][sel1["kept"]])


def _builder(npoints, **kw):
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    reset_cfg()
    return inputs.RefineInputBuilder(npoints, strides=(0.1, 0.2, 0.4, 0.8), **kw)


def _records(sel, types):
    """Host records of build() from the DOWNLOADED training candidates."""
    h = {k: sel[k].cpu().numpy() for k in ("points", "off", "pred_box3d", "pred_angle", "pred_size", "box3d", "heading", "size")}
    off = h["off"]
    return [{"points": h["points"][off[k]:off[k + 1]], "box3d": h["box3d"][k], "heading": float(h["heading"][k]), "size": h["size"][k],
             "pred_box3d": h["pred_box3d"][k], "pred_angle": float(h["pred_angle"][k]), "pred_size": h["pred_size"][k],
             "type": types[d]} for k, d in enumerate(sel["unit_cand"])]


def test_build_device_train_equals_build_on_host_records():
    """RefineInputBuilder.build_device_train on the device candidates against build(records) on host records made from the
    DOWNLOADED candidates, same draws, flip and shift on: the same launch on the same numbers, every key bit-identical."""
    from frustum_convnet_amd import inputs
    sc = _scene(4)
    _, sel = _train_sel(sc)
    N = 128
    b = _builder(N, random_flip=True, random_shift=True)
    types = [str(x) for x in sc["g"]["types"]]
    counts = sel["counts"]
    assert (counts < N).any() and (counts > N).any()                 # both resample modes
    draws = inputs.draw_refine(counts, N, True, True, rng=np.random.RandomState(3))
    assert (draws[1] > 0.5).any() and (draws[1] <= 0.5).any()        # flipped and unflipped samples
    got = b.build_device_train(sel, types, draws=draws)
    want = b.build(_records(sel, types), draws=draws)
    torch.cuda.synchronize()
    assert sorted(got.keys()) == sorted(want.keys())
    assert sorted(got.keys()) == sorted(["cls_label", "box3d_center", "box3d_heading", "box3d_size", "size_class", "one_hot",
                                         "center_ref1", "center_ref2", "center_ref3", "center_ref4", "point_cloud", "rot_angle",
                                         "ref_center", "lens"])
    for k in want:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert torch.equal(got[k].cpu(), want[k].cpu()), k
    assert ((got["cls_label"].cpu().numpy() == 1).sum(1) >= 1).all()  # a 1 in every row
    assert len(set(got["size_class"].cpu().numpy().ravel().tolist())) == 2      # Car and Pedestrian survive
    assert len(set(got["lens"].cpu().numpy()[:, 0].tolist())) > 1     # different window counts: the padding is exercised
    # drawn like the reference when no draws are given
    np.random.seed(5)
    got4 = b.build_device_train(sel, types)
    np.random.seed(5)
    want4 = b.build(_records(sel, types))
    assert all(torch.equal(got4[k].cpu(), want4[k].cpu()) for k in want4)


def test_draw_box3d_jitter_reproduces_the_references_draws():
    from frustum_convnet_amd import cascade
    g = golden()
    matched = np.nonzero(g["ref_gt_idx"] >= 0)[0]
    np.random.seed(int(g["meta_seed"]))
    draws = cascade.draw_box3d_jitter(len(matched), A)
    nxt = np.random.random()
    assert draws.shape == (6, A, 7) and draws.dtype == np.float64
    assert np.array_equal(draws, g["ref_draws"]) and nxt == float(g["ref_next_draw"])        # the numbers, and the generator's state
    jitter = np.zeros((8, A, 7))
    jitter[matched] = draws                                           # the documented loop: rows of unmatched candidates stay unread
    assert np.array_equal(jitter, g["jitter"])
    rs = np.random.RandomState(int(g["meta_seed"]))
    assert np.array_equal(cascade.draw_box3d_jitter(6, A, rng=rs), g["ref_draws"])
    assert cascade.draw_box3d_jitter(0, A).shape == (0, A, 7)


def test_one_training_step_on_the_device_built_batch():
    """The hash-initialised refine_b4_n512 model: one step on the build_device_train batch gives finite losses and gradients and
    moves the parameters; the losses equal those from the build(records) batch bit for bit."""
    from helpers import load_golden
    from test_gpu_model import _model
    from frustum_convnet_amd import inputs
    sc = _scene(4)
    _, sel = _train_sel(sc)
    g2 = load_golden("refine_b4_n512")
    m = _model(g2).train()                                            # (cfg now holds the refine strides: the builder reads them)
    b = inputs.RefineInputBuilder(int(g2["meta_npoint"]), random_flip=True, random_shift=True)
    types = [str(x) for x in sc["g"]["types"]]
    draws = inputs.draw_refine(sel["counts"], b.npoints, True, True, rng=np.random.RandomState(4))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    batch = b.build_device_train(sel, types, draws=draws)
    batch.pop("lens")
    losses, _ = m(batch)
    losses["total_loss"].backward()
    torch.cuda.synchronize()
    params = [p for p in m.parameters() if p.grad is not None]
    assert params and all(torch.isfinite(p.grad).all() for p in params)
    got = {k: v.detach().cpu().clone() for k, v in losses.items()}
    before = [p.detach().clone() for p in params]
    torch.optim.SGD(params, lr=1e-2).step()
    torch.cuda.synchronize()
    assert any(not torch.equal(p.detach(), q) for p, q in zip(params, before))
    assert all(torch.isfinite(p).all() for p in params)
    m.load_state_dict(sd)                                             # (the parameters and the running statistics moved)
    batch2 = b.build(_records(sel, types), draws=draws)
    batch2.pop("lens")
    losses2, _ = m(batch2)
    torch.cuda.synchronize()
    print({k: float(v) for k, v in got.items()})
    for k, v in losses2.items():
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], v.detach().cpu()), k
    assert float(got["total_loss"]) > 0
