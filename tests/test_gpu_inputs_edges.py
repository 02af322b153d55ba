"""-m gpu: the two batch-builder kernels of csrc/inputs.hip (prepare_inputs_kernel behind fcn_prepare_inputs / _infer / _sunrgbd / _sunrgbd_infer,
prepare_inputs_refine_kernel behind fcn_prepare_inputs_refine) OFF their recorded fixtures: the nearest-centre fallback on the last
real window of a padded row, one window next to many, more windows than threads (a thread's second trip, the cross-thread
(distance, index) reduction), exact distance ties, centres exactly on a box face, both clamps of both shifts, a coin of exactly
0.5, every flip / shift setting, SUN-RGBD without the height-shift pointer and with boxes that fall back through K and Rtilt,
B = 1, N = 1, N below / at / above a record's point count, the inference forms of both kernels, launches into poisoned buffers,
every refusal of the five C entries -- and RefineInputBuilder's refusal of a sample without a window.

The cases (records, draws, expected batch) come from tests/inputs_cases.py; the referee is always oracle/inputs_ref.py: integer
outputs exact, float outputs within 1e-6 * max(1, |ref|.max()) (fp64 arithmetic rounded to fp32 on both sides), the worst float
distance of every case printed.  The same functions run on the host emulation (tests/test_emu_gpu_subset.py); the barrier and
visibility order between thread 0's fallback store and the padding copy is only real on the hardware."""
import ctypes

import numpy as np
import pytest
import torch

import inputs_cases as ic

pytestmark = pytest.mark.gpu

FCN_E_BADARG = 10001
SENT64, SENT32 = -6510615555426900571, -1515870811        # 0xA5A5... as int64 / int32: no label, count or class looks like it


# ---------------------------------------------------------------------------------------------------------------- compare
def _compare(name, out, want, float_keys, int_keys):
    for k in int_keys:
        ref = np.asarray(want[k])
        got = out[k].cpu().numpy()
        assert got.shape == ref.shape and got.dtype == ref.dtype, (name, k, got.shape, got.dtype, ref.shape, ref.dtype)
        assert np.array_equal(got, ref), (name, k, np.argwhere(got != ref)[:8].tolist())
    worst, fails = ("", 0.0), []
    for k in float_keys:
        ref = np.asarray(want[k])
        assert out[k].dtype == torch.float32 and out[k].numel() == ref.size, (name, k, tuple(out[k].shape), ref.shape)
        got = out[k].cpu().numpy().reshape(ref.shape)
        d = float(np.abs(got.astype(np.float64) - ref.astype(np.float64)).max())
        bar = 1e-6 * max(1.0, float(np.abs(ref).max()))
        if d / bar >= worst[1]:
            worst = (k, d / bar)
        if not d <= bar:
            fails.append((k, d, bar))
    print("%s: worst float distance %.3e of its bar (%s)" % (name, worst[1], worst[0]))
    assert not fails, (name, fails)


def _builder(case):
    from frustum_convnet_amd import inputs
    from frustum_convnet_amd.config import reset_cfg
    reset_cfg()
    kw = dict(random_flip=case["flip"], random_shift=case["shift"])
    if case["kind"] == "refine":
        return inputs.RefineInputBuilder(case["npoints"], strides=case["strides"], **kw)
    cls = inputs.InputBuilder if case["kind"] == "kitti" else inputs.SunrgbdInputBuilder
    return cls(case["npoints"], case["strides"], case["max_depth"], **kw)


def _run(name):
    case = ic.built(name)
    out = _builder(case).build(ic.records(case), draws=ic.draws(case))
    torch.cuda.synchronize()
    if case["kind"] == "refine":
        _compare(name, out, case["want"], ic.REFINE_FLOAT_KEYS, ("cls_label", "lens", "size_class"))
    else:
        keys = ic.KITTI_FLOAT_KEYS if case["kind"] == "kitti" else ic.SUNRGBD_FLOAT_KEYS
        _compare(name, out, case["want"], keys, ("cls_label", "seg_label", "size_class"))
    return case, out


@pytest.mark.parametrize("name", list(ic.REFINE_CASES))
def test_refine_case(name):
    case, out = _run(name)
    want = case["want"]
    for s in range(4):                                    # the padded shapes are the batch maxima of the per-sample counts
        assert out["center_ref%d" % (s + 1)].shape == (len(want["lens"]), 3, int(want["lens"][:, s].max()))
    assert out["cls_label"].shape[1] == int(want["lens"][:, 1].max())


@pytest.mark.parametrize("name", list(ic.KITTI_CASES))
def test_first_stage_case(name):
    _run(name)


@pytest.mark.parametrize("name", list(ic.SUNRGBD_CASES))
def test_sunrgbd_matrix(name):
    _run(name)


# ----------------------------------------------------------------------------------------------------------- raw C entries
def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _inputs(case):
    """The case's records and draws as the device tensors the C entries take."""
    rec = case["rec"]
    f64 = lambda k, shape: _dev(np.asarray(rec[k], dtype=np.float64).reshape(shape))
    B = len(rec["raw_counts"])
    t = {"raw": _dev(rec["raw_points"]), "off": _dev(np.concatenate([[0], np.cumsum(rec["raw_counts"])]).astype(np.int64)),
         "choice": _dev(np.asarray(rec["draw_choice"], dtype=np.int32)), "corners": f64("box3d_corners", (B, 24)),
         "heading": f64("heading", (B,)), "size": f64("size", (B, 3)), "coin": f64("draw_coin", (B,)),
         "normal": f64("draw_normal", (B,))}
    if case["kind"] == "refine":
        t.update(pcorners=f64("pred_corners", (B, 24)), pangle=f64("pred_angle", (B,)), psize=f64("pred_size", (B, 3)))
    else:
        t.update(raw_seg=_dev(np.asarray(rec["raw_seg"], dtype=np.int64)), fangle=f64("frustum_angle", (B,)), box2d=f64("box2d", (B, 4)))
        if case["kind"] == "kitti":
            t["P"] = f64("P", (B, 12))
        else:
            t.update(K=f64("K", (B, 9)), Rtilt=f64("Rtilt", (B, 9)), hshift=f64("draw_hshift", (B,)))
    return t


def _poisoned(case, labels=True):
    """Every output of the case's entry, pre-filled: NaN in the floats, a sentinel in the integers."""
    want, B, N = case["want"], len(case["rec"]["raw_counts"]), case["npoints"]
    nsc = len(case["strides"])
    Ls = [want["center_ref%d" % (s + 1)].shape[-1] for s in range(nsc)]
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    out = {"point_cloud": nan(B, 3, N), "rot_angle": nan(B, 1)}
    for s in range(nsc):
        out["center_ref%d" % (s + 1)] = nan(B, 3, Ls[s])
    if labels:
        out.update(cls_label=torch.full((B, Ls[1]), SENT64, dtype=torch.int64, device="cuda"), box3d_center=nan(B, 3),
                   box3d_heading=nan(B, 1), box3d_size=nan(B, 3))
    if case["kind"] == "refine":
        out.update(ref_center=nan(B, 3), lens=torch.full((B, 4), SENT32, dtype=torch.int32, device="cuda"))
    elif labels:
        out["seg_label"] = torch.full((B, N), SENT64, dtype=torch.int64, device="cuda")
    return out, Ls


def _bits(t):
    return t.contiguous().view(torch.int32).cpu().clone() if t.dtype == torch.float32 else t.cpu().clone()


def _snapshot(out):
    return {k: _bits(v) for k, v in out.items()}


def _untouched(out, before, what):
    torch.cuda.synchronize()
    for k, v in out.items():
        assert torch.equal(_bits(v), before[k]), "%s: a refused call wrote to %s" % (what, k)


def _call(entry, case, t, out, Ls, desc=None, null=()):
    """One call of a C entry on the case's tensors.  desc: descriptor fields to override ('L0'..'L4' / 'stride0'..: one element);
    null: argument names handed over as NULL ('center_ref2': that element of the pointer array)."""
    from frustum_convnet_amd import _native
    desc = dict(desc or {})
    nsc = len(case["strides"])
    B, N, ps = len(case["rec"]["raw_counts"]), case["npoints"], int(case["rec"]["raw_points"].shape[1])
    L, st = list(Ls), list(case["strides"])
    for s in range(nsc):
        L[s], st[s] = desc.pop("L%d" % s, L[s]), desc.pop("stride%d" % s, st[s])
    B, N, ps = desc.pop("B", B), desc.pop("N", N), desc.pop("pt_stride", ps)
    flip, shift = desc.pop("random_flip", int(case["flip"])), desc.pop("random_shift", int(case["shift"]))
    assert not desc, desc
    ci, cd = ctypes.c_int32 * nsc, ctypes.c_double * nsc
    if entry == "fcn_prepare_inputs_refine":
        d = _native.InpRefineDesc(B, N, ps, ci(*L), cd(*st), flip, shift)
    else:
        d = (_native.Inp5Desc if nsc == 5 else _native.InpDesc)(B, N, ps, ci(*L), cd(*st), case.get("max_depth", 0.0), flip, shift)
    both = dict(t, **out)
    p = lambda k: None if (k in null or both.get(k) is None) else both[k].data_ptr()
    refs = (ctypes.c_void_p * nsc)(*[p("center_ref%d" % (s + 1)) for s in range(nsc)])
    head = ["raw", "off"]
    tail = ["cls_label", "box3d_center", "box3d_heading", "box3d_size", "rot_angle"]
    if entry == "fcn_prepare_inputs":
        names = head + ["raw_seg", "choice", "fangle", "box2d", "P", "corners", "heading", "size", "coin", "normal", "point_cloud",
                        refs] + tail + ["seg_label"]
    elif entry == "fcn_prepare_inputs_infer":
        names = head + ["choice", "fangle", "box2d", "P", "point_cloud", refs, "rot_angle"]
    elif entry == "fcn_prepare_inputs_sunrgbd_infer":
        names = head + ["choice", "fangle", "box2d", "K", "Rtilt", "point_cloud", refs, "rot_angle"]
    elif entry == "fcn_prepare_inputs_sunrgbd":
        names = head + ["raw_seg", "choice", "fangle", "box2d", "K", "Rtilt", "corners", "heading", "size", "coin", "normal", "hshift",
                        "point_cloud", refs] + tail + ["seg_label"]
    else:
        names = head + ["choice", "pcorners", "pangle", "psize", "corners", "heading", "size", "coin", "normal", "point_cloud",
                        refs] + tail + ["ref_center", "lens"]
    args = [p(a) if isinstance(a, str) else a for a in names]
    dev = t["raw"].device
    with torch.cuda.device(dev):
        return getattr(_native.lib(), entry)(None if "desc" in null else ctypes.byref(d), *args, _native.current_stream(dev))


def test_refine_inference_form():
    """build(..., with_labels=False) -- corners == NULL in the kernel -- equals, bit for bit, the training batch's points, window
    centres, rot_angle, ref_center and lens built with flip and shift off, and carries no label key.  (The training side of that
    comparison is checked against the oracle by test_refine_case[flip_shift_matrix-f0s0].)"""
    case = ic.built("flip_shift_matrix-f0s0")
    b = _builder(case)
    train = b.build(ic.records(case), draws=ic.draws(case))
    infer = b.build(ic.records(case), draws=ic.draws(case), with_labels=False)
    # a builder with both augmentations ON builds the same inference batch: the switches only act on labelled records
    on = ic.built("flip_shift_matrix-f1s1")
    infer_on = _builder(on).build(ic.records(on), draws=ic.draws(on), with_labels=False)
    torch.cuda.synchronize()
    for k in ("point_cloud", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "rot_angle", "ref_center", "lens"):
        assert torch.equal(_bits(infer[k]), _bits(train[k])), k
        assert torch.equal(_bits(infer_on[k]), _bits(train[k])), k
    for k in ("cls_label", "box3d_center", "box3d_heading", "box3d_size", "size_class"):
        assert k not in infer and k not in infer_on, k
    _compare("inference_form", infer, case["want"], ("point_cloud", "center_ref1", "center_ref2", "center_ref3", "center_ref4",
                                                     "rot_angle", "ref_center"), ("lens",))


@pytest.mark.parametrize("name", ["fallback_last_padded-off", "fallback_last_padded-on"])
def test_refine_every_element_written(name):
    """A direct launch into buffers pre-filled with NaN / a sentinel: no element keeps its poison, the padding of the window
    centres and of the label rows included; the result is the oracle's; a second launch into the same buffers reproduces the
    first bit for bit."""
    case = ic.built(name)
    t = _inputs(case)
    out, Ls = _poisoned(case)
    assert Ls == [16, 8, 4, 2]
    assert _call("fcn_prepare_inputs_refine", case, t, out, Ls) == 0
    torch.cuda.synchronize()
    first = _snapshot(out)
    for k, v in out.items():
        if v.dtype == torch.float32:
            assert not bool(torch.isnan(v).any()), k
        else:
            assert not bool((v == (SENT32 if v.dtype == torch.int32 else SENT64)).any()), k
    want = dict(case["want"])
    _compare(name + " (poisoned buffers)", out, want, ic.REFINE_FLOAT_KEYS, ("cls_label", "lens"))
    assert _call("fcn_prepare_inputs_refine", case, t, out, Ls) == 0
    torch.cuda.synchronize()
    for k, v in _snapshot(out).items():
        assert torch.equal(v, first[k]), k


def _kitti_fixture_case(flip=False, shift=False):
    g = ic.fixture("inputs_kitti_b6")
    case = dict(name="kitti_fixture", kind="kitti", rec=g, npoints=int(g["meta_npoint"]), strides=tuple(float(s) for s in g["meta_strides"]),
                max_depth=float(g["meta_max_depth"]), flip=flip, shift=shift)
    return ic._expected(case)


def test_kitti_infer_entry():
    """fcn_prepare_inputs_infer (the kernel with corners == NULL) on the fixture records equals the training entry's point_cloud,
    center_ref1..4 and rot_angle with flip and shift off, bit for bit -- in poisoned buffers, every element written --, and
    refuses a descriptor that asks for flip or shift."""
    case = _kitti_fixture_case()
    t = _inputs(case)
    train, Ls = _poisoned(case)
    assert _call("fcn_prepare_inputs", case, t, train, Ls) == 0
    infer, _ = _poisoned(case, labels=False)
    assert _call("fcn_prepare_inputs_infer", case, t, infer, Ls) == 0
    torch.cuda.synchronize()
    assert sorted(infer) == ["center_ref1", "center_ref2", "center_ref3", "center_ref4", "point_cloud", "rot_angle"]
    for k, v in infer.items():
        assert not bool(torch.isnan(v).any()), k
        assert torch.equal(_bits(v), _bits(train[k])), k
    _compare("kitti_infer_entry (training entry)", train, case["want"], ic.KITTI_FLOAT_KEYS, ("cls_label", "seg_label"))
    before = _snapshot(infer)
    assert _call("fcn_prepare_inputs_infer", case, t, infer, Ls, desc=dict(random_flip=1)) == FCN_E_BADARG
    assert _call("fcn_prepare_inputs_infer", case, t, infer, Ls, desc=dict(random_shift=1)) == FCN_E_BADARG
    _untouched(infer, before, "fcn_prepare_inputs_infer")


def test_sunrgbd_infer_entry():
    """fcn_prepare_inputs_sunrgbd_infer (the kernel with corners == NULL, centres through K and Rtilt) on the SUN-RGBD fixture's
    records equals the training entry's point_cloud, center_ref1..5 and rot_angle with flip and shift off, bit for bit -- in
    poisoned buffers, every element written --, and refuses a descriptor that asks for flip or shift."""
    case = ic.built("sunrgbd-f0s0-rec-n257")
    t = _inputs(case)
    train, Ls = _poisoned(case)
    assert _call("fcn_prepare_inputs_sunrgbd", case, t, train, Ls) == 0
    infer, _ = _poisoned(case, labels=False)
    assert _call("fcn_prepare_inputs_sunrgbd_infer", case, t, infer, Ls) == 0
    torch.cuda.synchronize()
    assert sorted(infer) == ["center_ref1", "center_ref2", "center_ref3", "center_ref4", "center_ref5", "point_cloud", "rot_angle"]
    for k, v in infer.items():
        assert not bool(torch.isnan(v).any()), k
        assert torch.equal(_bits(v), _bits(train[k])), k
    _compare("sunrgbd_infer_entry (training entry)", train, case["want"], ic.SUNRGBD_FLOAT_KEYS, ("cls_label", "seg_label"))
    before = _snapshot(infer)
    assert _call("fcn_prepare_inputs_sunrgbd_infer", case, t, infer, Ls, desc=dict(random_flip=1)) == FCN_E_BADARG
    assert _call("fcn_prepare_inputs_sunrgbd_infer", case, t, infer, Ls, desc=dict(random_shift=1)) == FCN_E_BADARG
    _untouched(infer, before, "fcn_prepare_inputs_sunrgbd_infer")


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusal_case(entry):
    if entry == "fcn_prepare_inputs_refine":
        return ic.built("fallback_last_padded-on")
    if entry in ("fcn_prepare_inputs_sunrgbd", "fcn_prepare_inputs_sunrgbd_infer"):
        return ic.built("sunrgbd-f1s1-rec-n257")
    return ic.built("kitti_shift_clamps-mid")


@pytest.mark.parametrize("entry", ["fcn_prepare_inputs", "fcn_prepare_inputs_infer", "fcn_prepare_inputs_sunrgbd",
                                   "fcn_prepare_inputs_sunrgbd_infer", "fcn_prepare_inputs_refine"])
def test_refusals_leave_the_outputs_alone(entry):
    """Every argument check of the C entry returns FCN_E_BADARG before any launch: the poisoned outputs stay as they were.  The
    unrefused call on the same tensors returns 0 (last, so that the poison is still there for the refusals)."""
    case = _refusal_case(entry)
    infer = entry in ("fcn_prepare_inputs_infer", "fcn_prepare_inputs_sunrgbd_infer")
    refine = entry == "fcn_prepare_inputs_refine"
    t = _inputs(case)
    out, Ls = _poisoned(case, labels=not infer)
    before = _snapshot(out)
    base = dict(random_flip=0, random_shift=0) if infer else {}
    nsc = len(case["strides"])
    bad = [("B = 0", dict(B=0), ()), ("B < 0", dict(B=-1), ()), ("N = 0", dict(N=0), ()), ("N < 0", dict(N=-3), ()),
           ("pt_stride = 2", dict(pt_stride=2), ()), ("no descriptor", {}, ("desc",)), ("no raw points", {}, ("raw",)), ("no offsets", {}, ("off",)), ("no choice", {}, ("choice",)),
           ("no point_cloud", {}, ("point_cloud",)), ("no rot_angle", {}, ("rot_angle",))]
    for s in range(nsc):
        bad += [("L[%d] = 0" % s, {"L%d" % s: 0}, ()), ("L[%d] < 0" % s, {"L%d" % s: -1}, ()),
                ("stride[%d] = 0" % s, {"stride%d" % s: 0.0}, ()), ("stride[%d] < 0" % s, {"stride%d" % s: -0.5}, ()),
                ("stride[%d] NaN" % s, {"stride%d" % s: float("nan")}, ()), ("no center_ref%d" % (s + 1), {}, ("center_ref%d" % (s + 1),))]
    if infer:
        bad += [("flip", dict(random_flip=1), ()), ("shift", dict(random_shift=1), ()),
                ("no frustum_angle", {}, ("fangle",)), ("no box2d", {}, ("box2d",))]
        bad += [("no P", {}, ("P",))] if nsc == 4 else [("no K", {}, ("K",)), ("no Rtilt", {}, ("Rtilt",))]
    else:
        bad += [("flip without coin", dict(random_flip=1), ("coin",)), ("shift without normal", dict(random_shift=1), ("normal",))]
    if refine:
        bad += [("cls_label without label corners", {}, ("corners",)), ("labels without heading", {}, ("heading",)),
                ("labels without size", {}, ("size",)), ("labels without box3d_center", {}, ("box3d_center",)),
                ("no pred_size", {}, ("psize",)), ("no pred_corners", {}, ("pcorners",)), ("no pred_angle", {}, ("pangle",)),
                ("no lens", {}, ("lens",)), ("no ref_center", {}, ("ref_center",))]
    elif not infer:
        bad += [("seg_label without raw_seg", {}, ("raw_seg",)), ("no label corners", {}, ("corners",)), ("no heading", {}, ("heading",)),
                ("no size", {}, ("size",)), ("no box3d_center", {}, ("box3d_center",)), ("no box3d_heading", {}, ("box3d_heading",)),
                ("no box3d_size", {}, ("box3d_size",)), ("no frustum_angle", {}, ("fangle",)), ("no box2d", {}, ("box2d",))]
        if entry == "fcn_prepare_inputs_sunrgbd":
            bad += [("shift without hshift", dict(random_shift=1), ("hshift",)), ("no K", {}, ("K",)), ("no Rtilt", {}, ("Rtilt",))]
        else:
            bad += [("no P", {}, ("P",))]
    for what, desc, null in bad:
        rc = _call(entry, case, t, out, Ls, desc=dict(base, **desc), null=null)
        assert rc == FCN_E_BADARG, (entry, what, rc)
    _untouched(out, before, entry)
    # what is NOT refused: flip / shift off need no coin / normal (/ hshift); no seg_label needs no raw_seg
    if not infer:
        ok_null = ("coin", "normal", "hshift") if not refine else ("coin", "normal")
        assert _call(entry, case, t, out, Ls, desc=dict(random_flip=0, random_shift=0), null=ok_null) == 0
        if not refine:
            assert _call(entry, case, t, out, Ls, null=("raw_seg", "seg_label")) == 0
    assert _call(entry, case, t, out, Ls, desc=base) == 0
    torch.cuda.synchronize()
    for k, v in out.items():
        if v.dtype == torch.float32:
            assert not bool(torch.isnan(v).any()), k


# ------------------------------------------------------------------------------------------- a sample without a window
def _bad_width_records(widths):
    case = ic.built("fallback_last_padded-off")
    recs = ic.records(case)
    assert len(recs) == len(widths)
    for r, w in zip(recs, widths):
        r["pred_size"] = np.array([r["pred_size"][0], w, r["pred_size"][2]])
    return case, recs


@pytest.mark.parametrize("widths,index,shown", [((1.6, -0.3, 0.0), 1, "-0.3"), ((1.6, 0.9, float("nan")), 2, "nan")])
@pytest.mark.parametrize("path", ["build", "build_infer", "build_device", "build_device_train"])
def test_a_sample_without_a_window_is_refused(path, widths, index, shown):
    """A predicted width <= 0 (or NaN) next to good ones: the kernel would leave that sample's cls_label row unwritten and the
    reference's collate cannot pad it.  Every path of RefineInputBuilder raises ValueError naming the sample and the width --
    before anything is launched."""
    case, recs = _bad_width_records(widths)
    b = _builder(case)
    rec = case["rec"]
    B = len(recs)
    counts = [len(r["points"]) for r in recs]
    psize = _dev(np.stack([r["pred_size"] for r in recs]).astype(np.float64))
    t = _inputs(case)
    dev = dict(points=t["raw"], off=t["off"], pred_box3d=t["pcorners"], pred_angle=t["pangle"], pred_size=psize,
               counts=np.asarray(counts, dtype=np.int64))
    with pytest.raises(ValueError, match=r"sample %d\b.*%s" % (index, shown)):
        if path == "build":
            b.build(recs, draws=ic.draws(case))
        elif path == "build_infer":
            b.build(recs, draws=ic.draws(case), with_labels=False)
        elif path == "build_device":
            b.build_device(dict(dev, score=torch.ones(B, dtype=torch.float32, device="cuda")), ["Car"] * B, draws=ic.draws(case))
        else:
            sel = dict(dev, kept=np.arange(B), unit_cand=np.arange(B), box3d=t["corners"].view(B, 8, 3), heading=t["heading"],
                       size=t["size"])
            b.build_device_train(sel, ["Car"] * B, draws=ic.draws(case))
    # the same records with their own widths go through all of these paths
    good = ic.records(case)
    out = b.build(good, draws=ic.draws(case))
    dev["pred_size"] = t["psize"]
    out_dev = b.build_device(dict(dev, score=torch.ones(B, dtype=torch.float32, device="cuda")), ["Car"] * B, draws=ic.draws(case))
    sel = dict(dev, kept=np.arange(B), unit_cand=np.arange(B), box3d=t["corners"].view(B, 8, 3), heading=t["heading"], size=t["size"])
    out_train = b.build_device_train(sel, ["Car"] * B, draws=ic.draws(case))
    torch.cuda.synchronize()
    for k in ("point_cloud", "center_ref2", "lens"):
        assert torch.equal(_bits(out_dev[k]), _bits(out[k])) and torch.equal(_bits(out_train[k]), _bits(out[k])), k
    assert torch.equal(out_train["cls_label"], out["cls_label"])
