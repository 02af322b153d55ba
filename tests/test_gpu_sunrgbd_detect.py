"""-m gpu: the SUN-RGBD decode rule (fcn_decode_detections_rule, detect.decode_detections(rule="sunrgbd"),
PointNetDet.detect(rule="sunrgbd")) and the corners of kept rows (fcn_box3d_corners, detect.box3d_corners) against the reference's
recorded run (tests/golden/sunrgbd_detect.npz) and its fp64 numpy restatement (tests/sunrgbd_detect_ref.py, pinned to the same
fixture by tests/test_sunrgbd_detect_referee.py).  tests/test_emu_det_eval.py runs the same functions on the host emulation."""
import numpy as np
import pytest
import torch

import sunrgbd_detect_ref as ref
from test_sunrgbd_detect_referee import VARIANTS, decode_inputs, golden

pytestmark = pytest.mark.gpu
BADARG = 10001                     # FCN_E_BADARG
NB, NS, B = 12, 10, 3
# floats: the fp32 kernel against the fp64 restatement -- cosf / sinf of the rotation on coordinates below 6 m (a few 1e-7), the
# heading (below 7 rad: ulp 4.8e-7, three operations) and the softmax of ten size scores in fp32 (1e-6 of a probability <= 1)
TOL = 1e-5


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def _p(t):
    return None if t is None else t.data_ptr()


def _padded(logits, ld):
    """The head rows in a buffer of row length ld; the columns behind the 69 used ones hold a poison the kernel must not read."""
    out = np.full((logits.shape[0], ld), 1e30, dtype=np.float32)
    out[:, :logits.shape[1]] = logits
    return out


def _raw(inp, L2, ld, method, rule, entry="fcn_decode_detections_rule", ld_arg=None):
    """The C entry on device tensors with poisoned outputs -> rc, dets, valid (ld_arg: the row length it is TOLD)."""
    from frustum_convnet_amd import _native
    t = [_dev(_padded(inp["logits"], ld)), _dev(inp["ref2"]), _dev(inp["mean_size"].astype(np.float32)), _dev(inp["rot"].reshape(-1)),
         _dev(inp["ref_center"]), _dev(None if inp["rgb_prob"] is None else inp["rgb_prob"].reshape(-1))]
    dets = torch.full((B * L2, 8), -7.0, dtype=torch.float32, device="cuda")
    valid = torch.full((B * L2,), -7, dtype=torch.int32, device="cuda")
    L = _native.lib()
    args = [_p(t[0]), ld if ld_arg is None else ld_arg] + [_p(x) for x in t[1:]] + [B, L2, NB, NS, 1 if method == "nms" else 0]
    if entry == "fcn_decode_detections_rule":
        args.append(rule)
    rc = getattr(L, entry)(*args, _p(dets), _p(valid), _native.current_stream())
    torch.cuda.synchronize()
    return rc, dets.cpu().numpy(), valid.cpu().numpy()


@pytest.mark.parametrize("L2", [5, 300])                       # 300: more positions than the workgroup's 256-thread stride
@pytest.mark.parametrize("ld", [69, 128])
def test_decode_rule_matches_the_fixture_and_the_restatement(L2, ld):
    from frustum_convnet_amd import detect
    g = golden()
    worst = 0.0
    for variant in VARIANTS:                                   # rgb_prob and ref_center each None
        inp = decode_inputs(g, L2, variant)
        for method in ("nms", "top"):
            e_dets, e_sel, e_valid, _ = ref.decode(method=method, **inp)
            rows = g["rows_dec%d_%s_%s" % (L2, variant, method)]
            rc, dets, valid = _raw(inp, L2, ld, method, 1)
            assert rc == 0
            t = lambda a: None if a is None else torch.from_numpy(a)         # loader fields arrive as CPU tensors
            d2, v2 = detect.decode_detections(_dev(_padded(inp["logits"], ld)), _dev(inp["ref2"]), t(inp["mean_size"]), t(inp["rot"]),
                                              t(inp["ref_center"]), t(inp["rgb_prob"]), NB, NS, method, rule="sunrgbd")
            assert np.array_equal(d2.cpu().numpy(), dets) and np.array_equal(v2.cpu().numpy(), valid)
            assert np.array_equal(valid, e_valid.astype(np.int32)), (variant, method)          # exact; every entry 0 or 1
            err_all = np.abs(dets - e_dets).max()                                               # every row is written
            err_fix = np.abs(dets[valid != 0] - rows).max()
            print("L2=%d ld=%d %s %s: %d valid, worst vs restatement %.3e, vs fixture %.3e" %
                  (L2, ld, variant, method, int(valid.sum()), err_all, err_fix))
            worst = max(worst, err_all, err_fix)
            assert err_all < TOL and err_fix < TOL, (variant, method)
            if method == "nms":
                assert valid.reshape(B, L2)[1].sum() == 1                    # frustum 1 has no p_fg > 0.5: the arg-max
                assert e_sel[2] and valid[2] == 0                            # selected, filtered by size
            else:
                assert (valid.reshape(B, L2).sum(1) <= 1).all()
    print("worst %.3e" % worst)


def test_the_kitti_rule_on_the_same_inputs_differs_and_is_the_old_entry():
    g = golden()
    L2 = 300
    inp = decode_inputs(g, L2, "full")
    rc, sun, sun_v = _raw(inp, L2, 69, "nms", 1)
    rc0, kit, kit_v = _raw(inp, L2, 69, "nms", 0)
    rc1, old, old_v = _raw(inp, L2, 69, "nms", None, entry="fcn_decode_detections")
    assert rc == 0 and rc0 == 0 and rc1 == 0
    assert np.array_equal(kit.view(np.uint32), old.view(np.uint32)) and np.array_equal(kit_v, old_v)     # bit for bit
    assert np.abs((kit[:, 1] - sun[:, 1]) - 0.5 * sun[:, 5]).max() < 1e-6          # ty: bottom centre there, centre here
    assert np.abs(kit[:, 1] - sun[:, 1]).max() > 0.1
    p_fg = g["dec300_p_fg"].reshape(-1)
    assert np.abs(kit[:, 7] - (p_fg + np.repeat(inp["rgb_prob"].reshape(-1), L2))).max() < 1e-5
    assert np.abs(kit[:, 7] - sun[:, 7]).max() > 0.1                               # the score is another quantity
    assert np.array_equal(kit[:, [0, 2, 3, 4, 5, 6]], sun[:, [0, 2, 3, 4, 5, 6]])  # everything else is one text
    assert np.array_equal(kit_v != 0, (sun_v != 0))                                # (p0 < p1 and p1 > 0.5 agree off the margin)


def test_decode_refusals_write_nothing():
    from frustum_convnet_amd import detect
    g = golden()
    inp = decode_inputs(g, 5, "full")
    for rule in (2, -1):
        rc, dets, valid = _raw(inp, 5, 69, "nms", rule)
        assert rc == BADARG and (dets == -7.0).all() and (valid == -7).all()
    rc, dets, valid = _raw(inp, 5, 69, "nms", 1, ld_arg=68)                        # a row shorter than its 69 columns
    assert rc == BADARG and (dets == -7.0).all()
    with pytest.raises(ValueError):
        detect.decode_detections(_dev(inp["logits"]), _dev(inp["ref2"]), _dev(inp["mean_size"]), _dev(inp["rot"]), None, None,
                                 NB, NS, "nms", rule="nuscenes")


def test_cpu_tensors_are_refused():
    from frustum_convnet_amd import detect, evaluate
    g = golden()
    with pytest.raises(RuntimeError):
        detect.box3d_corners(torch.from_numpy(g["ev_det_rows"]))
    with pytest.raises(RuntimeError):
        evaluate.match_detections_ap(torch.from_numpy(g["ev_det_corners"]), g["ev_scores"], g["ev_det_off"], g["ev_gt_corners"],
                                     g["ev_gt_off"], g["ev_group_class"], 4)


def test_corners_of_kept_rows():
    from frustum_convnet_amd import detect, _native
    g = golden()
    rows8 = g["ev_det_rows"]
    n = len(rows8)
    want = ref.corners(rows8)
    got = detect.box3d_corners(_dev(rows8)).cpu().numpy()
    print("corners worst vs restatement %.3e, vs compute_box_3d %.3e" % (np.abs(got - want).max(), np.abs(got - g["ev_det_corners"]).max()))
    assert got.shape == (n, 8, 3) and np.abs(got - want).max() < 1e-5 and np.abs(got - g["ev_det_corners"]).max() < 1e-5
    pick = np.asarray([n - 1, 0, 3, 3, -1, n], dtype=np.int64)                     # repeats; -1 and n: unused keep slots
    sub = detect.box3d_corners(_dev(rows8), _dev(pick)).cpu().numpy()
    assert np.array_equal(sub[:4], got[[n - 1, 0, 3, 3]]) and np.isnan(sub[4:]).all()
    assert np.array_equal(detect.box3d_corners(_dev(rows8), pick[:4].tolist()).cpu().numpy(), sub[:4])      # a host sequence
    assert detect.box3d_corners(_dev(rows8), []).shape == (0, 8, 3)
    # the raw entry: poisoned output behind the rows, refusals
    out = torch.full((n + 2, 8, 3), -7.0, dtype=torch.float32, device="cuda")
    d = _dev(rows8)
    L, s = _native.lib(), _native.current_stream()
    assert L.fcn_box3d_corners(_p(d), n, None, n, _p(out), s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out[:n].cpu().numpy(), got) and (out[n:].cpu().numpy() == -7.0).all()
    out.fill_(-7.0)
    for bad in ((None, n, None, n, _p(out)), (_p(d), n, None, n, None), (_p(d), n, None, n + 1, _p(out)), (_p(d), -1, None, n, _p(out)),
                (_p(d), n, None, -1, _p(out))):
        assert L.fcn_box3d_corners(*bad, s) == BADARG, bad
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.0).all()


def test_model_detect_takes_the_rule():
    """The B = 4 five-scale model on the sunrgbd_b4_n1024 inputs: detect(rule="sunrgbd") returns decode_detections(rule="sunrgbd")
    of that model's own logits; rule=None is "kitti", also for this model."""
    from helpers import load_golden, golden_inputs
    from test_gpu_model import _model
    from frustum_convnet_amd import detect, synth
    from frustum_convnet_amd.config import reset_cfg
    g = load_golden("sunrgbd_b4_n1024")
    data = synth.to_torch(golden_inputs(g), "cuda")
    try:
        m = _model(g)
        m.eval()
        Bm, L2 = data["center_ref2"].shape[0], data["center_ref2"].shape[2]
        dd = {k: v for k, v in data.items() if k in ("point_cloud", "one_hot") or k.startswith("center_ref")}
        dd["rot_angle"] = torch.linspace(-0.3, 0.3, Bm).view(Bm, 1)
        dd["rgb_prob"] = torch.linspace(0.2, 0.9, Bm).view(Bm, 1)
        ug = torch.tensor([0, 0, 1, 1], dtype=torch.int32)
        dets, valid, keep, cnt = m.detect(dd, unit_group=ug, num_groups=2, method="nms", thresh=0.1, rule="sunrgbd")
        lg = m.last_logits64.clone()
        e_dets, e_valid = detect.decode_detections(lg, data["center_ref2"], m._mean_size, dd["rot_angle"], None, dd["rgb_prob"],
                                                   m.num_bins, m.num_size_cluster, "nms", rule="sunrgbd")
        assert torch.equal(dets, e_dets) and torch.equal(valid, e_valid) and m.num_size_cluster == 10
        r_dets, r_sel, r_valid, _ = ref.decode(lg.cpu().numpy()[:, :69], data["center_ref2"].cpu().numpy(), m._mean_size.cpu().numpy(),
                                               dd["rot_angle"].numpy(), None, dd["rgb_prob"].numpy(), 12, 10, "nms")
        # (the restatement on the same fp32 logits; a p_fg inside fp32 rounding of 0.5 is not excluded for a model's own logits, so
        # the selection is compared where it is off that margin)
        off = np.abs(ref.softmax(lg.cpu().numpy()[:, :2].astype(np.float64))[:, 1] - 0.5) > 1e-5
        assert np.array_equal(valid.cpu().numpy()[off] != 0, r_valid[off]) and (np.abs(dets.cpu().numpy() - r_dets) <= TOL * np.maximum(1.0, np.abs(r_dets))).all()
        assert keep.shape == (2, 300)
        k_dets, k_valid, _, _ = m.detect(dd, unit_group=ug, num_groups=2, method="nms", thresh=0.1)
        k2 = m.detect(dd, unit_group=ug, num_groups=2, method="nms", thresh=0.1, rule="kitti")
        assert torch.equal(k_dets, k2[0]) and torch.equal(k_valid, k2[1])
        assert not torch.equal(k_dets[:, 1], dets[:, 1]) and not torch.equal(k_dets[:, 7], dets[:, 7])
        assert torch.equal(k_dets[:, [0, 2, 3, 4, 5, 6]], dets[:, [0, 2, 3, 4, 5, 6]])
    finally:
        reset_cfg()
