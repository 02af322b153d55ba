"""The numpy restatement of the SUN-RGBD inference tail (tests/sunrgbd_detect_ref.py) against the reference's own recorded run
(tests/golden/sunrgbd_detect.npz, written by tests/golden/make_golden_sunrgbd_detect.py): the rows test() of
train/test_net_det_sunrgbd.py produced from the same logits, the corners compute_box_3d made, and what eval_det_cls + voc_ap
returned for the same corners.  CPU only.  The GPU tests compare the kernels with this restatement and with the fixture."""
import functools

import numpy as np
import pytest

import sunrgbd_detect_ref as ref

VARIANTS = ("full", "norgb", "noref")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(ref.GOLDEN))


def decode_inputs(g, L2, variant):
    p = "dec%d_" % L2
    return dict(logits=g[p + "logits"], ref2=g[p + "ref2"], mean_size=g["mean_size"], rot=g[p + "rot"],
                ref_center=None if variant == "noref" else g[p + "ref_center"],
                rgb_prob=None if variant == "norgb" else g[p + "rgb_prob"], nb=int(g["meta_num_bins"]), ns=int(g["meta_num_sizes"]))


@pytest.mark.parametrize("L2", [5, 300])
@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("method", ["nms", "top"])
def test_decode_reproduces_the_references_rows(L2, variant, method):
    g = golden()
    dets, sel, valid, pfg = ref.decode(method=method, **decode_inputs(g, L2, variant))
    rows, counts = g["rows_dec%d_%s_%s" % (L2, variant, method)], g["counts_dec%d_%s_%s" % (L2, variant, method)]
    assert np.array_equal(valid.reshape(3, L2).sum(1), counts)                       # selection + filter, exact
    got = dets[valid]
    worst = np.abs(got - rows).max()
    print("decode L2=%d %s %s: %d rows, worst abs diff %.3e" % (L2, variant, method, len(rows), worst))
    # the reference rotates with a float32 cosine / sine (rot_angle is a float32 loader field): 2 terms x 3e-8 x |coordinate| < 6 m
    assert worst < 1e-6
    assert np.abs(pfg - g["dec%d_p_fg" % L2].reshape(-1)).max() < 1e-12 and (np.abs(pfg - 0.5) > 1e-3).all()
    assert (np.abs(dets[:, 3:6] - 0.01) > 1e-3).all()
    if method == "nms":
        assert sel.reshape(3, L2)[1].sum() == 1                                      # frustum 1: no p_fg > 0.5, the arg-max alone
        assert sel[2] and not valid[2]                                               # frustum 0, position 2: selected, size 0


def test_corners_reproduce_compute_box_3d():
    g = golden()
    got = ref.corners(g["ev_det_rows"])
    worst = np.abs(got - g["ev_det_corners"]).max()
    print("corners worst abs diff %.3e" % worst)
    # the reference computes them in float32 (float32 rows): half an ulp of a 6 m coordinate per operation, three operations
    assert worst < 3 * 2.4e-7 + 1e-7
    lab = ref.corners(g["ev_gt_rows"])
    assert np.abs(lab - g["ev_gt_corners"]).max() < 2.4e-7 + 1e-9                     # float64 there, stored as float32


def test_matching_and_ap_reproduce_eval_det_cls():
    g = golden()
    r = ref.evaluate(g["ev_det_corners"], g["ev_scores"], g["ev_det_off"], g["ev_gt_corners"], g["ev_gt_off"], g["ev_group_class"],
                     int(g["ev_num_classes"]), float(g["ev_thresh"]))
    assert np.array_equal(r["tp"], g["ev_tp"]) and np.array_equal(r["jmax"], g["ev_jmax"]) and np.array_equal(r["rank"], g["ev_rank"])
    assert np.array_equal(r["npos"], g["ev_npos"])
    fin = np.isfinite(g["ev_ovmax"])
    assert np.array_equal(fin, np.isfinite(r["ovmax"]))
    print("ovmax worst abs diff %.3e" % np.abs(r["ovmax"][fin] - g["ev_ovmax"][fin]).max())
    # the corners are float32 values, so the boxes are rectangles only to half an ulp of a 4 ... 8 m coordinate (2.4e-7 m) per
    # vertex; the reference's python takes a box's volume from three edge lengths, the restatement (as box_ops.h does) from the
    # polygon's area and the y extent: over edges of 0.5 m and more they agree to 3 x 2.4e-7 / 0.5 = 1.5e-6 relative, IoU <= 1
    assert np.abs(r["ovmax"][fin] - g["ev_ovmax"][fin]).max() < 2e-6
    for k in ("rec", "prec", "ap"):
        assert np.abs(r[k] - g["ev_" + k]).max() < 1e-12, k
    assert r["ap"][3] == 0.0 and r["tp"].sum() > 0
    # the cases the fixture holds by construction
    doff = g["ev_det_off"]
    a = int(g["ev_case_best_taken"])
    assert r["tp"][doff[a]:doff[a + 1]].tolist() == [1, 0] and r["jmax"][doff[a] + 1] == 0 and r["ovmax"][doff[a] + 1] > 0.25
    second = ref.iou3d(g["ev_det_corners"][doff[a] + 1], g["ev_gt_corners"][g["ev_gt_off"][a]:g["ev_gt_off"][a + 1]])[1]
    assert second > 0.25                                                             # a second label box would qualify
    b = int(g["ev_case_two_on_one"])
    assert sorted(r["tp"][doff[b]:doff[b + 1]].tolist()) == [0, 1]
    n = int(g["ev_case_no_label"])
    assert doff[n + 1] > doff[n] and not np.isfinite(r["ovmax"][doff[n]:doff[n + 1]]).any() and (r["jmax"][doff[n]:doff[n + 1]] == -1).all()
    e = int(g["ev_case_no_detection"])
    assert doff[e + 1] == doff[e] and g["ev_gt_off"][e + 1] > g["ev_gt_off"][e]


def test_equal_scores_walk_the_lower_index_first():
    """Defined here, where the reference is not (np.argsort is unstable): of two detections with one score on one label box the
    lower input index is the true positive and ranks first."""
    g = golden()
    box = g["ev_gt_corners"][:1]
    dets = np.repeat(box.mean(1, keepdims=True) + 0.9 * (box - box.mean(1, keepdims=True)), 2, 0)      # nested: IoU 0.729
    r = ref.evaluate(dets, np.asarray([0.7, 0.7], dtype=np.float32), [0, 2], box, [0, 1], [0], 1)
    assert r["tp"].tolist() == [1, 0] and r["rank"].tolist() == [0, 1] and abs(r["ap"][0] - 1.0) < 1e-15
