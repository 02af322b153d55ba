"""CPU: what makes tests/kitti_eval_ref.py (the fp64 restatement of the reference's KITTI evaluator, which needs boost and cannot be
built here) trustworthy as the referee of the device code: scenes whose answers are worked out by hand in the docstrings below,
properties of the protocol, the reference's own compute_alpha (tests/golden/kitti_eval.npz), and the knife-edge condition on
every scene the GPU tests use (tests/kitti_eval_scenes.py)."""
import numpy as np
import pytest

import kitti_eval_ref as ref
import kitti_eval_scenes as scenes

IMG, GROUND, BOX3D = 0, 1, 2
EASY, MODERATE, HARD = 0, 1, 2


def k(metric, cls, level):
    return (metric * 3 + cls) * 3 + level


def _lists(w, i):
    T = w["num_thresholds"][i]
    return w["thresholds"][i, :T].tolist(), w["tp"][i, :T].tolist(), w["fp"][i, :T].tolist(), w["fn"][i, :T].tolist()


def _lists_close(w, i, thr, tp, fp, fn):
    """(the thresholds are float32 scores: .9f is not .9)"""
    t, a, b, c = _lists(w, i)
    return np.allclose(t, thr, atol=1e-7) and (a, b, c) == (tp, fp, fn)


def test_compute_alpha_and_label_rows_match_the_reference():
    g = np.load(ref.GOLDEN)
    got = np.array([ref.compute_alpha(x, z, r) for (x, z), r in zip(g["xz"], g["ry"])])
    assert np.array_equal(got, g["alpha"])                                       # the same numpy expression on the same fp64 inputs
    assert g["xz"][0].tolist() == [0.0, 0.0] and got[0] == g["ry"][0]            # np.sign(0) = 0: alpha = ry
    assert (g["xz"][1:3, 0] == 0).all() and (g["xz"][3:5, 1] == 0).all()         # x = 0 and z = 0 are among the rows
    assert abs(got[4] - (-np.pi / 2 + np.pi + g["ry"][4])) < 1e-15               # z = 0, x < 0: beta = pi
    lab = g["label"]                                                             # h, w, l, tx, ty, tz, ry
    dets = np.concatenate([lab[:, 3:6], lab[:, [2, 1, 0]], lab[:, 6:7], np.ones((len(lab), 1))], 1)
    table, ok = ref.label_rows(dets, np.arange(len(lab)), np.tile([1.0, 2.0, 3.0, 4.0], (2, 1)), np.arange(len(lab)) % 2)
    assert np.array_equal(table[:, 0], g["label_alpha"]) and np.array_equal(table[:, 5:12], lab) and ok.all()
    assert table[:, 1:5].tolist() == [[1.0, 2.0, 3.0, 4.0]] * len(lab) and (table[:, 12] == 1).all()
    dets[3, 5] = 0.009
    assert ref.label_rows(dets, [3, 4], np.zeros((1, 4)), [0, 0])[1].tolist() == [False, True]


def test_overlaps_by_hand():
    """Image: boxes (0,0,10,10) and (5,0,15,10) meet in 50 of 100 + 100 - 50: 1/3; over the detection alone 1/2.  Ground: the hand
    scenes' nested pair, 3.51 x 1.44 inside 3.9 x 1.6: 5.0544 / 6.24 = 0.81, and as both are 1.5 high at the same ty the 3-D overlap
    is the same; lifted by 0.5 the common height is 1.0: 5.0544 / (7.5816 + 9.36 - 5.0544)."""
    d, g = scenes.D(0, 0, 10, 10, 0, 1.0), scenes.L(ref.CAR, 5, 0, 15, 10, 0)
    assert abs(ref.image_overlap(d, g) - 1 / 3) < 1e-15 and abs(ref.image_overlap(d, g, 0) - 0.5) < 1e-15
    assert ref.image_overlap(d, scenes.L(ref.CAR, 10, 0, 20, 10, 0)) == 0.0                      # touching: w <= 0
    assert abs(ref.ground_overlap(d, g) - 0.81) < 1e-6 and abs(ref.box3d_overlap(d, g) - 0.81) < 1e-6
    assert abs(ref.ground_overlap(d, g, 0) - 1.0) < 1e-6                                         # the detection lies inside
    d[9] -= 0.5
    assert abs(ref.box3d_overlap(d, g) - 5.0544 / (7.5816 + 9.36 - 5.0544)) < 1e-6
    assert ref.pair_overlaps(d, scenes.L(ref.CAR, 5, 0, 15, 10, 1), -1)[1:] == [0.0, 0.0]          # 10 m apart


def test_thresholds_by_hand():
    """getThresholds.  No score: no threshold.  Fewer scores than recall steps: with n_gt = 2 and one score, l = r = 0.5 at the last
    element, which is always taken.  n_gt = 4, scores .9 .8 .3: every step of 1/4 is further from the running recall (0, .025,
    .05) on its right than on its left, all three are taken.  More than 41: 200 scores over n_gt = 200 -- the walk takes the score
    whose recall (i + 1) / 200 is nearest to t / 40 from the left, i = 0, 4, 9, 14, ...: 41 of them, the last at i = 199."""
    assert ref.get_thresholds([], 5) == [] and ref.get_thresholds([], 0) == []
    assert ref.get_thresholds([0.4], 2) == [0.4]
    assert ref.get_thresholds([0.3, 0.9, 0.8], 4) == [0.9, 0.8, 0.3]
    v = [float(i) for i in range(200)]
    t = ref.get_thresholds(v, 200)
    assert len(t) == 41 and t[0] == 199.0 and t[-1] == 0.0 and t[1] == 199.0 - 4 and t[2] == 199.0 - 9
    assert len(ref.get_thresholds(v[:41], 41)) == 41 and len(ref.get_thresholds(v[:40], 40)) == 40
    assert len(ref.get_thresholds(v[:100], 200)) == 21                          # half the labels found: recall stops at 0.5


def test_max_element_is_the_first_of_the_largest_and_keeps_a_leading_nan():
    assert ref._max_element([1.0, 3.0, 3.0, 2.0]) == 3.0
    assert np.isnan(ref._max_element([np.nan, 1.0])) and ref._max_element([1.0, np.nan, 2.0]) == 2.0


def test_hand1_by_hand():
    """scenes.hand1.  Car, image metric.
    EASY: g1 (30 px) is ignored, n_gt = 3 (g0, g4, g5).  Pass A: g0 <- d0 (.9), g1 <- d1 (assigned only: label and detection are both
    too small), the Van <- d2 (assigned only), g4 nothing, g5 <- d5 (.3).  Scores [.9, .3], n_gt = 3: both are taken.
      thr .9: d0 alone is left: tp 1, fn 2 (g4, g5), fp 0.
      thr .3: tp 2, fn 1 (g4); unassigned, tall enough, of the class: d3, d4 -> fp 2, minus d3 which lies inside the DontCare box:
              fp 1.  The detection on the Van is neither.
      precision [1, 2/3], suffix maximum the same; only entry 0 is a sample point: AP = 100 / 11.
      AOS: d0's alpha is off by pi / 2: similarity 0.5; d5's is right: 1.  aos [0.5 / 1, 1.5 / 3] -> AP 0.5 * 100 / 11.
    MODERATE = HARD: n_gt = 4, scores [.9, .8, .3], all taken; tp [1, 2, 3], fn [3, 2, 1], fp [0, 0, 1];
      aos raw [.5, 1.5 / 2, 2.5 / 4] -> suffix maximum [.75, .75, .625] -> AP 0.75 * 100 / 11.
    Ground and 3-D: the DontCare area's box is nowhere near d3 in space: fp 2 at the last threshold."""
    _, w = scenes.scene("hand1")
    assert _lists_close(w, k(IMG, 0, EASY), [0.9, 0.3], [1, 2], [0, 1], [2, 1]) and w["n_gt"][k(IMG, 0, EASY)] == 3
    for level in (MODERATE, HARD):
        assert _lists_close(w, k(IMG, 0, level), [0.9, 0.8, 0.3], [1, 2, 3], [0, 0, 1], [3, 2, 1]) and w["n_gt"][k(IMG, 0, level)] == 4
    for m in (GROUND, BOX3D):
        assert _lists_close(w, k(m, 0, EASY), [0.9, 0.3], [1, 2], [0, 2], [2, 1])
        assert _lists_close(w, k(m, 0, HARD), [0.9, 0.8, 0.3], [1, 2, 3], [0, 0, 2], [3, 2, 1])
    assert np.allclose(w["precision"][IMG, 0, EASY, :3], [1, 2 / 3, 0], atol=1e-15)
    assert np.allclose(w["precision"][GROUND, 0, EASY, :3], [1, 0.5, 0], atol=1e-15)
    assert np.allclose(w["ap"][:, 0], 100 / 11, atol=1e-12)
    assert np.allclose(w["aos"][0, EASY, :3], [0.5, 0.5, 0], atol=1e-7) and abs(w["aos_ap"][0, EASY] - 50 / 11) < 1e-6
    assert np.allclose(w["aos"][0, MODERATE, :4], [0.75, 0.75, 0.625, 0], atol=1e-7) and abs(w["aos_ap"][0, HARD] - 75 / 11) < 1e-6
    assert np.isnan(w["ap"][:, 1:]).all() and np.isnan(w["aos_ap"][1:]).all()       # no pedestrian, no cyclist detected: not evaluated


def test_hand1_thresholds_are_the_float32_scores():
    sc, w = scenes.scene("hand1")
    assert w["thresholds"][0, 0] == float(np.float32(0.9)) and w["thresholds"][0, 1] == float(np.float32(0.3))


def test_detection_height_is_truncated_to_int_by_hand():
    """scenes.hand_trunc, Car, moderate (MIN_HEIGHT 25).  Frame 0: the detection is 25.9 px high -> int 25, not below 25: it counts
    (overlap 25.9 / 30 = .863).  Frame 1: 24.99 px -> int 24: 'ignored', so pass A assigns it without recording a score.  Scores
    [.9], n_gt = 2 -> one threshold; at .9 the second frame's detection (.8) is out, its label is a false negative: tp 1, fp 0, fn 1.
    Were the height compared as a double, 25.9 would pass either way but 24.99 < 25 all the same -- what the truncation changes is
    a height in [25, 26) ... [40, 41); the pair pins both sides of 25.  At easy (40) both labels are too small: n_gt = 0, nothing."""
    _, w = scenes.scene("hand_trunc")
    for m in range(3):
        assert _lists_close(w, k(m, 0, MODERATE), [0.9], [1], [0], [1]) and w["n_gt"][k(m, 0, MODERATE)] == 2
        assert w["num_thresholds"][k(m, 0, EASY)] == 0 and w["n_gt"][k(m, 0, EASY)] == 0 and w["ap"][m, 0, EASY] == 0.0
    # a 25.9 px LABEL is compared as a double: 25.9 >= 25 counts, 24.99 does not
    lab = [scenes.L(ref.CAR, 0, 0, 50, 25.9, 0), scenes.L(ref.CAR, 0, 0, 50, 24.99, 1)]
    assert ref.clean_data(0, lab, [0, 0], [], [], MODERATE)[0] == [0, 1]
    det = [scenes.D(0, 0, 50, 25.9, 0, 1.0), scenes.D(0, 0, 50, 24.99, 0, 1.0), scenes.D(0, 40.9, 50, 0, 0, 1.0)]
    assert ref.clean_data(0, [], [], det, [0, 0, 0], MODERATE)[2] == [0, 1, 0] and ref.clean_data(0, [], [], det, [0, 0, 1], EASY)[2] == [1, 1, -1]
    # the height is looked at BEFORE the class (:449-454): a short detection of another class is 'ignored' (1), not 'another class' (-1)
    assert ref.clean_data(0, [], [], det[:2], [1, 1], MODERATE)[2] == [-1, 1]


def test_ignored_detection_ahead_of_a_valid_one_by_hand():
    """scenes.hand_ignored, Pedestrian (MIN_OVERLAP .5).  g0 has two candidates: d0 (39 px, overlap 39 / 60 = .65, score .5, first) and
    d1 (exact, .9); g1 has d2 (.1).  Pass A takes the highest score: g0 <- d1, g1 <- d2: scores [.9, .1], n_gt = 2, both taken.
    EASY (d0 is below 40 px: 'ignored'):
      thr .9: d1 alone: tp 1, fn 1.
      thr .1: the search for g0 meets d0 first and notes it as an ignored candidate, then d1, which is valid and replaces it
              whatever its overlap (assigned_ignored_det): tp 2; d0 stays unassigned but is no false positive (ignored): fp 0.
    MODERATE (d0 counts): at thr .1 d0 is taken first (.65), d1 has the greater overlap and replaces it; d0 is a false positive."""
    _, w = scenes.scene("hand_ignored")
    for m in range(3):
        assert _lists_close(w, k(m, 1, EASY), [0.9, 0.1], [1, 2], [0, 0], [1, 0])
        assert _lists_close(w, k(m, 1, MODERATE), [0.9, 0.1], [1, 2], [0, 1], [1, 0])
    assert np.allclose(w["precision"][IMG, 1, MODERATE, :3], [1, 2 / 3, 0]) and np.allclose(w["precision"][IMG, 1, EASY, :3], [1, 1, 0])
    assert np.isnan(w["ap"][:, 0]).all()


def test_perfect_detections_score_100_everywhere_and_counts_of_true_positives():
    """Every label under one close detection of its class, nothing else: AP 100 at every level and metric (48 per class: more than
    41 true positives).  With 40: 40 thresholds, ten sample points; with exactly 0 (no detection at all): not evaluated."""
    _, w = scenes.scene("perfect")
    assert (w["ap"] == 100.0).all() and (w["num_thresholds"] == 41).all() and (w["fp"] == 0).all()
    assert all(len(v) == 48 for v in w["tp_scores"]) and (w["aos_ap"] > 95).all() and (w["aos_ap"] < 100).all()
    _, w40 = scenes.scene("tp40")
    assert np.allclose(w40["ap"][:, 0], 1000 / 11) and (w40["num_thresholds"][[0, 1, 2]] == 40).all()
    sc, _ = scenes.scene("tp40")
    none = ref.evaluate(sc["det"][:0], sc["det_class"][:0], np.zeros_like(sc["det_off"]), sc["gt"], sc["gt_type"], sc["gt_off"])
    assert np.isnan(none["ap"]).all() and (none["num_thresholds"] == 0).all() and (none["n_gt"][:3] == 40).all() and (none["tp"] == 0).all()
    # detections of the class that hit nothing: evaluated, no true positive, no threshold, AP 0
    far = sc["det"].copy(); far[:, [1, 3]] += 5000; far[:, 8] += 500
    miss = ref.evaluate(far, sc["det_class"], sc["det_off"], sc["gt"], sc["gt_type"], sc["gt_off"])
    assert (miss["ap"][:, 0] == 0).all() and (miss["num_thresholds"] == 0).all()


def test_a_detection_inside_a_dontcare_box_changes_nothing_in_the_image_metric():
    sc, w = scenes.scene("hand1")
    extra = scenes.D(710, 110, 790, 190, 9, 1.5)[None].astype(np.float32)          # 80 px high, the best score, alone in space
    det = np.concatenate([sc["det"], extra])
    w2 = ref.evaluate(det, np.append(sc["det_class"], 0), [0, len(det)], sc["gt"], sc["gt_type"], sc["gt_off"])
    for key in ("thresholds", "tp", "fp", "fn", "num_thresholds"):
        assert np.array_equal(w2[key][:9], w[key][:9]), key
    assert np.array_equal(w2["precision"][IMG], w["precision"][IMG], equal_nan=True) and np.array_equal(w2["aos"], w["aos"], equal_nan=True)
    assert w2["fp"][k(GROUND, 0, EASY), 1] == w["fp"][k(GROUND, 0, EASY), 1] + 1      # in space nothing holds it: one more false positive


def test_a_van_under_a_car_detection_is_neither_true_nor_false_positive():
    sc, w = scenes.scene("hand1")
    keep = np.arange(len(sc["det"])) != 2                                          # without d2, the detection on the Van
    w2 = ref.evaluate(sc["det"][keep], sc["det_class"][keep], [0, keep.sum()], sc["gt"], sc["gt_type"], sc["gt_off"])
    for key in ("thresholds", "tp", "fp", "fn", "precision", "ap"):
        assert np.array_equal(w2[key], w[key], equal_nan=True), key
    # the same detection over a label of ANOTHER type (a tram) is a false positive
    typ = sc["gt_type"].copy(); typ[2] = ref.OTHER
    w3 = ref.evaluate(sc["det"], sc["det_class"], sc["det_off"], sc["gt"], typ, sc["gt_off"])
    assert w3["fp"][k(IMG, 0, EASY), 1] == w["fp"][k(IMG, 0, EASY), 1] + 1


def test_alpha_minus_ten_and_undetected_classes():
    _, w = scenes.scene("alpha10")
    assert np.isnan(w["aos"]).all() and np.isnan(w["aos_ap"]).all() and np.isfinite(w["ap"]).all()
    _, w = scenes.scene("no_cyclist")
    assert np.isnan(w["ap"][:, 2]).all() and np.isfinite(w["ap"][:, :2]).all()


@pytest.mark.parametrize("name", scenes.NAMES)
def test_every_scene_meets_the_knife_edge_condition(name):
    sc, w = scenes.scene(name)
    det, gt = sc["det"].astype(np.float64), sc["gt"].astype(np.float64)
    assert scenes.heights_ok(det, 2, 4) and scenes.heights_ok(gt, 4, 6)
    assert (np.abs(gt[:, 0:1] - np.asarray(ref.MAX_TRUNCATION)) > 1e-3).all()
    at = 0
    for f in range(len(sc["det_off"]) - 1):
        n, m = sc["det_off"][f + 1] - sc["det_off"][f], sc["gt_off"][f + 1] - sc["gt_off"][f]
        ov = w["overlaps"][at:at + n * m].reshape(n, m, 3)
        at += n * m
        assert scenes.knife_edge_ok(ov), (name, f)
    assert at == len(w["overlaps"])
