"""CPU: the fp64 referee of the labelled frustum extraction (tests/frustum_label_ref.py) and frustum.perturb_boxes2d against the
reference's own functions, recorded in tests/golden/frustum_label.npz by tests/golden/make_golden_frustum_label.py
(kitti_util.compute_box_3d, kitti/prepare_data.py's extract_pc_in_box3d, random_shift_box2d and the lines of
extract_frustum_data around them, the reject rule of :354 included)."""
import os

import numpy as np
import pytest

import frustum_label_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_label.npz")
SMALL, AIR, SKY, RETRY = 3, 4, 7, 8       # the special boxes of the fixture (make_golden_frustum_label.py)


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def mine(g):
    return frustum_label_ref.select_labeled(g["points"], g["off"], g["P"], g["V2C"], g["R0"], g["img_wh"], g["ref_boxes"],
                                            g["box_frame"], g["gt_box3d"], g["gt_box2d"])


def test_fixture_is_small_and_holds_the_cases(g, mine):
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert len(g["off"]) == 3 and (np.diff(g["off"]) <= 3000).all() and g["points"].dtype == np.float32
    ry = g["gt_box3d"][:, 6]
    assert (ry < 0).any() and (np.abs(ry) > np.pi / 2).any() and len(ry) >= 8
    h = g["gt_box2d"][:, 3] - g["gt_box2d"][:, 1]
    assert h[SMALL] < 25 and mine["pos"][SMALL] > 0                          # rejected by its height alone
    assert mine["counts"][AIR] > 0 and mine["pos"][AIR] == 0 and h[AIR] >= 25    # background only
    assert mine["counts"][SKY] == 0 and h[SKY] >= 25                          # no point at all
    assert g["ref_draws"][RETRY] >= 8 and (np.delete(g["ref_draws"], RETRY) == 4).all()
    assert float(g["meta_margin"]) == 1e-6


def test_labels_masks_and_reject_decisions_equal_the_references(g, mine):
    off = g["off"]
    for d, f in enumerate(g["box_frame"]):
        n = int(off[f + 1] - off[f])
        idx = mine["index"][d]
        assert np.array_equal(idx, np.nonzero(g["ref_mask"][d, :n])[0]), d
        assert np.array_equal(mine["seg"][d] > 0, g["ref_label"][d, :n][idx]), d
        assert not g["ref_label"][d][~g["ref_mask"][d]].any()
        want = g["ref_rect"][off[f]:off[f + 1]][idx]
        assert np.array_equal(mine["rows"][d][:, :3].view(np.uint32), want.view(np.uint32)), d
    assert np.array_equal(mine["reject"], g["ref_reject"])
    assert np.array_equal(mine["kept"], np.nonzero(~g["ref_reject"])[0]) and 0 < len(mine["kept"]) < len(g["box_frame"])
    err = np.abs(mine["frustum_angle"] - g["ref_angle"])
    assert (err <= 1e-12).all()


def test_corners_equal_compute_box_3d_exactly(g, mine):
    """Exactly, when the referee restates the arithmetic np.dot used when the fixture was recorded (numpy's cos and sin, the last
    product fused into the sum); the left-to-right sum the kernels state rounds once more: within one spacing of a coordinate."""
    fused = np.stack([frustum_label_ref.corners(b, fused=True) for b in g["gt_box3d"]])
    assert np.array_equal(fused.view(np.uint64), g["ref_corners"].view(np.uint64))
    assert mine["corners"].shape == (len(g["box_frame"]), 8, 3)
    err = np.abs(mine["corners"] - g["ref_corners"])
    print("left-to-right corners: %d of %d coordinates differ from np.dot's, worst %.3e m" % ((err > 0).sum(), err.size, err.max()))
    assert (err <= np.spacing(np.abs(g["ref_corners"]))).all()
    assert np.array_equal(mine["corners"][:, :, 1], g["ref_corners"][:, :, 1])


def test_fixture_keeps_the_margin_and_exercises_it(g, mine):
    face = np.concatenate(mine["face"])
    print("smallest face distance %.3e m; %d rows within 1e-4 m, %d within 1e-3 m" %
          (face.min(), int((face < 1e-4).sum()), int((face < 1e-3).sum())))
    assert face.min() >= float(g["meta_margin"])
    assert (face < 1e-4).sum() >= 30
    near = [s[f < 1e-3] for s, f in zip(mine["seg"], mine["face"])]
    assert sum(int(s.sum()) for s in near) >= 10 and sum(int((s == 0).sum()) for s in near) >= 10      # both sides of a face


def test_perturb_boxes2d_equals_random_shift_box2d_bit_for_bit(g):
    from frustum_convnet_amd import frustum
    wh = g["img_wh"][g["box_frame"]]
    np.random.seed(int(g["meta_seed"]))
    got = frustum.perturb_boxes2d(g["gt_box2d"], wh)
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), g["ref_boxes"].view(np.uint64))
    assert np.random.random() == float(g["ref_next_draw"])                    # the generator is in the reference's state
    rs = np.random.RandomState(int(g["meta_seed"]))                           # an rng of the caller's
    assert np.array_equal(frustum.perturb_boxes2d(g["gt_box2d"], wh, rng=rs), g["ref_boxes"])
    assert rs.random_sample() == float(g["ref_next_draw"])
    # one image size for every box
    rs = np.random.RandomState(1)
    one = frustum.perturb_boxes2d(g["gt_box2d"][:5], g["img_wh"][0], rng=rs)
    rs = np.random.RandomState(1)
    assert np.array_equal(one, frustum.perturb_boxes2d(g["gt_box2d"][:5], wh[:5], rng=rs))
    assert not np.array_equal(one, g["gt_box2d"][:5])


def test_perturb_boxes2d_refuses_what_the_reference_cannot_finish():
    from frustum_convnet_amd import frustum
    rs = np.random.RandomState(0)
    state = rs.get_state()[1].copy()
    for bad in ([10.0, 10.0, 10.0, 50.0], [10.0, 50.0, 60.0, 50.0], [30.0, 10.0, 20.0, 50.0], [np.nan, 1.0, 2.0, 3.0]):
        with pytest.raises(ValueError):                                       # the reference asserts
            frustum.perturb_boxes2d([bad], [1242.0, 375.0], rng=rs)
    for beyond in ([1300.0, 100.0, 1400.0, 200.0], [-300.0, 100.0, -100.0, 200.0], [100.0, 500.0, 200.0, 600.0],
                   [100.0, -90.0, 200.0, -20.0]):
        with pytest.raises(ValueError):                                       # the reference would loop for ever
            frustum.perturb_boxes2d([beyond], [1242.0, 375.0], rng=rs)
    assert np.array_equal(rs.get_state()[1], state)                           # refused before a draw
    assert frustum.perturb_boxes2d(np.zeros((0, 4)), [1242.0, 375.0]).shape == (0, 4)
