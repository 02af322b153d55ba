"""CPU: the fp64 referee of the frustum extraction (tests/frustum_ref.py) against the reference's own functions, recorded in
tests/golden/frustum_select.npz by tests/golden/make_golden_frustum.py (kitti_util.Calibration, project_velo_to_rect,
draw_util.get_lidar_in_image_fov, project_image_to_rect and the clipping / mask / skip lines of kitti/prepare_data.py:523-548)."""
import os

import numpy as np
import pytest

import frustum_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frustum_select.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(GOLDEN))


@pytest.fixture(scope="module")
def mine(g):
    return frustum_ref.select(g["points"], g["off"], g["P"], g["V2C"], g["R0"], g["img_wh"], g["boxes"], g["box_frame"])


def test_fixture_is_small_and_shaped_as_documented(g):
    assert os.path.getsize(GOLDEN) < 256 * 1024
    assert len(g["off"]) == 3 and (np.diff(g["off"]) <= 3000).all() and g["points"].dtype == np.float32
    assert g["ref_rect"].dtype == np.float32 and len(g["boxes"]) >= 8


def test_every_mask_equals_the_references(g, mine):
    off = g["off"]
    for f in range(2):
        pts = g["points"][off[f]:off[f + 1]]
        _, u, v = frustum_ref.project(pts[:, :3], g["P"][f], g["V2C"][f], g["R0"][f])
        fov = frustum_ref.fov_mask(pts, u, v, g["img_wh"][f][0], g["img_wh"][f][1])
        assert np.array_equal(fov, g["ref_fov"][off[f]:off[f + 1]]), f
    for d, f in enumerate(g["box_frame"]):
        n = int(off[f + 1] - off[f])
        assert np.array_equal(mine["index"][d], np.nonzero(g["ref_mask"][d, :n])[0]), d
        assert not g["ref_mask"][d, n:].any()
    assert np.array_equal(mine["box2d"], g["ref_box2d"])
    got_skip = [frustum_ref.skip(mine["box2d"][d], mine["counts"][d]) for d in range(len(g["boxes"]))]
    assert got_skip == g["ref_skip"].tolist()
    assert 0 < sum(got_skip) < len(got_skip)
    # the three skip rules each decide a box of the fixture
    b, c = mine["box2d"], mine["counts"]
    assert ((b[:, 3] - b[:, 1] < 5) & (c > 0)).any() and (b[:, 2] - b[:, 0] < 1).any()
    assert ((c == 0) & (b[:, 3] - b[:, 1] >= 5) & (b[:, 2] - b[:, 0] >= 1)).any()


def test_every_float32_rect_coordinate_equals_the_references(g, mine):
    off = g["off"]
    for f in range(2):
        rect, _, _ = frustum_ref.project(g["points"][off[f]:off[f + 1], :3], g["P"][f], g["V2C"][f], g["R0"][f])
        assert np.array_equal(rect.astype(np.float32).view(np.uint32), g["ref_rect"][off[f]:off[f + 1]].view(np.uint32)), f
    for d, f in enumerate(g["box_frame"]):
        want = g["ref_rect"][off[f]:off[f + 1]][mine["index"][d]]
        assert np.array_equal(mine["rows"][d][:, :3].view(np.uint32), want.view(np.uint32)), d
        assert np.array_equal(mine["rows"][d][:, 3].view(np.uint32), g["points"][off[f]:off[f + 1]][mine["index"][d], 3].view(np.uint32))


def test_angles_agree(g, mine):
    """1e-12 rad: the consumer stores the angle as float32, whose spacing near pi is 2e-7."""
    err = np.abs(mine["frustum_angle"] - g["ref_angle"])
    print("angle worst abs err %.3e" % err.max())
    assert (err <= 1e-12).all()
    assert np.ptp(g["ref_angle"]) > 0.5


def test_fixture_keeps_the_margin_and_exercises_it(g, mine):
    """A condition on the FIXTURE: every point stays >= 1e-6 px from every edge of the image and of the clipped boxes of its frame,
    and at least 50 points lie within 1e-3 px of one."""
    assert float(g["meta_margin"]) == 1e-6
    off = g["off"]
    near = 0
    for f in range(2):
        ds = [mine["edge"][d] for d in range(len(g["boxes"])) if g["box_frame"][d] == f]
        assert all(len(e) == off[f + 1] - off[f] for e in ds)                 # (every fixture point is finite)
        e = np.min(np.stack(ds), 0)
        print("frame %d: smallest edge distance %.3e px, %d points within 1e-3 px" % (f, e.min(), int((e < 1e-3).sum())))
        assert e.min() >= 1e-6
        near += int((e < 1e-3).sum())
    assert near >= 50
    # the clip distance is exact: x == 2.0 is out, the next float32 is in
    x = g["points"][:, 0]
    assert (x == np.float32(2.0)).any() and (x == np.nextafter(np.float32(2.0), np.float32(3.0))).any()
