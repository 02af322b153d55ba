"""CPU: the fp64 referee of the cascade link (tests/cascade_ref.py) against the reference's own compute_box_3d_obj_array and
extract_pc_in_box3d, recorded in tests/golden/cascade_select.npz (make_golden_cascade.py).  The fixture's points keep at least
meta_margin (1 mm) from every face plane of their enlarged box: the reference's Delaunay test has a tolerance at the faces, the
referee's box is closed and exact, and beyond that margin the two must agree on EVERY point."""
import numpy as np

import cascade_ref
from helpers import load_golden


def test_referee_matches_the_reference_corners_and_masks():
    g = load_golden("cascade_select")
    ratio, margin = float(g["meta_ratio"]), float(g["meta_margin"])
    assert ratio == 1.2 and margin == 1e-3
    dets, pts = g["dets"], g["points"]
    assert dets.dtype == np.float32 and pts.dtype == np.float32
    close = 0
    for b in range(len(dets)):
        centre, size, ry = cascade_ref.enlarged_box(dets[b], ratio)
        # the un-enlarged and the enlarged box: corner order and centre convention of prepare_data_refine.py:715-727
        for r, key in ((1.0, "ref_corners"), (ratio, "ref_corners_enlarged")):
            c, s, a = cascade_ref.enlarged_box(dets[b], r)
            mine_c = cascade_ref.box_corners(c, s, a)
            assert cascade_ref.within(mine_c, g[key][b], extent=s.max()), (b, key, cascade_ref.worst(mine_c, g[key][b], s.max()))
        dist = cascade_ref.face_distance(pts[b], centre, size, ry)
        assert dist.min() >= margin, (b, dist.min())
        close += int((dist < 5e-3).sum())
        mine = cascade_ref.inside(pts[b], centre, size, ry)
        assert np.array_equal(mine, g["ref_mask"][b]), (b, int((mine != g["ref_mask"][b]).sum()))
        assert 0 < mine.sum() < len(mine)
    assert close >= 100          # the margin is tested: points within 5 mm of a face exist in numbers


def test_referee_select_and_non_finite_points():
    rng = np.random.RandomState(5)
    pts = rng.uniform(-1, 1, (50, 4)).astype(np.float32)
    pts[3, 0], pts[4, 1], pts[5, 2], pts[6, 3] = np.nan, np.inf, -np.inf, np.nan
    dets = np.array([[0, 5, 0, 10, 10, 10, 0.3, 0.9]], dtype=np.float32)          # holds every finite point
    out = cascade_ref.select(pts, [0, 50, 50], dets, [0, 0], [0, 1])
    assert out["index"][0].tolist() == [i for i in range(50) if i not in (3, 4, 5)]      # a NaN in column 3 does not matter
    assert out["counts"].tolist() == [47, 0] and out["pred_size"][0].tolist() == [12.0, 12.0, 12.0]
    assert out["pred_angle"][0] == np.float64(np.float32(0.3))
