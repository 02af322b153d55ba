"""TEST INFRASTRUCTURE ONLY: the fp64 numpy referee of the cascade link (fcn_refine_select_count / _fill): the enlarged box of
kitti/prepare_data_refine.py:715-727, its corners in the order of compute_box_3d_obj_array (:56-79) and the closed-box inside
test the kernels state.  tests/golden/cascade_select.npz pins it to the reference's own functions
(tests/golden/make_golden_cascade.py, tests/test_cascade_referee.py).  Never imported by the product."""
import numpy as np


def enlarged_box(det_row, ratio=1.2):
    """A label-format row [tx, ty, tz, l, w, h, ry, ...] (ty = box bottom) -> centre (3), size (l, w, h) * ratio, ry; fp64."""
    r = np.asarray(det_row, dtype=np.float64)
    l, w, h = r[3], r[4], r[5]
    centre = np.array([r[0], r[1] - h / 2.0, r[2]])
    return centre, np.array([l * ratio, w * ratio, h * ratio]), r[6]


def box_corners(centre, size, ry):
    """(8,3): x = l/2 * (+ + - - + + - -), y = h/2 * (+ + + + - - - -), z = w/2 * (+ - - + + - - +), rotated by roty(ry), + centre."""
    l, w, h = size
    c, s = np.cos(ry), np.sin(ry)
    x = np.array([l, l, -l, -l, l, l, -l, -l]) / 2.0
    y = np.array([h, h, h, h, -h, -h, -h, -h]) / 2.0
    z = np.array([w, -w, -w, w, w, -w, -w, w]) / 2.0
    return np.stack([(c * x + s * z) + centre[0], y + centre[1], (-s * x + c * z) + centre[2]], 1)


def box_frame(xyz, centre, ry):
    """Points (n,3) -> (x', dy, z'): p - centre rotated back by ry; fp64."""
    p = np.asarray(xyz, dtype=np.float64)
    dx, dy, dz = p[:, 0] - centre[0], p[:, 1] - centre[1], p[:, 2] - centre[2]
    c, s = np.cos(ry), np.sin(ry)
    return c * dx - s * dz, dy, s * dx + c * dz


def inside(xyz, centre, size, ry):
    """Closed box: |x'| <= l/2, |dy| <= h/2, |z'| <= w/2; a point with a non-finite coordinate is outside."""
    l, w, h = size
    with np.errstate(invalid="ignore"):
        lx, dy, lz = box_frame(xyz, centre, ry)
        m = (np.abs(lx) <= l / 2.0) & (np.abs(dy) <= h / 2.0) & (np.abs(lz) <= w / 2.0)
    return m & np.isfinite(np.asarray(xyz, dtype=np.float64)[:, :3]).all(1)


def face_distance(xyz, centre, size, ry):
    """Distance (n,) of each point to the nearest of the box's six face PLANES."""
    l, w, h = size
    lx, dy, lz = box_frame(xyz, centre, ry)
    return np.minimum(np.minimum(np.abs(np.abs(lx) - l / 2.0), np.abs(np.abs(dy) - h / 2.0)), np.abs(np.abs(lz) - w / 2.0))


def within(got, want, extent=0.0, rel=1e-12):
    """Element-wise |got - want| <= rel * max(|want|, extent).  `extent` (the box's largest edge) is the floor for a corner
    coordinate: it is centre + rotated half edge, a sum that may cancel to nearly zero while its rounding error stays that of
    its terms, so a bound relative to the coordinate alone is not meaningful there.  Heading and size use extent = 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= rel * np.maximum(np.abs(want), extent)).all())


def worst(got, want, extent=0.0):
    """The largest |got - want| / max(|want|, extent) (0 where both are 0): the figure `within` bounds."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    den = np.maximum(np.abs(want), extent)
    return float(np.max(np.where(den > 0, np.abs(got - want) / np.where(den > 0, den, 1.0), np.abs(got - want)), initial=0.0))


def select(frame_pts, frame_off, dets, cand_row, cand_frame, ratio=1.2):
    """What the two entry points produce: pred_box3d (D,8,3), pred_angle (D), pred_size (D,3) fp64, counts (D) and, per
    candidate, the INDICES (ascending, frame-relative) of its frame's rows inside the enlarged box."""
    D = len(cand_row)
    out = {"pred_box3d": np.zeros((D, 8, 3)), "pred_angle": np.zeros(D), "pred_size": np.zeros((D, 3)),
           "counts": np.zeros(D, dtype=np.int64), "index": []}
    for d in range(D):
        centre, size, ry = enlarged_box(dets[cand_row[d]], ratio)
        f = int(cand_frame[d])
        pts = frame_pts[int(frame_off[f]):int(frame_off[f + 1])]
        idx = np.nonzero(inside(pts[:, :3], centre, size, ry))[0]
        out["pred_box3d"][d], out["pred_angle"][d], out["pred_size"][d] = box_corners(centre, size, ry), ry, size
        out["counts"][d] = len(idx)
        out["index"].append(idx)
    return out
