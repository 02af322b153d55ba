"""TEST INFRASTRUCTURE ONLY: the fp64 numpy referee of the labelled frustum extraction (fcn_frustum_label_count / _fill,
frustum.frustum_training_candidates): the in-box mask on float32 rect rows (the analytic restatement of
kitti/prepare_data.py::extract_pc_in_box3d :31-41 on compute_box_3d's corners), the corners of kitti_util.compute_box_3d
(:324-359), the reject rule (prepare_data.py:354), and select_labeled on top of frustum_ref.select, in the operation order the
kernels state (every sum left to right).  tests/golden/frustum_label.npz pins it to the reference's own functions
(tests/golden/make_golden_frustum_label.py, tests/test_frustum_label_referee.py).  Never imported by the product."""
from fractions import Fraction

import numpy as np

import frustum_ref


def _box(gt):
    tx, ty, tz, l, w, h, ry = (float(v) for v in np.asarray(gt, dtype=np.float64).reshape(7))
    return tx, ty, tz, l, w, h, np.cos(ry), np.sin(ry)


def box_axes(rect32, gt):
    """float32 rect rows (n,3) -> ax, dy, az (fp64): the rows in the box's own axes, from its bottom centre."""
    tx, ty, tz, _, _, _, c, s = _box(gt)
    p = np.asarray(rect32, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    dx, dy, dz = p[:, 0] - tx, p[:, 1] - ty, p[:, 2] - tz
    return c * dx - s * dz, dy, s * dx + c * dz


def in_box(rect32, gt):
    """Inside iff |ax| <= l/2, |az| <= w/2 and -h <= dy <= 0; a face counts as inside."""
    _, _, _, l, w, h, _, _ = _box(gt)
    ax, dy, az = box_axes(rect32, gt)
    return (np.abs(ax) <= l / 2.0) & (np.abs(az) <= w / 2.0) & (dy >= -h) & (dy <= 0.0)


def face_distance(rect32, gt):
    """Per row the distance (metres) to the nearest of the six face PLANES of the box."""
    _, _, _, l, w, h, _, _ = _box(gt)
    ax, dy, az = box_axes(rect32, gt)
    return np.min(np.stack([np.abs(np.abs(ax) - l / 2.0), np.abs(np.abs(az) - w / 2.0), np.abs(dy), np.abs(dy + h)]), 0)


def _fma(a, b, c):
    """round(a * b + c) with ONE rounding, through exact rational arithmetic: the same on every machine."""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def corners(gt, fused=False):
    """compute_box_3d: roty(ry) . (x_k, y_k, z_k) + t in its corner order -> (8,3).  As the kernels state it: every product
    rounded, sums left to right.  fused=True: as the reference's np.dot evaluated it when the fixture was recorded -- the BLAS
    kernel keeps the first product and adds the last with a fused multiply-add, acc = c * x_k (+ 0 * y_k), fma(s, z_k, acc) --
    which differs from the plain sum by at most one rounding of a coordinate."""
    tx, ty, tz, l, w, h, c, s = _box(gt)
    xc = np.array([l / 2, l / 2, -l / 2, -l / 2, l / 2, l / 2, -l / 2, -l / 2])
    yc = np.array([0.0, 0.0, 0.0, 0.0, -h, -h, -h, -h])
    zc = np.array([w / 2, -w / 2, -w / 2, w / 2, w / 2, -w / 2, -w / 2, w / 2])
    if fused:
        x = np.array([_fma(s, zc[k], c * xc[k]) for k in range(8)])
        z = np.array([_fma(c, zc[k], (-s) * xc[k]) for k in range(8)])
    else:
        x, z = c * xc + s * zc, (-s) * xc + c * zc
    return np.stack([x + tx, yc + ty, z + tz], 1)


def reject(gt_box2d, positives, min_box_height=25.0):
    """prepare_data.py:354."""
    return bool((gt_box2d[3] - gt_box2d[1]) < min_box_height or positives == 0)


def select_labeled(frame_pts, frame_off, P, V2C, R0, img_wh, boxes, box_frame, gt_box3d, gt_box2d=None, min_box_height=25.0,
                   clip_distance=2.0):
    """frustum_ref.select without clipping, plus per box: seg (the labels of its rows, int64), pos (their sum), corners (8,3),
    face (the rows' face distances) and reject; 'kept': the indices of the boxes that are not rejected."""
    out = frustum_ref.select(frame_pts, frame_off, P, V2C, R0, img_wh, boxes, box_frame, clip_boxes=False, clip_distance=clip_distance)
    gt2d = np.asarray(boxes if gt_box2d is None else gt_box2d, dtype=np.float64).reshape(-1, 4)
    D = len(box_frame)
    out.update(seg=[], face=[], pos=np.zeros(D, dtype=np.int64), corners=np.zeros((D, 8, 3)), reject=np.zeros(D, dtype=bool))
    for d in range(D):
        seg = in_box(out["rows"][d][:, :3], gt_box3d[d]).astype(np.int64)
        out["seg"].append(seg)
        out["face"].append(face_distance(out["rows"][d][:, :3], gt_box3d[d]))
        out["pos"][d] = seg.sum()
        out["corners"][d] = corners(gt_box3d[d])
        out["reject"][d] = reject(gt2d[d], out["pos"][d], min_box_height)
    out["kept"] = np.nonzero(~out["reject"])[0].astype(np.int64)
    return out
