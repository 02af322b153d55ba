"""TEST INFRASTRUCTURE ONLY: the fp64 numpy referee of the SUN-RGBD frustum extraction (fcn_frustum_sunrgbd_count / _fill /
_label_count / _label_fill, fcn_frustum_subset_pos, frustum.sunrgbd_candidates / sunrgbd_training_candidates) in the operation
order the kernels state, every sum left to right: the projection of sunrgbd_utils.SUNRGBD_Calibration
.project_upright_depth_to_image (:109-123), the frustum angle through project_image_to_upright_camera (:131-145), the closed
analytic in-box test (against the reference's Delaunay hull, extract_pc_in_box3d :231-234), compute_box_3d's corners (:237-268)
flipped to upright camera, and the reject rules of sunrgbd/prepare_data.py (:226, :352).  tests/golden/frustum_sunrgbd.npz pins
it to the reference's own run (tests/golden/make_golden_frustum_sunrgbd.py, tests/test_frustum_sunrgbd_referee.py).  Never
imported by the product."""
import numpy as np


def project(xyz32, K, Rtilt):
    """float32 upright-depth rows (n,3) -> u, v, camera depth (fp64)."""
    p = np.asarray(xyz32, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    k, r = np.asarray(K, dtype=np.float64).reshape(9), np.asarray(Rtilt, dtype=np.float64).reshape(9)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):             # (non-finite rows: box_mask never selects them)
        d0 = r[0] * x + r[3] * y + r[6] * z
        d1 = r[1] * x + r[4] * y + r[7] * z
        d2 = r[2] * x + r[5] * y + r[8] * z
        c0, c1, c2 = d0, -d2, d1
        i0 = k[0] * c0 + k[1] * c1 + k[2] * c2
        i1 = k[3] * c0 + k[4] * c1 + k[5] * c2
        i2 = k[6] * c0 + k[7] * c1 + k[8] * c2
        return i0 / i2, i1 / i2, c2


def box_mask(xyz32, u, v, box):
    """xmin <= u < xmax and ymin <= v < ymax; a row with a non-finite coordinate is never selected."""
    finite = np.isfinite(np.asarray(xyz32, dtype=np.float32).reshape(-1, 3)).all(1)
    with np.errstate(invalid="ignore"):
        return finite & (u >= box[0]) & (u < box[2]) & (v >= box[1]) & (v < box[3])


def edge_distance(u, v, box):
    """Per row the distance (pixels) to the nearest of the four edge LINES of the box."""
    return np.min(np.stack([np.abs(u - box[0]), np.abs(u - box[2]), np.abs(v - box[1]), np.abs(v - box[3])]), 0)


def frustum_angle(box, K, Rtilt):
    k, r = np.asarray(K, dtype=np.float64).reshape(9), np.asarray(Rtilt, dtype=np.float64).reshape(9)
    cu, cv = (box[0] + box[2]) / 2.0, (box[1] + box[3]) / 2.0
    X = ((cu - k[2]) * 20.0) / k[0]
    Y = ((cv - k[5]) * 20.0) / k[4]
    e0, e1, e2 = X, 20.0, -Y
    ud0 = r[0] * e0 + r[1] * e1 + r[2] * e2
    ud1 = r[3] * e0 + r[4] * e1 + r[5] * e2
    return -np.arctan2(ud1, ud0)


def _gt(gt):
    cx, cy, cz, l, w, h, heading = (float(x) for x in np.asarray(gt, dtype=np.float64).reshape(7))
    return cx, cy, cz, l, w, h, np.cos(-heading), np.sin(-heading)


def box_axes(xyz32, gt):
    """float32 upright-depth rows -> ax, ay, dz (fp64): the rows in the box's own axes, from its centroid."""
    cx, cy, cz, _, _, _, c, s = _gt(gt)
    p = np.asarray(xyz32, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    dx, dy, dz = p[:, 0] - cx, p[:, 1] - cy, p[:, 2] - cz
    return c * dx + s * dy, (-s) * dx + c * dy, dz


def in_box(xyz32, gt):
    """|ax| <= l, |ay| <= w, |dz| <= h with l, w, h the HALF extents; a face counts as inside."""
    _, _, _, l, w, h, _, _ = _gt(gt)
    ax, ay, dz = box_axes(xyz32, gt)
    return (np.abs(ax) <= l) & (np.abs(ay) <= w) & (np.abs(dz) <= h)


def face_distance(xyz32, gt):
    """Per row the distance (metres) to the nearest of the six face PLANES of the box."""
    _, _, _, l, w, h, _, _ = _gt(gt)
    ax, ay, dz = box_axes(xyz32, gt)
    return np.min(np.stack([np.abs(np.abs(ax) - l), np.abs(np.abs(ay) - w), np.abs(np.abs(dz) - h)]), 0)


def corners(gt):
    """compute_box_3d's corners in its order, flipped to upright camera (X, -Z, Y) -> (8,3)."""
    cx, cy, cz, l, w, h, c, s = _gt(gt)
    xc = np.array([-l, l, l, -l, -l, l, l, -l])
    yc = np.array([w, w, -w, -w, w, w, -w, -w])
    zc = np.array([h, h, h, h, -h, -h, -h, -h])
    X = (c * xc + (-s) * yc) + cx
    Y = (s * xc + c * yc) + cy
    Z = zc + cz
    return np.stack([X, -Z, Y], 1)


def to_upright_camera(rows):
    """(x, -z, y) of the input rows, the other columns untouched: an exact swap and negation."""
    out = np.array(rows, dtype=np.float32, copy=True)
    out[:, 1] = -rows[:, 2]
    out[:, 2] = rows[:, 1]
    return out


def select(frame_pts, frame_off, K, Rtilt, boxes, box_frame, gt_box3d=None):
    """Per box: index (the selected rows of its frame, ascending), rows (upright camera + untouched columns), edge (their edge
    distances), depth (their camera depth); counts, frustum_angle.  With gt_box3d also seg (int64 labels), face, pos, corners."""
    D = len(box_frame)
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    out = {"index": [], "rows": [], "edge": [], "depth": [], "counts": np.zeros(D, dtype=np.int64), "frustum_angle": np.zeros(D)}
    if gt_box3d is not None:
        out.update(seg=[], face=[], pos=np.zeros(D, dtype=np.int64), corners=np.zeros((D, 8, 3)))
    cache = {}
    for d in range(D):
        f = int(box_frame[d])
        if f not in cache:
            fr = frame_pts[int(frame_off[f]):int(frame_off[f + 1])]
            cache[f] = (fr,) + project(fr[:, :3], K[f], Rtilt[f])
        fr, u, v, depth = cache[f]
        idx = np.nonzero(box_mask(fr[:, :3], u, v, boxes[d]))[0]
        out["index"].append(idx)
        out["rows"].append(to_upright_camera(fr[idx]))
        out["edge"].append(edge_distance(u[idx], v[idx], boxes[d]))
        out["depth"].append(depth[idx])
        out["counts"][d] = len(idx)
        out["frustum_angle"][d] = frustum_angle(boxes[d], K[f], Rtilt[f])
        if gt_box3d is not None:
            seg = in_box(fr[idx, :3], gt_box3d[d]).astype(np.int64)
            out["seg"].append(seg)
            out["face"].append(face_distance(fr[idx, :3], gt_box3d[d]))
            out["pos"][d] = seg.sum()
            out["corners"][d] = corners(gt_box3d[d])
    return out


def training_kept(pos_full, seg, sub, min_positives=5):
    """The reject rule of prepare_data.py:226 on the positives AFTER the subsample -> the kept boxes' indices and their positives."""
    pos = np.asarray([int(s.sum()) if ix is None else int(s[np.asarray(ix)].sum()) for s, ix in zip(seg, sub)], dtype=np.int64)
    assert (pos <= np.asarray(pos_full)).all()
    return np.nonzero(pos >= min_positives)[0].astype(np.int64), pos


# ---- tests/golden/frustum_sunrgbd.npz (make_golden_frustum_sunrgbd.py)
def fixture_sub(g, which):
    """The reference's recorded subsample draws of the `which` ("train" / "det") run: one entry per box, None without a draw."""
    D = len(g["train_boxes"] if which == "train" else g["det_boxes"])
    sub = [None] * D
    for d, ix in zip(g[which + "_sub_box"], g[which + "_sub"]):
        sub[int(d)] = ix.astype(np.int32)
    return sub


def fixture_records(g, which):
    """Per record the reference pickled: (box index, row indices into its frame in record order, labels or None)."""
    off = g[which + "_index_off"]
    lab = np.unpackbits(g["train_label"])[:int(off[-1])].astype(np.int64) if which == "train" else None
    return [(int(d), g[which + "_index"][int(off[k]):int(off[k + 1])].astype(np.int64),
             None if lab is None else lab[int(off[k]):int(off[k + 1])]) for k, d in enumerate(g[which + "_kept"])]
