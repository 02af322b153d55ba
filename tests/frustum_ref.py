"""TEST INFRASTRUCTURE ONLY: the fp64 numpy referee of the frustum extraction (fcn_frustum_select_count / _fill): the projection
chain of kitti_util.Calibration (project_velo_to_rect, project_rect_to_image), the FOV and box masks of
draw_util.get_lidar_in_image_fov and kitti/prepare_data.py:523-548, the box clipping and the frustum angle, in the operation order
the kernels state (every sum left to right).  tests/golden/frustum_select.npz pins it to the reference's own functions
(tests/golden/make_golden_frustum.py, tests/test_frustum_referee.py).  Never imported by the product."""
import numpy as np


def project(xyz, P, V2C, R0):
    """(n,3) float32 velodyne rows -> rect (n,3) fp64 and u, v (n,) fp64.  Non-finite inputs give non-finite outputs."""
    p = np.asarray(xyz, dtype=np.float64)
    P, V2C, R0 = (np.asarray(m, dtype=np.float64).reshape(s) for m, s in ((P, (3, 4)), (V2C, (3, 4)), (R0, (3, 3))))
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        ref = [V2C[r, 0] * x + V2C[r, 1] * y + V2C[r, 2] * z + V2C[r, 3] for r in range(3)]
        rect = [R0[r, 0] * ref[0] + R0[r, 1] * ref[1] + R0[r, 2] * ref[2] for r in range(3)]
        img = [P[r, 0] * rect[0] + P[r, 1] * rect[1] + P[r, 2] * rect[2] + P[r, 3] for r in range(3)]
        u, v = img[0] / img[2], img[1] / img[2]
    return np.stack(rect, 1), u, v


def clip_box(box, W, H, clip=True):
    """prepare_data.py:523-524: x to [0, W-1], y to [0, H-1]."""
    b = np.asarray(box, dtype=np.float64).copy()
    if clip:
        b[[0, 2]] = np.clip(b[[0, 2]], 0, W - 1)
        b[[1, 3]] = np.clip(b[[1, 3]], 0, H - 1)
    return b


def frustum_angle(box, P):
    """prepare_data.py:537-543 through project_image_to_rect: -arctan2(20, x of the box centre's ray at depth 20)."""
    P = np.asarray(P, dtype=np.float64).reshape(3, 4)
    cu = (box[0] + box[2]) / 2.0
    x = ((cu - P[0, 2]) * 20.0) / P[0, 0] + P[0, 3] / (-P[0, 0])
    return -np.arctan2(20.0, x)


def fov_mask(xyz, u, v, W, H, clip_distance=2.0):
    """get_lidar_in_image_fov(pc_velo, calib, 0, 0, W, H): in the image and VELODYNE x > clip_distance; finite rows only."""
    xyz = np.asarray(xyz)
    with np.errstate(invalid="ignore"):
        m = (u < W) & (u >= 0) & (v < H) & (v >= 0) & (xyz[:, 0].astype(np.float64) > clip_distance)
    return m & np.isfinite(xyz[:, :3].astype(np.float64)).all(1)


def box_mask(u, v, box):
    with np.errstate(invalid="ignore"):
        return (u < box[2]) & (u >= box[0]) & (v < box[3]) & (v >= box[1])


def edge_distance(u, v, box, W, H):
    """Per point: the smallest of |u - e| over xmin, xmax, 0, W and |v - e| over ymin, ymax, 0, H (inf where u / v is not finite)."""
    with np.errstate(invalid="ignore"):
        du = np.min(np.abs(np.stack([u - box[0], u - box[2], u - 0.0, u - W])), 0)
        dv = np.min(np.abs(np.stack([v - box[1], v - box[3], v - 0.0, v - H])), 0)
        d = np.minimum(du, dv)
    return np.where(np.isfinite(d), d, np.inf)


def skip(box, count, img_height_threshold=5, lidar_point_threshold=1):
    """prepare_data.py:546-548."""
    return bool(box[3] - box[1] < img_height_threshold or box[2] - box[0] < 1 or count < lidar_point_threshold)


def select(frame_pts, frame_off, P, V2C, R0, img_wh, boxes, box_frame, clip_boxes=True, clip_distance=2.0):
    """What the two entry points produce: box2d (D,4), frustum_angle (D), counts (D), per box the INDICES (ascending,
    frame-relative) of the selected rows and the rows themselves: float32 rect x, y, z + the untouched columns."""
    D = len(box_frame)
    out = {"box2d": np.zeros((D, 4)), "frustum_angle": np.zeros(D), "counts": np.zeros(D, dtype=np.int64), "index": [],
           "rows": [], "edge": []}
    for d in range(D):
        f = int(box_frame[d])
        W, H = float(img_wh[f][0]), float(img_wh[f][1])
        pts = np.asarray(frame_pts[int(frame_off[f]):int(frame_off[f + 1])], dtype=np.float32)
        rect, u, v = project(pts[:, :3], P[f], V2C[f], R0[f])
        box = clip_box(boxes[d], W, H, clip_boxes)
        idx = np.nonzero(box_mask(u, v, box) & fov_mask(pts, u, v, W, H, clip_distance))[0]
        rows = pts[idx].copy()
        rows[:, :3] = rect[idx].astype(np.float32)
        out["box2d"][d], out["frustum_angle"][d], out["counts"][d] = box, frustum_angle(box, P[f]), len(idx)
        out["index"].append(idx)
        out["rows"].append(rows)
        fin = np.isfinite(pts[:, :3].astype(np.float64)).all(1)
        out["edge"].append(edge_distance(u[fin], v[fin], box, W, H))
    return out
