#!/usr/bin/env python
"""Golden fixture that pins the frustum extraction's referee (tests/frustum_ref.py) to the reference: runs the reference's OWN
kitti_util.Calibration(None, calib_dict=...), project_velo_to_rect, draw_util.get_lidar_in_image_fov and project_image_to_rect
(imported read-only from /root/reference, CPU; cv2 is not installed and is stood in by an empty module) on two synthetic frames
of float32 velodyne points with KITTI-like calibrations, and around them applies the box clipping and mask lines of
kitti/prepare_data.py:523-548.  Stored: the inputs, the reference's float32 pc_rect, its FOV mask and, per box, its mask, the
clipped box, the frustum angle and the skip decision.

Condition on the inputs: the reference multiplies with np.dot (BLAS order), the referee sums left to right, so their u, v may
differ in the last bits; a point closer than MARGIN pixels (judged by the fp64 referee) to an edge of the image or of a clipped
box of its frame is not admitted.  Points are PLACED next to the edges on purpose -- edge pixels back-projected at a random
depth, nudged by up to 1e-3 px, rounded to float32, kept when outside the margin -- so that the margin is what separates the two,
not a lack of close points.  On every admitted point the reference's masks must equal the referee's (asserted here).

Usage:  python tests/golden/make_golden_frustum.py
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import frustum_ref  # noqa: E402

MARGIN = 1e-6          # pixels
NEAR = 1e-3            # pixels: "next to an edge"
COUNTS = (2600, 2200)
NEAR_PER_FRAME = 160

# KITTI-like calibrations (the layout and magnitudes of a KITTI object calib file; frame 1 is a perturbed copy)
P2 = np.array([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
R0 = np.array([[0.9999239, 0.00983776, -0.007445048], [-0.009869795, 0.9999421, -0.004278459], [0.007402527, 0.004351614, 0.9999631]])
V2C = np.array([[0.007533745, -0.9999714, -0.000616602, -0.004069766], [0.01480249, 0.0007280733, -0.9998902, -0.07631618],
                [0.9998621, 0.00752379, 0.01480755, -0.2717806]])
IMG_WH = np.array([[1242.0, 375.0], [1224.0, 370.0]])
# xmin ymin xmax ymax as a 2-D detector writes them, frame of each
BOXES = np.array([[300.25, 150.5, 520.75, 300.0],        # 0: inside the image
                  [-40.0, 100.0, 200.5, 420.0],          # 1: straddles the left and bottom border: clipped
                  [1100.0, -30.0, 1300.0, 200.0],        # 2: straddles the right and top border: clipped
                  [1400.0, 100.0, 1500.0, 200.0],        # 3: outside the image: xmin = xmax = W - 1 after clipping, skipped
                  [600.0, 180.0, 700.0, 183.5],          # 4: 3.5 px high: skipped by img_height_threshold
                  [500.0, 20.0, 760.0, 330.0],           # 5: frame 1, inside
                  [0.0, 0.0, 1223.0, 369.0],             # 6: frame 1, the whole (clipped) image
                  [640.0, 2.0, 660.0, 9.0],              # 7: frame 1, sky: no LiDAR point, skipped by lidar_point_threshold
                  [900.2, 160.0, 900.9, 260.0]])         # 8: frame 1, 0.7 px wide: skipped
BOX_FRAME = np.array([0, 0, 0, 0, 0, 1, 1, 1, 1], dtype=np.int32)
EMPTY_BOX = 7          # no point is placed next to this box's edges either


def import_reference():
    """kitti_util and draw_util import OpenCV (and draw_util the dataset readers) at module level; the functions used here need
    numpy only, so modules that are not installed are stood in by empty ones."""
    import importlib
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "kitti"))
    if "cv2" not in sys.modules:
        try:
            importlib.import_module("cv2")
        except ImportError:
            sys.modules["cv2"] = types.ModuleType("cv2")
    for _ in range(16):
        try:
            return importlib.import_module("kitti.kitti_util"), importlib.import_module("kitti.draw_util")
        except ImportError as e:
            name = getattr(e, "name", None)
            if not name:
                raise
            mod = types.ModuleType(name)
            mod.__path__ = []
            mod.__getattr__ = lambda attr: None
            sys.modules[name] = mod
    raise RuntimeError("could not import the reference modules")


def calibs():
    rng = np.random.RandomState(5)
    out = [(P2, V2C, R0)]
    out.append((P2 * (1.0 + 1e-3 * rng.uniform(-1, 1, P2.shape)) * (P2 != 0), V2C + 1e-3 * rng.uniform(-1, 1, V2C.shape),
                R0 + 1e-4 * rng.uniform(-1, 1, R0.shape)))
    return out


def rect_to_velo(rect, V2C_, R0_):
    ref = np.linalg.solve(R0_, rect.T).T
    return np.linalg.solve(V2C_[:, :3], (ref - V2C_[:, 3]).T).T


def edge_all(pts, f, cal, boxes_f):
    """Smallest edge distance of every point over the image and ALL clipped boxes of frame f (inf for points that cannot matter)."""
    _, u, v = frustum_ref.project(pts[:, :3], *cal)
    W, H = IMG_WH[f]
    d = np.full(len(pts), np.inf)
    for b in boxes_f:
        d = np.minimum(d, frustum_ref.edge_distance(u, v, frustum_ref.clip_box(b, W, H), W, H))
    return d


def near_edge_points(rng, n, f, cal, boxes_f):
    """Candidates next to an edge: a pixel on a random edge (of the image or of a clipped box), nudged across it by up to NEAR,
    back-projected at a random depth and rounded to float32."""
    P_, V2C_, R0_ = cal
    W, H = IMG_WH[f]
    rects = [np.array([0.0, 0.0, W, H])] + [frustum_ref.clip_box(b, W, H) for b in boxes_f if not np.array_equal(b, BOXES[EMPTY_BOX])]
    out = []
    for _ in range(n):
        r = rects[rng.randint(len(rects))]
        nudge = rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-5.5, -3.0)
        if rng.rand() < 0.5:
            u, v = r[[0, 2]][rng.randint(2)] + nudge, rng.uniform(max(r[1], 0.0), max(min(r[3], H), 1.0))
        else:
            u, v = rng.uniform(max(r[0], 0.0), max(min(r[2], W), 1.0)), r[[1, 3]][rng.randint(2)] + nudge
        z = rng.uniform(4.0, 60.0)
        x = ((u - P_[0, 2]) * z) / P_[0, 0] + P_[0, 3] / (-P_[0, 0])
        y = ((v - P_[1, 2]) * z) / P_[1, 1] + P_[1, 3] / (-P_[1, 1])
        out.append(rect_to_velo(np.array([[x, y, z]]), V2C_, R0_)[0])
    return np.asarray(out, dtype=np.float32)


def main():
    ku, du = import_reference()
    rng = np.random.RandomState(20261018)
    cals = calibs()
    frames, near_kept = [], []
    for f, n in enumerate(COUNTS):
        boxes_f = BOXES[BOX_FRAME == f]
        cand = near_edge_points(rng, 40 * NEAR_PER_FRAME, f, cals[f], boxes_f)
        d = edge_all(cand, f, cals[f], boxes_f)
        _, cu, cv = frustum_ref.project(cand, *cals[f])
        empty = frustum_ref.box_mask(cu, cv, BOXES[EMPTY_BOX]) if BOX_FRAME[EMPTY_BOX] == f else np.zeros(len(cand), dtype=bool)
        cand = cand[(d >= MARGIN) & (d < NEAR) & ~empty][:NEAR_PER_FRAME]
        near_kept.append(len(cand))
        m = n - len(cand)
        xyz = np.stack([rng.uniform(-5.0, 70.0, m), rng.uniform(-30.0, 30.0, m), rng.uniform(-2.5, 1.5, m)], 1).astype(np.float32)
        xyz[:8, 0] = [2.0, np.nextafter(np.float32(2.0), np.float32(3.0)), 1.9999999, 2.5, 0.0, -3.0, 2.0, 2.0000002]
        for _ in range(100):
            close = edge_all(xyz, f, cals[f], boxes_f) < MARGIN
            if not close.any():
                break
            xyz[close, 1] = rng.uniform(-30.0, 30.0, int(close.sum())).astype(np.float32)
        else:
            raise RuntimeError("re-draw did not terminate")
        xyz = np.concatenate([xyz, cand], 0)
        xyz = xyz[rng.permutation(len(xyz))]
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)).astype(np.float32)], 1))
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    pts = np.concatenate(frames, 0)
    # ---- the reference, frame by frame and box by box (prepare_data.py:504-548)
    D, nmax = len(BOXES), max(COUNTS)
    ref_rect = np.zeros((len(pts), 3), dtype=np.float32)
    ref_fov = np.zeros(len(pts), dtype=bool)
    ref_mask = np.zeros((D, nmax), dtype=bool)
    ref_box, ref_angle, ref_skip = np.zeros((D, 4)), np.zeros(D), np.zeros(D, dtype=bool)
    cache = {}
    for d in range(D):
        f = int(BOX_FRAME[d])
        P_, V2C_, R0_ = cals[f]
        img_width, img_height = int(IMG_WH[f][0]), int(IMG_WH[f][1])
        if f not in cache:
            calib = ku.Calibration(None, calib_dict={"P2": P_.reshape(12).copy(), "Tr_velo_to_cam": V2C_.reshape(12).copy(),
                                                     "R0_rect": R0_.reshape(9).copy()})
            pc_velo = frames[f]
            pc_rect = np.zeros_like(pc_velo)
            pc_rect[:, 0:3] = calib.project_velo_to_rect(pc_velo[:, 0:3])
            pc_rect[:, 3] = pc_velo[:, 3]
            _, pc_image_coord, img_fov_inds = du.get_lidar_in_image_fov(pc_velo[:, 0:3], calib, 0, 0, img_width, img_height, True)
            cache[f] = (calib, pc_rect, pc_image_coord, img_fov_inds)
            ref_rect[off[f]:off[f + 1]] = pc_rect[:, :3]
            ref_fov[off[f]:off[f + 1]] = img_fov_inds
        calib, pc_rect, pc_image_coord, img_fov_inds = cache[f]
        det_box2d = BOXES[d].copy()
        det_box2d[[0, 2]] = np.clip(det_box2d[[0, 2]], 0, img_width - 1)
        det_box2d[[1, 3]] = np.clip(det_box2d[[1, 3]], 0, img_height - 1)
        xmin, ymin, xmax, ymax = det_box2d
        box_fov_inds = (pc_image_coord[:, 0] < xmax) & (pc_image_coord[:, 0] >= xmin) & \
                       (pc_image_coord[:, 1] < ymax) & (pc_image_coord[:, 1] >= ymin)
        box_fov_inds = box_fov_inds & img_fov_inds
        uvdepth = np.zeros((1, 3))
        uvdepth[0, 0:2] = np.array([(xmin + xmax) / 2.0, (ymin + ymax) / 2.0])
        uvdepth[0, 2] = 20
        box2d_center_rect = calib.project_image_to_rect(uvdepth)
        ref_angle[d] = -1 * np.arctan2(box2d_center_rect[0, 2], box2d_center_rect[0, 0])
        ref_skip[d] = bool(ymax - ymin < 5 or xmax - xmin < 1 or int(box_fov_inds.sum()) < 1)
        ref_box[d] = det_box2d
        ref_mask[d, :len(box_fov_inds)] = box_fov_inds
    # ---- the referee must agree on every admitted point
    Ps, Vs, Rs = (np.stack([c[i] for c in cals]) for i in range(3))
    mine = frustum_ref.select(pts, off, Ps, Vs, Rs, IMG_WH, BOXES, BOX_FRAME)
    for d in range(D):
        n = COUNTS[BOX_FRAME[d]]
        assert np.array_equal(np.nonzero(ref_mask[d, :n])[0], mine["index"][d]), "box %d: masks differ" % d
        assert mine["edge"][d].min() >= MARGIN, (d, mine["edge"][d].min())
    out = {"meta_margin": np.float64(MARGIN), "points": pts, "off": off, "P": Ps, "V2C": Vs, "R0": Rs, "img_wh": IMG_WH,
           "boxes": BOXES, "box_frame": BOX_FRAME, "ref_rect": ref_rect, "ref_fov": ref_fov, "ref_mask": ref_mask,
           "ref_box2d": ref_box, "ref_angle": ref_angle, "ref_skip": ref_skip}
    dst = os.path.join(HERE, "frustum_select.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; selected per box", ref_mask.sum(1).tolist(), "; fov", int(ref_fov.sum()),
          "; placed within %g px of an edge" % NEAR, near_kept, "; skipped", ref_skip.tolist())


if __name__ == "__main__":
    main()
