#!/usr/bin/env python
"""Golden fixture that pins the labelled frustum extraction's referee (tests/frustum_label_ref.py) and
frustum.perturb_boxes2d to the reference: runs the reference's OWN kitti_util.compute_box_3d, kitti/prepare_data.py's
extract_pc_in_box3d (a scipy Delaunay hull of the corners), random_shift_box2d (seeded) and, around them, the lines of
extract_frustum_data (:299-356, the reject rule of :354 included) on two synthetic frames of float32 velodyne points with
KITTI-like calibrations and ten ground-truth boxes.  The reference is imported read-only as make_golden_frustum.py does;
kitti.prepare_data also wants ops.pybind11.rbbox_iou, which is stood in by an empty module like every module that is missing.

The boxes: several headings (ry < 0 and |ry| > pi/2 among them), one under 25 px high, one whose frustum holds background only
(its 3-D box hangs in the air), one 2-D box in the sky (no point at all), and one 0.12 px wide 2-D box straddling x = W - 1, for
which random_shift_box2d's loop retries under SEED (asserted below).  The 2-D boxes that select are the PERTURBED ones; the reject
rule looks at the plain ones.

Condition on the inputs: the reference labels through a Delaunay hull, the referee through the analytic test in the box's own
axes; a point whose distance to a face plane of a box of its frame, by the fp64 referee on the float32 rect row, is below MARGIN
= 1e-6 m is not admitted, nor one within MARGIN_PX = 1e-6 px of an edge of the image or of a perturbed box of its frame (the
reference's np.dot order against the referee's left-to-right sums, as in make_golden_frustum.py).  Points are PLACED next to the
faces on purpose, 1e-5 ... 1e-2 m to either side, before that filter.  On every admitted point the reference's labels and masks
must equal the referee's (asserted here).

Usage:  python tests/golden/make_golden_frustum_label.py
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import frustum_label_ref  # noqa: E402
import frustum_ref  # noqa: E402
import make_golden_frustum as base  # noqa: E402

MARGIN = 1e-6          # metres, to a face plane
MARGIN_PX = 1e-6       # pixels, to a 2-D edge
SEED = 20261022
BACKGROUND = (1300, 1100)
AROUND, NEAR = 150, 48     # per furnished box: points in 1.6 x its extent, and points placed next to its faces
IMG_WH = base.IMG_WH

# frame, tx, ty, tz, l, w, h, ry (rect camera coordinates, t the bottom centre), type, furnished with points
GT = [(0, -3.0, 1.65, 12.0, 3.9, 1.6, 1.5, 0.3, "Car", True),
      (0, 4.0, 1.7, 20.0, 4.2, 1.7, 1.6, -1.2, "Car", True),
      (0, 1.0, 1.6, 32.0, 0.8, 0.6, 1.8, 2.5, "Pedestrian", True),
      (0, -6.0, 1.8, 62.0, 3.9, 1.6, 1.5, -2.8, "Car", True),            # 3: under 25 px high
      (0, 0.0, -4.0, 15.0, 3.9, 1.6, 1.5, 0.0, "Car", False),            # 4: in the air: its frustum holds background only
      (1, -5.0, 1.7, 9.0, 3.9, 1.6, 1.5, 1.6, "Car", True),
      (1, 6.0, 1.6, 25.0, 1.8, 0.6, 1.7, -0.4, "Cyclist", True),
      (1, 2.0, 1.6, 18.0, 3.9, 1.6, 1.5, 3.0, "Car", False),             # 7: its 2-D box is in the sky: no point at all
      (1, 12.0, 1.6, 14.0, 3.9, 1.6, 1.5, 0.7, "Car", False),            # 8: the 2-D box random_shift_box2d retries on
      (1, 0.5, 1.65, 16.0, 4.0, 1.6, 1.5, -3.0, "Car", True)]
# 2-D boxes that are not the projection of the 3-D box
BOX2D = {4: [500.0, 150.0, 700.0, 300.0], 7: [640.0, 2.0, 700.0, 40.0], 8: [1222.995, 150.0, 1223.115, 200.0]}
SMALL, AIR, SKY, RETRY = 3, 4, 7, 8


def import_reference():
    base.import_reference()
    for _ in range(16):
        try:
            return importlib.import_module("kitti.kitti_util"), importlib.import_module("kitti.prepare_data")
        except ImportError as e:
            name = getattr(e, "name", None)
            if not name:
                raise
            mod = types.ModuleType(name)
            mod.__path__ = []
            mod.__getattr__ = lambda attr: None
            sys.modules[name] = mod
    raise RuntimeError("could not import the reference modules")


def local_to_rect(loc, gt):
    """(n,3) points in a box's own axes (ax, dy, az from the bottom centre) -> rect camera coordinates."""
    c, s = np.cos(gt[6]), np.sin(gt[6])
    return np.stack([c * loc[:, 0] + s * loc[:, 2] + gt[0], loc[:, 1] + gt[1], -s * loc[:, 0] + c * loc[:, 2] + gt[2]], 1)


def around_box(rng, gt, n):
    l, w, h = gt[3:6]
    loc = np.stack([rng.uniform(-0.8 * l, 0.8 * l, n), rng.uniform(-1.3 * h, 0.3 * h, n), rng.uniform(-0.8 * w, 0.8 * w, n)], 1)
    return local_to_rect(loc, gt)


def near_faces(rng, gt, n):
    """On a random face of the box, nudged across it by 1e-5 ... 1e-2 m to either side."""
    l, w, h = gt[3:6]
    loc = np.stack([rng.uniform(-l / 2, l / 2, n), rng.uniform(-h, 0.0, n), rng.uniform(-w / 2, w / 2, n)], 1)
    face = rng.randint(6, size=n)
    nudge = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.0, -2.0, n)
    at = np.array([l / 2, -l / 2, 0.0, -h, w / 2, -w / 2])[face] + nudge
    loc[np.arange(n), face // 2] = at
    return local_to_rect(loc, gt)


def main():
    ku, pd = import_reference()
    cals = base.calibs()
    gt_frame = np.array([g[0] for g in GT], dtype=np.int32)
    gt3d = np.array([g[1:8] for g in GT], dtype=np.float64)
    names = np.array([g[8] for g in GT])
    D = len(GT)
    objs = [types.SimpleNamespace(t=(g[0], g[1], g[2]), l=g[3], w=g[4], h=g[5], ry=g[6]) for g in gt3d]
    # ---- the label's 2-D boxes: the bounding rectangle of the projected corners, as a KITTI label has it
    gt2d = np.zeros((D, 4))
    ref_corners = np.zeros((D, 8, 3))
    for d in range(D):
        P_ = cals[gt_frame[d]][0]
        c2d, c3d = ku.compute_box_3d(objs[d], P_)
        ref_corners[d] = c3d
        gt2d[d] = BOX2D[d] if d in BOX2D else [c2d[:, 0].min(), c2d[:, 1].min(), c2d[:, 0].max(), c2d[:, 1].max()]
    assert gt2d[SMALL, 3] - gt2d[SMALL, 1] < 25 and (np.delete(gt2d[:, 3] - gt2d[:, 1], SMALL) >= 25).all()
    # ---- the reference's perturbation, seeded, box after box (:318-321); its draws are counted
    calls = [0]
    plain = np.random.random

    def counted():
        calls[0] += 1
        return plain()
    np.random.seed(SEED)
    np.random.random = counted
    try:
        boxes, draws = np.zeros((D, 4)), []
        for d in range(D):
            before = calls[0]
            W, H = IMG_WH[gt_frame[d]]
            boxes[d] = pd.random_shift_box2d(gt2d[d], int(H), int(W), 0.1)
            draws.append(calls[0] - before)
    finally:
        np.random.random = plain
    next_draw = np.random.random()
    assert draws[RETRY] >= 8 and all(n == 4 for d, n in enumerate(draws) if d != RETRY), draws
    # ---- the frames
    rng = np.random.RandomState(SEED + 1)
    frames = []
    for f, nb in enumerate(BACKGROUND):
        P_, V2C_, R0_ = cals[f]
        W, H = IMG_WH[f]
        mine = [d for d in range(D) if gt_frame[d] == f]
        xyz = np.stack([rng.uniform(5.0, 70.0, nb), rng.uniform(-30.0, 30.0, nb), rng.uniform(-2.5, 0.5, nb)], 1)
        for d in mine:
            if GT[d][9]:
                rect = np.concatenate([around_box(rng, gt3d[d], AROUND), near_faces(rng, gt3d[d], NEAR)], 0)
                xyz = np.concatenate([xyz, base.rect_to_velo(rect, V2C_, R0_)], 0)
        xyz = xyz.astype(np.float32)
        rect, u, v = frustum_ref.project(xyz, P_, V2C_, R0_)
        ok = np.ones(len(xyz), dtype=bool)
        for d in mine:
            ok &= frustum_label_ref.face_distance(rect.astype(np.float32), gt3d[d]) >= MARGIN
            ok &= frustum_ref.edge_distance(u, v, boxes[d], W, H) >= MARGIN_PX
        xyz = xyz[ok]
        xyz = xyz[rng.permutation(len(xyz))]
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)).astype(np.float32)], 1))
    counts = [len(fr) for fr in frames]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.concatenate(frames, 0)
    # ---- the reference, frame by frame and box by box (prepare_data.py:299-356)
    nmax = max(counts)
    ref_rect = np.zeros((len(pts), 3), dtype=np.float32)
    ref_mask, ref_label = np.zeros((D, nmax), dtype=bool), np.zeros((D, nmax), dtype=bool)
    ref_angle, ref_reject = np.zeros(D), np.zeros(D, dtype=bool)
    cache = {}
    for d in range(D):
        f = int(gt_frame[d])
        P_, V2C_, R0_ = cals[f]
        img_width, img_height = int(IMG_WH[f][0]), int(IMG_WH[f][1])
        if f not in cache:
            calib = ku.Calibration(None, calib_dict={"P2": P_.reshape(12).copy(), "Tr_velo_to_cam": V2C_.reshape(12).copy(),
                                                     "R0_rect": R0_.reshape(9).copy()})
            pc_velo = frames[f]
            pc_rect = np.zeros_like(pc_velo)
            pc_rect[:, 0:3] = calib.project_velo_to_rect(pc_velo[:, 0:3])
            pc_rect[:, 3] = pc_velo[:, 3]
            _, pc_image_coord, img_fov_inds = pd.get_lidar_in_image_fov(pc_velo[:, 0:3], calib, 0, 0, img_width, img_height, True)
            cache[f] = (calib, pc_rect, pc_image_coord, img_fov_inds)
            ref_rect[off[f]:off[f + 1]] = pc_rect[:, :3]
        calib, pc_rect, pc_image_coord, img_fov_inds = cache[f]
        box2d = gt2d[d]
        xmin, ymin, xmax, ymax = boxes[d]
        box_fov_inds = (pc_image_coord[:, 0] < xmax) & (pc_image_coord[:, 0] >= xmin) & \
                       (pc_image_coord[:, 1] < ymax) & (pc_image_coord[:, 1] >= ymin)
        box_fov_inds = box_fov_inds & img_fov_inds
        pc_in_box_fov = pc_rect[box_fov_inds, :]
        uvdepth = np.zeros((1, 3))
        uvdepth[0, 0:2] = np.array([(xmin + xmax) / 2.0, (ymin + ymax) / 2.0])
        uvdepth[0, 2] = 20
        box2d_center_rect = calib.project_image_to_rect(uvdepth)
        ref_angle[d] = -1 * np.arctan2(box2d_center_rect[0, 2], box2d_center_rect[0, 0])
        box3d_pts_2d, box3d_pts_3d = ku.compute_box_3d(objs[d], calib.P)
        assert np.array_equal(box3d_pts_3d, ref_corners[d])
        label = np.zeros((pc_in_box_fov.shape[0]))
        _, inds = pd.extract_pc_in_box3d(pc_in_box_fov, box3d_pts_3d)
        label[inds] = 1
        ref_reject[d] = bool((box2d[3] - box2d[1]) < 25 or np.sum(label) == 0)
        ref_mask[d, :len(box_fov_inds)] = box_fov_inds
        ref_label[d, np.nonzero(box_fov_inds)[0]] = label > 0
    # ---- the referee must agree on every admitted point
    Ps, Vs, Rs = (np.stack([c[i] for c in cals]) for i in range(3))
    mine = frustum_label_ref.select_labeled(pts, off, Ps, Vs, Rs, IMG_WH, boxes, gt_frame, gt3d, gt2d)
    near = 0
    for d in range(D):
        n = counts[gt_frame[d]]
        assert np.array_equal(np.nonzero(ref_mask[d, :n])[0], mine["index"][d]), "box %d: masks differ" % d
        assert np.array_equal(ref_label[d, :n][mine["index"][d]], mine["seg"][d] > 0), "box %d: labels differ" % d
        if len(mine["face"][d]):
            assert mine["face"][d].min() >= MARGIN, (d, mine["face"][d].min())
            near += int((mine["face"][d] < 1e-4).sum())
    assert np.array_equal(mine["reject"], ref_reject)
    pos, cnt = mine["pos"], mine["counts"]
    assert near >= 30, near
    assert cnt[SKY] == 0 and cnt[AIR] > 50 and pos[AIR] == 0 and pos[SMALL] > 0 and ref_reject[[SMALL, AIR, SKY, RETRY]].all()
    assert (~ref_reject).sum() == D - 4 and (pos[~ref_reject] % 64 != 0).all()
    out = {"meta_margin": np.float64(MARGIN), "meta_margin_px": np.float64(MARGIN_PX), "meta_seed": np.int64(SEED),
           "points": pts, "off": off, "P": Ps, "V2C": Vs, "R0": Rs, "img_wh": IMG_WH, "box_frame": gt_frame, "gt_box3d": gt3d,
           "gt_box2d": gt2d, "types": names, "ref_boxes": boxes, "ref_draws": np.asarray(draws, dtype=np.int64),
           "ref_next_draw": np.float64(next_draw), "ref_rect": ref_rect, "ref_mask": ref_mask, "ref_label": ref_label,
           "ref_corners": ref_corners, "ref_angle": ref_angle, "ref_reject": ref_reject}
    dst = os.path.join(HERE, "frustum_label.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; points", counts, "; selected", cnt.tolist(), "; positive", pos.tolist(),
          "; within 1e-4 m of a face", near, "; draws per box", draws, "; rejected", ref_reject.tolist())


if __name__ == "__main__":
    main()
