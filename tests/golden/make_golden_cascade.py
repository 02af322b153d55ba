#!/usr/bin/env python
"""Golden fixture that pins the cascade link's referee (tests/cascade_ref.py) to the reference: runs the reference's OWN
compute_box_3d_obj_array and extract_pc_in_box3d (kitti/prepare_data_refine.py :56-79, :120-130, scipy.spatial.Delaunay;
imported read-only from /root/reference, CPU) on synthetic first-stage rows and points -- the box as predicted and the box
enlarged by 1.2, as its rgb-detection extraction uses them -- and stores inputs, the reference's corners and its inside masks.

Condition on the inputs: the reference's Delaunay test has a tolerance at the faces, the referee's box is closed and exact, so a
point closer than MARGIN to a face plane of its enlarged box (judged by the fp64 referee) is re-drawn.  A fifth of the points is
drawn within 5 mm of a face on purpose, so that the margin is what separates the two tests, not a lack of close points.  On every
remaining point the reference's mask must equal the referee's (asserted here; no point is dropped from the comparison).

The reference is only imported and called; the arguments of the two calls come from tests/cascade_ref.py.  Usage:  python tests/golden/make_golden_cascade.py
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

import cascade_ref  # noqa: E402

MARGIN = 1e-3          # metres; the issue allows widening to at most 1e-2 when the masks disagree
RATIO = 1.2
NBOX, NPTS = 6, 700


def import_reference():
    """kitti/prepare_data_refine.py imports its whole tool chain at module level (OpenCV, the dataset readers, compiled box
    ops); the two functions used here need numpy and scipy only, so modules that are not installed are stood in by empty ones."""
    import importlib
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "kitti"))
    for _ in range(16):
        try:
            return importlib.import_module("prepare_data_refine")
        except ImportError as e:
            name = getattr(e, "name", None)
            if not name:
                raise
            mod = types.ModuleType(name)
            mod.__path__ = []
            mod.__getattr__ = lambda attr: None
            sys.modules[name] = mod
    raise RuntimeError("could not import the reference module")


def draw_points(rng, n, centre, size, ry):
    """Points around the enlarged box in ITS frame: uniform over 1.5x its extent, a fifth within 5 mm of a random face."""
    l, w, h = size
    half = np.array([l, h, w]) / 2.0
    q = rng.uniform(-1.5, 1.5, (n, 3)) * half
    near = rng.rand(n) < 0.2
    axis = rng.randint(0, 3, n)
    sign = rng.choice([-1.0, 1.0], n)
    q_in = rng.uniform(-1.0, 1.0, (n, 3)) * half
    q_in[np.arange(n), axis] = sign * (half[axis] + rng.uniform(-5e-3, 5e-3, n))
    q[near] = q_in[near]
    c, s = np.cos(ry), np.sin(ry)
    return np.stack([c * q[:, 0] + s * q[:, 2] + centre[0], q[:, 1] + centre[1], -s * q[:, 0] + c * q[:, 2] + centre[2]], 1)


def main():
    ref = import_reference()
    rng = np.random.RandomState(20261017)
    dets = np.zeros((NBOX, 8), dtype=np.float32)
    pts = np.zeros((NBOX, NPTS, 3), dtype=np.float32)
    corners = np.zeros((NBOX, 8, 3))
    corners_l = np.zeros((NBOX, 8, 3))
    mask = np.zeros((NBOX, NPTS), dtype=bool)
    redrawn = 0
    for b in range(NBOX):
        depth, ang = rng.uniform(6.0, 60.0), rng.uniform(-0.6, 0.6)
        lwh = np.array([3.88, 1.63, 1.53]) * rng.uniform(0.7, 1.3, 3)
        ry = [0.0, np.pi / 2, -np.pi / 2, 2.5, -3.1, rng.uniform(-np.pi, np.pi)][b]
        dets[b] = [depth * np.sin(ang), rng.uniform(1.0, 2.0), depth * np.cos(ang), lwh[0], lwh[1], lwh[2], ry, rng.rand()]
        centre, size, ryd = cascade_ref.enlarged_box(dets[b], RATIO)
        p = draw_points(rng, NPTS, centre, size, ryd).astype(np.float32)
        for _ in range(100):
            close = cascade_ref.face_distance(p, centre, size, ryd) < MARGIN
            if not close.any():
                break
            redrawn += int(close.sum())
            p[close] = draw_points(rng, int(close.sum()), centre, size, ryd).astype(np.float32)
        else:
            raise RuntimeError("re-draw did not terminate")
        pts[b] = p
        # ---- the reference's two functions on arguments built here: a 7-vector (centre, l, w, h, ry) of the box as predicted
        # and of the enlarged one, then the frame points against the enlarged corners
        box_plain = np.r_[cascade_ref.enlarged_box(dets[b], 1.0)]
        box_large = np.r_[centre, size, ryd]
        corners[b] = ref.compute_box_3d_obj_array(box_plain)
        corners_l[b] = ref.compute_box_3d_obj_array(box_large)
        mask[b] = ref.extract_pc_in_box3d(p, corners_l[b])[1]
        mine = cascade_ref.inside(p, centre, size, ryd)
        nd = int((mine != mask[b]).sum())
        assert nd == 0, "box %d: the reference's mask and the referee's differ on %d points at margin %g" % (b, nd, MARGIN)
        mine_c = cascade_ref.box_corners(centre, size, ryd)
        assert cascade_ref.within(mine_c, corners_l[b], extent=size.max()), (b, cascade_ref.worst(mine_c, corners_l[b], size.max()))
    out = {"meta_ratio": np.float64(RATIO), "meta_margin": np.float64(MARGIN), "dets": dets, "points": pts,
           "ref_corners": corners, "ref_corners_enlarged": corners_l, "ref_mask": mask}
    dst = os.path.join(HERE, "cascade_select.npz")
    np.savez_compressed(dst, **out)
    near = [int((cascade_ref.face_distance(pts[b], *cascade_ref.enlarged_box(dets[b], RATIO)) < 5e-3).sum()) for b in range(NBOX)]
    print("wrote", dst, os.path.getsize(dst), "bytes; inside per box", mask.sum(1).tolist(), "of", NPTS,
          "; within 5 mm of a face", near, "; re-drawn", redrawn)


if __name__ == "__main__":
    main()
