#!/usr/bin/env python
"""Golden fixture that pins the SUN-RGBD frustum extraction's referee (tests/frustum_sunrgbd_ref.py),
frustum.perturb_boxes2d_sunrgbd and frustum.draw_frustum_subsample to the reference: runs the reference's OWN
sunrgbd/prepare_data.py::extract_frustum_data (perturbed, augmentX = 2) and extract_frustum_data_from_rgb_detection on a synthetic
dataset directory in a temp dir (calib/%06d.txt, pc/%06d.mat, label/%06d.txt, a detections .txt), then
datasets/provider_sample_sunrgbd.py::ProviderDataset on the pickles they write, in training and in from_rgb_detection form, with
default_collate.  The reference is imported read-only as make_golden_frustum_label.py does, modules that are not installed stood
in by empty ones; np.bool (removed from numpy, used at prepare_data.py:233) is given back as bool.  Every np.random.random,
np.random.choice and np.random.randn is recorded.

Two frames of about 6 000 float32 upright-depth rows with rgb quantised to k/255, a real tilt with small off-diagonal terms and a
different K each; rows behind the camera among them.  The label boxes: several headings (|heading| > pi/2 among them), FEW (fewer
than 5 positives in total), and -- the LAST two labels of the last frame, so that every perturbation before them is a pure prefix
of the generator's stream -- BIG (more than 2048 rows: the subsample path) and SUBFEW (more than 2048 rows, 6 positives: whether
its recorded subsamples keep fewer than 5 is asserted and stored).  The detections: one of more than 2048 rows, one of fewer than
5 rows, several in between.

Condition on the inputs: the reference multiplies with np.dot and labels through a Delaunay hull, the referee sums left to right
and labels through the closed analytic test.  Rows are PLACED 1e-5 ... 1e-2 m to either side of box faces and within 1e-3 px of
box edges on purpose; any row closer than MARGIN = 1e-6 m to a face plane of a label box of its frame or MARGIN_PX = 1e-6 px to an
edge of a selecting box of its frame, by the fp64 referee, is drawn AGAIN (not dropped; the perturbations of BIG and SUBFEW depend
on the row counts before them, so this repeats until nothing moves).  On every row of every box the reference's own projection,
mask and hull label must then equal the referee's (asserted here), and the records the reference pickles must be the referee's
rows.

Stored: the frames, calibrations, labels, detections, the recorded draws and perturbed boxes, per record the selected row INDICES
into its frame (in record order, i.e. after the subsample) with packed labels -- the rows are a function of the indices -- and the
loader's batches.

Usage:  python tests/golden/make_golden_frustum_sunrgbd.py
"""
import contextlib
import importlib
import io
import os
import pickle
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import frustum_sunrgbd_ref as ref  # noqa: E402
from make_golden_inputs_sunrgbd import DrawLog  # noqa: E402

MARGIN = 1e-6          # metres, to a face plane
MARGIN_PX = 1e-6       # pixels, to a 2-D edge
NEAR_PX = 1e-3         # pixels: "next to an edge"
SEED = 20261101
NPOINT = 512           # the loader's resample size (cfg.DATA.NUM_SAMPLES is 2048; the batches are stored, so a small one)
CAP = 2048
AUGMENT = 2
BACKGROUND, BEHIND = (4000, 4400), (160, 140)
AROUND, NEAR, EDGE = 140, 48, 12
WHITELIST = ["bed", "table", "sofa", "chair", "toilet", "desk", "dresser", "night_stand", "bookshelf", "bathtub"]
K0 = np.array([[529.5, 0.0, 365.0], [0.0, 529.5, 265.0], [0.0, 0.0, 1.0]])
K1 = np.array([[518.86, 0.0, 284.58], [0.0, 519.47, 208.74], [0.0, 0.0, 1.0]])

# frame, cx, cy, cz, l, w, h (HALF extents), heading wanted, type, furnished with points, 2-D box (None: around the projection)
GT = [(0, -0.9, 2.6, -0.4, 1.0, 0.8, 0.45, 0.3, "bed", True, None),
      (0, 0.9, 3.4, -0.3, 0.3, 0.28, 0.42, -1.2, "chair", True, None),
      (0, 0.1, 4.6, -0.2, 0.7, 0.4, 0.38, 2.5, "table", True, None),
      (0, 1.0, 3.0, 1.45, 0.3, 0.3, 0.12, 0.9, "dresser", False, None),                              # FEW: 3 positives
      (1, -0.6, 2.9, -0.5, 0.35, 0.3, 0.4, -2.8, "toilet", True, None),
      (1, 1.0, 3.8, -0.1, 0.75, 0.35, 0.5, 1.9, "desk", True, None),
      (1, 0.0, 3.2, -0.2, 1.1, 0.5, 0.45, -0.4, "sofa", True, [30.0, 20.0, 560.0, 400.0]),            # BIG: > 2048 rows
      (1, -0.3, 3.5, 1.45, 0.25, 0.25, 0.1, 0.6, "night_stand", False, [20.0, -150.0, 570.0, 410.0])]   # SUBFEW: > 2048 rows, 6 positives
FEW, BIG, SUBFEW = 3, 6, 7
PLANTED = {FEW: 3, SUBFEW: 6}
# frame, type, prob, xmin ymin xmax ymax
DETS = [(0, "bed", 0.93, 100.25, 150.5, 420.75, 380.0),
        (0, "chair", 0.41, 430.0, 180.0, 520.5, 330.25),
        (0, "sofa", 0.77, 10.0, 5.0, 700.0, 520.0),                  # more than 2048 rows
        (0, "lamp", 0.88, 200.0, 200.0, 300.0, 300.0),               # not in the whitelist: skipped before anything is drawn
        (0, "desk", 0.30, 300.0, -420.0, 340.0, -380.0),             # TINY: 3 rows
        (1, "toilet", 0.66, 150.0, 200.0, 290.5, 330.0),
        (1, "table", 0.52, -40.0, 100.0, 250.0, 460.0),
        (1, "bookshelf", 0.12, 25.0, 15.0, 565.0, 405.0)]            # more than 2048 rows
TINY = 3               # (index among the whitelisted detections)


def rot_x(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]], dtype=np.float64)


def rot_z(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], dtype=np.float64)


def rot_y(t):
    c, s = np.cos(t), np.sin(t)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], dtype=np.float64)


def calibs():
    """A real tilt about x with small off-diagonal terms, and a different K per frame."""
    return [(K0, rot_x(0.19) @ rot_z(0.012) @ rot_y(-0.008)), (K1, rot_x(-0.11) @ rot_y(0.015) @ rot_z(-0.02))]


def import_reference():
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "sunrgbd"))
    if not hasattr(np, "bool"):
        np.bool = bool                                     # prepare_data.py:233
    for _ in range(16):
        try:
            return importlib.import_module("sunrgbd_utils"), importlib.import_module("sunrgbd.prepare_data")
        except ImportError as e:
            name = getattr(e, "name", None)
            if not name:
                raise
            mod = types.ModuleType(name)
            mod.__path__ = []
            mod.__getattr__ = lambda attr: None
            sys.modules[name] = mod
    raise RuntimeError("could not import the reference modules")


def back_project(u, v, zc, K, Rt):
    """Pixels at camera depth zc -> upright-depth points (fp64)."""
    c0, c1 = (u - K[0, 2]) * zc / K[0, 0], (v - K[1, 2]) * zc / K[1, 1]
    return (Rt @ np.stack([c0, zc, -c1])).T


def local_to_depth(loc, gt):
    """(n,3) points in a box's own axes -> upright depth: rotz(-heading) . loc + centroid."""
    c, s = np.cos(-gt[6]), np.sin(-gt[6])
    return np.stack([c * loc[:, 0] - s * loc[:, 1] + gt[0], s * loc[:, 0] + c * loc[:, 1] + gt[1], loc[:, 2] + gt[2]], 1)


def around_box(rng, gt, n, scale=1.6):
    l, w, h = gt[3:6]
    return local_to_depth(np.stack([rng.uniform(-scale * l, scale * l, n), rng.uniform(-scale * w, scale * w, n),
                                    rng.uniform(-scale * h, scale * h, n)], 1), gt)


def near_faces(rng, gt, n):
    """On a random face of the box, nudged across it by 1e-5 ... 1e-2 m to either side."""
    ext = np.asarray(gt[3:6])
    loc = rng.uniform(-1, 1, (n, 3)) * ext
    face = rng.randint(6, size=n)
    nudge = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.0, -2.0, n)
    loc[np.arange(n), face // 2] = np.where(face % 2 == 0, 1.0, -1.0) * ext[face // 2] + nudge
    return local_to_depth(loc, gt)


def near_edges(rng, box, n, K, Rt):
    """Pixels on a random edge of the 2-D box, nudged by up to NEAR_PX, at a random depth."""
    u, v = rng.uniform(box[0], box[2], n), rng.uniform(box[1], box[3], n)
    edge = rng.randint(4, size=n)
    nudge = rng.uniform(-NEAR_PX, NEAR_PX, n)
    u = np.where(edge == 0, box[0] + nudge, np.where(edge == 1, box[2] + nudge, u))
    v = np.where(edge == 2, box[1] + nudge, np.where(edge == 3, box[3] + nudge, v))
    return back_project(u, v, rng.uniform(1.5, 5.5, n), K, Rt)


def background(rng, n):
    return np.stack([rng.uniform(-2.2, 2.2, n), rng.uniform(1.5, 6.0, n), rng.uniform(-1.2, 1.2, n)], 1)


def label_objects(cals):
    """The label lines (classname xmin ymin w h cx cy cz w l h basis(4) orientation(2)) and what SUNObject3d makes of them."""
    lines = [[] for _ in cals]
    for g in GT:
        f, cx, cy, cz, l, w, h, heading, name, _, b2 = g
        o0, o1 = np.cos(-heading), np.sin(-heading)        # heading_angle = -arctan2(o1, o0)
        if b2 is None:
            pts = ref.corners([cx, cy, cz, l, w, h, heading])
            depth = np.stack([pts[:, 0], pts[:, 2], -pts[:, 1]], 1).astype(np.float32)      # back to upright depth
            u, v, _ = ref.project(depth, *cals[f])
            b2 = [u.min(), v.min(), u.max(), v.max()]
        vals = [b2[0], b2[1], b2[2] - b2[0], b2[3] - b2[1], cx, cy, cz, w, l, h, 1.0, 0.0, 0.0, 1.0, o0, o1]
        lines[f].append(name + " " + " ".join(repr(float(x)) for x in vals))
    return lines


def predict_boxes(su, objs, obj_frame, frames, cals):
    """The perturbed boxes extract_frustum_data will draw for these frames: four draws per copy, and a subsample draw behind
    every copy that selects more than CAP rows (which moves every later perturbation)."""
    from frustum_convnet_amd import frustum
    np.random.seed(SEED)
    boxes = []
    for o, f in zip(objs, obj_frame):
        u, v, _ = ref.project(frames[f][:, :3], *cals[f])
        for _ in range(AUGMENT):
            b = frustum.perturb_boxes2d_sunrgbd(o.box2d[None])[0]
            n = int(ref.box_mask(frames[f][:, :3], u, v, b).sum())
            if n > CAP:
                np.random.choice(n, CAP, replace=False)
            boxes.append(b)
    return np.asarray(boxes)


def ragged(arrs, dtype):
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
    return (np.concatenate(arrs).astype(dtype) if len(arrs) else np.zeros(0, dtype)), off


def row_lookup(frame):
    keys = {r.tobytes(): i for i, r in enumerate(frame)}
    assert len(keys) == len(frame), "rows of a frame must be distinct"
    return keys


def main():
    su, pd = import_reference()
    cals = calibs()
    F = len(cals)
    with tempfile.TemporaryDirectory() as td:
        split = os.path.join(td, "training")
        for sub in ("calib", "pc", "label"):
            os.makedirs(os.path.join(split, sub))
        ids = [1, 2]
        for f, (K, Rt) in enumerate(cals):
            with open(os.path.join(split, "calib", "%06d.txt" % ids[f]), "w") as fh:        # Rtilt then K, column-major
                fh.write(" ".join(repr(float(x)) for x in Rt.reshape(-1, order="F")) + "\n")
                fh.write(" ".join(repr(float(x)) for x in K.reshape(-1, order="F")) + "\n")
        cals = []
        for f in range(F):                                                                   # (as the reference reads them back)
            c = su.SUNRGBD_Calibration(os.path.join(split, "calib", "%06d.txt" % ids[f]))
            cals.append((c.K.copy(), c.Rtilt.copy()))
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(cals, calibs()))
        for f, lines in enumerate(label_objects(cals)):
            with open(os.path.join(split, "label", "%06d.txt" % ids[f]), "w") as fh:
                fh.write("\n".join(lines) + "\n")
        objs, obj_frame = [], []
        for f in range(F):
            for o in su.read_sunrgbd_label(os.path.join(split, "label", "%06d.txt" % ids[f])):
                objs.append(o)
                obj_frame.append(f)
        G = len(objs)
        assert G == len(GT) and [g[0] for g in GT] == obj_frame
        gt3d = np.array([[o.centroid[0], o.centroid[1], o.centroid[2], o.l, o.w, o.h, o.heading_angle] for o in objs])
        assert np.abs(gt3d[:, 6] - np.array([g[7] for g in GT])).max() < 1e-12 and np.array_equal(gt3d[:, 3:6], np.array([g[4:7] for g in GT]))
        gt2d = np.stack([o.box2d for o in objs])
        names = np.array([o.classname for o in objs])
        dets = [d for d in DETS if d[1] in WHITELIST]
        det_frame = np.array([d[0] for d in dets], dtype=np.int32)
        det_boxes = np.array([d[3:7] for d in dets], dtype=np.float64)
        # ---- the frames
        rng = np.random.RandomState(SEED + 1)
        # the perturbations of every copy before BIG's first subsample are a pure prefix of the stream: rows can be placed
        # next to their edges before the frames exist
        np.random.seed(SEED)
        from frustum_convnet_amd import frustum
        prefix = frustum.perturb_boxes2d_sunrgbd(np.repeat(gt2d[:BIG], AUGMENT, 0))
        frames = []
        for f, (K, Rt) in enumerate(cals):
            xyz = [background(rng, BACKGROUND[f]),
                   np.stack([rng.uniform(-2.0, 2.0, BEHIND[f]), rng.uniform(-3.0, -0.5, BEHIND[f]), rng.uniform(-1.0, 1.0, BEHIND[f])], 1)]
            for d in range(G):
                if obj_frame[d] != f:
                    continue
                if GT[d][9]:
                    xyz += [around_box(rng, gt3d[d], AROUND), near_faces(rng, gt3d[d], NEAR)]
                if d in PLANTED:
                    xyz.append(around_box(rng, gt3d[d], PLANTED[d], scale=0.8))
                if d < BIG:
                    xyz += [near_edges(rng, prefix[AUGMENT * d + a], EDGE, K, Rt) for a in range(AUGMENT)]
            for i, d in enumerate(dets):
                if d[0] == f:
                    if i != TINY:
                        xyz.append(near_edges(rng, det_boxes[i], EDGE, K, Rt))
                    else:
                        b = det_boxes[i]
                        xyz.append(back_project(rng.uniform(b[0] + 5, b[2] - 5, 3), rng.uniform(b[1] + 5, b[3] - 5, 3),
                                                rng.uniform(2.0, 4.0, 3), K, Rt))
            xyz = np.concatenate(xyz, 0).astype(np.float32)
            xyz = xyz[rng.permutation(len(xyz))]
            rgb = (rng.randint(0, 256, (len(xyz), 3)) / 255.0).astype(np.float32)
            frames.append(np.concatenate([xyz, rgb], 1))
        # ---- any row too close to a face or an edge is drawn again, until neither the rows nor the boxes move
        boxes = None
        for _ in range(20):
            new = predict_boxes(su, objs, obj_frame, frames, cals)
            moved = boxes is None or not np.array_equal(new, boxes)
            boxes = new
            for f in range(F):
                u, v, _ = ref.project(frames[f][:, :3], *cals[f])
                close = np.zeros(len(frames[f]), dtype=bool)
                for d in range(G):
                    if obj_frame[d] == f:
                        close |= ref.face_distance(frames[f][:, :3], gt3d[d]) < MARGIN
                        for a in range(AUGMENT):
                            close |= ref.edge_distance(u, v, boxes[AUGMENT * d + a]) < MARGIN_PX
                for i in range(len(dets)):
                    if det_frame[i] == f:
                        close |= ref.edge_distance(u, v, det_boxes[i]) < MARGIN_PX
                if close.any():
                    frames[f][close, :3] = background(rng, int(close.sum())).astype(np.float32)
                    moved = True
            if not moved:
                break
        else:
            raise RuntimeError("re-draw did not terminate")
        assert np.array_equal(boxes[:AUGMENT * BIG], prefix)
        for f in range(F):
            import scipy.io as sio
            sio.savemat(os.path.join(split, "pc", "%06d.mat" % ids[f]), {"x": frames[f]})
            assert np.array_equal(su.load_depth_points(os.path.join(split, "pc", "%06d.mat" % ids[f])), frames[f])
        lookup = [row_lookup(ref.to_upright_camera(fr)) for fr in frames]
        off = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.int64)
        pts = np.concatenate(frames, 0)
        Ks, Rs = np.stack([c[0] for c in cals]), np.stack([c[1] for c in cals])
        idx_file = os.path.join(td, "idx.txt")
        with open(idx_file, "w") as fh:
            fh.write("\n".join(str(i) for i in ids) + "\n")
        det_file = os.path.join(td, "dets.txt")
        with open(det_file, "w") as fh:
            for d in DETS:
                fh.write("%d %s %s %s\n" % (ids[d[0]], d[1], repr(d[2]), " ".join(repr(x) for x in d[3:7])))
        # ---- random_shift_box2d ALONE under the seed: what frustum.perturb_boxes2d_sunrgbd must equal
        np.random.seed(SEED)
        alone = np.stack([su.random_shift_box2d(gt2d[d]) for d in range(G) for _ in range(AUGMENT)])
        alone_next = np.random.random()
        # ---- the reference's training extraction, its perturbed boxes recorded
        shifted = []
        plain_shift = pd.random_shift_box2d

        def recording_shift(box2d, *a):
            out = plain_shift(box2d, *a)
            shifted.append(np.array(out, dtype=np.float64))
            return out
        train_pickle = os.path.join(td, "sunrgbd_train_aug5x.pickle")
        det_pickle = os.path.join(td, "sunrgbd_rgb_det_val.pickle")
        pd.random_shift_box2d = recording_shift
        try:
            np.random.seed(SEED)
            with DrawLog() as tlog, contextlib.redirect_stdout(io.StringIO()):
                pd.extract_frustum_data(td, idx_file, "training", train_pickle, WHITELIST, perturb_box2d=True, augmentX=AUGMENT)
            train_next = np.random.random()
        finally:
            pd.random_shift_box2d = plain_shift
        np.random.seed(SEED)
        with DrawLog() as dlog, contextlib.redirect_stdout(io.StringIO()):
            pd.extract_frustum_data_from_rgb_detection(td, det_file, "training", det_pickle, WHITELIST)
        det_next = np.random.random()
        ref_boxes = np.stack(shifted)
        D = AUGMENT * G
        assert ref_boxes.shape == (D, 4) and np.array_equal(ref_boxes, boxes), "the predicted perturbations are the reference's"
        assert len(tlog.uniform) == 4 * D and not tlog.normal and not dlog.uniform and not dlog.normal
        assert not np.array_equal(ref_boxes, alone) and np.array_equal(ref_boxes[:AUGMENT * BIG + 1], alone[:AUGMENT * BIG + 1])
        with open(train_pickle, "rb") as fh:
            tp = pickle.load(fh)
        with open(det_pickle, "rb") as fh:
            dp = pickle.load(fh)
        # ---- the referee on every box, against the reference's own projection, mask and hull label on EVERY row
        box_frame = np.repeat(np.asarray(obj_frame, dtype=np.int32), AUGMENT)
        gt_rep, names_rep = np.repeat(gt3d, AUGMENT, 0), np.repeat(names, AUGMENT)
        mine = ref.select(pts, off, Ks, Rs, ref_boxes, box_frame, gt_rep)
        mine_det = ref.select(pts, off, Ks, Rs, det_boxes, det_frame)
        near_face = near_edge = 0
        for which, bx, bf, got in (("train", ref_boxes, box_frame, mine), ("det", det_boxes, det_frame, mine_det)):
            for d in range(len(bx)):
                f = int(bf[d])
                calib = su.SUNRGBD_Calibration(Rtilt=Rs[f], K=Ks[f])
                coord, _ = calib.project_upright_depth_to_image(frames[f])
                xmin, ymin, xmax, ymax = bx[d]
                m = (coord[:, 0] < xmax) & (coord[:, 0] >= xmin) & (coord[:, 1] < ymax) & (coord[:, 1] >= ymin)
                assert np.array_equal(np.nonzero(m)[0], got["index"][d]), "%s box %d: masks differ" % (which, d)
                assert len(got["edge"][d]) == 0 or got["edge"][d].min() >= MARGIN_PX
                near_edge += int((got["edge"][d] < 2 * NEAR_PX).sum())
                if which == "train":
                    _, c3d = su.compute_box_3d(objs[d // AUGMENT], calib)
                    c3d = calib.project_upright_depth_to_upright_camera(c3d)
                    cerr = np.abs(c3d - got["corners"][d]).max()
                    assert cerr <= 1e-12, cerr
                    _, inds = su.extract_pc_in_box3d(got["rows"][d], c3d)
                    assert np.array_equal(inds, got["seg"][d] > 0), "box %d: labels differ" % d
                    assert got["face"][d].min() >= MARGIN
                    near_face += int((got["face"][d] < 1e-4).sum())
        assert near_face >= 30 and near_edge >= 30, (near_face, near_edge)
        assert any((dep < 0).any() for dep in mine["depth"] + mine_det["depth"]), "rows behind the camera are selected"

        # ---- the recorded draws against the counts, and the records against the referee's rows
        def records(p, got, log, bx, labelled):
            sub = [None] * len(bx)
            big = [d for d in range(len(bx)) if got["counts"][d] > CAP]
            assert len(log.choice) == len(big) and all(len(c) == CAP for c in log.choice)
            for d, c in zip(big, log.choice):
                sub[d] = np.asarray(c, dtype=np.int32)
            want32 = np.asarray(bx, dtype=np.float32) if labelled else None
            kept, index, labels = [], [], []
            for k in range(len(p["input"])):
                if labelled:
                    d = [i for i in range(len(bx)) if np.array_equal(want32[i], p["box2d"][k])]
                else:
                    d = [i for i in range(len(bx)) if np.array_equal(bx[i], p["box2d"][k])]
                assert len(d) == 1, "a record's box identifies it"
                d = d[0]
                kept.append(d)
                rows = p["input"][k]
                assert rows.dtype == np.float32
                ix = np.asarray([lookup[int(box_frame[d] if labelled else det_frame[d])][r.tobytes()] for r in rows], dtype=np.int64)
                full = got["index"][d]
                assert np.array_equal(ix, full if sub[d] is None else full[sub[d]]), "record %d is not the referee's selection" % k
                index.append(ix)
                if labelled:
                    seg = got["seg"][d] if sub[d] is None else got["seg"][d][sub[d]]
                    assert np.array_equal(np.asarray(p["label"][k]).astype(np.int64), seg)
                    labels.append(seg.astype(bool))
                assert p["frustum_angle"][k] == got["frustum_angle"][d], "frustum angle, exact"
            return sub, np.asarray(kept, dtype=np.int64), index, labels
        tsub, tkept, tindex, tlabel = records(tp, mine, tlog, ref_boxes, True)
        dsub, dkept, dindex, _ = records(dp, mine_det, dlog, det_boxes, False)
        want_kept, pos_after = ref.training_kept(mine["pos"], mine["seg"], tsub)
        assert np.array_equal(tkept, want_kept)
        assert np.array_equal(dkept, np.nonzero(np.minimum(mine_det["counts"], CAP) >= 5)[0])
        assert np.array_equal(np.asarray(tp["box3d_heading"]), gt_rep[tkept, 6]) and np.array_equal(np.stack(tp["box3d_size"]), 2 * gt_rep[tkept, 3:6])
        # ---- the cases the fixture must hold
        few, bigc, subfew = [AUGMENT * FEW + a for a in range(AUGMENT)], [AUGMENT * BIG + a for a in range(AUGMENT)], [AUGMENT * SUBFEW + a for a in range(AUGMENT)]
        assert all(0 < mine["pos"][d] < 5 and mine["counts"][d] >= 5 for d in few) and not set(few) & set(tkept.tolist())
        assert all(mine["counts"][d] > CAP and d in tkept for d in bigc)
        assert all(mine["counts"][d] > CAP and mine["pos"][d] >= 5 for d in subfew)
        subfew_dropped = np.asarray([pos_after[d] < 5 for d in subfew])
        assert subfew_dropped.any(), "no copy of SUBFEW loses its positives under this seed: pick another"
        assert 0 < mine_det["counts"][TINY] < 5 and (mine_det["counts"] > CAP).sum() == 2 and TINY not in dkept
        assert len(set(np.sign(gt3d[:, 6]))) == 2 and (np.abs(gt3d[:, 6]) > np.pi / 2).any()
        # ---- the loader on both pickles
        import yaml
        _orig = yaml.load
        yaml.load = lambda s, Loader=None: _orig(s, Loader=Loader or yaml.FullLoader)
        from configs.config import cfg, merge_cfg_from_file
        merge_cfg_from_file(os.path.join(REF, "cfgs", "det_sample_sunrgbd.yaml"))
        cfg.immutable(False)
        cfg.DATA.DATA_ROOT = td
        from datasets.provider_sample_sunrgbd import ProviderDataset, collate_fn
        ds = ProviderDataset(NPOINT, split="train", random_flip=True, random_shift=True, one_hot=True)
        np.random.seed(SEED + 2)
        with DrawLog() as llog:
            tbatch = collate_fn([ds[i] for i in range(len(ds))])
        B = len(ds)
        assert B == len(tkept) and len(llog.choice) == B and len(llog.uniform) == 2 * B and len(llog.normal) == B
        ds = ProviderDataset(NPOINT, split="val", one_hot=True, from_rgb_detection=True, overwritten_data_path=det_pickle)
        np.random.seed(SEED + 3)
        with DrawLog() as ilog:
            dbatch = collate_fn([ds[i] for i in range(len(ds))])
        assert len(ds) == len(dkept) and len(ilog.choice) == len(dkept) and not ilog.uniform and not ilog.normal
        rows_t = np.asarray([len(ix) for ix in tindex])
        assert (rows_t < NPOINT).any() and (rows_t > NPOINT).any()

        def pack_sub(sub):
            has = [d for d, s in enumerate(sub) if s is not None]
            return np.asarray(has, dtype=np.int64), (np.stack([sub[d] for d in has]).astype(np.int32) if has else np.zeros((0, CAP), np.int32))
        tix, toff = ragged(tindex, np.int32)
        dix, doff = ragged(dindex, np.int32)
        tsb, tsv = pack_sub(tsub)
        dsb, dsv = pack_sub(dsub)
        out = {"meta_margin": np.float64(MARGIN), "meta_margin_px": np.float64(MARGIN_PX), "meta_seed": np.int64(SEED),
               "meta_npoint": np.int64(NPOINT), "meta_cap": np.int64(CAP), "meta_augment": np.int64(AUGMENT),
               "meta_strides": np.asarray(cfg.DATA.STRIDE, dtype=np.float64), "meta_max_depth": np.float64(cfg.DATA.MAX_DEPTH),
               "meta_numpy": np.bytes_(np.__version__.encode()),
               "meta_few": np.asarray(few), "meta_big": np.asarray(bigc), "meta_subfew": np.asarray(subfew),
               "meta_subfew_dropped": subfew_dropped, "meta_det_tiny": np.int64(TINY),
               "points": pts, "off": off, "K": Ks, "Rtilt": Rs,
               "gt_box3d": gt3d, "gt_box2d": gt2d, "gt_frame": np.asarray(obj_frame, dtype=np.int32), "gt_types": names,
               "alone_boxes": alone, "alone_next": np.float64(alone_next),
               "train_boxes": ref_boxes, "train_box_frame": box_frame, "train_types": names_rep, "train_next": np.float64(train_next),
               "train_sub_box": tsb, "train_sub": tsv, "train_kept": tkept, "train_index": tix, "train_index_off": toff,
               "train_label": np.packbits(np.concatenate(tlabel)), "train_box2d": np.stack(tp["box2d"]),
               "train_angle": np.asarray(tp["frustum_angle"]), "train_box3d": np.stack(tp["box3d"]),
               "train_heading": np.asarray(tp["box3d_heading"]), "train_size": np.stack(tp["box3d_size"]),
               "det_boxes": det_boxes, "det_frame": det_frame, "det_types": np.array([d[1] for d in dets]),
               "det_prob": np.array([d[2] for d in dets]), "det_next": np.float64(det_next),
               "det_sub_box": dsb, "det_sub": dsv, "det_kept": dkept, "det_index": dix, "det_index_off": doff,
               "det_box2d": np.stack(dp["box2d"]), "det_angle": np.asarray(dp["frustum_angle"]),
               "train_draw_choice": np.stack(llog.choice).astype(np.int32), "train_draw_coin": np.asarray(llog.uniform[0::2]),
               "train_draw_normal": np.asarray(llog.normal), "train_draw_hshift": np.asarray(llog.uniform[1::2]),
               "det_draw_choice": np.stack(ilog.choice).astype(np.int32)}
        for k, v in tbatch.items():
            out["train_batch_" + k] = v.numpy()
        for k, v in dbatch.items():
            out["det_batch_" + k] = v.numpy()
    dst = os.path.join(HERE, "frustum_sunrgbd.npz")
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    assert size < 500 * 1000, size
    print("wrote", dst, size, "bytes; rows", [len(fr) for fr in frames], "; selected", mine["counts"].tolist(), "; positive",
          mine["pos"].tolist(), "after subsample", pos_after.tolist(), "; kept", tkept.tolist(), "; SUBFEW dropped",
          subfew_dropped.tolist(), "; detections", mine_det["counts"].tolist(), "kept", dkept.tolist(),
          "; within 1e-4 m of a face", near_face, "; within 2e-3 px of an edge", near_edge)


if __name__ == "__main__":
    main()
