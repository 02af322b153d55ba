#!/usr/bin/env python
"""Golden fixture that pins the referee of the refinement stage's training link (tests/refine_label_ref.py) and
cascade.draw_box3d_jitter to the reference: runs the reference's OWN kitti/prepare_data_refine.py functions --
random_shift_rotate_box3d (seeded), compute_box_3d_obj_array, extract_pc_in_box3d (a scipy Delaunay hull of the corners) -- chained
as extract_frustum_det_data chains them (:483-548): centre form, enlarge by 1.2, per copy jitter the RESULT of the copy before,
select the frame's rows inside the enlarged box, count those inside the label box, reject a copy without one.  The match (:493-499)
needs rbbox_iou_3d, which is boost-built and not installed; its IoU comes from the reference's pure-python utils/box_util.box3d_iou
on the corners of both centre forms, as make_golden_iou.py uses it.  The reference is imported read-only as make_golden_cascade.py
does; only inputs and results are stored.

The scene: three image-FOV frames in rect camera coordinates (float32, stride 4) of about 700, 0 and 8 500 rows -- the last crosses
two segment boundaries of 4 096 rows -- seven label boxes and eight first-stage detections (float32 rows, handed to the reference
as their float64 casts) with augmentX = 3:
  0  frame 0, matched                         4  frame 2, matched, ry = 3.1: the jittered angle wraps past +pi
  1  frame 0, IoU below the threshold         5  frame 2, matched, points in the enlarged box but none in the label box
  2  frame 0, two IDENTICAL label boxes       6  frame 2, matched, no point at all
  3  frame 1, which has no label box          7  frame 2, matched to candidate 4's label, ry = -3.1: wraps past -pi
Points are PLACED next to the faces of every label box and of every jittered enlarged box, 1e-5 ... 1e-2 m to either side; rows
with NaN / inf coordinates sit in the middle of boxes (the reference is handed the finite rows; a non-finite row is never inside).

Conditions (asserted): a row closer than MARGIN_PRED to a face plane of an enlarged box of its frame, or than MARGIN_LABEL to one
of a matched label box, by the fp64 referee, is not admitted; beyond those margins the hull tests and the referee's closed boxes
agree on EVERY row.  Every candidate's best fp64 IoU keeps IOU_MARGIN = 1e-3 from the threshold and from its runner-up (the exact
tie excepted): twenty times the 5e-5 bar of the float32 IoU core, so no decision can depend on float32 rounding.  The referee's
jittered boxes equal the reference's bit for bit, its corners at 1e-12 (np.dot's fused product).

Usage:  python tests/golden/make_golden_refine_label.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)

import cascade_ref  # noqa: E402
import make_golden_cascade as base  # noqa: E402
import refine_label_ref as rr  # noqa: E402

MARGIN_PRED = 1e-6     # metres, to a face plane of an enlarged box: the hull test agrees down to here on this scene (tried 1e-3,
                       # the margin make_golden_cascade.py keeps, 1e-4, 1e-5 and 1e-6; the placed rows start at 1e-5)
MARGIN_LABEL = 1e-6    # metres, to a face plane of a label box (the margin make_golden_frustum_label.py needs)
IOU_MARGIN = 1e-3
SEED = 20261019
THRESH, RATIO, SHIFT, AUG = 0.5, 1.2, 0.05, 3
BACKGROUND = (250, 0, 8100)
AROUND, NEAR = 110, 14

# frame, tx, ty, tz, l, w, h, ry: label boxes in label format (t the bottom centre), frame after frame
GT = [(0, -4.0, 1.7, 10.0, 3.9, 1.6, 1.5, 0.3),
      (0, 5.0, 1.6, 16.0, 4.1, 1.7, 1.6, -1.2),
      (0, 0.5, 1.65, 24.0, 3.8, 1.6, 1.5, 1.9),
      (0, 0.5, 1.65, 24.0, 3.8, 1.6, 1.5, 1.9),          # 3: identical to 2
      (2, -3.0, 1.7, 12.0, 4.0, 1.65, 1.55, 3.12),
      (2, 6.0, 1.8, 22.0, 3.6, 1.5, 1.4, -0.5),
      (2, 30.0, 1.6, 70.0, 3.9, 1.6, 1.5, 0.8)]          # 6: beyond every point
# candidate -> (frame, label it is derived from, offsets dx dy dz, scales l w h, heading offset)
CAND = [(0, 0, (0.15, 0.03, -0.1), (1.04, 0.97, 1.02), 0.05),
        (0, 1, (1.6, 0.1, 0.9), (0.9, 1.1, 1.0), 0.5),              # below the threshold
        (0, 2, (-0.1, 0.02, 0.12), (0.98, 1.03, 0.97), -0.04),      # the tie
        (1, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 0.0),              # no label box in its frame
        (2, 4, (0.1, -0.02, 0.15), (1.02, 0.98, 1.03), -0.02),      # ry 3.1
        (2, 5, (0.05, 0.02, -0.08), (1.03, 1.02, 0.98), 0.03),      # no positive
        (2, 6, (0.1, 0.0, 0.1), (1.0, 1.0, 1.0), 0.02),             # no point
        (2, 4, (-0.12, 0.03, -0.1), (0.97, 1.04, 1.0), -6.22)]      # ry -3.1, the same label
CAND_ROW = (7, 2, 9, 0, 4, 5, 1, 3)
NO_POSITIVE, NO_POINT, TIE, BELOW, NO_LABEL = 5, 6, 2, 1, 3


def local_to_rect(loc, box7):
    """(n,3) points in a centre-form box's own axes (x' along l, dy, z' along w) -> rect camera coordinates."""
    c, s = np.cos(box7[6]), np.sin(box7[6])
    return np.stack([c * loc[:, 0] + s * loc[:, 2] + box7[0], loc[:, 1] + box7[1], -s * loc[:, 0] + c * loc[:, 2] + box7[2]], 1)


def around_box(rng, box7, n, scale=0.8):
    l, w, h = box7[3:6]
    return local_to_rect(rng.uniform(-scale, scale, (n, 3)) * np.array([l, h, w]), box7)


def near_faces(rng, box7, n):
    """On a random face of the box, nudged across it by 1e-5 ... 1e-2 m to either side."""
    l, w, h = box7[3:6]
    half = np.array([l, h, w]) / 2.0
    loc = rng.uniform(-1.0, 1.0, (n, 3)) * half
    axis, sign = rng.randint(3, size=n), rng.choice([-1.0, 1.0], n)
    nudge = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-5.0, -2.0, n)
    loc[np.arange(n), axis] = sign * half[axis] + nudge
    return local_to_rect(loc, box7)


def main():
    ref = base.import_reference()
    from utils import box_util                                      # (the reference's)
    rng = np.random.RandomState(SEED + 1)
    gt_frame = np.array([g[0] for g in GT], dtype=np.int64)
    gt = np.array([g[1:] for g in GT], dtype=np.float64)
    F, G, D = len(BACKGROUND), len(GT), len(CAND)
    gt_off = np.concatenate([[0], np.cumsum(np.bincount(gt_frame, minlength=F))]).astype(np.int64)
    cand_frame = np.array([c[0] for c in CAND], dtype=np.int32)
    cand_row = np.array(CAND_ROW, dtype=np.int32)
    dets = rng.uniform(-1, 1, (10, 8)).astype(np.float32)           # rows no candidate points at: noise
    for d, (f, j, dt, sc, da) in enumerate(CAND):
        g = gt[j]
        dets[cand_row[d]] = [g[0] + dt[0], g[1] + dt[1], g[2] + dt[2], g[3] * sc[0], g[4] * sc[1], g[5] * sc[2], g[6] + da, rng.rand()]
    assert (np.abs(dets[cand_row, 6]) <= np.pi).all()
    d64 = dets.astype(np.float64)
    # ---- the match: the reference's IoU of the centre forms' corners, candidate against every label box of its frame
    gt_corners = np.stack([ref.compute_box_3d_obj_array(rr.centre_form(g)) for g in gt])
    gmax = int(np.diff(gt_off).max())
    ref_iou = np.full((D, gmax), np.nan)
    ref_gt_idx = np.full(D, -1, dtype=np.int32)
    for d in range(D):
        f = cand_frame[d]
        obj_array = rr.centre_form(d64[cand_row[d]])
        mine = ref.compute_box_3d_obj_array(obj_array)
        n = int(gt_off[f + 1] - gt_off[f])
        if n == 0:
            continue                                                # (:458: a frame without label boxes is skipped)
        overlap = np.array([box_util.box3d_iou(mine, gt_corners[j])[0] for j in range(gt_off[f], gt_off[f + 1])])
        ref_iou[d, :n] = overlap
        if not (overlap.max(0) < THRESH):                           # (:498)
            ref_gt_idx[d] = gt_off[f] + overlap.argmax(0)
    mine_idx, mine_best, mine_every = rr.match(dets, cand_row, cand_frame, gt, gt_off, THRESH)
    assert np.array_equal(mine_idx, ref_gt_idx), (mine_idx, ref_gt_idx)
    for d in range(D):
        n = len(mine_every[d])
        assert np.abs(mine_every[d] - ref_iou[d, :n]).max(initial=0.0) <= 1e-9, d
        if n:
            top = np.sort(ref_iou[d, :n])[::-1]
            assert abs(top[0] - THRESH) >= IOU_MARGIN, (d, top[0])
            if n > 1 and d != TIE:
                assert top[0] - top[1] >= IOU_MARGIN, (d, top)
    assert ref_iou[TIE, 2] == ref_iou[TIE, 3] > THRESH and ref_gt_idx[TIE] == 2
    assert 0.05 < np.nanmax(ref_iou[BELOW]) < THRESH and ref_gt_idx[BELOW] == -1 and ref_gt_idx[NO_LABEL] == -1
    assert (ref_gt_idx[[0, 4, 5, 6, 7]] == [0, 4, 5, 6, 4]).all()
    # ---- the reference's jitter, seeded, matched candidates in order, copies chained (:513-519); its draws are recorded
    plain = np.random.random
    seen = []

    def recorded():
        seen.append(plain())
        return seen[-1]
    np.random.seed(SEED)
    np.random.random = recorded
    ref_box = np.zeros((D, AUG, 7))
    try:
        for d in range(D):
            if ref_gt_idx[d] < 0:
                continue
            obj_array = rr.centre_form(d64[cand_row[d]])
            enlarge_obj_array = obj_array.copy()
            enlarge_obj_array[3:6] = enlarge_obj_array[3:6] * RATIO
            for a in range(AUG):
                enlarge_obj_array = ref.random_shift_rotate_box3d(enlarge_obj_array, SHIFT)
                ref_box[d, a] = enlarge_obj_array
    finally:
        np.random.random = plain
    next_draw = np.random.random()
    matched = np.nonzero(ref_gt_idx >= 0)[0]
    draws = np.asarray(seen).reshape(len(matched), AUG, 7)
    jitter = np.zeros((D, AUG, 7))
    jitter[matched] = draws
    wraps_hi = wraps_lo = 0
    for d in matched:
        chain = rr.enlarged_chain(dets[cand_row[d]], jitter[d], RATIO, SHIFT)
        assert np.array_equal(chain, ref_box[d]), d                 # bit for bit
        prev = np.concatenate([[d64[cand_row[d], 6]], chain[:-1, 6]])
        raw = (prev + np.pi) + SHIFT * (jitter[d, :, 6] * 2 - 1) * np.pi
        wraps_hi += int((raw >= 2 * np.pi).sum())
        wraps_lo += int((raw < 0).sum())
    assert wraps_hi > 0 and wraps_lo > 0, (wraps_hi, wraps_lo)      # both branches of the floored modulo
    # ---- the frames
    frames = []
    for f, nb in enumerate(BACKGROUND):
        xyz = np.stack([rng.uniform(-12.0, 12.0, nb), rng.uniform(-1.0, 2.5, nb), rng.uniform(4.0, 40.0, nb)], 1)
        mine = [d for d in matched if cand_frame[d] == f and d != NO_POINT]
        for d in mine:
            label = rr.centre_form(gt[ref_gt_idx[d]])
            add = [around_box(rng, ref_box[d, 0], AROUND)]
            add += [near_faces(rng, ref_box[d, a], NEAR) for a in range(AUG)]
            if d != NO_POSITIVE:
                add += [around_box(rng, label, 40, 0.5), near_faces(rng, label, 2 * NEAR)]
            xyz = np.concatenate([xyz] + add, 0)
        xyz = xyz.astype(np.float32)
        ok = np.ones(len(xyz), dtype=bool)
        for d in [d for d in range(D) if cand_frame[d] == f and ref_gt_idx[d] >= 0]:
            label = rr.centre_form(gt[ref_gt_idx[d]])
            ok &= rr.face_distance(xyz, label) >= MARGIN_LABEL
            for a in range(AUG):
                ok &= rr.face_distance(xyz, ref_box[d, a]) >= MARGIN_PRED
            if d == NO_POSITIVE:                                    # nothing inside its label box (nor within 2 cm of it)
                grown = label.copy()
                grown[3:6] += 0.04
                ok &= ~rr.inside(xyz, grown)
            if d == NO_POINT:
                ok &= ~rr.inside(xyz, np.r_[label[:3], label[3:6] * 3.0, label[6]])
        xyz = xyz[ok]
        xyz = xyz[rng.permutation(len(xyz))]
        frames.append(np.concatenate([xyz, rng.uniform(0, 1, (len(xyz), 1)).astype(np.float32)], 1))
    # rows with a non-finite coordinate in the middle of candidate 0's and candidate 4's label boxes
    for f, j, at in ((0, 0, (5, 6, 7)), (2, 4, (4100, 4101, 8200))):
        c = rr.centre_form(gt[j])[:3].astype(np.float32)
        for k, (i, bad) in enumerate(zip(at, (np.nan, np.inf, -np.inf))):
            frames[f][i, :3] = c
            frames[f][i, k] = bad
    counts = [len(fr) for fr in frames]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    pts = np.concatenate(frames, 0)
    assert counts[1] == 0 and 600 <= counts[0] <= 800 and 2 * 4096 + 100 < counts[2] < 3 * 4096, counts
    # ---- the reference's selection, candidate by candidate and copy by copy (:511-548)
    nmax = max(counts)
    U = D * AUG
    ref_mask, ref_label = np.zeros((U, nmax), dtype=bool), np.zeros((U, nmax), dtype=bool)
    ref_reject = np.ones(U, dtype=bool)
    ref_pred_corners = np.zeros((U, 8, 3))
    for d in matched:
        f = cand_frame[d]
        pc_rect = frames[f]
        finite = np.isfinite(pc_rect[:, :3]).all(1)
        rows = np.nonzero(finite)[0]
        box3d_pts_3d = ref.compute_box_3d_obj_array(rr.centre_form(gt[ref_gt_idx[d]]))
        assert np.array_equal(box3d_pts_3d, gt_corners[ref_gt_idx[d]])
        for a in range(AUG):
            u = d * AUG + a
            box3d_corners_enlarge = ref.compute_box_3d_obj_array(ref_box[d, a])
            ref_pred_corners[u] = box3d_corners_enlarge
            if len(rows) == 0:
                continue
            _, inds = ref.extract_pc_in_box3d(pc_rect[rows], box3d_corners_enlarge)
            pc_in_cuboid = pc_rect[rows][inds]
            label = np.zeros((pc_in_cuboid.shape[0]))
            if len(pc_in_cuboid):
                _, inds2 = ref.extract_pc_in_box3d(pc_in_cuboid, box3d_pts_3d)
                label[inds2] = 1
            ref_reject[u] = bool(np.sum(label) == 0)
            ref_mask[u, rows[inds]] = True
            ref_label[u, rows[inds][label > 0]] = True
    # ---- the referee must agree on every row
    cand_gt = ref_gt_idx
    mine = rr.select_labeled(pts, off, dets, cand_row, cand_frame, cand_gt, gt, jitter, RATIO, SHIFT)
    near_p = near_l = 0
    for d in range(D):
        n = counts[cand_frame[d]]
        fr = pts[off[cand_frame[d]]:off[cand_frame[d] + 1], :3]
        for a in range(AUG):
            u = d * AUG + a
            assert np.array_equal(np.nonzero(ref_mask[u, :n])[0], mine["index"][u]), "unit %d: masks differ" % u
            assert np.array_equal(ref_label[u, :n][mine["index"][u]], mine["positive"][u]), "unit %d: labels differ" % u
            if cand_gt[d] < 0:
                assert mine["counts"][u] == 0
                continue
            assert np.array_equal(mine["box"][u], ref_box[d, a])
            ext = ref_box[d, a, 3:6].max()
            assert cascade_ref.within(mine["pred_box3d"][u], ref_pred_corners[u], extent=ext)
            assert cascade_ref.within(mine["box3d"][u], gt_corners[cand_gt[d]], extent=gt[cand_gt[d], 3:6].max())
            fin = np.isfinite(fr).all(1)
            if fin.any():
                dp, dl = rr.face_distance(fr[fin], ref_box[d, a]), rr.face_distance(fr[fin], rr.centre_form(gt[cand_gt[d]]))
                assert dp.min() >= MARGIN_PRED and dl.min() >= MARGIN_LABEL, (u, dp.min(), dl.min())
                near_p += int((dp < 1e-2).sum())
                near_l += int((dl < 1e-4).sum())
    cnt, pos = mine["counts"].reshape(D, AUG), mine["pos"].reshape(D, AUG)
    assert np.array_equal(mine["pos"] == 0, ref_reject)
    assert (cnt[NO_POSITIVE] > 20).all() and (pos[NO_POSITIVE] == 0).all() and (cnt[NO_POINT] == 0).all()
    assert (pos[[0, 2, 4, 7]] > 10).all() and (cnt[[BELOW, NO_LABEL]] == 0).all()
    assert near_p >= 100 and near_l >= 30, (near_p, near_l)
    seg = 4096
    assert all(len(set((mine["index"][4 * AUG + a] // seg).tolist())) == 3 for a in range(AUG))      # every segment of frame 2
    assert any(not np.array_equal(mine["index"][4 * AUG], mine["index"][4 * AUG + a]) for a in (1, 2))   # the copies differ
    out = {"meta_margin_pred": np.float64(MARGIN_PRED), "meta_margin_label": np.float64(MARGIN_LABEL),
           "meta_iou_margin": np.float64(IOU_MARGIN), "meta_seed": np.int64(SEED), "meta_thresh": np.float64(THRESH),
           "meta_ratio": np.float64(RATIO), "meta_shift": np.float64(SHIFT), "points": pts, "off": off, "dets": dets,
           "cand_row": cand_row, "cand_frame": cand_frame, "gt_box3d": gt, "gt_off": gt_off,
           "types": np.array(["Car", "Car", "Pedestrian", "Car", "Car", "Cyclist", "Car", "Car"]),
           "ref_iou": ref_iou, "ref_gt_idx": ref_gt_idx, "ref_draws": draws, "jitter": jitter,
           "ref_next_draw": np.float64(next_draw), "ref_box": ref_box, "ref_pred_corners": ref_pred_corners,
           "ref_gt_corners": gt_corners, "ref_mask": np.packbits(ref_mask, axis=1), "ref_label": np.packbits(ref_label, axis=1),
           "ref_reject": ref_reject}
    dst = os.path.join(HERE, "refine_label.npz")
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes; rows", counts, "; selected", cnt.tolist(), "; positive", pos.tolist(),
          "; best IoU", np.round(np.nanmax(np.nan_to_num(ref_iou, nan=-1.0), 1), 4).tolist(), "; gt_idx", ref_gt_idx.tolist(),
          "; within 1 cm of an enlarged face", near_p, ", within 0.1 mm of a label face", near_l, "; wraps", wraps_hi, wraps_lo)


if __name__ == "__main__":
    main()
