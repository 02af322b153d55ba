"""TEST INFRASTRUCTURE ONLY: the fp64 numpy referee of the refinement stage's training link (fcn_refine_match,
fcn_refine_label_count / _fill): kitti/prepare_data_refine.py::extract_frustum_det_data (:406-592) restated -- the centre forms
(:25-53, :483-491), the match (:493-499) with the Sutherland-Hodgman IoU of oracle/box_ref.py in fp64, the chained jitter of
random_shift_rotate_box3d (:203-236, :513-519), and the closed-box tests of tests/cascade_ref.py for the enlarged and the label
box.  tests/golden/refine_label.npz pins it to the reference's own functions (tests/golden/make_golden_refine_label.py,
tests/test_refine_label_referee.py).  Never imported by the product."""
import numpy as np

import cascade_ref
from oracle import box_ref


def centre_form(row):
    """A label-format row [tx, ty, tz, l, w, h, ry, ...] (t the bottom centre) -> (cx, cy, cz, l, w, h, ry) fp64 (:483-488)."""
    r = np.asarray(row, dtype=np.float64)
    return np.array([r[0], r[1] - r[5] / 2.0, r[2], r[3], r[4], r[5], r[6]])


def iou3d(a7, b7):
    """3-D IoU of two centre-form boxes, fp64."""
    c = box_ref.boxes3d2corners(np.stack([np.asarray(a7, dtype=np.float64), np.asarray(b7, dtype=np.float64)]))
    return float(box_ref.iou_pair(c[0:1], c[1:2])[0, 1])


def match(dets, cand_row, cand_frame, gt, gt_off, thresh):
    """-> gt_idx (D) (the first maximum of the frame's label boxes, -1: none or below thresh), best (D), and per candidate the
    fp64 IoU against every label box of its frame."""
    D = len(cand_row)
    gt_idx, best, every = np.full(D, -1, dtype=np.int64), np.zeros(D), []
    for d in range(D):
        f = int(cand_frame[d])
        g0, g1 = int(gt_off[f]), int(gt_off[f + 1])
        ious = np.array([iou3d(centre_form(dets[cand_row[d]]), centre_form(gt[j])) for j in range(g0, g1)])
        every.append(ious)
        if len(ious):
            best[d] = ious.max()
            if not (best[d] < thresh):
                gt_idx[d] = g0 + int(ious.argmax())
    return gt_idx, best, every


def jitter_step(box7, q, r=0.05):
    """random_shift_rotate_box3d (:203-236) with its seven draws q in the order l, h, w, cx, cy, cz, angle; Python floats, so
    every product is grouped and rounded as the reference's."""
    cx, cy, cz, l, w, h, angle = (float(x) for x in box7)
    q = [float(x) for x in q]
    angle = angle + np.pi
    l1 = l + l * r * (q[0] * 2 - 1)
    h1 = h + h * r * (q[1] * 2 - 1)
    w1 = w + w * r * (q[2] * 2 - 1)
    cx1 = cx + l * r * (q[3] * 2 - 1)
    cy1 = cy + h * r * (q[4] * 2 - 1)
    cz1 = cz + w * r * (q[5] * 2 - 1)
    angle1 = angle + r * (q[6] * 2 - 1) * np.pi
    angle1 = angle1 % (2 * np.pi)
    return np.array([cx1, cy1, cz1, l1, w1, h1, angle1 - np.pi])


def enlarged_chain(det_row, draws=None, ratio=1.2, r=0.05):
    """The enlarged box of every copy (A,7) in centre form: draws (A,7) -> copy a perturbs copy a - 1 (:513-519); None -> the one
    un-jittered box."""
    box = centre_form(det_row)
    box[3:6] = box[3:6] * ratio
    if draws is None:
        return box[None]
    out = []
    for q in draws:
        box = jitter_step(box, q, r)
        out.append(box)
    return np.stack(out)


def corners(box7):
    return cascade_ref.box_corners(np.asarray(box7[:3], dtype=np.float64), np.asarray(box7[3:6], dtype=np.float64), float(box7[6]))


def inside(xyz, box7):
    return cascade_ref.inside(xyz, np.asarray(box7[:3]), np.asarray(box7[3:6]), float(box7[6]))


def face_distance(xyz, box7):
    return cascade_ref.face_distance(xyz, np.asarray(box7[:3]), np.asarray(box7[3:6]), float(box7[6]))


def select_labeled(frame_pts, frame_off, dets, cand_row, cand_frame, cand_gt, gt, jitter=None, ratio=1.2, r=0.05):
    """What fcn_refine_label_count / _fill produce, per unit u = d * A + a: box (U,7) the jittered enlarged box in centre form,
    pred_box3d (U,8,3), pred_angle, pred_size, box3d (U,8,3), heading, size of the label box, index (ascending, frame-relative
    rows inside the enlarged box), positive (bool per selected row), counts, pos.  An unmatched candidate's units (cand_gt < 0)
    are empty: zeros, no rows."""
    D = len(cand_row)
    A = 1 if jitter is None else int(np.asarray(jitter).shape[1])
    U = D * A
    out = {"box": np.zeros((U, 7)), "pred_box3d": np.zeros((U, 8, 3)), "pred_angle": np.zeros(U), "pred_size": np.zeros((U, 3)),
           "box3d": np.zeros((U, 8, 3)), "heading": np.zeros(U), "size": np.zeros((U, 3)), "counts": np.zeros(U, dtype=np.int64),
           "pos": np.zeros(U, dtype=np.int64), "index": [np.zeros(0, dtype=np.int64)] * U, "positive": [np.zeros(0, dtype=bool)] * U}
    for d in range(D):
        if cand_gt[d] < 0:
            continue
        f = int(cand_frame[d])
        pts = frame_pts[int(frame_off[f]):int(frame_off[f + 1]), :3]
        chain = enlarged_chain(dets[cand_row[d]], None if jitter is None else np.asarray(jitter)[d], ratio, r)
        label = centre_form(gt[cand_gt[d]])
        for a in range(A):
            u = d * A + a
            idx = np.nonzero(inside(pts, chain[a]))[0]
            positive = inside(pts[idx], label)
            out["box"][u] = chain[a]
            out["pred_box3d"][u], out["pred_angle"][u], out["pred_size"][u] = corners(chain[a]), chain[a][6], chain[a][3:6]
            out["box3d"][u], out["heading"][u], out["size"][u] = corners(label), label[6], label[3:6]
            out["index"][u], out["positive"][u] = idx, positive
            out["counts"][u], out["pos"][u] = len(idx), int(positive.sum())
    return out
