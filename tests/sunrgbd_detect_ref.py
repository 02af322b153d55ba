"""TEST INFRASTRUCTURE ONLY: fp64 numpy restatement of the SUN-RGBD inference tail of the reference --
  decode            the per-frustum loop of train/test_net_det_sunrgbd.py:208-252 on head logits: foreground p_fg > 0.5 (else the
                    arg-max of p_fg; 'top': the arg-max only), arg-max heading bin / size cluster decode
                    (models/box_transform.py:5-12,28-41), from_prediction_to_label_format of
                    datasets/provider_sample_sunrgbd.py:374-385 (the box CENTRE, no h/2 shift), the h/w/l >= 0.01 filter and
                    score = rgb_prob + max softmax(size scores)
  corners           datasets/data_utils.py:44-70 compute_box_3d
  iou3d             what eval_det.py:84-86 get_iou_cc asks of rbbox_iou_3d_pair (oracle/box_ref.iou_pair)
  match, curves     train/sunrgbd_eval/eval_det.py:89-169 eval_det_cls + voc_ap (:41-72, use_07_metric=False), in the CSR form of
                    fcn_det_match / fcn_det_ap: groups = (image, class); equal scores walk the lower input index first
tests/golden/sunrgbd_detect.npz (make_golden_sunrgbd_detect.py, the reference's own python) pins it:
tests/test_sunrgbd_detect_referee.py."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import box_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sunrgbd_detect.npz")


def softmax(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def decode(logits, ref2, mean_size, rot, ref_center=None, rgb_prob=None, nb=12, ns=10, method="nms"):
    """logits (B*L2, >= 2 + 3 + 2 nb + 4 ns) head rows, ref2 (B,3,L2), rot (B) -> dets (B*L2,8) fp64 [tx,ty,tz,l,w,h,ry,score],
    sel (B*L2) bool (the selected positions), valid (B*L2) bool (selected and no size below 0.01), p_fg (B*L2)."""
    ref2 = np.asarray(ref2, dtype=np.float64)
    B, _, L2 = ref2.shape
    lg = np.asarray(logits, dtype=np.float64).reshape(B, L2, -1)
    ms = np.asarray(mean_size, dtype=np.float64).reshape(ns, 3)
    rot = np.asarray(rot, dtype=np.float64).reshape(B)
    rc = np.zeros((B, 3)) if ref_center is None else np.asarray(ref_center, dtype=np.float64).reshape(B, 3)
    rgb = np.ones(B) if rgb_prob is None else np.asarray(rgb_prob, dtype=np.float64).reshape(B)
    dets, sel = np.zeros((B, L2, 8)), np.zeros((B, L2), dtype=bool)
    pfg = softmax(lg[:, :, :2])[:, :, 1]
    per = 2 * np.pi / nb
    for b in range(B):
        o = lg[b, :, 2:]
        fg = np.nonzero(pfg[b] > 0.5)[0]
        if method != "nms" or fg.size == 0:
            fg = np.array([np.argmax(pfg[b])])
        sel[b, fg] = True
        ah = np.argmax(o[:, 3:3 + nb], 1)
        a_s = np.argmax(o[:, 3 + 2 * nb:3 + 2 * nb + ns], 1)
        ang = ah * per + o[np.arange(L2), 3 + nb + ah] * (per / 2)
        ang = np.where(ang > np.pi, ang - 2 * np.pi, ang)
        res = np.stack([o[np.arange(L2), 3 + 2 * nb + ns + 3 * a_s + j] for j in range(3)], 1)
        size = res * ms[a_s] + ms[a_s]
        ctr = o[:, :3] + ref2[b].T
        c, s = np.cos(-rot[b]), np.sin(-rot[b])
        dets[b, :, 0] = c * ctr[:, 0] - s * ctr[:, 2] + rc[b, 0]
        dets[b, :, 1] = ctr[:, 1] + rc[b, 1]
        dets[b, :, 2] = s * ctr[:, 0] + c * ctr[:, 2] + rc[b, 2]
        dets[b, :, 3:6] = size
        dets[b, :, 6] = ang + rot[b]
        dets[b, :, 7] = rgb[b] + softmax(o[:, 3 + 2 * nb:3 + 2 * nb + ns]).max(1)
    valid = sel & ~(dets[:, :, 3:6] < 0.01).any(2)
    return dets.reshape(B * L2, 8), sel.reshape(-1), valid.reshape(-1), pfg.reshape(-1)


def corners(rows):
    """(n, >= 7) [cx,cy,cz,l,w,h,ry,...] -> (n,8,3): compute_box_3d per row."""
    r = np.asarray(rows, dtype=np.float64).reshape(-1, np.shape(rows)[-1])
    l, w, h, t = r[:, 3], r[:, 4], r[:, 5], r[:, 6]
    xs = np.stack([l, l, -l, -l, l, l, -l, -l], 1) / 2
    ys = np.stack([h, h, h, h, -h, -h, -h, -h], 1) / 2
    zs = np.stack([w, -w, -w, w, w, -w, -w, w], 1) / 2
    c, s = np.cos(t)[:, None], np.sin(t)[:, None]
    return np.stack([c * xs + s * zs + r[:, 0:1], ys + r[:, 1:2], -s * xs + c * zs + r[:, 2:3]], 2)


def iou3d(det_c, gt_c):
    """(8,3) against (m,8,3) -> (m,) 3-D IoU.  Pairs whose axis-aligned footprints or y extents are apart are 0 without a clip (the
    clip of disjoint polygons is empty)."""
    g = np.asarray(gt_c, dtype=np.float64).reshape(-1, 8, 3)
    d = np.asarray(det_c, dtype=np.float64)
    out = np.zeros(len(g))
    lo, hi = d.min(0), d.max(0)
    near = np.nonzero(((g.min(1) < hi) & (g.max(1) > lo)).all(1))[0]
    if len(near):
        out[near] = box_ref.iou_pair(np.repeat(d[None], len(near), 0), g[near])[:, 1]
    return out


def match(det_corners, scores, det_off, gt_corners, gt_off, thresh=0.25):
    """-> tp (nd) int32, ovmax (nd) fp64 (-inf without a label box), jmax (nd) int32 (index inside the group, -1 without one):
    the walk of eval_det.py:134-159 per group, descending score, equal scores by the lower input index."""
    scores = np.asarray(scores, dtype=np.float64)
    nd = len(scores)
    tp, ovmax, jmax = np.zeros(nd, dtype=np.int32), np.full(nd, -np.inf), np.full(nd, -1, dtype=np.int32)
    for g in range(len(det_off) - 1):
        d0, d1, g0, g1 = int(det_off[g]), int(det_off[g + 1]), int(gt_off[g]), int(gt_off[g + 1])
        taken = [False] * (g1 - g0)
        for d in d0 + np.argsort(-scores[d0:d1], kind="stable"):
            if g1 > g0:
                for j, iou in enumerate(iou3d(det_corners[d], gt_corners[g0:g1])):
                    if iou > ovmax[d]:
                        ovmax[d], jmax[d] = iou, j
            if ovmax[d] > thresh and not taken[jmax[d]]:
                tp[d] = 1
                taken[jmax[d]] = True
    return tp, ovmax, jmax


def curves(tp, scores, det_class, npos):
    """-> rank (nd) int32, rec (nd), prec (nd) (class c's curve in rank order behind the curves of the classes below it), ap (C)."""
    tp, scores, det_class = np.asarray(tp), np.asarray(scores, dtype=np.float64), np.asarray(det_class)
    nd, C = len(tp), len(npos)
    rank, rec, prec, ap = np.zeros(nd, dtype=np.int32), np.zeros(nd), np.zeros(nd), np.zeros(C)
    base = 0
    for c in range(C):
        idx = np.nonzero(det_class == c)[0]
        order = idx[np.argsort(-scores[idx], kind="stable")]
        rank[order] = np.arange(len(order))
        t = np.cumsum(tp[order].astype(np.float64))
        f = np.cumsum(1.0 - tp[order].astype(np.float64))
        r = t / float(npos[c])
        p = t / np.maximum(t + f, np.finfo(np.float64).eps)
        rec[base:base + len(idx)], prec[base:base + len(idx)] = r, p
        # recall 0 in front and 1 behind, precision 0 on both sides; envelope = running maximum from the right; area = sum of
        # (step of recall) x (envelope at the step's right end)
        rr, env = np.concatenate(([0.0], r, [1.0])), np.maximum.accumulate(np.concatenate(([0.0], p, [0.0]))[::-1])[::-1]
        step = np.nonzero(np.diff(rr) != 0)[0]
        ap[c] = np.sum(np.diff(rr)[step] * env[step + 1])
        base += len(idx)
    return rank, rec, prec, ap


def evaluate(det_corners, scores, det_off, gt_corners, gt_off, group_class, num_classes, thresh=0.25):
    det_off, gt_off, group_class = (np.asarray(x, dtype=np.int64) for x in (det_off, gt_off, group_class))
    tp, ovmax, jmax = match(det_corners, scores, det_off, gt_corners, gt_off, thresh)
    det_class = np.repeat(group_class, np.diff(det_off))
    npos = np.bincount(group_class, weights=np.diff(gt_off), minlength=num_classes).astype(np.int64)
    rank, rec, prec, ap = curves(tp, scores, det_class, npos)
    return {"tp": tp, "ovmax": ovmax, "jmax": jmax, "rank": rank, "rec": rec, "prec": prec, "ap": ap, "npos": npos}
