"""TEST INFRASTRUCTURE ONLY: fp64 numpy restatement of the reference's KITTI evaluation, sequential exactly as the C++ walks --
  label_rows          train/test_net_det.py:88-105,284-293 with compute_alpha of datasets/provider_sample.py:389-394
  image_overlap, ground_overlap, box3d_overlap
                      train/kitti_eval/evaluate_object_3d_offline.cpp:229-263, :296-316, :319-346 ("the evaluator" below), the
                      polygons clipped by oracle/box_ref.py (pinned to the reference's utils/box_util.py) where the evaluator
                      calls boost::geometry
  clean_data          :383-456        compute_statistics  :458-616        get_thresholds  :348-381
  evaluate            eval_class (:622-704) for every metric, class and difficulty + the host-side rules of eval (:158-172,
                      :855-874) + the AP of saveAndPlotPlots (:716-720, summed in fp64)
The evaluator itself needs boost and cannot be built here, so this restatement is the referee of the device code
(tests/test_gpu_kitti_eval.py); tests/test_kitti_eval_referee.py makes it trustworthy on its own with hand-worked scenes.
Frames come in the CSR form of evaluate.kitti_eval: det (nd,13) [alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry, score], det_class (nd)
in {0,1,2} or anything else, gt (ng,14) [truncation, occlusion, alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry], gt_type (ng) over
TYPES (6: any other type)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import box_ref  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kitti_eval.npz")
TYPES = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare")
CAR, PEDESTRIAN, CYCLIST, VAN, PERSON_SITTING, DONTCARE, OTHER = range(7)
MIN_HEIGHT = (40, 25, 25)                   # :43-45
MAX_OCCLUSION = (0, 1, 2)
MAX_TRUNCATION = (0.15, 0.3, 0.5)
MIN_OVERLAP = (0.7, 0.5, 0.5)               # :56, the same row for the three metrics
N_SAMPLE_PTS = 41
NO_DETECTION = -10000000.0


def compute_alpha(x, z, ry):
    beta = np.arctan2(z, x)
    return -np.sign(beta) * np.pi / 2 + beta + ry


def label_rows(dets, rows, boxes2d, row_box):
    """dets (R,8) [tx,ty,tz,l,w,h,ry,score] -> table (n,13) fp64, ok (n) bool (False: the reference drops the row)."""
    d = np.asarray(dets, dtype=np.float64)[np.asarray(rows, dtype=np.int64)]
    b = np.asarray(boxes2d, dtype=np.float64)[np.asarray(row_box, dtype=np.int64)]
    alpha = np.array([compute_alpha(r[0], r[2], r[6]) for r in d]).reshape(-1)
    table = np.concatenate([alpha[:, None], b, d[:, [5, 4, 3]], d[:, [0, 1, 2]], d[:, [6]], d[:, [7]]], 1)
    ok = ~((d[:, 5] < 0.01) | (d[:, 4] < 0.01) | (d[:, 3] < 0.01))
    return table, ok


# ---- overlaps: d a detection row (13), g a label row (14); criterion -1 union, 0 over the detection
def image_overlap(d, g, criterion=-1):
    x1, y1, x2, y2 = max(d[1], g[3]), max(d[2], g[4]), min(d[3], g[5]), min(d[4], g[6])
    w, h = x2 - x1, y2 - y1
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    a_area, b_area = (d[3] - d[1]) * (d[4] - d[2]), (g[5] - g[3]) * (g[6] - g[4])
    return inter / (a_area + b_area - inter) if criterion == -1 else inter / a_area


def _polygon(ry, l, w, t1, t3):
    """toPolygon (:271-293): mref = [[cos, sin], [-sin, cos]] times the corners (+-l/2, +-w/2), moved to (t1, t3)."""
    c, s = np.cos(ry), np.sin(ry)
    xs, zs = np.array([l, l, -l, -l]) / 2, np.array([w, -w, -w, w]) / 2
    return np.stack([c * xs + s * zs + t1, -s * xs + c * zs + t3], 1)


def _inter_area(d, g):
    dp, gp = _polygon(d[11], d[7], d[6], d[8], d[10]), _polygon(g[13], g[9], g[8], g[10], g[12])
    return box_ref._area(box_ref._clip(gp, dp)), box_ref._area(dp), box_ref._area(gp)


def ground_overlap(d, g, criterion=-1):
    inter, da, ga = _inter_area(d, g)
    return inter / (da + ga - inter) if criterion == -1 else inter / da          # (area of the union = sum - intersection)


def box3d_overlap(d, g, criterion=-1):
    inter, _, _ = _inter_area(d, g)
    ymax, ymin = min(d[9], g[11]), max(d[9] - d[5], g[11] - g[7])
    inter_vol = inter * max(0.0, ymax - ymin)
    det_vol, gt_vol = d[5] * d[7] * d[6], g[7] * g[9] * g[8]
    return inter_vol / (det_vol + gt_vol - inter_vol) if criterion == -1 else inter_vol / det_vol


OVERLAP = (image_overlap, ground_overlap, box3d_overlap)


def pair_overlaps(d, g, criterion):
    """The three overlaps of one pair with ONE clip (ground and 3-D share it).  Two rectangles whose centres lie further apart
    than their half diagonals add up to cannot meet: their intersection is 0 without the clip (a shortcut of this restatement;
    the value is the clip's)."""
    out = [image_overlap(d, g, criterion), 0.0, 0.0]
    if np.hypot(d[8] - g[10], d[10] - g[12]) < 0.5 * (np.hypot(d[7], d[6]) + np.hypot(g[9], g[8])):
        out[1], out[2] = ground_overlap(d, g, criterion), box3d_overlap(d, g, criterion)
    return out


def frame_overlaps(det, gt, gt_type):
    """(nd_f, ng_f, 3): what the device stores -- criterion 0 against a DontCare label (the only one asked of it), -1 otherwise."""
    out = np.zeros((len(det), len(gt), 3))
    for j in range(len(det)):
        for i in range(len(gt)):
            out[j, i] = pair_overlaps(det[j], gt[i], 0 if gt_type[i] == DONTCARE else -1)
    return out


def get_thresholds(v, n_groundtruth):
    v = sorted(v, reverse=True)
    t, current_recall = [], 0.0
    for i in range(len(v)):
        with np.errstate(all="ignore"):
            l_recall = np.float64(i + 1) / np.float64(n_groundtruth)
            r_recall = np.float64(i + 2) / np.float64(n_groundtruth) if i < len(v) - 1 else l_recall
        if (r_recall - current_recall) < (current_recall - l_recall) and i < len(v) - 1:
            continue
        t.append(v[i])
        current_recall += 1.0 / (N_SAMPLE_PTS - 1.0)
    return t


def clean_data(cls, gt, gt_type, det, det_class, difficulty):
    """-> ignored_gt, dontcare (indices), ignored_det, n_gt of one frame."""
    ignored_gt, n_gt = [], 0
    for i in range(len(gt)):
        height = gt[i][6] - gt[i][4]
        if gt_type[i] == cls:
            valid_class = 1
        elif cls == PEDESTRIAN and gt_type[i] == PERSON_SITTING:
            valid_class = 0
        elif cls == CAR and gt_type[i] == VAN:
            valid_class = 0
        else:
            valid_class = -1
        ignore = int(gt[i][1]) > MAX_OCCLUSION[difficulty] or gt[i][0] > MAX_TRUNCATION[difficulty] or height < MIN_HEIGHT[difficulty]
        if valid_class == 1 and not ignore:
            ignored_gt.append(0)
            n_gt += 1
        elif valid_class == 0 or (ignore and valid_class == 1):
            ignored_gt.append(1)
        else:
            ignored_gt.append(-1)
    dc = [i for i in range(len(gt)) if gt_type[i] == DONTCARE]
    ignored_det = []
    for j in range(len(det)):
        valid_class = 1 if det_class[j] == cls else -1
        height = int(np.fabs(det[j][2] - det[j][4]))             # int32_t height = fabs(...): truncated
        if height < MIN_HEIGHT[difficulty]:
            ignored_det.append(1)
        elif valid_class == 1:
            ignored_det.append(0)
        else:
            ignored_det.append(-1)
    return ignored_gt, dc, ignored_det, n_gt


def candidates(ov, metric, cls):
    """Per label the detections (ascending) whose overlap exceeds the minimum: every branch of the searches below asks for it, so
    walking these alone skips nothing (it makes the 41 repetitions per list affordable in Python)."""
    return [np.nonzero(ov[:, i, metric] > MIN_OVERLAP[cls])[0].tolist() for i in range(ov.shape[1])]


def compute_statistics(cls, gt, det, dc, ignored_gt, ignored_det, compute_fp, ov, metric, compute_aos=False, thresh=0.0, cand=None):
    """ov (nd_f, ng_f, 3) of frame_overlaps; cand: candidates(ov, metric, cls) when the caller has them.
    -> dict tp, fp, fn, similarity, v (the true positives' scores)."""
    cand = candidates(ov, metric, cls) if cand is None else cand
    tp = fp = fn = 0
    v, delta = [], []
    similarity = 0.0
    nd = len(det)
    assigned_detection = [False] * nd
    ignored_threshold = [bool(compute_fp and det[j][12] < thresh) for j in range(nd)]
    mo = MIN_OVERLAP[cls]
    for i in range(len(gt)):
        if ignored_gt[i] == -1:
            continue
        det_idx, valid_detection, max_overlap, assigned_ignored_det = -1, NO_DETECTION, 0.0, False
        for j in cand[i]:
            if ignored_det[j] == -1 or assigned_detection[j] or ignored_threshold[j]:
                continue
            overlap = ov[j, i, metric]
            if not compute_fp and overlap > mo and det[j][12] > valid_detection:
                det_idx, valid_detection = j, det[j][12]
            elif compute_fp and overlap > mo and (overlap > max_overlap or assigned_ignored_det) and ignored_det[j] == 0:
                max_overlap, det_idx, valid_detection, assigned_ignored_det = overlap, j, 1, False
            elif compute_fp and overlap > mo and valid_detection == NO_DETECTION and ignored_det[j] == 1:
                det_idx, valid_detection, assigned_ignored_det = j, 1, True
        if valid_detection == NO_DETECTION and ignored_gt[i] == 0:
            fn += 1
        elif valid_detection != NO_DETECTION and (ignored_gt[i] == 1 or ignored_det[det_idx] == 1):
            assigned_detection[det_idx] = True
        elif valid_detection != NO_DETECTION:
            tp += 1
            v.append(det[det_idx][12])
            if compute_aos:
                delta.append(gt[i][2] - det[det_idx][0])
            assigned_detection[det_idx] = True
    if compute_fp:
        for j in range(nd):
            if not (assigned_detection[j] or ignored_det[j] == -1 or ignored_det[j] == 1 or ignored_threshold[j]):
                fp += 1
        nstuff = 0
        for i in dc:
            for j in cand[i]:
                if assigned_detection[j] or ignored_det[j] == -1 or ignored_det[j] == 1 or ignored_threshold[j]:
                    continue
                if ov[j, i, metric] > mo:                        # (criterion 0: frame_overlaps stores it for DontCare)
                    assigned_detection[j] = True
                    nstuff += 1
        fp -= nstuff
        if compute_aos:
            if tp > 0 or fp > 0:
                for x in delta:                                  # accumulate(tmp): fp zeros first, then the true positives in order
                    similarity += (1.0 + np.cos(x)) / 2.0
            else:
                similarity = -1
    return {"tp": tp, "fp": fp, "fn": fn, "similarity": similarity, "v": v}


def _max_element(a):
    """*std::max_element: the first of the largest under <."""
    largest = 0
    for j in range(1, len(a)):
        if a[largest] < a[j]:
            largest = j
    return a[largest]


def eval_class(cls, frames, ovs, compute_aos, difficulty, metric):
    n_gt, v, cleaned = 0, [], []
    for (det, det_class, gt, gt_type), ov in zip(frames, ovs):
        i_gt, dc, i_det, n = clean_data(cls, gt, gt_type, det, det_class, difficulty)
        n_gt += n
        cleaned.append((i_gt, dc, i_det, candidates(ov, metric, cls)))
        v += compute_statistics(cls, gt, det, dc, i_gt, i_det, False, ov, metric, cand=cleaned[-1][3])["v"]
    thresholds = get_thresholds(v, n_gt)
    T = len(thresholds)
    tp, fp, fn, sim = np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T, np.int64), np.zeros(T)
    for (det, det_class, gt, gt_type), ov, (i_gt, dc, i_det, cand) in zip(frames, ovs, cleaned):
        for t in range(T):
            st = compute_statistics(cls, gt, det, dc, i_gt, i_det, True, ov, metric, compute_aos, thresholds[t], cand)
            tp[t] += st["tp"]; fp[t] += st["fp"]; fn[t] += st["fn"]
            if st["similarity"] != -1:
                sim[t] += st["similarity"]
    precision, aos = np.zeros(N_SAMPLE_PTS), np.zeros(N_SAMPLE_PTS)
    with np.errstate(all="ignore"):
        for i in range(T):
            precision[i] = np.float64(tp[i]) / np.float64(tp[i] + fp[i])
            aos[i] = np.float64(sim[i]) / np.float64(tp[i] + fp[i])
    for i in range(T):
        precision[i] = _max_element(precision[i:])
        aos[i] = _max_element(aos[i:])
    return {"n_gt": n_gt, "thresholds": thresholds, "tp": tp, "fp": fp, "fn": fn, "precision": precision, "aos": aos, "tp_scores": v}


def evaluate(det, det_class, det_off, gt, gt_type, gt_off, classes=(0, 1, 2)):
    """The whole evaluation in the layout of evaluate.kitti_eval (numpy arrays) + overlaps (npairs,3) and tp_scores (27 lists)."""
    det, gt = np.asarray(det, dtype=np.float64).reshape(-1, 13), np.asarray(gt, dtype=np.float64).reshape(-1, 14)
    det_class, gt_type = np.asarray(det_class).reshape(-1), np.asarray(gt_type).reshape(-1)
    F = len(det_off) - 1
    frames = [(det[det_off[f]:det_off[f + 1]], det_class[det_off[f]:det_off[f + 1]], gt[gt_off[f]:gt_off[f + 1]],
               gt_type[gt_off[f]:gt_off[f + 1]]) for f in range(F)]
    ovs = [frame_overlaps(fr[0], fr[2], fr[3]) for fr in frames]
    compute_aos = not (det[:, 0] == -10).any()
    col = (1, 8, 9)                                  # eval_image: x1 >= 0; eval_ground: t1 != -1000; eval_3d: t2 != -1000
    out = {"precision": np.full((3, 3, 3, 41), np.nan), "aos": np.full((3, 3, 41), np.nan), "ap": np.full((3, 3, 3), np.nan),
           "aos_ap": np.full((3, 3), np.nan), "thresholds": np.zeros((27, 41)), "num_thresholds": np.zeros(27, np.int32),
           "n_gt": np.zeros(27, np.int32), "tp": np.zeros((27, 41), np.int32), "fp": np.zeros((27, 41), np.int32),
           "fn": np.zeros((27, 41), np.int32), "tp_scores": [[] for _ in range(27)],
           "overlaps": np.concatenate([o.reshape(-1, 3) for o in ovs] + [np.zeros((0, 3))])}
    for m in range(3):
        for c in range(3):
            if c not in classes:
                continue
            mine = det[det_class == c]
            evaluated = bool(((mine[:, 1] >= 0) if m == 0 else (mine[:, col[m]] != -1000)).any())
            for dl in range(3):
                k = (m * 3 + c) * 3 + dl
                r = eval_class(c, frames, ovs, m == 0, dl, m)      # (the similarity is summed whatever compute_aos says)
                T = len(r["thresholds"])
                out["thresholds"][k, :T] = r["thresholds"]
                out["num_thresholds"][k], out["n_gt"][k], out["tp_scores"][k] = T, r["n_gt"], r["tp_scores"]
                out["tp"][k, :T], out["fp"][k, :T], out["fn"][k, :T] = r["tp"], r["fp"], r["fn"]
                if not evaluated:
                    continue
                out["precision"][m, c, dl] = r["precision"]
                out["ap"][m, c, dl] = _ap(r["precision"])
                if m == 0 and compute_aos:
                    out["aos"][c, dl] = r["aos"]
                    out["aos_ap"][c, dl] = _ap(r["aos"])
    return out


def _ap(vals):
    """saveAndPlotPlots :716-720, in fp64 (the reference's float sum is for printing only): entries 0, 4, .., 40 in order."""
    s = 0.0
    for i in range(0, len(vals), 4):
        s += vals[i]
    return s / 11 * 100
