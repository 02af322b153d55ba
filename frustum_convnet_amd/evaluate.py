"""SUN-RGBD detection on the device from depth frames to per-class AP (C-ABI fcn_decode_detections_rule, fcn_box3d_corners,
fcn_det_match, fcn_det_ap; csrc/det_eval.h).

Reference: train/test_net_det_sunrgbd.py -- test() (:148-278) decodes in numpy, write_detection_results_nms (:120-145) suppresses
per (image, class), write_detection_results (:85-117) turns every kept row into the corners of datasets/data_utils.py:44-70, and
train/sunrgbd_eval/eval_det.py:89-169 (eval_det_cls + voc_ap) clips every detection against every label box of its image and
class in Python, matches greedily in descending score and sums the precision / recall curve to an AP per class.  Here no point,
logit, box or IoU crosses to the host: the keep lists are read between the NMS and the corners (they size the buffers), and the
result is a dict of device tensors -- the AP table is what a caller reads.  No CPU fallback: CPU tensors raise.
SunrgbdFrameChain (SunrgbdDetector.frame_link) is detect_frames as ONE capturable sequence of launches at fixed sizes: a
frustum.SunrgbdDetectSource, the model's detect(rule="sunrgbd") over all F * C (frame, class) groups, the keep lists packed on the
device (C-ABI fcn_det_rows) and the corners -- nothing is read until result().

KITTI detections and labels to AP per class, difficulty and metric (C-ABI fcn_kitti_*; csrc/kitti_eval.h): kitti_label_rows,
kitti_eval, kitti_results below -- the reference's train/test_net_det.py:88-123 + train/kitti_eval/evaluate_object_3d_offline.cpp.
"""
import numpy as np
import torch

from . import _native
from .detect import _need_cuda, box3d_corners


def _offsets(who, name, off, total):
    """A CSR offset array as host int64, checked: it starts at 0, never decreases, ends at `total`."""
    o = torch.as_tensor(off).detach().cpu().numpy().reshape(-1).astype(np.int64)
    if len(o) < 1 or o[0] != 0 or (np.diff(o) < 0).any() or o[-1] != total:
        raise ValueError("%s: %s must ascend from 0 to %d, got %s%s" % (who, name, total, o[:8].tolist(), " ..." if len(o) > 8 else ""))
    if total >= 2 ** 31:
        raise ValueError("%s: %s counts %d rows; the entry points index with int32" % (who, name, total))
    return o


def match_detections_ap(det_corners, scores, det_off, gt_corners, gt_off, group_class, num_classes, thresh=0.25):
    """Matching and AP of eval_det.py:89-169 for every class at once.  The detections and label boxes come grouped by (image, class)
    in CSR form: det_corners (nd,8,3) float32 and scores (nd) on the device, det_off (G+1); gt_corners (ng,8,3) on the device,
    gt_off (G+1); group_class (G) the class of each group in [0, num_classes) -- the offsets and classes are host sequences.
    A group may lack detections (its label boxes count in npos only) or label boxes (its detections are false positives).
    Corners in the order of compute_box_3d (detect.box3d_corners), label boxes too.
    Returns a dict of device tensors: tp (nd) int32, ovmax (nd) float32 (-inf in a group without a label box), jmax (nd) int32 (the
    best label's index inside its group, first maximum; -1 without one), rank (nd) int32 (place inside the class by descending
    score, equal scores by the lower input index), rec / prec (nd) float64 (class c's curve in rank order, behind the curves of the
    classes below c), ap (num_classes) float64 (0 for a class without a detection) and npos (num_classes) int32.
    Refused with ValueError: offsets that do not ascend from 0 to nd / ng, a class outside the range, a class without a label
    box (npos == 0: the reference divides by it)."""
    who = "match_detections_ap"
    _need_cuda(det_corners, who)
    dev = det_corners.device
    dc = det_corners.detach().to(dtype=torch.float32).contiguous()
    if dc.dim() != 3 or tuple(dc.shape[1:]) != (8, 3):
        raise ValueError("%s: det_corners must be (nd, 8, 3), got %s" % (who, tuple(det_corners.shape)))
    nd = int(dc.shape[0])
    sc = torch.as_tensor(scores).detach().to(device=dev, dtype=torch.float32).contiguous().view(-1)
    if sc.numel() != nd:
        raise ValueError("%s: %d detections but %d scores" % (who, nd, sc.numel()))
    gc = torch.as_tensor(gt_corners).detach().to(device=dev, dtype=torch.float32).contiguous()
    if gc.dim() != 3 or tuple(gc.shape[1:]) != (8, 3):
        raise ValueError("%s: gt_corners must be (ng, 8, 3), got %s" % (who, tuple(gc.shape)))
    ng, C = int(gc.shape[0]), int(num_classes)
    doff, goff = _offsets(who, "det_off", det_off, nd), _offsets(who, "gt_off", gt_off, ng)
    gcls = torch.as_tensor(group_class).detach().cpu().numpy().reshape(-1).astype(np.int64)
    G = len(gcls)
    if len(doff) != G + 1 or len(goff) != G + 1:
        raise ValueError("%s: %d groups but %d / %d offsets" % (who, G, len(doff), len(goff)))
    if C < 1 or (G and (gcls.min() < 0 or gcls.max() >= C)):
        raise ValueError("%s: group_class must lie in [0, %d)" % (who, C))
    npos_h = np.bincount(gcls, weights=np.diff(goff), minlength=C).astype(np.int32)
    if (npos_h == 0).any():
        raise ValueError("%s: no label box of class(es) %s (npos == 0): leave such a class out" % (who, np.nonzero(npos_h == 0)[0].tolist()))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    doff_d, goff_d, npos = up(doff.astype(np.int32)), up(goff.astype(np.int32)), up(npos_h)
    dcls = up(np.repeat(gcls, np.diff(doff)).astype(np.int32))
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    out = {"tp": torch.zeros((nd,), **i32), "ovmax": torch.zeros((nd,), dtype=torch.float32, device=dev),
           "jmax": torch.full((nd,), -1, **i32), "rank": torch.zeros((nd,), **i32), "rec": torch.zeros((nd,), **f64),
           "prec": torch.zeros((nd,), **f64), "ap": torch.zeros((C,), **f64), "npos": npos}
    p = lambda t: t.data_ptr() if t.numel() else None
    L = _native.lib()
    with torch.cuda.device(dev):
        s = _native.current_stream(dev)
        _native.check(L.fcn_det_match(p(doff_d), p(goff_d), G, p(dc), p(sc), nd, p(gc), ng, float(thresh), p(out["tp"]),
                                      p(out["ovmax"]), p(out["jmax"]), s), "fcn_det_match")
        _native.check(L.fcn_det_ap(p(out["tp"]), p(sc), p(dcls), nd, p(npos), C, p(out["rank"]), p(out["rec"]), p(out["prec"]),
                                   p(out["ap"]), s), "fcn_det_ap")
    for t in (doff_d, goff_d, dcls, dc, sc, gc):
        t.record_stream(torch.cuda.current_stream(dev))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# KITTI: detections and labels to AP per class, difficulty and metric (C-ABI fcn_kitti_*; csrc/kitti_eval.h).
#
# Reference: train/test_net_det.py:88-123 writes every kept row as a line of label-format text and
# train/kitti_eval/evaluate_object_3d_offline.cpp ("the evaluator") reads the files back and clips every (detection, label) pair
# with boost polygons once per class x difficulty x metric x (1 + thresholds).  Here a pair is clipped once in fp32 and the
# detections never leave the device.  OUT OF SCOPE: the '%.4f' / '%f' text round trip of the result files (the evaluator sees
# numbers rounded to 4 decimals, this code the float32 values), the gnuplot plots and the mail.
KITTI_CLASSES = ("Car", "Pedestrian", "Cyclist")                                       # det_class 0, 1, 2
KITTI_TYPES = ("Car", "Pedestrian", "Cyclist", "Van", "Person_sitting", "DontCare")    # gt_type 0 .. 5; anything else: 6
KITTI_LISTS, KITTI_SLOTS = 27, 41


def kitti_type_codes(names, table=KITTI_TYPES):
    """Type names -> int codes: the place of each name in `table` (lower / upper case ignored, as the evaluator's strcasecmp does),
    len(table) for a name that is not in it.  table=KITTI_TYPES: gt_type.  table=KITTI_CLASSES: det_class, where 3 -- like any value
    outside 0..2 -- is a type that is not evaluated."""
    low = [t.lower() for t in table]
    return np.asarray([low.index(str(n).lower()) if str(n).lower() in low else len(table) for n in names], dtype=np.int32)


def kitti_label_rows(dets, rows, boxes2d, row_box):
    """The label-format row of every kept detection (train/test_net_det.py:88-105, :284-293): dets (R,8) [tx,ty,tz,l,w,h,ry,score]
    as decode_detections(rule="kitti") writes them, rows (n) the kept rows (None: all), boxes2d (D,4) the 2-D boxes and row_box
    (n) the box each kept row's frustum came from.  Device tensors in (rows / row_box may be host sequences), device tensors out:
    table (n,13) float32 [alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry, score] with alpha = compute_alpha(tx, tz, ry)
    (datasets/provider_sample.py:389-394) and ok (n) int32, 0 where h, w or l < 0.01 -- the reference drops such a row."""
    who = "kitti_label_rows"
    _need_cuda(dets, who)
    d = dets.detach().contiguous().float()
    if d.dim() != 2 or d.shape[1] != 8:
        raise ValueError("%s: dets must be (R, 8), got %s" % (who, tuple(dets.shape)))
    dev = d.device
    b = torch.as_tensor(boxes2d).detach().to(device=dev, dtype=torch.float32).contiguous()
    if b.dim() != 2 or b.shape[1] != 4:
        raise ValueError("%s: boxes2d must be (D, 4), got %s" % (who, tuple(b.shape)))
    r = None if rows is None else torch.as_tensor(rows).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    rb = torch.as_tensor(row_box).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    n = int(d.shape[0]) if r is None else int(r.numel())
    if rb.numel() != n:
        raise ValueError("%s: %d rows but %d row_box entries" % (who, n, rb.numel()))
    table = torch.empty((n, 13), dtype=torch.float32, device=dev)
    ok = torch.empty((n,), dtype=torch.int32, device=dev)
    p = lambda t: t.data_ptr() if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        _native.check(_native.lib().fcn_kitti_label_rows(p(d), int(d.shape[0]), p(r), n, p(b), int(b.shape[0]), p(rb), p(table), p(ok),
                                                         _native.current_stream(dev)), "fcn_kitti_label_rows")
    return table, ok


def kitti_eval(det_table, det_class, det_off, gt_table, gt_type, gt_off, classes=(0, 1, 2)):
    """The official KITTI evaluation of every class, difficulty and metric at once.  Detections and labels come per frame in CSR
    form: det_table (nd,13) float32 on the device (kitti_label_rows' rows), det_class (nd) int codes over KITTI_CLASSES (anything
    else: a type that is not evaluated), det_off (F+1); gt_table (ng,14) [truncation, occlusion, alpha, x1,y1,x2,y2, h,w,l,
    tx,ty,tz, ry], gt_type (ng) int codes over KITTI_TYPES (6: any other type), gt_off (F+1) -- the offsets are host sequences.
    classes: the classes to evaluate.
    Returns a dict of device tensors, indexed [metric (image, ground, 3-D)][class][difficulty (easy, moderate, hard)]:
    precision (3,3,3,41) float64, aos (3,3,41), ap (3,3,3), aos_ap (3,3); per list k = (metric * 3 + class) * 3 + difficulty:
    thresholds (27,41) float64 with num_thresholds (27), n_gt (27), tp / fp / fn (27,41) int32; and overlaps (npairs,3) float32
    (pair (d, g) of frame f at pair_off[f] + (d - det_off[f]) * labels_of_f + (g - gt_off[f]); pair_off: host int64), flags (10).
    The evaluator's host-side rules: a class without a detection (x1 >= 0 / tx != -1000 / ty != -1000 for the three metrics) is
    not evaluated, nor one left out of `classes` -- its precision / ap rows are NaN; aos / aos_ap are NaN throughout when any
    detection's alpha equals -10.  0 / 0 (no true and no false positive at a threshold) is NaN as IEEE has it and the evaluator
    prints it.  AP is summed in fp64 (the evaluator: in float, for printing only; 11 * 2^-24 * 100 < 7e-5 away)."""
    who = "kitti_eval"
    _need_cuda(det_table, who)
    dev = det_table.device
    dt = det_table.detach().to(dtype=torch.float32).contiguous()
    if dt.dim() != 2 or dt.shape[1] != 13:
        raise ValueError("%s: det_table must be (nd, 13), got %s" % (who, tuple(det_table.shape)))
    gtab = torch.as_tensor(gt_table).detach().to(device=dev, dtype=torch.float32).contiguous()
    if gtab.dim() != 2 or gtab.shape[1] != 14:
        raise ValueError("%s: gt_table must be (ng, 14), got %s" % (who, tuple(gtab.shape)))
    nd, ng = int(dt.shape[0]), int(gtab.shape[0])
    dcl = torch.as_tensor(det_class).detach().to(device=dev, dtype=torch.int32).contiguous().view(-1)
    gty = torch.as_tensor(gt_type).detach().to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if dcl.numel() != nd or gty.numel() != ng:
        raise ValueError("%s: %d detections / %d classes, %d labels / %d types" % (who, nd, dcl.numel(), ng, gty.numel()))
    doff, goff = _offsets(who, "det_off", det_off, nd), _offsets(who, "gt_off", gt_off, ng)
    F = len(doff) - 1
    if len(goff) != F + 1:
        raise ValueError("%s: %d / %d offsets: detections and labels must count the same frames" % (who, len(doff), len(goff)))
    cl = sorted(set(int(c) for c in classes))
    if not cl or cl[0] < 0 or cl[-1] > 2:
        raise ValueError("%s: classes must be a non-empty subset of (0, 1, 2), got %r" % (who, classes))
    mask = sum(1 << c for c in cl)
    poff = np.concatenate([[0], np.cumsum(np.diff(doff) * np.diff(goff))]).astype(np.int64)
    npairs = int(poff[-1])
    if npairs >= 2 ** 31:
        raise ValueError("%s: %d (detection, label) pairs; the entry points index with int32" % (who, npairs))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev, non_blocking=True)
    doff_d, goff_d, poff_d = up(doff.astype(np.int32)), up(goff.astype(np.int32)), up(poff.astype(np.int32))
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    i32, f32, f64 = torch.int32, torch.float32, torch.float64
    ov, flags = z((npairs, 3), f32), z((10,), i32)
    assigned, tp_score, srt = z((KITTI_LISTS, nd, 2), i32), z((KITTI_LISTS, ng), f32), z((KITTI_LISTS, ng), f32)
    tp_count, n_gt, nthr = z((KITTI_LISTS,), i32), z((KITTI_LISTS,), i32), z((KITTI_LISTS,), i32)
    thr, counts, sim = z((KITTI_LISTS, KITTI_SLOTS), f64), z((3, KITTI_LISTS, KITTI_SLOTS), i32), z((F, 9, KITTI_SLOTS), f64)
    prec, aos, ap, aos_ap = z((3, 3, 3, KITTI_SLOTS), f64), z((3, 3, KITTI_SLOTS), f64), z((3, 3, 3), f64), z((3, 3), f64)
    p = lambda t: t.data_ptr() if t.numel() else None
    scene = lambda: (p(doff_d), p(goff_d), p(poff_d), F, p(dt), p(dcl), nd, p(gtab), p(gty), ng, p(ov), npairs)
    L = _native.lib()
    with torch.cuda.device(dev):
        s = _native.current_stream(dev)
        _native.check(L.fcn_kitti_overlaps(*scene(), p(flags), s), "fcn_kitti_overlaps")
        _native.check(L.fcn_kitti_pass_a(*scene(), mask, p(assigned), p(tp_score), p(tp_count), p(n_gt), s), "fcn_kitti_pass_a")
        _native.check(L.fcn_kitti_thresholds(p(tp_score), p(tp_count), p(n_gt), ng, p(srt), p(thr), p(nthr), s), "fcn_kitti_thresholds")
        _native.check(L.fcn_kitti_pass_b(*scene(), mask, p(thr), p(nthr), p(assigned), p(counts), p(sim), s), "fcn_kitti_pass_b")
        _native.check(L.fcn_kitti_curves(p(counts), p(nthr), p(sim), F, p(flags), mask, p(prec), p(aos), p(ap), p(aos_ap), s),
                      "fcn_kitti_curves")
    for t in (doff_d, goff_d, poff_d, dt, dcl, gtab, gty, assigned, tp_score, srt, tp_count, sim):
        t.record_stream(torch.cuda.current_stream(dev))
    return {"precision": prec, "aos": aos, "ap": ap, "aos_ap": aos_ap, "thresholds": thr, "num_thresholds": nthr, "n_gt": n_gt,
            "tp": counts[0], "fp": counts[1], "fn": counts[2], "overlaps": ov, "pair_off": poff, "flags": flags}


def kitti_results(result, boxes2d, box_frame, types, num_frames=None):
    """From what a detector returned to the CSR detection table of kitti_eval.  result: the dict of TwoStageDetector.detect_frames
    (the second stage's dets / keep / cnt, stage1_row, stage1, kept), a dict with dets / keep / cnt / kept of a single-stage run
    over the boxes `kept`, or the tuple (dets, valid, keep, cnt) of PointNetDet.detect over ALL boxes in order; boxes2d (D,4),
    box_frame (D) and types (D): the 2-D detector's boxes, their frames and class names (host sequences; boxes2d may be a device
    tensor); num_frames: F (default: the largest frame index + 1).  Only the keep lists are read back, as
    SunrgbdDetector.detect_frames does.  The kept rows are ordered by frame (inside a frame: group after group in keep order).
    Returns a dict: det_table (n,13), det_class (n) int32, ok (n) int32 (device); det_off (F+1), rows (n), row_box (n) int64
    (host).  A row with ok == 0 (impossible behind the NMS, whose `valid` holds the same test) gets det_class -1 on the device
    instead of being dropped."""
    who = "kitti_results"
    if isinstance(result, dict):
        dets, keep, cnt = result["dets"], result["keep"], result["cnt"]
        unit_box = np.asarray(result["kept"], dtype=np.int64).reshape(-1)
        if "stage1_row" in result and dets is not None:
            l1 = int(result["stage1"][0].shape[0]) // max(1, len(unit_box))          # rows per first-stage frustum
            unit_box = unit_box[np.asarray(result["stage1_row"], dtype=np.int64) // l1]
    else:
        dets, _, keep, cnt = result
        unit_box = np.arange(len(types), dtype=np.int64)
    frame_all = torch.as_tensor(box_frame).cpu().numpy().reshape(-1).astype(np.int64)
    if len(frame_all) != len(types) or (len(frame_all) and frame_all.min() < 0):
        raise ValueError("%s: %d boxes have %d frames (all >= 0) and %d types" % (who, len(types), len(frame_all), len(types)))
    F = int(num_frames) if num_frames is not None else (int(frame_all.max()) + 1 if len(frame_all) else 0)
    if len(frame_all) and frame_all.max() >= F:
        raise ValueError("%s: frame %d with num_frames = %d" % (who, frame_all.max(), F))
    if dets is None:                                                             # nothing survived
        dev = torch.as_tensor(boxes2d).device if torch.is_tensor(boxes2d) and boxes2d.is_cuda else torch.device("cuda")
        zi = np.zeros((0,), dtype=np.int64)
        return {"det_table": torch.zeros((0, 13), dtype=torch.float32, device=dev), "det_class": torch.zeros((0,), dtype=torch.int32, device=dev),
                "ok": torch.zeros((0,), dtype=torch.int32, device=dev), "det_off": np.zeros((F + 1,), dtype=np.int64), "rows": zi, "row_box": zi}
    _need_cuda(dets, who)
    dev = dets.device
    if len(unit_box) == 0 or dets.shape[0] % len(unit_box):
        raise ValueError("%s: %d rows of dets do not divide into %d units" % (who, dets.shape[0], len(unit_box)))
    l2 = int(dets.shape[0]) // len(unit_box)
    keep_h, cnt_h = keep.cpu().numpy(), np.maximum(cnt.cpu().numpy().astype(np.int64), 0)
    rows = np.concatenate([keep_h[g, :cnt_h[g]] for g in range(len(cnt_h))] + [np.zeros((0,), dtype=np.int64)]).astype(np.int64)
    row_box = unit_box[rows // l2]
    order = np.argsort(frame_all[row_box], kind="stable")
    rows, row_box = rows[order], row_box[order]
    det_off = np.concatenate([[0], np.cumsum(np.bincount(frame_all[row_box], minlength=F))]).astype(np.int64)
    code = kitti_type_codes([types[i] for i in row_box], KITTI_CLASSES)
    table, ok = kitti_label_rows(dets, rows, boxes2d, row_box)
    cls = torch.from_numpy(np.where(code == len(KITTI_CLASSES), -1, code).astype(np.int32)).to(dev)
    cls = torch.where(ok != 0, cls, torch.full_like(cls, -1))
    return {"det_table": table, "det_class": cls, "ok": ok, "det_off": det_off, "rows": rows, "row_box": row_box}


class SunrgbdDetector:
    """model: the five-scale PointNetDet (det_base_sunrgbd) in eval mode; input_builder: the SunrgbdInputBuilder of its
    configuration.  detect_frames mirrors TwoStageDetector.detect_frames for the single-stage SUN-RGBD model; evaluate scores its
    result against label boxes."""

    def __init__(self, model, input_builder):
        self.model, self.input_builder = model, input_builder

    def detect_frames(self, frame_points, frame_off, K, Rtilt, boxes2d, box_frame, types, prob, method, thresh, top_k=300,
                      draws=None, sub=None):
        """From depth frames and a 2-D detector's boxes to the corners of the kept detections: frame_points / frame_off, K, Rtilt,
        boxes2d (D,4), box_frame (D), sub as frustum.sunrgbd_candidates takes them; types (D) / prob (D): class name and score of
        each box; draws: the resample indices of the builder.  Steps: sunrgbd_candidates -> input_builder.build_device (drops
        boxes with too few points: 'kept') -> model.detect(rule="sunrgbd") with one NMS group per (frame, class) of the surviving
        boxes -> keep lists to the host -> detect.box3d_corners of the kept rows.
        Returns a dict: dets, valid, keep, cnt (device, as PointNetDet.detect returns them); rows (n) int64 (host) the kept rows
        of dets, group after group in keep order; corners (n,8,3), scores (n) (device); det_off (G+1) int64, group_frame (G),
        group_class (G) int64 (host): the groups, ordered by (frame, class index); kept (B) int64 (host) the box each frustum
        came from.  With no surviving box every entry but kept, rows and the three group arrays (all empty) is None."""
        from . import frustum
        sel = frustum.sunrgbd_candidates(frame_points, frame_off, K, Rtilt, boxes2d, box_frame, sub=sub)
        batch = self.input_builder.build_device(sel, K, Rtilt, types, prob, draws=draws)
        kept = batch.pop("kept")
        z = np.zeros((0,), dtype=np.int64)
        if len(kept) == 0:
            return {"dets": None, "valid": None, "keep": None, "cnt": None, "rows": z, "corners": None, "scores": None,
                    "det_off": np.zeros((1,), dtype=np.int64), "group_frame": z, "group_class": z, "kept": kept}
        frame = torch.as_tensor(box_frame).cpu().numpy().reshape(-1).astype(np.int64)[kept]
        cls = np.asarray([self.input_builder.classes.index(types[i]) for i in kept], dtype=np.int64)
        pairs, ug = np.unique(np.stack([frame, cls], 1), axis=0, return_inverse=True)
        G = len(pairs)
        dev = batch["point_cloud"].device
        dets, valid, keep, cnt = self.model.detect(batch, unit_group=torch.from_numpy(ug.reshape(-1).astype(np.int32)).to(dev),
                                                   num_groups=G, method=method, thresh=thresh, top_k=top_k, rule="sunrgbd")
        keep_h, cnt_h = keep.cpu().numpy(), np.maximum(cnt.cpu().numpy().astype(np.int64), 0)
        rows = np.concatenate([keep_h[g, :cnt_h[g]] for g in range(G)]).astype(np.int64)
        rows_d = torch.from_numpy(rows).to(dev)
        return {"dets": dets, "valid": valid, "keep": keep, "cnt": cnt, "rows": rows, "corners": box3d_corners(dets, rows_d),
                "scores": dets[:, 7].index_select(0, rows_d), "det_off": np.concatenate([[0], np.cumsum(cnt_h)]).astype(np.int64),
                "group_frame": pairs[:, 0].copy(), "group_class": pairs[:, 1].copy(), "kept": kept}

    def evaluate(self, result, gt_corners, gt_frame, gt_class, thresh=0.25):
        """result: what detect_frames returned; gt_corners (ng,8,3) the label boxes as corners in the order of compute_box_3d
        (a device tensor or an array), gt_frame (ng) / gt_class (ng) the frame and class index of each (host sequences).
        As the reference's eval_det loops over the classes of the labels only, the classes evaluated are those with a label box:
        detections of any other class are left out.  Builds the (frame, class) groups -- those of the detections, then those
        that hold label boxes only -- and calls match_detections_ap.  Returns its dict + classes (the evaluated class indices,
        ascending: row c of ap / npos is class classes[c]) + det_index (host int64: the rows of result["corners"] that were
        evaluated, in the order of tp / ovmax / jmax / rank)."""
        dev = self.input_builder.device
        gc = torch.as_tensor(gt_corners).to(device=dev, dtype=torch.float32).reshape(-1, 8, 3)
        _need_cuda(gc, "SunrgbdDetector.evaluate")
        gf = np.asarray(gt_frame, dtype=np.int64).reshape(-1)
        gk = np.asarray(gt_class, dtype=np.int64).reshape(-1)
        if len(gf) != gc.shape[0] or len(gk) != gc.shape[0]:
            raise ValueError("evaluate: %d label boxes, %d frames, %d classes" % (gc.shape[0], len(gf), len(gk)))
        classes = np.unique(gk)
        if len(classes) == 0:
            raise ValueError("evaluate: no label box")
        doff = np.asarray(result["det_off"], dtype=np.int64)
        groups, dsel, dcount = [], [], []
        for g, (f, c) in enumerate(zip(result["group_frame"].tolist(), result["group_class"].tolist())):
            if c in classes:
                groups.append((f, c))
                dsel.append(np.arange(doff[g], doff[g + 1]))
                dcount.append(int(doff[g + 1] - doff[g]))
        have = set(groups)
        for f, c in sorted(set(zip(gf.tolist(), gk.tolist()))):
            if (f, c) not in have:
                groups.append((f, c))
                dcount.append(0)
        index = {fc: i for i, fc in enumerate(groups)}
        gt_group = np.asarray([index[fc] for fc in zip(gf.tolist(), gk.tolist())], dtype=np.int64)
        order = np.argsort(gt_group, kind="stable")
        goff = np.concatenate([[0], np.cumsum(np.bincount(gt_group, minlength=len(groups)))]).astype(np.int64)
        dsel = np.concatenate(dsel).astype(np.int64) if dsel else np.zeros((0,), dtype=np.int64)
        if result["corners"] is None or len(dsel) == 0:
            dcor = torch.zeros((0, 8, 3), dtype=torch.float32, device=dev)
            dsc = torch.zeros((0,), dtype=torch.float32, device=dev)
        else:
            pick = torch.from_numpy(dsel).to(dev)
            dcor, dsc = result["corners"].index_select(0, pick), result["scores"].index_select(0, pick)
        remap = {int(c): i for i, c in enumerate(classes)}
        out = match_detections_ap(dcor, dsc, np.concatenate([[0], np.cumsum(dcount)]), gc.index_select(0, torch.from_numpy(order).to(dev)),
                                  goff, [remap[c] for _, c in groups], len(classes), thresh)
        out["classes"] = classes
        out["det_index"] = dsel
        return out

    def frame_link(self, frame_points, frame_off, K, Rtilt, B, D, capacity, seed, method, thresh, top_k=300, **kw):
        """detect_frames() as one capturable sequence of launches at fixed sizes: a SunrgbdFrameChain over this detector's model and
        a frustum.SunrgbdDetectSource on its builder -- frame_points (held), frame_off, K, Rtilt, B (slots), D (rows of the
        detection table), capacity (rows of the point buffer), seed and, by keyword, cap, point_threshold, sub, choice as the source
        takes them.  The boxes, their frames, types and scores go into the returned chain's detection table
        (.source.set_boxes(...), or in place).  frame_link(...).step() then stands where detect_frames(...) stood."""
        from . import frustum
        source = frustum.SunrgbdDetectSource(frame_points, frame_off, K, Rtilt, self.input_builder, B, D, capacity, seed, **kw)
        return SunrgbdFrameChain(self.model, source, method, thresh, top_k)


# ---------------------------------------------------------------------------------------------------------------------------
# SUN-RGBD inference as ONE capturable sequence of launches: depth frames and 2-D boxes to corners, scores and group offsets
class SunrgbdFrameChain:
    """Resident depth frames and a resident table of 2-D detections -> the corners and scores of the kept detections, grouped by
    (frame, class), with no host read, no upload and no validation per step: what SunrgbdDetector.detect_frames does behind its
    synchronisations, as ONE sequence of launches that can be captured into a hipGraph and replayed on boxes and points overwritten
    in place (INTEGRATION.md "Capturable SUN-RGBD inference" states the contract).  model: the five-scale PointNetDet in eval mode;
    source: a frustum.SunrgbdDetectSource on the model's builder; method, thresh, top_k: as PointNetDet.detect.  The NMS groups are
    ALL F * C (frame, class) pairs, group g = frame * C + class; an empty slot belongs to the spare group F * C, which no NMS
    workgroup takes.  AP is a sum over the dataset and stays outside: SunrgbdDetector.evaluate takes result() unchanged."""

    KEYS = ("point_cloud", "rot_angle", "rgb_prob", "one_hot", "center_ref1", "center_ref2", "center_ref3", "center_ref4", "center_ref5")

    def __init__(self, model, source, method, thresh, top_k=300):
        who = "SunrgbdFrameChain"
        if model.training:
            raise ValueError("%s: the model must be in eval mode" % who)
        if method not in ("nms", "top"):
            raise ValueError("%s: method must be 'nms' or 'top', got %r" % (who, method))
        top_k = int(top_k)
        if not (1 <= top_k <= 4096):
            raise ValueError("%s: top_k must lie in [1, 4096] (the NMS sorts at most 4096 rows of a group), got %d" % (who, top_k))
        if not np.isfinite(float(thresh)):
            raise ValueError("%s: thresh must be finite, got %r" % (who, thresh))
        G = source.F * source.C
        if not (1 <= G <= 65536) or G * top_k >= 2 ** 31:
            raise ValueError("%s: F * C = %d groups (at most 65536) of %d rows" % (who, G, top_k))
        self.model, self.source, self.method, self.thresh, self.top_k, self.G = model, source, method, float(thresh), top_k, G
        dev = self.device = source.device
        self.R = source.B * source.builder.L[1]
        f32, i32 = dict(dtype=torch.float32, device=dev), dict(dtype=torch.int32, device=dev)
        n = G * top_k
        # det_off (G+1), n_rows, n_kept, rows (n) and slot_box (B) share ONE int32 buffer: result() reads it in one copy
        self.ints = torch.zeros((G + 3 + n + source.B,), **i32)
        self.det_off, self.n_rows, self.n_kept = self.ints[:G + 1], self.ints[G + 1:G + 2], self.ints[G + 2:G + 3]
        self.rows, self.slot_box = self.ints[G + 3:G + 3 + n], self.ints[G + 3 + n:]
        self.status = torch.zeros((1,), **i32)
        self.res = {"dets": torch.zeros((self.R, 8), **f32), "valid": torch.zeros((self.R,), **i32),
                    "keep": torch.full((G, top_k), -1, **i32), "cnt": torch.zeros((G,), **i32), "rows": self.rows,
                    "n_rows": self.n_rows, "det_off": self.det_off, "corners": torch.zeros((n, 8, 3), **f32),
                    "scores": torch.zeros((n,), **f32)}

    def step(self):
        """Enqueues on the current stream source.step(), model.detect(rule="sunrgbd") with the slots' groups, fcn_det_rows and
        fcn_box3d_corners -- and nothing else: no host read, no upload (capturable).  Returns a dict, the same device tensors every
        step: dets (B * L2, 8), valid, keep (G, top_k), cnt (G) as PointNetDet.detect returns them; rows (G * top_k) int32 the kept
        rows group after group in keep order (-1 behind n_rows), n_rows (1), det_off (G+1) int32, corners (G * top_k, 8, 3) and scores
        (G * top_k) of those rows (NaN behind n_rows); for inspection batch (the model's input), slot_box (B) and n_kept (1)."""
        src, res, G = self.source, self.res, self.G
        got = src.step()
        batch = {k: got[k] for k in self.KEYS if k in got}
        d, v, k, c = self.model.detect(batch, unit_group=src.slot_group, num_groups=G, method=self.method, thresh=self.thresh,
                                       top_k=self.top_k, rule="sunrgbd")
        if tuple(d.shape) != (self.R, 8) or tuple(k.shape) != (G, self.top_k):      # (attributes: nothing is read)
            raise ValueError("SunrgbdFrameChain.step: the model must give %d rows and %d groups of %d" % (self.R, G, self.top_k))
        res["dets"].copy_(d); res["valid"].copy_(v); res["keep"].copy_(k); res["cnt"].copy_(c)
        self.slot_box.copy_(src.slot_box); self.n_kept.copy_(src.n_kept)
        L, p = _native.lib(), (lambda x: x.data_ptr())
        with torch.cuda.device(self.device):
            s = _native.current_stream(self.device)
            _native.check(L.fcn_det_rows(p(res["keep"]), p(res["cnt"]), G, self.top_k, p(res["dets"]), self.R, p(self.det_off),
                                         p(self.rows), p(res["scores"]), p(self.n_rows), p(self.status), s), "fcn_det_rows")
            _native.check(L.fcn_box3d_corners(p(res["dets"]), self.R, p(self.rows), G * self.top_k, p(res["corners"]), s),
                          "fcn_box3d_corners")
        out = dict(res)
        out.update(batch=batch, slot_box=self.slot_box, n_kept=self.n_kept)
        return out

    def result(self):
        """The dict SunrgbdDetector.detect_frames returns, from the last step() -- ONE synchronisation: n_rows, det_off (and rows,
        the slots' boxes) are read in one copy.  The groups are all F * C (frame, class) pairs in that order; rows, corners and
        scores are cut to the n_rows kept rows (views of the chain's tensors: the next step() overwrites them)."""
        src, G, res = self.source, self.G, self.res
        h = self.ints.cpu().numpy().astype(np.int64)
        n, nk = int(h[G + 1]), int(h[G + 2])
        g = np.arange(G, dtype=np.int64)
        return {"dets": res["dets"], "valid": res["valid"], "keep": res["keep"], "cnt": res["cnt"], "rows": h[G + 3:G + 3 + n].copy(),
                "corners": res["corners"][:n], "scores": res["scores"][:n], "det_off": h[:G + 1].copy(), "group_frame": g // src.C,
                "group_class": g % src.C, "kept": h[G + 3 + G * self.top_k:][:nk].copy()}

    def check(self):
        """check() of the source and of the tail in one: reads their status words (a synchronisation), raises ValueError naming the
        bits set since the last check() and clears them."""
        from .frustum import check_status, STATUS_BITS
        src = self.source
        check_status("SunrgbdFrameChain", (src.status, src.draws.status, src.draws_sub.status, self.status), STATUS_BITS)
