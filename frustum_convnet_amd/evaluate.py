"""SUN-RGBD detection on the device from depth frames to per-class AP (C-ABI fcn_decode_detections_rule, fcn_box3d_corners,
fcn_det_match, fcn_det_ap; csrc/det_eval.h).

Reference: train/test_net_det_sunrgbd.py -- test() (:148-278) decodes in numpy, write_detection_results_nms (:120-145) suppresses
per (image, class), write_detection_results (:85-117) turns every kept row into the corners of datasets/data_utils.py:44-70, and
train/sunrgbd_eval/eval_det.py:89-169 (eval_det_cls + voc_ap) clips every detection against every label box of its image and
class in Python, matches greedily in descending score and sums the precision / recall curve to an AP per class.  Here no point,
logit, box or IoU crosses to the host: the keep lists are read between the NMS and the corners (they size the buffers), and the
result is a dict of device tensors -- the AP table is what a caller reads.  No CPU fallback: CPU tensors raise.
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
