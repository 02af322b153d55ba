"""The two-stage cascade on the device: first-stage boxes -> refinement-stage inputs (C-ABI fcn_refine_select_count / _fill,
csrc/refine_select.h) and a thin driver over both stages.

Reference: kitti/prepare_data_refine.py::extract_frustum_data_rgb_detection (:649-773) reads the first stage's result files,
enlarges every predicted box by 1.2, selects the frame's LiDAR points inside it with scipy.spatial.Delaunay(...).find_simplex
on the host -- once per box over the frame's whole point cloud -- and pickles them for datasets/provider_sample_refine.py.
Here the selection is two HIP launches and the selected points go straight into RefineInputBuilder.build_device; between the
stages the host reads the first stage's keep lists, D point counts and D predicted widths, and each of the two entry points
reads the 2 * D candidate indices back to range-check them (five small reads that wait for the stream; no point data).  No CPU
fallback.

Training the refinement stage on the first stage's output (extract_frustum_det_data :406-592: match to the labels, enlarge, jitter,
select, count the positives, reject) is match_detections + draw_box3d_jitter + refine_training_candidates (C-ABI fcn_refine_match,
fcn_refine_label_count / _fill, csrc/refine_label.h) and RefineInputBuilder.build_device_train.
"""
import numpy as np
import torch

from . import _native
from .detect import _need_cuda


def refine_candidates(frame_points, frame_off, dets, cand_row, cand_frame, ratio=1.2):
    """frame_points (sum m_f, stride >= 3) float32 rect camera coordinates of F frames packed behind each other (columns from 3
    on travel untouched), frame_off (F+1) int64 row offsets, dets (R,8) float32 label-format rows [tx,ty,tz,l,w,h,ry,score] as
    decode_detections / PointNetDet.detect return them, cand_row (D) indices into dets, cand_frame (D) the frame of each --
    device tensors (the two lists may be host sequences).  Every candidate box is enlarged by `ratio` about its centre.
    Returns a dict: points (sum cnt, stride) the frame rows inside each enlarged box, candidate after candidate in frame order;
    off (D+1) int64; pred_box3d (D,8,3), pred_angle (D), pred_size (D,3) fp64 (the enlarged box: corners in the order of
    compute_box_3d_obj_array, ry, l/w/h); cnt (D) int32; score (D) float32 (column 7 of the candidates' rows) -- on the device --
    and counts (D) int64 on the host: the one read between the two launches."""
    _need_cuda(frame_points, "refine_candidates")
    dev = frame_points.device
    pts = frame_points.detach().contiguous().float()
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("refine_candidates: frame_points must be (n, >= 3), got %s" % (tuple(frame_points.shape),))
    foff = torch.as_tensor(frame_off).to(device=dev, dtype=torch.int64).contiguous()
    d8 = dets.detach().to(device=dev, dtype=torch.float32).contiguous()
    if d8.dim() != 2 or d8.shape[1] != 8:
        raise ValueError("refine_candidates: dets must be (R, 8), got %s" % (tuple(dets.shape),))
    crow = torch.as_tensor(cand_row).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    cframe = torch.as_tensor(cand_frame).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if crow.numel() != cframe.numel():
        raise ValueError("refine_candidates: %d rows but %d frames" % (crow.numel(), cframe.numel()))
    F, R, D, ps = int(foff.numel()) - 1, int(d8.shape[0]), int(crow.numel()), int(pts.shape[1])
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"pred_box3d": torch.zeros((D, 8, 3), **f64), "pred_angle": torch.zeros((D,), **f64),
           "pred_size": torch.zeros((D, 3), **f64), "cnt": torch.zeros((D,), dtype=torch.int32, device=dev)}
    L = _native.lib()
    args = (pts.data_ptr(), foff.data_ptr(), F, ps, d8.data_ptr(), R, crow.data_ptr(), cframe.data_ptr(), D, float(ratio))
    with torch.cuda.device(dev):
        _native.check(L.fcn_refine_select_count(*args, out["pred_box3d"].data_ptr(), out["pred_angle"].data_ptr(),
                                                out["pred_size"].data_ptr(), out["cnt"].data_ptr(),
                                                _native.current_stream(dev)), "fcn_refine_select_count")
        counts = out["cnt"].cpu().numpy().astype(np.int64)                 # D integers: the size of `points`
        off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        out["off"] = torch.from_numpy(off).to(dev, non_blocking=True)
        out["points"] = torch.empty((int(off[-1]), ps), dtype=torch.float32, device=dev)
        if off[-1] > 0:
            _native.check(L.fcn_refine_select_fill(*args, out["off"].data_ptr(), out["points"].data_ptr(),
                                                   _native.current_stream(dev)), "fcn_refine_select_fill")
    out["score"] = d8[:, 7].index_select(0, crow.to(torch.int64)) if D else d8[:0, 7]
    out["counts"] = counts
    return out



def _candidates(who, frame_points, dets, cand_row, cand_frame):
    """The device tensors the match and the labelled selection share: dets (R,8) float32, cand_row / cand_frame (D) int32."""
    dev = frame_points.device
    d8 = dets.detach().to(device=dev, dtype=torch.float32).contiguous()
    if d8.dim() != 2 or d8.shape[1] != 8:
        raise ValueError("%s: dets must be (R, 8), got %s" % (who, tuple(dets.shape)))
    crow = torch.as_tensor(cand_row).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    cframe = torch.as_tensor(cand_frame).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    if crow.numel() != cframe.numel():
        raise ValueError("%s: %d rows but %d frames" % (who, crow.numel(), cframe.numel()))
    return d8, crow, cframe


def match_detections(dets, cand_row, cand_frame, gt_box3d, gt_off, thresh):
    """Matches first-stage detections to the label boxes of their frames (kitti/prepare_data_refine.py:483-499; C-ABI
    fcn_refine_match).  dets (R,8) float32 label-format rows on the device, cand_row (D) / cand_frame (D) as refine_candidates
    takes them; gt_box3d (G,7) tx, ty, tz, l, w, h, ry of every label box (t the bottom centre), frame after frame; gt_off (F+1)
    int64: the label boxes of frame f are rows [gt_off[f], gt_off[f+1]); thresh: the reference uses 0.5 for Car and 0.25 otherwise.
    Returns (gt_idx (D) int32, best_iou (D) float32) on the device: the row of gt_box3d with the largest 3-D IoU (the lowest row
    among equal maxima), or -1 when the frame has no label box or the IoU is below thresh, and that IoU."""
    _need_cuda(dets, "match_detections")
    dev = dets.device
    d8, crow, cframe = _candidates("match_detections", dets, dets, cand_row, cand_frame)
    gt = torch.as_tensor(gt_box3d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 7)
    goff = torch.as_tensor(gt_off).to(device=dev, dtype=torch.int64).contiguous().view(-1)
    D, F = int(crow.numel()), int(goff.numel()) - 1
    gt_idx = torch.full((D,), -1, dtype=torch.int32, device=dev)
    best = torch.zeros((D,), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _native.check(_native.lib().fcn_refine_match(d8.data_ptr(), int(d8.shape[0]), crow.data_ptr(), cframe.data_ptr(), D,
                                                     gt.data_ptr() if gt.numel() else None, int(gt.shape[0]), goff.data_ptr(), F,
                                                     float(thresh), gt_idx.data_ptr(), best.data_ptr(),
                                                     _native.current_stream(dev)), "fcn_refine_match")
    return gt_idx, best


def draw_box3d_jitter(n, augmentX, rng=np.random):
    """The uniform draws of kitti/prepare_data_refine.py::random_shift_rotate_box3d (:203-236) for n candidates with augmentX
    chained copies each: (n, augmentX, 7) float64 in the reference's order -- candidates outer, copies inner, seven rng.random()
    per copy (l, h, w, cx, cy, cz, angle) -- so with the same seed the numbers are the reference's and the generator is left in
    its state.  The reference draws for MATCHED candidates only: draw for those (gt_idx >= 0) and scatter the rows into the
    (D, augmentX, 7) array refine_training_candidates takes; the rows of unmatched candidates are never read."""
    out = np.empty((int(n), int(augmentX), 7), dtype=np.float64)
    for i in range(int(n)):
        for a in range(int(augmentX)):
            for k in range(7):
                out[i, a, k] = rng.random()
    return out


def refine_training_candidates(frame_points, frame_off, dets, cand_row, cand_frame, cand_gt, gt_box3d, jitter=None, ratio=1.2,
                               shift_ratio=0.05):
    """The refinement stage's TRAINING records from first-stage detections and their matched label boxes, on the device: what
    kitti/prepare_data_refine.py::extract_frustum_det_data (:406-592) pickles.  frame_points ... cand_frame as refine_candidates
    takes them; cand_gt (D) the row of gt_box3d matched to each candidate (match_detections), negative: unmatched, skipped;
    gt_box3d (G,7) tx, ty, tz, l, w, h, ry; jitter (D,A,7) float64 uniform draws (draw_box3d_jitter) for A chained perturbed
    copies per candidate, or None: one un-jittered copy.  Units are u = d * A + a.  A unit without a point inside its label box
    is rejected (:547) and takes no room in the packed buffers.
    With label boxes as dets rows and cand_gt = arange this is extract_frustum_data (:239-403).
    Returns a dict over the K kept units: points (sum cnt, stride) float32; off (K+1) int64; pred_box3d (K,8,3), pred_angle (K),
    pred_size (K,3) of the jittered enlarged box and box3d (K,8,3), heading (K), size (K,3) of the label box, fp64; cnt (K), pos
    (K) int32 -- on the device -- and kept (K) int64 (unit indices), unit_cand (K) int64 (the candidate of each kept unit), counts
    (K) int64 on the host.  With no kept unit the dict holds 'kept' alone.
    The host reads the 2 * U * S selected and positive segment counts once, together, between the two launches."""
    who = "refine_training_candidates"
    _need_cuda(frame_points, who)
    dev = frame_points.device
    pts = frame_points.detach().contiguous().float()
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("%s: frame_points must be (n, >= 3), got %s" % (who, tuple(frame_points.shape)))
    foff_h = torch.as_tensor(frame_off).detach().cpu().to(torch.int64).contiguous().view(-1)      # F + 1 integers: they decide S
    foff = foff_h.to(dev, non_blocking=True)
    d8, crow, cframe = _candidates(who, frame_points, dets, cand_row, cand_frame)
    cgt = torch.as_tensor(cand_gt).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    gt = torch.as_tensor(gt_box3d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 7)
    F, R, D, G, ps = int(foff_h.numel()) - 1, int(d8.shape[0]), int(crow.numel()), int(gt.shape[0]), int(pts.shape[1])
    if cgt.numel() != D:
        raise ValueError("%s: %d candidates but %d cand_gt" % (who, D, cgt.numel()))
    A, jit = 1, None
    if jitter is not None:
        jit = torch.as_tensor(jitter).to(device=dev, dtype=torch.float64).contiguous()
        if jit.dim() != 3 or jit.shape[0] != D or jit.shape[2] != 7 or jit.shape[1] < 1:
            raise ValueError("%s: jitter must be (%d, A >= 1, 7), got %s" % (who, D, tuple(jit.shape)))
        A = int(jit.shape[1])
    none = {"kept": np.zeros(0, dtype=np.int64)}
    if D == 0 or F == 0 or G == 0:
        return none
    U = D * A
    L = _native.lib()
    seg = int(L.fcn_frustum_select_seg())
    S = max(1, -(-int((foff_h[1:] - foff_h[:-1]).max()) // seg))
    if pts.shape[0] == 0:
        pts = torch.zeros((1, ps), dtype=torch.float32, device=dev)        # (an address to hand in: every frame is empty)
    f64 = dict(dtype=torch.float64, device=dev)
    pc, pa, psz = torch.zeros((U, 8, 3), **f64), torch.zeros((U,), **f64), torch.zeros((U, 3), **f64)
    gc, gh, gs = torch.zeros((U, 8, 3), **f64), torch.zeros((U,), **f64), torch.zeros((U, 3), **f64)
    both = torch.zeros((2, U, S), dtype=torch.int32, device=dev)            # selected, positive: one read
    args = (pts.data_ptr(), foff.data_ptr(), F, ps, d8.data_ptr(), R, crow.data_ptr(), cframe.data_ptr(), D, float(ratio),
            cgt.data_ptr(), gt.data_ptr(), G, A, None if jit is None else jit.data_ptr(), float(shift_ratio), S)
    with torch.cuda.device(dev):
        _native.check(L.fcn_refine_label_count(*args, both[0].data_ptr(), both[1].data_ptr(), pc.data_ptr(), pa.data_ptr(),
                                               psz.data_ptr(), gc.data_ptr(), gh.data_ptr(), gs.data_ptr(),
                                               _native.current_stream(dev)), "fcn_refine_label_count")
        both_h = both.cpu().numpy().astype(np.int64)                        # 2 * U * S integers
        seg_counts, positives = both_h[0], both_h[1].sum(1)
        drop = positives == 0                                               # (an unmatched candidate's units count nothing)
        kept = np.nonzero(~drop)[0].astype(np.int64)
        if len(kept) == 0:
            return {"kept": kept}
        seg_counts[drop] = 0
        seg_off = np.concatenate([[0], np.cumsum(seg_counts.reshape(-1))]).astype(np.int64)
        soff = torch.from_numpy(seg_off).to(dev, non_blocking=True)
        points = torch.empty((int(seg_off[-1]), ps), dtype=torch.float32, device=dev)
        _native.check(L.fcn_refine_label_fill(*args, soff.data_ptr(), points.data_ptr(), _native.current_stream(dev)),
                      "fcn_refine_label_fill")
    idx = torch.from_numpy(kept).to(dev, non_blocking=True)
    pick = lambda x: x.index_select(0, idx).contiguous()
    # a rejected unit has no rows, so a kept unit ends where the next kept one starts
    off = torch.cat([soff[::S][:U].index_select(0, idx), soff[-1:]])
    return {"points": points, "off": off, "pred_box3d": pick(pc), "pred_angle": pick(pa), "pred_size": pick(psz),
            "box3d": pick(gc), "heading": pick(gh), "size": pick(gs), "cnt": pick(both[0].sum(1, dtype=torch.int32)),
            "pos": pick(both[1].sum(1, dtype=torch.int32)), "kept": kept, "unit_cand": kept // A,
            "counts": seg_counts.sum(1)[kept]}


class TwoStageDetector:
    """stage1, stage2: two PointNetDet models in eval mode, each built by the caller under its own configuration (cfg is
    global: build one, then the other); refine_builder: the RefineInputBuilder of the second stage's configuration;
    input_builder: the InputBuilder of the first stage's configuration (detect_frames alone needs it)."""

    def __init__(self, stage1, stage2, refine_builder, input_builder=None):
        self.stage1, self.stage2, self.refine_builder, self.input_builder = stage1, stage2, refine_builder, input_builder

    def detect_frames(self, frame_points_velo, frame_off, calib, img_size, boxes2d, box_frame, types, prob, method, thresh,
                      unit_group=None, num_groups=None, top_k=300, ratio=1.2, draws=None, refine_draws=None,
                      clip_distance=2.0, clip_boxes=True, img_height_threshold=5, lidar_point_threshold=1):
        """From LiDAR frames and a 2-D detector's boxes to second-stage detections: frame_points_velo / frame_off, calib,
        img_size, boxes2d (D,4), box_frame (D), clip_distance, clip_boxes as frustum.frustum_candidates takes them; types (D) /
        prob (D): class name and score of each box; unit_group (D) / num_groups: the (frame, class) group of each BOX (default:
        every surviving box its own); draws / refine_draws: the resample indices of the first / second stage's builder.
        Steps: frustum_candidates -> input_builder.build_device (drops boxes too small or without points: 'kept') ->
        image_fov_points -> detect(...) with the kept boxes' frames, types and groups.
        Returns detect()'s dict + kept (B,) int64 (host): the box each first-stage frustum came from.  With no surviving box
        every other entry is None (stage1_row is empty)."""
        from . import frustum
        if self.input_builder is None:
            raise ValueError("TwoStageDetector.detect_frames needs the first stage's InputBuilder (input_builder=...)")
        sel = frustum.frustum_candidates(frame_points_velo, frame_off, calib, img_size, boxes2d, box_frame, clip_distance, clip_boxes)
        batch = self.input_builder.build_device(sel, calib["P"], types, prob, draws=draws,
                                                img_height_threshold=img_height_threshold,
                                                lidar_point_threshold=lidar_point_threshold)
        kept = batch.pop("kept")
        if len(kept) == 0:
            return {"dets": None, "valid": None, "keep": None, "cnt": None, "stage1_row": np.zeros((0,), dtype=np.int64),
                    "stage1": None, "kept": kept}
        fov_pts, fov_off = frustum.image_fov_points(frame_points_velo, frame_off, calib, img_size, clip_distance)
        frame = torch.as_tensor(box_frame).cpu().numpy().reshape(-1).astype(np.int64)[kept]
        ug = None if unit_group is None else torch.as_tensor(unit_group).cpu().numpy().reshape(-1)[kept]
        if ug is not None and num_groups is None:
            num_groups = int(ug.max()) + 1
        res = self.detect(batch, fov_pts, fov_off, frame, [types[i] for i in kept], method, thresh,
                          unit_group=None if ug is None else torch.from_numpy(ug.astype(np.int32)), num_groups=num_groups,
                          top_k=top_k, ratio=ratio, draws=refine_draws)
        res["kept"] = kept
        return res

    def detect(self, data_dicts, frame_points, frame_off, frustum_frame, types, method, thresh, unit_group=None,
               num_groups=None, top_k=300, ratio=1.2, draws=None):
        """data_dicts: the first stage's batch of B frustums; frame_points / frame_off: the points to search, per frame (see
        refine_candidates); frustum_frame (B) the frame of each frustum and types (B) its class name (host sequences);
        method / thresh: as PointNetDet.detect, for both stages; unit_group (B) / num_groups: the (frame, class) group of
        each frustum (default: every frustum its own) -- a second-stage unit inherits its frustum's group.
        Steps: stage1.detect -> keep lists to the host -> refine_candidates -> refine_builder.build_device (draws: its
        resample indices, for reproducible runs) -> stage2.detect.
        Returns a dict: dets, valid, keep, cnt of the second stage (device), stage1_row (B2,) int64 (host) the first-stage
        row of dets each second-stage unit refines, and stage1 = the first stage's (dets, valid, keep, cnt).  When the
        first stage keeps nothing, or no kept box holds a point, the second-stage entries are None and stage1_row is empty."""
        s1 = self.stage1.detect(data_dicts, unit_group=unit_group, num_groups=num_groups, method=method, thresh=thresh,
                                top_k=top_k)
        dets1, _, keep1, cnt1 = s1
        L2 = int(data_dicts["center_ref2"].shape[2])
        B = int(data_dicts["center_ref2"].shape[0])
        keep_h, cnt_h = keep1.cpu().numpy(), cnt1.cpu().numpy()
        rows = [keep_h[g, :c] for g, c in enumerate(cnt_h) if c > 0]
        rows = np.concatenate(rows).astype(np.int64) if rows else np.zeros((0,), dtype=np.int64)
        res = {"dets": None, "valid": None, "keep": None, "cnt": None, "stage1_row": rows[:0], "stage1": s1}
        if len(rows) == 0:
            return res
        unit = rows // L2                                                    # the frustum each kept row came from
        frame = np.asarray(frustum_frame, dtype=np.int64).reshape(B)[unit]
        cands = refine_candidates(frame_points, frame_off, dets1, rows.astype(np.int32), frame.astype(np.int32), ratio)
        batch = self.refine_builder.build_device(cands, [types[u] for u in unit], draws=draws)
        kept = batch.pop("kept")
        if len(kept) == 0:
            return res
        batch.pop("lens")
        ug1 = np.arange(B) if unit_group is None else torch.as_tensor(unit_group).cpu().numpy().reshape(B)
        ng = B if unit_group is None else (int(ug1.max()) + 1 if num_groups is None else num_groups)
        ug2 = torch.from_numpy(ug1[unit[kept]].astype(np.int32)).to(dets1.device)
        d2, v2, k2, c2 = self.stage2.detect(batch, unit_group=ug2, num_groups=ng, method=method, thresh=thresh, top_k=top_k)
        res.update(dets=d2, valid=v2, keep=k2, cnt=c2, stage1_row=rows[kept])
        return res
