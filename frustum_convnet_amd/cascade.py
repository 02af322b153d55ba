"""The two-stage cascade on the device: first-stage boxes -> refinement-stage inputs (C-ABI fcn_refine_select_count / _fill,
csrc/refine_select.h) and a thin driver over both stages.

Reference: kitti/prepare_data_refine.py::extract_frustum_data_rgb_detection (:649-773) reads the first stage's result files,
enlarges every predicted box by 1.2, selects the frame's LiDAR points inside it with scipy.spatial.Delaunay(...).find_simplex
on the host -- once per box over the frame's whole point cloud -- and pickles them for datasets/provider_sample_refine.py.
Here the selection is two HIP launches and the selected points go straight into RefineInputBuilder.build_device; between the
stages the host reads the first stage's keep lists, D point counts and D predicted widths, and each of the two entry points
reads the 2 * D candidate indices back to range-check them (five small reads that wait for the stream; no point data).  No CPU
fallback.  CascadeLink (TwoStageDetector.link) is the same link as ONE capturable sequence of launches at a fixed number of
candidates, a fixed batch size and fixed window counts, with no host read (C-ABI fcn_cascade_candidates, fcn_refine_detect_count /
_plan / _fill, csrc/cascade_plan.h).  FrameCascade (TwoStageDetector.frame_link) puts frustum.FrameDetectSource in front of it:
velodyne frames and a resident table of 2-D detections to second-stage detections, what detect_frames does, as one such sequence.

Training the refinement stage on the first stage's output (extract_frustum_det_data :406-592: match to the labels, enlarge, jitter,
select, count the positives, reject) is match_detections + draw_box3d_jitter + refine_training_candidates (C-ABI fcn_refine_match,
fcn_refine_label_count / _fill, csrc/refine_label.h) and RefineInputBuilder.build_device_train.  RefineTrainSource is the same link
as ONE capturable sequence of launches at a fixed batch size and fixed window counts, with no host read (C-ABI
fcn_refine_train_match / _count / _plan / _fill, fcn_box3d_jitter_draw, csrc/refine_plan.h).  The constructors' shared checks, the
spare corners and the batch skeleton of RefineTrainSource and CascadeLink are resident.py's, as for the four sources of frustum.py.
"""
import ctypes

import numpy as np
import torch

from . import _native, resident
from .detect import _need_cuda
from .frustum import FrameDetectSource, _frames, _packed, check_status
from .inputs import DeviceDraws


def refine_candidates(frame_points, frame_off, dets, cand_row, cand_frame, ratio=1.2):
    """frame_points (sum m_f, stride >= 3) float32 rect camera coordinates of F frames packed behind each other (columns from 3
    on travel untouched), frame_off (F+1) int64 row offsets, dets (R,8) float32 label-format rows [tx,ty,tz,l,w,h,ry,score] as
    decode_detections / PointNetDet.detect return them, cand_row (D) indices into dets, cand_frame (D) the frame of each --
    device tensors (the two lists may be host sequences).  Every candidate box is enlarged by `ratio` about its centre.
    Returns a dict: points (sum cnt, stride) the frame rows inside each enlarged box, candidate after candidate in frame order;
    off (D+1) int64; pred_box3d (D,8,3), pred_angle (D), pred_size (D,3) fp64 (the enlarged box: corners in the order of
    compute_box_3d_obj_array, ry, l/w/h); cnt (D) int32; score (D) float32 (column 7 of the candidates' rows) -- on the device --
    and counts (D) int64 on the host: the one read between the two launches."""
    pts, foff, F, ps, _ = _frames("refine_candidates", frame_points, frame_off)       # (one workgroup per box: no segments)
    dev = frame_points.device
    d8, crow, cframe = _candidates("refine_candidates", frame_points, dets, cand_row, cand_frame)
    R, D = int(d8.shape[0]), int(crow.numel())
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
        out["off"], out["points"] = _packed(counts, ps, dev)
        if out["points"].shape[0] > 0:
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
    pts, foff, F, ps, S = _frames(who, frame_points, frame_off)
    dev = frame_points.device
    d8, crow, cframe = _candidates(who, frame_points, dets, cand_row, cand_frame)
    cgt = torch.as_tensor(cand_gt).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    gt = torch.as_tensor(gt_box3d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 7)
    R, D, G = int(d8.shape[0]), int(crow.numel()), int(gt.shape[0])
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
        soff, points = _packed(seg_counts, ps, dev)
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


# ------------------------------------------------------------------------------------------------
# The refinement stage's training input as ONE capturable sequence of launches (csrc/refine_plan.h)
STATUS_BITS = ((1, "bit 0: a slot had no row to draw from (its choice row is zeros)"),
               (2, "bit 1: fewer units survived than the batch has slots (the empty slots hold the spare unit box over no rows)"),
               (4, "bit 2: the selected rows exceed the capacity of the point buffer (the overflow was dropped)"),
               (32, "bit 5: a unit's predicted width needs more windows than lpad on some stride (the unit was dropped)"),
               (64, "bit 6: a unit's predicted width is not a positive finite number (the unit was dropped)"),
               (128, "bit 7: the first stage kept more rows than the link has candidates (the rest were dropped)"),
               (256, "bit 8: more candidates survived than the batch has slots (the rest were dropped)"),
               (512, "bit 9: a first-stage group overflowed the NMS (cnt = -1) or reports cnt > top_k (it was passed on to nobody)"),
               (1024, "bit 10: n_boxes lies outside [0, D] or a box's frame outside [0, F) (the overflow or the box was ignored)"))


class RefineTrainSource:
    """Resident frames, a resident table of first-stage detections and the label boxes -> the RefineInputBuilder training batch at
    a FIXED batch size B and FIXED window counts lpad, every step, with no host read and no upload: what match_detections +
    draw_box3d_jitter + refine_training_candidates + RefineInputBuilder.build_device_train(draws=DeviceDraws) do behind their
    synchronisations, as one sequence of launches that can be captured into a hipGraph and draws anew on every replay
    (INTEGRATION.md "Capturable refine-stage training input" states the contract).
    frame_points / frame_off as refine_candidates takes them; dets (R,8) float32 ON THE DEVICE, contiguous: HELD, not copied -- a
    caller may overwrite it in place between steps with the first stage's fresh output; det_frame (R) the frame and det_types (R
    names) the class of each row; gt_box3d (G,7) / gt_off (F+1) as match_detections takes them; builder: a RefineInputBuilder;
    B: slots of the batch; D: detections tried per step; A: chained jittered copies per detection (units u = d * A + a; B <= D * A,
    D <= R, D * A <= 2048); capacity: rows of the point buffer (rows beyond it are dropped and flagged); lpad: four ints, the
    padded window counts of center_ref1..4 (a unit whose predicted width needs more is dropped and flagged); seed: the three
    generators are DeviceDraws keyed seed (detection pick), seed + 1 (box jitter), seed + 2 (per-sample draws), each one step
    further after every step().  pick=False: the first D detections in order; jitter=False: A = 1 without jitter; jitter=<(D,A,7)
    array>: that fixed table of uniforms on every step.  pick="epoch": the D detections are a rank window of the EPOCH's permutation
    of the R rows (inputs.EpochSampler keyed seed, held as self.sampler: every row at most once per epoch, the tail of
    R mod (D * world) dropped); rank / world, with this mode only: this rank's window among `world` sources built alike
    (D * world <= R).  The three DeviceDraws step on as under pick=False.
    Everything is validated here, once, on the host; step() validates nothing and reads nothing."""

    def __init__(self, frame_points, frame_off, dets, det_frame, det_types, gt_box3d, gt_off, builder, B, D, A, capacity, lpad,
                 seed, thresh=0.5, ratio=1.2, shift_ratio=0.05, pick=True, jitter=True, rank=None, world=None):
        who = "RefineTrainSource"
        pts, foff, F, ps, S = _frames(who, frame_points, frame_off, resident=True)
        dev = frame_points.device
        resident.held(who, dets, "dets", "(R, 8)", lambda t: t.shape[1] == 8)
        R = int(dets.shape[0])
        host, up = resident.host, lambda x: resident.up(x, dev)
        dfr = np.ascontiguousarray(host(det_frame)).reshape(-1)
        types = [str(t) for t in det_types]
        if len(dfr) != R or len(types) != R:
            raise ValueError("%s: %d dets, %d det_frame, %d det_types" % (who, R, len(dfr), len(types)))
        if R == 0 or dfr.dtype.kind not in "iu" or int(dfr.min()) < 0 or int(dfr.max()) >= F:
            raise ValueError("%s: det_frame must hold integers in [0, %d)" % (who, F))
        gt = np.ascontiguousarray(host(gt_box3d), dtype=np.float64).reshape(-1, 7)
        goff_h = np.ascontiguousarray(host(gt_off)).reshape(-1).astype(np.int64)
        G = len(gt)
        if len(goff_h) != F + 1 or goff_h[0] < 0 or (np.diff(goff_h) < 0).any() or goff_h[-1] > G:
            raise ValueError("%s: gt_off must be %d ascending row offsets into the %d label boxes" % (who, F + 1, G))
        if G == 0:
            raise ValueError("%s: no label box" % who)
        fixed = None
        if isinstance(jitter, (bool, np.bool_)):
            if not jitter and int(A) != 1:
                raise ValueError("%s: jitter=False goes with A = 1, got A = %d" % (who, int(A)))
        else:
            fixed = np.ascontiguousarray(host(jitter), dtype=np.float64)
            if fixed.shape != (int(D), int(A), 7):
                raise ValueError("%s: a jitter table must be (D, A, 7) = (%d, %d, 7), got %s" % (who, int(D), int(A), fixed.shape))
        B, D, A, capacity = int(B), int(D), int(A), int(capacity)
        max_u, max_segs = self.limits()
        if not (1 <= A <= 64):
            raise ValueError("%s: A must lie in [1, 64], got %d" % (who, A))
        U = D * A
        if not (1 <= B <= U and 1 <= D <= R) or U > max_u:
            raise ValueError("%s: need 1 <= B <= D * A, D <= R and D * A <= %d, got B = %d, D = %d, A = %d, R = %d" %
                             (who, max_u, B, D, A, R))
        if U * S > max_segs:
            raise ValueError("%s: D * A * S = %d * %d segments exceed the plan's %d" % (who, U, S, max_segs))
        resident.check_capacity(who, capacity)
        lpad = [int(x) for x in lpad]
        if len(lpad) != 4 or min(lpad) < 1:
            raise ValueError("%s: lpad must be four window counts >= 1, got %r" % (who, lpad))
        r = float(shift_ratio)
        if not (0.0 <= r < 1.0) or not (float(ratio) > 0.0):
            raise ValueError("%s: shift_ratio must lie in [0, 1) and ratio be positive, got %r, %r" % (who, shift_ratio, ratio))
        resident.need_device_builder(builder)
        cls = resident.class_index(who, builder.classes, types)
        pick, self.sampler = resident.pick_mode(who, pick, rank, world, seed, builder.device, D, R, "R")
        self.device, self.builder, self.lpad = dev, builder, lpad
        self.B, self.D, self.A, self.U, self.R, self.G, self.F, self.S, self.ps, self.capacity = B, D, A, U, R, G, F, S, ps, capacity
        self.pick, self.draw_jitter = pick, fixed is None and bool(jitter)
        self.thresh, self.ratio, self.shift_ratio = float(thresh), float(ratio), r
        f64, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.float64, torch.int32, torch.int64))
        N = builder.npoints
        # ---- resident: the frames, the detections (held), the labels
        self.frames = (pts, foff)
        self.dets = dets
        self.det_frame, self.det_class = up(dfr.astype(np.int32)), up(np.asarray(cls, dtype=np.int64).reshape(R, 1))
        self.gt, self.gt_off = up(gt), up(goff_h)
        self.eye = torch.eye(len(builder.classes), dtype=torch.float32, device=dev)
        self.r_count = torch.full((1,), R, **i64)
        self.strides_c = (ctypes.c_double * 4)(*builder.strides)
        self.lpad_c = (ctypes.c_int32 * 4)(*lpad)
        # ---- the generators
        seed = int(seed)
        self.draws_pick, self.draws_jitter, self.draws_sample = (DeviceDraws(seed + k, builder.device) for k in range(3))
        # ---- the batch and every intermediate
        self.points, self.seg_off, self.off, self.counts, self.slot_unit, self.n_kept, self.status = \
            resident.batch_skeleton(dev, B, U, S, capacity, ps, U)
        self.cand_row = torch.arange(D, **i32).view(1, D)
        self.pick_scalars = (torch.zeros((1,), **f64), torch.zeros((1,), **f64))
        self.cand_frame = torch.zeros((D,), **i32)
        self.cand_class = torch.zeros((D + 1, 1), **i64)        # row D: the spare entry's class, 0
        self.gt_idx, self.best_iou = torch.full((D,), -1, **i32), torch.zeros((D,), dtype=torch.float32, device=dev)
        self.jitter = None if (fixed is None and not jitter) else (torch.zeros((D, A, 7), **f64) if fixed is None else up(fixed))
        self.both = torch.zeros((2, U, S), **i32)               # selected, positive
        # the per-unit tables have U + 1 rows: row U is the spare entry an empty slot gathers -- a unit box at the origin, its
        # label box equal to the predicted one -- written here once and never by a kernel
        self.pred_box3d, self.box3d = torch.zeros((U + 1, 24), **f64), torch.zeros((U + 1, 24), **f64)
        self.pred_angle, self.heading = torch.zeros((U + 1,), **f64), torch.zeros((U + 1,), **f64)
        self.pred_size, self.size = torch.zeros((U + 1, 3), **f64), torch.zeros((U + 1, 3), **f64)
        for tab in (self.pred_box3d, self.box3d):
            tab[U] = resident.spare_corners(dev)
        for tab in (self.pred_size, self.size):
            tab[U] = 1.0
        self.slot_cand = torch.full((B,), D, **i32)
        self.unit_cand = torch.div(torch.arange(U + 1, **i32), A, rounding_mode="floor").to(torch.int32)     # row U -> D
        self.t = {"raw": self.points, "off": self.off, "choice": torch.zeros((B, N), **i32),
                  "pcorners": torch.zeros((B, 24), **f64), "pangle": torch.zeros((B,), **f64), "psize": torch.zeros((B, 3), **f64),
                  "corners": torch.zeros((B, 24), **f64), "heading": torch.zeros((B,), **f64), "size": torch.zeros((B, 3), **f64),
                  "coin": torch.zeros((B,), **f64), "normal": torch.zeros((B,), **f64)}
        self.out = builder.alloc(B, lpad, True)
        self.out["size_class"] = torch.zeros((B, 1), **i64)
        if builder.one_hot:
            self.out["one_hot"] = torch.zeros((B, len(builder.classes)), dtype=torch.float32, device=dev)
        if not self.pick:                                       # the first D detections, gathered once
            self._gather_candidates()

    @staticmethod
    def limits():
        """(the largest D * A, the largest D * A * S) of the plan."""
        return resident.limits("fcn_refine_train_plan_limits", 2)

    def _gather_candidates(self):
        idx = self.cand_row.view(-1)
        torch.index_select(self.det_frame, 0, idx, out=self.cand_frame)
        torch.index_select(self.det_class, 0, idx, out=self.cand_class[:self.D])

    def step(self):
        """Enqueues one batch on the current stream -- pick, gather, match, jitter draw, count, plan, fill, gather, draw,
        fcn_prepare_inputs_refine -- and nothing else: no allocation, no host read, no upload (capturable).  Returns the batch dict
        of RefineInputBuilder.build(), same keys and dtypes, at batch size B and window counts lpad; the same tensors every step.
        Kept for inspection: cand_row (1,D) the detections tried, gt_idx / best_iou (D) their match, jitter (D,A,7) the step's
        uniforms, pred_box3d / pred_angle / pred_size (U+1 rows) the jittered enlarged boxes, slot_unit (B) the unit of each slot
        (U: empty), n_kept (1) the filled slots; check() reads the status words."""
        L, dev, bld = _native.lib(), self.device, self.builder
        B, D, A, U, S, t = self.B, self.D, self.A, self.U, self.S, self.t
        p = lambda x: None if x is None else x.data_ptr()
        pts, foff = self.frames
        with torch.cuda.device(dev):
            s = _native.current_stream(dev)
            if self.sampler is not None:
                self.sampler.pick(self.r_count, D, out=self.cand_row)
                self._gather_candidates()
            elif self.pick:
                self.draws_pick.draw(self.r_count, D, False, False, out=(self.cand_row,) + self.pick_scalars)
                self._gather_candidates()
            if self.sampler is not None or not self.pick:       # (the three step counters stay equal)
                _native.check(L.fcn_box3d_jitter_draw(0, 1, self.draws_pick.seed, p(self.draws_pick.state), 1, p(self.pick_scalars[0]), s),
                              "fcn_box3d_jitter_draw")
            crow = self.cand_row.view(-1)
            _native.check(L.fcn_refine_train_match(p(self.dets), self.R, p(crow), p(self.cand_frame), D, p(self.gt), self.G,
                                                   p(self.gt_off), self.F, self.thresh, p(self.gt_idx), p(self.best_iou), s),
                          "fcn_refine_train_match")
            _native.check(L.fcn_box3d_jitter_draw(D if self.draw_jitter else 0, A, self.draws_jitter.seed, p(self.draws_jitter.state), 1,
                                                  p(self.jitter if self.draw_jitter else self.pick_scalars[0]), s),
                          "fcn_box3d_jitter_draw")
            args = (p(pts), p(foff), self.F, self.ps, p(self.dets), self.R, p(crow), p(self.cand_frame), D, self.ratio, p(self.gt_idx),
                    p(self.gt), self.G, A, p(self.jitter), self.shift_ratio, S)
            _native.check(L.fcn_refine_train_count(*args, p(self.both[0]), p(self.both[1]), p(self.pred_box3d), p(self.pred_angle),
                                                   p(self.pred_size), p(self.box3d), p(self.heading), p(self.size), s),
                          "fcn_refine_train_count")
            _native.check(L.fcn_refine_train_plan(p(self.both[0]), p(self.both[1]), p(self.pred_size), self.strides_c, self.lpad_c, U, S,
                                                  B, self.capacity, p(self.slot_unit), p(self.n_kept), p(self.seg_off), p(self.off),
                                                  p(self.counts), p(self.status), s), "fcn_refine_train_plan")
            _native.check(L.fcn_refine_train_fill(*args, p(self.seg_off), p(self.points), s), "fcn_refine_train_fill")
            for src, dst in ((self.pred_box3d, t["pcorners"]), (self.pred_angle, t["pangle"]), (self.pred_size, t["psize"]),
                             (self.box3d, t["corners"]), (self.heading, t["heading"]), (self.size, t["size"])):
                torch.index_select(src, 0, self.slot_unit, out=dst)
            torch.index_select(self.unit_cand, 0, self.slot_unit, out=self.slot_cand)
            torch.index_select(self.cand_class, 0, self.slot_cand, out=self.out["size_class"])
            if "one_hot" in self.out:
                torch.index_select(self.eye, 0, self.out["size_class"].view(-1), out=self.out["one_hot"])
            self.draws_sample.draw(self.counts, bld.npoints, bld.random_flip, bld.random_shift,
                                   out=(t["choice"], t["coin"], t["normal"]))
            return bld.launch(t, self.out, self.ps, self.lpad, True)

    def check(self):
        """Reads the status words of the plan and the three generators (a synchronisation: not for a captured region); raises
        ValueError naming the bits set since the last check() and clears them."""
        check_status("RefineTrainSource", (self.status, self.draws_pick.status, self.draws_jitter.status, self.draws_sample.status),
                     STATUS_BITS, self.sampler)


# ------------------------------------------------------------------------------------------------
# Two-stage inference as ONE capturable sequence of launches (csrc/cascade_plan.h)
class CascadeLink:
    """A first-stage batch -> second-stage detections at a FIXED number of candidates D, a FIXED second-stage batch size B and
    FIXED window counts lpad, with no host read, no upload and no validation per step: what TwoStageDetector.detect does behind its
    five synchronisations, as one sequence of launches that can be captured into a hipGraph and replayed on new first-stage batches
    written into the same tensors (INTEGRATION.md "Capturable two-stage inference" states the contract).
    stage1, stage2: two PointNetDet models in eval mode; refine_builder: the second stage's RefineInputBuilder; frame_points: a
    contiguous (n, >= 3) float32 device tensor, HELD, not copied -- a caller may overwrite it in place between replays -- and
    frame_off (F+1) as refine_candidates takes it (copied to the device as .frame_off; S, the segments of the longest frame, is
    fixed here: frames written later must not be longer than S * fcn_frustum_select_seg() rows); B1 / L2: frustums and windows of
    the first-stage batch step() takes; G: the (frame, class) groups of the first stage; top_k, method, thresh: as PointNetDet.detect,
    for both stages; D: candidates per step (kept rows beyond D are dropped and flagged); B: slots of the second-stage batch (B <= D;
    survivors beyond B are dropped and flagged); capacity: rows of the point buffer (rows beyond it are dropped and flagged); lpad:
    four ints, the padded window counts of center_ref1..4 (a candidate whose predicted width needs more is dropped and flagged);
    seed: keys the DeviceDraws of the per-sample resample, one step further after every step().
    unit_frame, unit_class (index into refine_builder.classes), unit_group (B1) int32 device tensors describe the frustums of the
    first-stage batch: zeros at first -- fill them with set_units() or overwrite them in place between replays.
    Everything is validated here, once, on the host; step() validates nothing and reads nothing."""

    def __init__(self, stage1, stage2, refine_builder, frame_points, frame_off, B1, L2, G, top_k, D, B, capacity, lpad, seed, method,
                 thresh, ratio=1.2):
        who = "CascadeLink"
        resident.held(who, frame_points)
        pts, foff, F, ps, S = _frames(who, frame_points, frame_off, resident=True)
        dev = frame_points.device
        if stage1.training or stage2.training:
            raise ValueError("%s: both models must be in eval mode" % who)
        builder = refine_builder
        resident.need_device_builder(builder)
        B1, L2, G, top_k, D, B, capacity = (int(x) for x in (B1, L2, G, top_k, D, B, capacity))
        max_u, max_segs = RefineTrainSource.limits()
        if B1 < 1 or L2 < 1 or G < 1 or G > 65536:
            raise ValueError("%s: need B1 >= 1, L2 >= 1 and 1 <= G <= 65536, got B1 = %d, L2 = %d, G = %d" % (who, B1, L2, G))
        if not (1 <= top_k <= 4096):
            raise ValueError("%s: top_k must lie in [1, 4096] (the NMS sorts at most 4096 rows of a group), got %d" % (who, top_k))
        resident.check_slots(who, B, D, max_u)
        resident.check_segments(who, D, S, max_segs)
        resident.check_capacity(who, capacity)
        lpad = [int(x) for x in lpad]
        if len(lpad) != 4 or min(lpad) < 1:
            raise ValueError("%s: lpad must be four window counts >= 1, got %r" % (who, lpad))
        if any(lpad[s + 1] != (lpad[s] + 1) // 2 for s in range(3)):       # (what RefineInputBuilder._lpad gives for any width)
            raise ValueError("%s: the second stage halves the windows level by level: lpad[s + 1] must be ceil(lpad[s] / 2), got %r" %
                             (who, lpad))
        if method not in ("nms", "top"):
            raise ValueError("%s: method must be 'nms' or 'top', got %r" % (who, method))
        if not (float(ratio) > 0.0) or not np.isfinite(float(thresh)):
            raise ValueError("%s: ratio must be positive and thresh finite, got %r, %r" % (who, ratio, thresh))
        self.device, self.stage1, self.stage2, self.builder, self.lpad = dev, stage1, stage2, builder, lpad
        self.B1, self.L2, self.G, self.top_k, self.D, self.B, self.F, self.S, self.ps = B1, L2, G, top_k, D, B, F, S, ps
        self.R, self.capacity, self.method, self.thresh, self.ratio = B1 * L2, capacity, method, float(thresh), float(ratio)
        f32, f64, i32 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.float64, torch.int32))
        N, C = builder.npoints, len(builder.classes)
        # ---- resident: the frames (held) and the frustums' tables
        self.frames, self.frame_off = (pts, foff), foff
        self.unit_frame, self.unit_class, self.unit_group = (torch.zeros((B1,), **i32) for _ in range(3))
        self.eye = torch.eye(C, **f32)
        self.strides_c = (ctypes.c_double * 4)(*builder.strides)
        self.lpad_c = (ctypes.c_int32 * 4)(*lpad)
        self.draws = DeviceDraws(int(seed), builder.device)
        # ---- the batch and every intermediate.  The per-candidate tables have D + 1 rows: row D is the spare entry an empty slot gathers -- no
        # first-stage row, class 0, the spare group G, score 0, a unit box at the origin -- written here once and never by a kernel
        self.points, self.seg_off, self.off, self.counts, self.slot_unit, self.n_kept, self.status = \
            resident.batch_skeleton(dev, B, D, S, capacity, ps, D)
        self.cand_row, self.cand_frame = torch.full((D + 1,), -1, **i32), torch.full((D + 1,), -1, **i32)
        self.cand_class, self.cand_group = torch.zeros((D + 1,), **i32), torch.full((D + 1,), G, **i32)
        self.cand_score, self.n_cand = torch.zeros((D + 1, 1), **f32), torch.zeros((1,), **i32)
        self.seg_cnt = torch.zeros((D, S), **i32)
        self.pred_box3d, self.pred_angle, self.pred_size = torch.zeros((D + 1, 24), **f64), torch.zeros((D + 1,), **f64), torch.zeros((D + 1, 3), **f64)
        self.pred_box3d[D] = resident.spare_corners(dev)
        self.pred_size[D] = 1.0
        self.slot_class, self.slot_group, self.stage1_row = torch.zeros((B,), **i32), torch.full((B,), G, **i32), torch.full((B,), -1, **i32)
        self.t = {"raw": self.points, "off": self.off, "choice": torch.zeros((B, N), **i32),
                  "pcorners": torch.zeros((B, 24), **f64), "pangle": torch.zeros((B,), **f64), "psize": torch.zeros((B, 3), **f64),
                  "coin": torch.zeros((B,), **f64), "normal": torch.zeros((B,), **f64)}
        self.out = builder.alloc(B, lpad, False)
        if builder.one_hot:
            self.out["one_hot"] = torch.zeros((B, C), **f32)
        self.out["rgb_prob"] = torch.zeros((B, 1), **f32)
        self.batch = {k: v for k, v in self.out.items() if k != "lens"}      # what stage2.detect takes (as detect() passes it)
        self.res = {"dets": torch.zeros((B * lpad[1], 8), **f32), "valid": torch.zeros((B * lpad[1],), **i32),
                    "keep": torch.full((G, top_k), -1, **i32), "cnt": torch.zeros((G,), **i32)}

    def set_units(self, frustum_frame, types, unit_group=None):
        """Fills unit_frame / unit_class / unit_group in place from host sequences of length B1 (validated here: frames in [0, F),
        class names of refine_builder.classes, groups in [0, G); unit_group None: every frustum its own group, which needs
        G >= B1).  An upload: not for a captured region."""
        who = "CascadeLink.set_units"
        fr = np.asarray(torch.as_tensor(frustum_frame).cpu().numpy()).reshape(-1)
        ug = np.arange(self.B1) if unit_group is None else np.asarray(torch.as_tensor(unit_group).cpu().numpy()).reshape(-1)
        types = [str(t) for t in types]
        if len(fr) != self.B1 or len(ug) != self.B1 or len(types) != self.B1:
            raise ValueError("%s: %d frustums, got %d frames, %d types, %d groups" % (who, self.B1, len(fr), len(types), len(ug)))
        resident.check_rows(who, fr, self.F, ug, self.G)
        cls = resident.class_index(who, self.builder.classes, types)
        for dst, src in ((self.unit_frame, fr), (self.unit_class, cls), (self.unit_group, ug)):
            dst.copy_(resident.up(np.asarray(src, dtype=np.int32)))
        return self

    def step(self, data_dicts):
        """Enqueues on the current stream stage1.detect, candidates, count, plan, fill, the gathers through slot_unit, the draw,
        fcn_prepare_inputs_refine and stage2.detect with the slots' groups and the spare group G -- and nothing else: no host read,
        no upload (capturable).  data_dicts: the first-stage batch of B1 frustums at L2 windows on the second stride.
        Returns a dict, the same tensors of the link every step: dets (B * lpad[1], 8), valid, keep (G, top_k), cnt (G) of the
        second stage (an empty slot's rows belong to the spare group: no keep entry points at them), stage1_row (B) int32 the
        first-stage row each slot refines (-1: empty), n_kept (1) the filled slots; for inspection batch (the second stage's
        input), slot_unit (B) the candidate of each slot (D: empty), cand_row (D+1) / n_cand (1) the candidate table, and stage1 =
        the first stage's (dets, valid, keep, cnt) of this call.  check() reads the status words."""
        L, dev, bld = _native.lib(), self.device, self.builder
        G, D, B, S, t = self.G, self.D, self.B, self.S, self.t
        p = lambda x: None if x is None else x.data_ptr()
        pts, foff = self.frames
        s1 = self.stage1.detect(data_dicts, unit_group=self.unit_group, num_groups=G, method=self.method, thresh=self.thresh,
                                top_k=self.top_k)
        dets1, _, keep1, cnt1 = s1
        if tuple(dets1.shape) != (self.R, 8) or tuple(keep1.shape) != (G, self.top_k):      # (attributes: nothing is read)
            raise ValueError("CascadeLink.step: the first-stage batch must hold %d frustums of %d windows" % (self.B1, self.L2))
        with torch.cuda.device(dev):
            s = _native.current_stream(dev)
            _native.check(L.fcn_cascade_candidates(p(keep1), p(cnt1), G, self.top_k, self.L2, p(self.unit_frame), p(self.unit_class),
                                                   p(self.unit_group), self.B1, p(dets1), self.R, D, p(self.cand_row), p(self.cand_frame),
                                                   p(self.cand_class), p(self.cand_group), p(self.cand_score), p(self.n_cand),
                                                   p(self.status), s), "fcn_cascade_candidates")
            args = (p(pts), p(foff), self.F, self.ps, p(dets1), self.R, p(self.cand_row), p(self.cand_frame), D, self.ratio, S)
            _native.check(L.fcn_refine_detect_count(*args, p(self.seg_cnt), p(self.pred_box3d), p(self.pred_angle), p(self.pred_size), s),
                          "fcn_refine_detect_count")
            _native.check(L.fcn_refine_detect_plan(p(self.seg_cnt), p(self.pred_size), self.strides_c, self.lpad_c, D, S, B, self.capacity,
                                                   p(self.slot_unit), p(self.n_kept), p(self.seg_off), p(self.off), p(self.counts),
                                                   p(self.status), s), "fcn_refine_detect_plan")
            _native.check(L.fcn_refine_detect_fill(*args, p(self.seg_off), p(self.points), s), "fcn_refine_detect_fill")
            for src, dst in ((self.pred_box3d, t["pcorners"]), (self.pred_angle, t["pangle"]), (self.pred_size, t["psize"]),
                             (self.cand_class, self.slot_class), (self.cand_score, self.out["rgb_prob"]),
                             (self.cand_group, self.slot_group), (self.cand_row, self.stage1_row)):
                torch.index_select(src, 0, self.slot_unit, out=dst)
            if "one_hot" in self.out:
                torch.index_select(self.eye, 0, self.slot_class, out=self.out["one_hot"])
            self.draws.draw(self.counts, bld.npoints, False, False, out=(t["choice"], t["coin"], t["normal"]))
            bld.launch(t, self.out, self.ps, self.lpad, False)
        d2, v2, k2, c2 = self.stage2.detect(self.batch, unit_group=self.slot_group, num_groups=G + 1, method=self.method,
                                            thresh=self.thresh, top_k=self.top_k)
        res = self.res
        res["dets"].copy_(d2); res["valid"].copy_(v2); res["keep"].copy_(k2[:G]); res["cnt"].copy_(c2[:G])
        return {"dets": res["dets"], "valid": res["valid"], "keep": res["keep"], "cnt": res["cnt"], "stage1_row": self.stage1_row,
                "n_kept": self.n_kept, "stage1": s1, "batch": self.batch, "slot_unit": self.slot_unit, "cand_row": self.cand_row,
                "n_cand": self.n_cand}

    def check(self):
        """Reads the status words of the link and of its draws (a synchronisation: not for a captured region); raises ValueError
        naming the bits set since the last check() and clears them.  Bit 0 is the draws' own: an EMPTY slot has no row to draw
        from either, so it is set by every step with fewer survivors than slots."""
        check_status("CascadeLink", (self.status, self.draws.status), STATUS_BITS)


class FrameCascade:
    """Resident velodyne frames and a resident table of 2-D detections -> second-stage detections with no host read, no upload and no
    validation per step: what TwoStageDetector.detect_frames does, as ONE sequence of launches that can be captured into a hipGraph
    and replayed on boxes and points overwritten in place (INTEGRATION.md "Capturable inference front" states the contract).  A
    frustum.FrameDetectSource(fov=True) wired to a CascadeLink:
      * the link searches source.fov_points, built on the VELODYNE frame_off as the worst case -- a frame's image-FOV subset is no
        longer than the frame, so the link's S and its row check hold for every later step;
      * the source writes the frames' FOV offsets into link.frame_off (the link holds ONE offsets tensor: link.frames[1] is the same
        object) and the slots' frame, class and group into link.unit_frame / unit_class / unit_group;
      * spare_group = G: the first stage runs its NMS over groups 0..G-1 and a group only takes units of its own number, so an empty
        first-stage slot never reaches a keep list, hence never the candidate table.
    stage1, stage2, refine_builder, G, top_k, D, B, capacity, lpad, method, thresh, ratio: as CascadeLink takes them; input_builder,
    frame_points, frame_off, calib, img_size, B1, D1 (rows of the detection table), capacity1 (rows of the first stage's point buffer),
    clip_distance, clip_boxes, img_height_threshold, lidar_point_threshold: as FrameDetectSource takes them; seed keys the source's
    draws, seed + 1 the link's.  .source and .link are the two parts; fill the table with source.set_boxes() or in place."""

    def __init__(self, stage1, stage2, input_builder, refine_builder, frame_points, frame_off, calib, img_size, B1, D1, capacity1, G,
                 top_k, D, B, capacity, lpad, seed, method, thresh, ratio=1.2, clip_distance=2.0, clip_boxes=True,
                 img_height_threshold=5, lidar_point_threshold=1):
        if tuple(input_builder.classes) != tuple(refine_builder.classes):
            raise ValueError("FrameCascade: the two builders must share their classes, got %r and %r" %
                             (tuple(input_builder.classes), tuple(refine_builder.classes)))
        self.source = FrameDetectSource(frame_points, frame_off, calib, img_size, input_builder, B1, D1, capacity1, seed, int(G),
                                        clip_distance, clip_boxes, img_height_threshold, lidar_point_threshold, fov=True)
        src = self.source
        self.link = CascadeLink(stage1, stage2, refine_builder, src.fov_points, src.frames[1].cpu().clone(), B1, input_builder.L[1], G, top_k, D,
                                B, capacity, lpad, int(seed) + 1, method, thresh, ratio)
        lk = self.link
        src.bind(fov_off=lk.frame_off, slot_frame=lk.unit_frame, slot_class=lk.unit_class, slot_group=lk.unit_group)
        self.keys = ("point_cloud", "rot_angle", "rgb_prob", "one_hot", "center_ref1", "center_ref2", "center_ref3", "center_ref4")

    def step(self):
        """source.step() followed by link.step() on its batch, on the current stream (capturable).  Returns the link's dict plus
        slot_box (B1) the box of each first-stage slot (D1: empty), n_kept1 (1) the filled first-stage slots and batch1, the first
        stage's input; the same tensors every step."""
        got = self.source.step()
        batch = {k: got[k] for k in self.keys if k in got}
        res = self.link.step(batch)
        res.update(slot_box=got["slot_box"], n_kept1=got["n_kept"], batch1=batch)
        return res

    def check(self):
        """check() of both parts in one: reads their status words (a synchronisation), raises ValueError naming the bits set since
        the last check() and clears them."""
        check_status("FrameCascade", (self.source.status, self.source.draws.status, self.link.status, self.link.draws.status),
                     STATUS_BITS)


class TwoStageDetector:
    """stage1, stage2: two PointNetDet models in eval mode, each built by the caller under its own configuration (cfg is
    global: build one, then the other); refine_builder: the RefineInputBuilder of the second stage's configuration;
    input_builder: the InputBuilder of the first stage's configuration (detect_frames alone needs it)."""

    def __init__(self, stage1, stage2, refine_builder, input_builder=None):
        self.stage1, self.stage2, self.refine_builder, self.input_builder = stage1, stage2, refine_builder, input_builder

    def link(self, frame_points, frame_off, frustum_frame, types, B1, L2, D, B, capacity, lpad, seed, method, thresh, unit_group=None,
             num_groups=None, top_k=300, ratio=1.2):
        """detect() as one capturable sequence of launches at fixed sizes: a CascadeLink over this detector's two stages and
        refine builder, its frustum tables filled from frustum_frame (B1) / types (B1) / unit_group (B1; default: every frustum its
        own group) as detect() takes them.  link(...).step(data_dicts) then stands where detect(data_dicts, ...) stood."""
        if num_groups is None:
            num_groups = int(B1) if unit_group is None else int(torch.as_tensor(unit_group).max()) + 1
        lk = CascadeLink(self.stage1, self.stage2, self.refine_builder, frame_points, frame_off, B1, L2, num_groups, top_k, D, B,
                         capacity, lpad, seed, method, thresh, ratio)
        return lk.set_units(frustum_frame, types, unit_group)

    def frame_link(self, frame_points_velo, frame_off, calib, img_size, B1, D1, capacity1, num_groups, D, B, capacity, lpad, seed,
                   method, thresh, top_k=300, ratio=1.2, clip_distance=2.0, clip_boxes=True, img_height_threshold=5,
                   lidar_point_threshold=1):
        """detect_frames() as one capturable sequence of launches at fixed sizes: a FrameCascade over this detector's two stages and
        builders -- the arguments of link() and of frustum.FrameDetectSource together; the boxes, their frames, types, scores and
        groups go into the returned cascade's detection table (.source.set_boxes(...), or in place).  frame_link(...).step() then
        stands where detect_frames(...) stood."""
        if self.input_builder is None:
            raise ValueError("TwoStageDetector.frame_link needs the first stage's InputBuilder (input_builder=...)")
        return FrameCascade(self.stage1, self.stage2, self.input_builder, self.refine_builder, frame_points_velo, frame_off, calib,
                            img_size, B1, D1, capacity1, num_groups, top_k, D, B, capacity, lpad, seed, method, thresh, ratio,
                            clip_distance, clip_boxes, img_height_threshold, lidar_point_threshold)

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
