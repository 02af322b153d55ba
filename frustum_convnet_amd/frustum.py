"""Frustum extraction on the device: LiDAR frames in velodyne coordinates + calibration + 2-D detection boxes -> the first
stage's raw frustum points and the refine stage's search set (C-ABI fcn_frustum_select_count / _fill, csrc/frustum_select.h), and,
with a ground-truth 3-D box beside each 2-D box, the first stage's training records: points, per-point labels, corners
(fcn_frustum_label_count / _fill, csrc/frustum_label.h; kitti/prepare_data.py::extract_frustum_data :260-391 in the reference).
The SUN-RGBD configuration has the same two paths from upright-depth frames, K and Rtilt (sunrgbd_candidates,
sunrgbd_training_candidates; fcn_frustum_sunrgbd_count / _fill / _label_count / _label_fill, csrc/frustum_sunrgbd.h;
sunrgbd/prepare_data.py::extract_frustum_data :132-267 and extract_frustum_data_from_rgb_detection :270-381 in the reference).

Reference: kitti/prepare_data.py::extract_frustum_data_rgb_detection (:462-568) projects the whole frame to the image once per
frame in numpy (kitti_util.Calibration.project_velo_to_rect / project_rect_to_image, draw_util.get_lidar_in_image_fov) and masks
it once per detection on the host, pickling D ragged copies of the same frame for datasets/provider_sample.py;
kitti/prepare_data_refine.py:689-699 builds the rect-camera, image-FOV subset the refinement stage searches.  Here both are the
same two HIP launches over a grid of (segments, boxes); the host reads the D * S segment counts between them (they size the
point buffer) and each entry point reads box_frame and frame_off back to range-check them.  No point data crosses to the host.
FrameTrainSource (at the end) is the KITTI training path again with NOTHING read back: frames and labels resident, boxes perturbed
on the device, a one-workgroup plan in place of the host's kept list and prefix sum, a fixed batch size -- capturable
(fcn_box2d_perturb, fcn_frustum_train_count / _plan / _fill, csrc/frustum_plan.h).  SunrgbdTrainSource is the same for the SUN-RGBD
training path, with the frustum subsamples drawn on the device as well (csrc/frustum_sunrgbd_plan.h).  FrameDetectSource is the
KITTI INFERENCE path the same way: resident frames and a resident table of 2-D detections -> the first-stage batch at a fixed number
of slots and, when asked, the image-FOV search set of the second stage (fcn_frustum_detect_count / _plan / _fill,
fcn_frustum_fov_plan, csrc/frustum_detect_plan.h).  SunrgbdDetectSource is the SUN-RGBD inference path the same way, the frustum
subsamples drawn on the device and every (frame, class) NMS group numbered by the plan (fcn_frustum_sunrgbd_detect_count / _plan /
_fill, csrc/frustum_sunrgbd_detect_plan.h); evaluate.SunrgbdFrameChain carries it on to corners and scores.
What the four sources do once on the host -- refusals, the label and detection tables, the batch skeleton -- is resident.py's, shared
with cascade.py's two; a source states its own calibration, options, intermediates and step().  No CPU fallback.
"""
import ctypes

import numpy as np
import torch

from . import _native, resident
from .detect import _need_cuda
from .inputs import DeviceDraws
from .resident import DetectTable, LabelTable


def _calib(calib, img_size, F, dev):
    out = []
    for key, shape in (("P", (F, 12)), ("V2C", (F, 12)), ("R0", (F, 9))):
        t = torch.as_tensor(calib[key]).to(device=dev, dtype=torch.float64).contiguous()
        if t.numel() != shape[0] * shape[1]:
            raise ValueError("frustum: calib[%r] must hold %d x %d numbers, got %s" % (key, F, shape[1], tuple(t.shape)))
        out.append(t.view(shape))
    wh = torch.as_tensor(img_size).to(device=dev, dtype=torch.float64).contiguous()
    if wh.numel() != 2 * F:
        raise ValueError("frustum: img_size must be (%d, 2) as width, height, got %s" % (F, tuple(wh.shape)))
    return out + [wh.view(F, 2)]


def _frames(who, frame_points, frame_off, resident=False):
    """What every entry point of the input side takes its frames as: the points as contiguous float32 (n, >= 3) on the device (one
    placeholder row when the buffer is empty), frame_off on the device as int64, and F, ps, S -- S the longest frame in segments
    of fcn_frustum_select_seg() rows, from the F + 1 offsets on the host.  resident (the *TrainSource classes, which check the
    frames HERE, once, and launch without a read-back): refuse offsets that are not ascending within the buffer."""
    _need_cuda(frame_points, who)
    dev = frame_points.device
    pts = frame_points.detach().contiguous().float()
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("%s: frame_points must be (n, >= 3), got %s" % (who, tuple(frame_points.shape)))
    foff_h = torch.as_tensor(frame_off).detach().cpu().to(torch.int64).contiguous().view(-1)      # F + 1 integers: they decide S
    F, ps = int(foff_h.numel()) - 1, int(pts.shape[1])
    lengths = foff_h[1:] - foff_h[:-1]
    if resident and (F < 1 or int(foff_h[0]) < 0 or bool((lengths < 0).any()) or int(foff_h[-1]) > pts.shape[0]):
        raise ValueError("%s: frame_off must be F + 1 >= 2 ascending row offsets into the %d rows" % (who, pts.shape[0]))
    foff = foff_h.to(dev, non_blocking=True)
    seg = int(_native.lib().fcn_frustum_select_seg())
    S = max(1, -(-(int(lengths.max()) if F > 0 else 0) // seg))
    if pts.shape[0] == 0:
        pts = torch.zeros((1, ps), dtype=torch.float32, device=dev)        # (an address to hand in: every frame is empty)
    return pts, foff, F, ps, S


def _boxes(who, boxes2d, box_frame, dev):
    """The D 2-D boxes of a reading entry point and the frame of each, on the device: (D,4) fp64, (D) int32, D."""
    boxes = torch.as_tensor(boxes2d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 4)
    bframe = torch.as_tensor(box_frame).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    D = int(bframe.numel())
    if boxes.shape[0] != D:
        raise ValueError("%s: %d boxes but %d frames" % (who, boxes.shape[0], D))
    return boxes, bframe, D


def _packed(seg_counts, ps, dev):
    """Between the count and the fill of a reading entry point: from the (boxes, S) segment counts the host has just read, their
    exclusive prefix sum on the device (one entry more: the total) and the point buffer it sizes."""
    seg_off = np.concatenate([[0], np.cumsum(seg_counts.reshape(-1))]).astype(np.int64)
    soff = torch.from_numpy(seg_off).to(dev, non_blocking=True)
    return soff, torch.empty((int(seg_off[-1]), ps), dtype=torch.float32, device=dev)


def _setup(who, frame_points, frame_off, calib, img_size, boxes2d, box_frame, clip_distance, clip_boxes):
    """The arguments both pairs of entry points share (fs_in of _native.py) from the Python-level inputs, the tensors that back
    them, and F, ps, D, S."""
    pts, foff, F, ps, S = _frames(who, frame_points, frame_off)
    dev = frame_points.device
    P, V2C, R0, wh = _calib(calib, img_size, F, dev)
    boxes, bframe, D = _boxes(who, boxes2d, box_frame, dev)
    args = (pts.data_ptr(), foff.data_ptr(), F, ps, P.data_ptr(), V2C.data_ptr(), R0.data_ptr(), wh.data_ptr(), boxes.data_ptr(),
            bframe.data_ptr(), D, S, 1 if clip_boxes else 0, float(clip_distance))
    return args, (pts, foff, P, V2C, R0, wh, boxes, bframe), ps, D, S


def frustum_candidates(frame_points, frame_off, calib, img_size, boxes2d, box_frame, clip_distance=2.0, clip_boxes=True):
    """frame_points (sum m_f, stride >= 3) float32 VELODYNE x, y, z (+ intensity, ...) of F frames packed behind each other,
    frame_off (F+1) int64 row offsets, calib {"P": (F,3,4), "V2C": (F,3,4), "R0": (F,3,3)} float64, img_size (F,2) as width,
    height, boxes2d (D,4) xmin ymin xmax ymax, box_frame (D) the frame of each box -- device tensors (everything but the points
    may be host arrays).  clip_boxes: clip every box to the image first, as the reference does.
    Returns a dict: points (sum cnt, stride) -- per box, in frame order, the frame's rows that project into it, as float32 rect
    camera x, y, z followed by the untouched columns; off (D+1) int64; box2d (D,4) fp64 the box actually used; frustum_angle
    (D) fp64; cnt (D) int32; box_frame (D) int32 -- on the device -- and counts (D) int64 on the host.  The host reads the D * S
    segment counts once, between the two launches (S = the longest frame in segments of fcn_frustum_select_seg() rows)."""
    args, held, ps, D, S = _setup("frustum_candidates", frame_points, frame_off, calib, img_size, boxes2d, box_frame,
                                  clip_distance, clip_boxes)
    dev = frame_points.device
    L = _native.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"box2d": torch.zeros((D, 4), **f64), "frustum_angle": torch.zeros((D,), **f64), "box_frame": held[-1]}
    scnt = torch.zeros((D, S), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.check(L.fcn_frustum_select_count(*args, out["box2d"].data_ptr(), out["frustum_angle"].data_ptr(),
                                                 scnt.data_ptr(), _native.current_stream(dev)), "fcn_frustum_select_count")
        seg_counts = scnt.cpu().numpy().astype(np.int64)                    # D * S integers: the size of `points`
        soff, out["points"] = _packed(seg_counts, ps, dev)
        if out["points"].shape[0] > 0:
            _native.check(L.fcn_frustum_select_fill(*args, soff.data_ptr(), out["points"].data_ptr(),
                                                    _native.current_stream(dev)), "fcn_frustum_select_fill")
    out["off"] = soff[::S].contiguous()                                     # every S-th entry is a box's offset
    out["cnt"] = scnt.sum(1, dtype=torch.int32)
    out["counts"] = seg_counts.sum(1)
    return out


def image_fov_points(frame_points, frame_off, calib, img_size, clip_distance=2.0):
    """The rect-camera, image-FOV subset of every frame (kitti/prepare_data_refine.py:689-699): the frame_points / frame_off
    pair cascade.refine_candidates searches.  The same selection as frustum_candidates with one box (0, 0, W, H) per frame and
    no clipping.  Returns (points (sum cnt, stride) float32, off (F+1) int64) on the device."""
    wh = torch.as_tensor(img_size).detach().cpu().to(torch.float64).reshape(-1, 2)
    F = int(wh.shape[0])
    boxes = torch.cat([torch.zeros((F, 2), dtype=torch.float64), wh], 1)
    sel = frustum_candidates(frame_points, frame_off, calib, wh, boxes, np.arange(F, dtype=np.int32), clip_distance, False)
    return sel["points"], sel["off"]


def perturb_boxes2d(boxes2d, img_wh, shift_ratio=0.1, rng=np.random):
    """kitti/prepare_data.py::random_shift_box2d (:55-77) for D boxes in order: the centre moves by up to shift_ratio of the width
    / height, both scale by 1 +- shift_ratio, then x is clipped to [0, W-1] and y to [0, H-1]; an attempt whose clipped box is
    degenerate is drawn again.  Four rng.random() draws per attempt, in the reference's order, so with the same seed the boxes
    equal the reference's bit for bit and the generator is left in the reference's state.  boxes2d (D,4) xmin ymin xmax ymax;
    img_wh (2,) or (D,2) as width, height.  augmentX perturbed copies of a box: repeat its row.  Returns (D,4) float64 (host).
    ValueError: a box with xmin >= xmax or ymin >= ymax (the reference asserts), and a box that no draw can make valid (it lies
    beyond the image: the reference would loop for ever)."""
    boxes = np.asarray(boxes2d, dtype=np.float64).reshape(-1, 4)
    wh = np.broadcast_to(np.asarray(img_wh, dtype=np.float64).reshape(-1, 2), (len(boxes), 2))
    r = shift_ratio
    out = np.empty_like(boxes)
    for d, (xmin, ymin, xmax, ymax) in enumerate(boxes.tolist()):
        if not (xmin < xmax and ymin < ymax):
            raise ValueError("perturb_boxes2d: box %d is degenerate: %r" % (d, (xmin, ymin, xmax, ymax)))
        W, H = float(wh[d, 0]), float(wh[d, 1])
        h, w = ymax - ymin, xmax - xmin
        cx, cy = (xmin + xmax) / 2.0, (ymin + ymax) / 2.0
        # the furthest any draw reaches: centre shift w * r plus half the largest width w * (1 + r) / 2
        rx, ry = w * r + w * (1 + r) / 2.0, h * r + h * (1 + r) / 2.0
        if not (cx - rx < W - 1 and cx + rx > 0 and cy - ry < H - 1 and cy + ry > 0):
            raise ValueError("perturb_boxes2d: box %d cannot be perturbed into the %g x %g image: %r" % (d, W, H, (xmin, ymin, xmax, ymax)))
        for _ in range(100000):
            cx2 = cx + w * r * (rng.random() * 2 - 1)
            cy2 = cy + h * r * (rng.random() * 2 - 1)
            h2 = h * (1 + rng.random() * 2 * r - r)
            w2 = w * (1 + rng.random() * 2 * r - r)
            new = np.array([cx2 - w2 / 2.0, cy2 - h2 / 2.0, cx2 + w2 / 2.0, cy2 + h2 / 2.0])
            new[[0, 2]] = np.clip(new[[0, 2]], 0, W - 1)
            new[[1, 3]] = np.clip(new[[1, 3]], 0, H - 1)
            if new[0] < new[2] and new[1] < new[3]:
                break
        else:
            raise ValueError("perturb_boxes2d: no valid draw for box %d in 100000 attempts: %r" % (d, (xmin, ymin, xmax, ymax)))
        out[d] = new
    return out


def frustum_training_candidates(frame_points, frame_off, calib, img_size, boxes2d, box_frame, gt_box3d, gt_box2d=None,
                                min_box_height=25.0, clip_distance=2.0):
    """The first stage's TRAINING records from LiDAR frames and label boxes, on the device: what
    kitti/prepare_data.py::extract_frustum_data (:260-391) pickles.  frame_points ... box_frame as frustum_candidates takes them;
    boxes2d (D,4): the boxes that select the points -- perturbed (perturb_boxes2d) or plain, used WITHOUT clipping as the
    reference does; gt_box3d (D,7): tx, ty, tz, l, w, h, ry of the label beside each box (rect camera coordinates, t the bottom
    centre); gt_box2d (D,4): the unperturbed label boxes the reject rule looks at (default: boxes2d).
    Box d is dropped when gt_box2d[d,3] - gt_box2d[d,1] < min_box_height or none of its points lies inside its 3-D box (:354);
    dropped boxes take no room in the packed buffers.
    Returns a dict over the K kept boxes: points (sum cnt, stride) float32 rect x, y, z + the untouched columns and seg (sum cnt)
    int64 (1 inside the 3-D box) ; off (K+1) int64; box2d (K,4), frustum_angle (K), box3d (K,8,3) corners, heading (K), size (K,3)
    fp64; box_frame (K), cnt (K), pos (K) int32 -- on the device -- and kept (K) int64 (the kept boxes' indices), counts (K) int64
    on the host.  With no survivor the dict holds 'kept' alone.
    The host reads the D * S selected and positive segment counts once, together, between the two launches; nothing else."""
    who = "frustum_training_candidates"
    args, held, ps, D, S = _setup(who, frame_points, frame_off, calib, img_size, boxes2d, box_frame, clip_distance, False)
    dev = frame_points.device
    bframe = held[-1]
    gt = torch.as_tensor(gt_box3d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 7)
    # the reject rule's boxes live on the host (label files are read there); boxes2d given as a device tensor costs a read of D boxes
    gt2d = boxes2d if gt_box2d is None else gt_box2d
    gt2d = (gt2d.detach().cpu().numpy() if isinstance(gt2d, torch.Tensor) else np.asarray(gt2d)).astype(np.float64).reshape(-1, 4)
    if gt.shape[0] != D or gt2d.shape[0] != D:
        raise ValueError("%s: %d boxes, %d gt_box3d, %d gt_box2d" % (who, D, gt.shape[0], gt2d.shape[0]))
    if D == 0:
        return {"kept": np.zeros(0, dtype=np.int64)}
    L = _native.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    box2d, angle, corners = torch.zeros((D, 4), **f64), torch.zeros((D,), **f64), torch.zeros((D, 8, 3), **f64)
    both = torch.zeros((2, D, S), dtype=torch.int32, device=dev)            # selected, positive: one read
    with torch.cuda.device(dev):
        _native.check(L.fcn_frustum_label_count(*args, gt.data_ptr(), box2d.data_ptr(), angle.data_ptr(), both[0].data_ptr(),
                                                both[1].data_ptr(), corners.data_ptr(), _native.current_stream(dev)),
                      "fcn_frustum_label_count")
        both_h = both.cpu().numpy().astype(np.int64)                        # 2 * D * S integers
        seg_counts, positives = both_h[0], both_h[1].sum(1)
        drop = (gt2d[:, 3] - gt2d[:, 1] < min_box_height) | (positives == 0)
        kept = np.nonzero(~drop)[0].astype(np.int64)
        if len(kept) == 0:
            return {"kept": kept}
        seg_counts[drop] = 0
        soff, points = _packed(seg_counts, ps, dev)
        seg = torch.empty((points.shape[0],), dtype=torch.int64, device=dev)
        _native.check(L.fcn_frustum_label_fill(*args, gt.data_ptr(), soff.data_ptr(), points.data_ptr(), seg.data_ptr(),
                                               _native.current_stream(dev)), "fcn_frustum_label_fill")
    idx = torch.from_numpy(kept).to(dev, non_blocking=True)
    pick = lambda x: x.index_select(0, idx).contiguous()
    # a dropped box has no rows, so a kept box ends where the next kept one starts
    off = torch.cat([soff[::S][:D].index_select(0, idx), soff[-1:]])
    return {"points": points, "seg": seg, "off": off, "box2d": pick(box2d), "frustum_angle": pick(angle), "box3d": pick(corners),
            "heading": pick(gt[:, 6]), "size": pick(gt[:, 3:6]), "box_frame": pick(bframe),
            "cnt": pick(both[0].sum(1, dtype=torch.int32)), "pos": pick(both[1].sum(1, dtype=torch.int32)),
            "kept": kept, "counts": seg_counts.sum(1)[kept]}


# ------------------------------------------------------------------------------------------------
# SUN-RGBD: upright-depth frames (xyz + rgb), per-frame K and Rtilt, 2-D boxes (csrc/frustum_sunrgbd.h)
SUNRGBD_CAP = 2048                     # sunrgbd/prepare_data.py:220, :346: a frustum of more rows is subsampled to this many
SUNRGBD_MIN = 5                        # :226 (positives, training), :352 (rows, detections)


def perturb_boxes2d_sunrgbd(boxes2d, shift_ratio=0.1, rng=np.random):
    """sunrgbd/sunrgbd_utils.py::random_shift_box2d (:208-221) for D boxes in order: the centre moves by up to shift_ratio of the
    width / height, both scale by 1 +- shift_ratio.  Four rng.random() draws per box in the reference's order, no clip, no retry:
    with the same seed the boxes equal the reference's bit for bit and the generator is left in the reference's state.  augmentX
    perturbed copies of a box: repeat its row.  Returns (D,4) float64 (host)."""
    boxes = np.asarray(boxes2d, dtype=np.float64).reshape(-1, 4)
    r = shift_ratio
    out = np.empty_like(boxes)
    for d, (xmin, ymin, xmax, ymax) in enumerate(boxes.tolist()):
        h, w = ymax - ymin, xmax - xmin
        cx, cy = (xmin + xmax) / 2.0, (ymin + ymax) / 2.0
        cx2 = cx + w * r * (rng.random() * 2 - 1)
        cy2 = cy + h * r * (rng.random() * 2 - 1)
        h2 = h * (1 + rng.random() * 2 * r - r)
        w2 = w * (1 + rng.random() * 2 * r - r)
        out[d] = [cx2 - w2 / 2.0, cy2 - h2 / 2.0, cx2 + w2 / 2.0, cy2 + h2 / 2.0]
    return out


def draw_frustum_subsample(counts, cap=SUNRGBD_CAP, rng=np.random):
    """The reference's subsample of a large frustum (sunrgbd/prepare_data.py:219-224, :345-349): per box, in order, one
    rng.choice(n, cap, replace=False) when the box selects n > cap rows, else None (no draw).  Returns a list of D entries."""
    return [rng.choice(int(n), cap, replace=False) if int(n) > cap else None for n in counts]


def _check_sub(who, sub, counts):
    """Host-made subsample indices are range-checked here, before any of them is uploaded."""
    if len(sub) != len(counts):
        raise ValueError("%s: %d subsamples for %d boxes" % (who, len(sub), len(counts)))
    out = []
    for d, (ix, n) in enumerate(zip(sub, counts)):
        if ix is None:
            out.append(None)
            continue
        ix = np.asarray(ix)
        if ix.ndim != 1 or ix.dtype.kind not in "iu" or len(ix) == 0:
            raise ValueError("%s: sub[%d] must be a non-empty 1-D integer array" % (who, d))
        if int(ix.min()) < 0 or int(ix.max()) >= int(n):
            raise ValueError("%s: sub[%d] indexes outside the box's %d rows" % (who, d, int(n)))
        out.append(ix.astype(np.int32))
    return out


def subsampled_counts(counts, sub):
    """Rows of each record: the length of its subsample where it has one, else its selected rows."""
    return np.asarray([int(n) if ix is None else len(ix) for n, ix in zip(counts, sub)], dtype=np.int64)


def _setup_sunrgbd(who, frame_points, frame_off, K, Rtilt, boxes2d, box_frame):
    """The arguments the four entry points share (sr_in of _native.py), the tensors that back them, and ps, D, S."""
    pts, foff, F, ps, S = _frames(who, frame_points, frame_off)
    dev = frame_points.device
    cal = resident.intrinsics(who, K, Rtilt, F, dev)
    boxes, bframe, D = _boxes(who, boxes2d, box_frame, dev)
    args = (pts.data_ptr(), foff.data_ptr(), F, ps, cal[0].data_ptr(), cal[1].data_ptr(), boxes.data_ptr(), bframe.data_ptr(), D, S)
    return args, (pts, foff, cal[0], cal[1], boxes, bframe), ps, D, S


def sunrgbd_candidates(frame_points, frame_off, K, Rtilt, boxes2d, box_frame, sub=None, cap=SUNRGBD_CAP, rng=np.random):
    """The SUN-RGBD inference side (extract_frustum_data_from_rgb_detection :270-381).  frame_points (sum m_f, stride >= 3)
    float32 UPRIGHT DEPTH x, y, z (+ r, g, b, ...) of F frames packed behind each other, frame_off (F+1) int64, K (F,3,3) and
    Rtilt (F,3,3) float64, boxes2d (D,4) xmin ymin xmax ymax -- used as given, the reference does not clip them -- and box_frame
    (D): device tensors (everything but the points may be host arrays).
    Returns a dict: points (sum cnt, stride) -- per box, in frame order, the frame's rows that project into it, as upright
    CAMERA (x, -z, y) followed by the untouched columns; off (D+1) int64; box2d (D,4) fp64 (the boxes, unrounded: :357);
    frustum_angle (D) fp64; cnt (D) int32; box_frame (D) int32 -- on the device -- and, on the host, counts (D) int64 and sub: per
    box the reference's subsample of a frustum of more than `cap` rows (row indices into the box's slice of `points`, drawn by
    draw_frustum_subsample(counts, cap, rng) when not given, range-checked when given) or None.  The subsample is NOT applied to
    `points`: SunrgbdInputBuilder.build_device composes it with its own draw.  The host reads the D * S segment counts once."""
    who = "sunrgbd_candidates"
    args, held, ps, D, S = _setup_sunrgbd(who, frame_points, frame_off, K, Rtilt, boxes2d, box_frame)
    dev = frame_points.device
    L = _native.lib()
    out = {"box2d": held[4], "frustum_angle": torch.zeros((D,), dtype=torch.float64, device=dev), "box_frame": held[5]}
    scnt = torch.zeros((D, S), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _native.check(L.fcn_frustum_sunrgbd_count(*args, out["frustum_angle"].data_ptr(), scnt.data_ptr(),
                                                  _native.current_stream(dev)), "fcn_frustum_sunrgbd_count")
        seg_counts = scnt.cpu().numpy().astype(np.int64)                    # D * S integers: the size of `points`
        counts = seg_counts.sum(1)
        sub = draw_frustum_subsample(counts, cap, rng) if sub is None else _check_sub(who, sub, counts)
        soff, out["points"] = _packed(seg_counts, ps, dev)
        if out["points"].shape[0] > 0:
            _native.check(L.fcn_frustum_sunrgbd_fill(*args, soff.data_ptr(), out["points"].data_ptr(),
                                                     _native.current_stream(dev)), "fcn_frustum_sunrgbd_fill")
    out["off"] = soff[::S].contiguous()                                     # every S-th entry is a box's offset
    out["cnt"] = scnt.sum(1, dtype=torch.int32)
    out["counts"] = counts
    out["sub"] = sub
    return out


def sunrgbd_training_candidates(frame_points, frame_off, K, Rtilt, boxes2d, box_frame, gt_box3d, sub=None, cap=SUNRGBD_CAP,
                                min_positives=SUNRGBD_MIN, rng=np.random):
    """The SUN-RGBD TRAINING records (extract_frustum_data :132-267), on the device.  frame_points ... box_frame as
    sunrgbd_candidates takes them; boxes2d (D,4): the boxes that select -- perturbed (perturb_boxes2d_sunrgbd) or plain;
    gt_box3d (D,7): cx, cy, cz, l, w, h, heading of the label beside each box in UPRIGHT DEPTH, l w h the label file's HALF
    extents (SUNObject3d.l / .w / .h), heading = SUNObject3d.heading_angle.
    The reference subsamples a frustum of more than `cap` rows and rejects a box with fewer than min_positives labelled rows
    AFTER that (:219-227).  Here: a box whose full positive count is below the bar is dropped before the fill (it cannot pass);
    after it fcn_frustum_subset_pos counts the positives the subsamples keep and the boxes below the bar are dropped too --
    their rows stay in `points`, unlisted.  sub: as sunrgbd_candidates (one entry per box, all D of them, in order).
    Returns a dict over the K kept boxes: points (rows, stride) float32 upright camera + the untouched columns and seg (rows)
    int64; off (K+1) int64 -- off[k] is box k's FIRST row (its rows are off[k] ... off[k] + cnt[k]; the last entry is the end of
    the buffer); box2d (K,4) fp64 = the float32 value the reference records (:230), widened -- selection and the frustum angle use
    the unrounded box; frustum_angle (K), box3d (K,8,3) upright camera corners, heading (K), size (K,3) = 2l, 2w, 2h fp64;
    box_frame (K), cnt (K), pos (K) int32 (the positives of the record, after its subsample) -- on the device -- and, on the host,
    kept (K) int64, counts (K) int64 and sub (K entries).  With no survivor the dict holds 'kept' alone.
    The host reads the 2 * D * S segment counts once, and one integer per pre-kept box when any of them is subsampled."""
    who = "sunrgbd_training_candidates"
    args, held, ps, D, S = _setup_sunrgbd(who, frame_points, frame_off, K, Rtilt, boxes2d, box_frame)
    dev = frame_points.device
    boxes, bframe = held[4], held[5]
    gt = torch.as_tensor(gt_box3d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 7)
    if gt.shape[0] != D:
        raise ValueError("%s: %d boxes, %d gt_box3d" % (who, D, gt.shape[0]))
    if D == 0:
        return {"kept": np.zeros(0, dtype=np.int64)}
    L = _native.lib()
    f64 = dict(dtype=torch.float64, device=dev)
    angle, corners = torch.zeros((D,), **f64), torch.zeros((D, 8, 3), **f64)
    both = torch.zeros((2, D, S), dtype=torch.int32, device=dev)            # selected, positive: one read
    with torch.cuda.device(dev):
        _native.check(L.fcn_frustum_sunrgbd_label_count(*args, gt.data_ptr(), angle.data_ptr(), both[0].data_ptr(),
                                                        both[1].data_ptr(), corners.data_ptr(), _native.current_stream(dev)),
                      "fcn_frustum_sunrgbd_label_count")
        both_h = both.cpu().numpy().astype(np.int64)                        # 2 * D * S integers
        seg_counts, positives = both_h[0], both_h[1].sum(1)
        counts = seg_counts.sum(1)
        sub = draw_frustum_subsample(counts, cap, rng) if sub is None else _check_sub(who, sub, counts)
        drop = positives < min_positives
        kept = np.nonzero(~drop)[0].astype(np.int64)
        if len(kept) == 0:
            return {"kept": kept}
        seg_counts[drop] = 0
        soff, points = _packed(seg_counts, ps, dev)
        seg = torch.empty((points.shape[0],), dtype=torch.int64, device=dev)
        _native.check(L.fcn_frustum_sunrgbd_label_fill(*args, gt.data_ptr(), soff.data_ptr(), points.data_ptr(), seg.data_ptr(),
                                                       _native.current_stream(dev)), "fcn_frustum_sunrgbd_label_fill")
        idx = torch.from_numpy(kept).to(dev, non_blocking=True)
        starts = soff[::S][:D].index_select(0, idx).contiguous()
        cnt = both[0].sum(1, dtype=torch.int32).index_select(0, idx).contiguous()
        pos = both[1].sum(1, dtype=torch.int32).index_select(0, idx).contiguous()
        if any(sub[d] is not None for d in kept):
            # the positives the subsamples keep: one launch over the pre-kept boxes, one read of their counts
            lens = [0 if sub[d] is None else len(sub[d]) for d in kept]
            sub_off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)).to(dev, non_blocking=True)
            flat = torch.from_numpy(np.concatenate([sub[d] for d in kept if sub[d] is not None]).astype(np.int32)).to(dev, non_blocking=True)
            pos = torch.zeros((len(kept),), dtype=torch.int32, device=dev)
            _native.check(L.fcn_frustum_subset_pos(seg.data_ptr(), starts.data_ptr(), cnt.data_ptr(), flat.data_ptr(),
                                                   sub_off.data_ptr(), len(kept), pos.data_ptr(), _native.current_stream(dev)),
                          "fcn_frustum_subset_pos")
            ok = pos.cpu().numpy() >= min_positives
            if not ok.all():
                kept = kept[ok]
                if len(kept) == 0:
                    return {"kept": kept}
                okd = torch.from_numpy(np.nonzero(ok)[0]).to(dev, non_blocking=True)
                idx, starts, cnt, pos = (x.index_select(0, okd).contiguous() for x in (idx, starts, cnt, pos))
    pick = lambda x: x.index_select(0, idx).contiguous()
    size = gt[:, 3:6] * 2.0                                                 # box3d_size = 2l, 2w, 2h (:217)
    return {"points": points, "seg": seg, "off": torch.cat([starts, soff[-1:]]), "box2d": pick(boxes.float().double()),
            "frustum_angle": pick(angle), "box3d": pick(corners), "heading": pick(gt[:, 6]), "size": pick(size),
            "box_frame": pick(bframe), "cnt": cnt, "pos": pos, "kept": kept, "counts": counts[kept], "sub": [sub[d] for d in kept]}


# ------------------------------------------------------------------------------------------------
# The KITTI first stage's training input as ONE capturable sequence of launches (csrc/frustum_plan.h)
def check_status(who, words, bits, sampler=None):
    """The check() of every capturable source: reads the status words (a synchronisation); where a bit is set, clears the words and
    raises ValueError naming who and the texts of the set bits (bits: a STATUS_BITS table).  sampler: the source's EpochSampler or
    None -- its word (whose bit 0 would read as the draws') is reported as EPOCH_STATUS_BIT."""
    if sampler is not None:
        words = tuple(words) + (sampler.status,)
    vals = [int(v) for v in torch.cat(words).cpu().tolist()]
    s = 0
    for v in (vals if sampler is None else vals[:-1]):
        s |= v
    if sampler is not None and vals[-1]:
        s |= EPOCH_STATUS_BIT[0]
    if s:
        for w in words:
            w.zero_()
        raise ValueError("%s: status %d -- %s" % (who, s, "; ".join(text for bit, text in tuple(bits) + (EPOCH_STATUS_BIT,) if s & bit)))


EPOCH_STATUS_BIT = (4096, "bit 12: the epoch sampler had no window -- a turn outside the epoch, or D * world labels exceed the table "
                          "(its pick is zeros: label 0 repeated; its state stayed)")


STATUS_BITS = ((1, "bit 0: a slot had no row to draw from (its choice row is zeros)"),
               (2, "bit 1: fewer boxes survived than the batch has slots (the empty slots repeat box 0's labels over no rows)"),
               (4, "bit 2: the selected rows exceed the capacity of the point buffer (the overflow was dropped)"),
               (16, "bit 4: a box had no valid perturbation within the attempt cap (its label box was used as it is)"),
               (256, "bit 8: more boxes survived than the batch has slots (the rest were dropped)"),
               (1024, "bit 10: n_boxes lies outside [0, D] or a box's frame outside [0, F) -- SUN-RGBD: or its class outside [0, C) -- (the overflow or the box was ignored)"),
               (2048, "bit 11: an NMS group held more than 4096 candidates (it has no keep list: none of its rows was kept)"))


class FrameTrainSource:
    """Resident LiDAR frames and label boxes -> the InputBuilder training batch at a FIXED batch size B, every step, with no host
    read and no upload: what perturb_boxes2d + frustum_training_candidates + InputBuilder.build_device_train(draws=DeviceDraws) do
    behind three synchronisations, as one sequence of launches that can be captured into a hipGraph and draws anew on every replay
    (INTEGRATION.md "Capturable first-stage training input" states the contract).
    frame_points ... img_size as frustum_candidates takes them; gt_box2d (G,4), gt_box3d (G,7), box_frame (G), types (G names): the
    G labels; builder: an InputBuilder (its npoints, strides, flip / shift); B: slots of the batch; D: labels tried per step
    (B <= D <= G, D <= 2048); capacity: rows of the point buffer (rows beyond it are dropped and flagged); seed: the three
    generators are DeviceDraws keyed seed (label pick), seed + 1 (box perturbation), seed + 2 (per-sample draws), each one step
    further after every step().  pick=False: the first D labels in order; perturb=False: the boxes as they are -- select_box2d
    (G,4) then optionally gives boxes that select in place of gt_box2d, which keeps deciding the reject rule.
    pick="epoch": the D labels are a rank window of the EPOCH's permutation (inputs.EpochSampler keyed seed, held as self.sampler:
    every label at most once per epoch, the tail of G mod (D * world) dropped, as the reference's shuffling loader does); rank /
    world, with this mode only: the window of this rank among `world` sources built alike (D * world <= G).  The three DeviceDraws
    step on as under pick=False.
    Everything is validated here, once, on the host; step() validates nothing and reads nothing."""

    def __init__(self, frame_points, frame_off, calib, img_size, gt_box2d, gt_box3d, box_frame, types, builder, B, D, capacity,
                 seed, perturb=True, pick=True, shift_ratio=0.1, min_box_height=25.0, clip_distance=2.0, select_box2d=None,
                 rank=None, world=None):
        who = "FrameTrainSource"
        pts, foff, F, ps, S = _frames(who, frame_points, frame_off, resident=True)
        dev = frame_points.device
        P, V2C, R0, wh = _calib(calib, img_size, F, dev)
        lab = self.labels = LabelTable(who, gt_box2d, gt_box3d, box_frame, types, F)
        B, D, G, capacity = int(B), int(D), lab.G, int(capacity)
        max_d, max_segs = resident.limits("fcn_frustum_train_plan_limits", 2)
        resident.check_slots(who, B, D, max_d, G)
        resident.check_segments(who, D, S, max_segs)
        resident.check_capacity(who, capacity)
        r = float(shift_ratio)
        if not (0.0 <= r < 1.0):
            raise ValueError("%s: shift_ratio must lie in [0, 1), got %r" % (who, shift_ratio))
        pick, self.sampler = resident.pick_mode(who, pick, rank, world, seed, builder.device, D, G)
        self.device, self.builder = dev, builder
        self.B, self.D, self.G, self.F, self.S, self.ps, self.capacity = B, D, G, F, S, ps, capacity
        self.perturb, self.pick, self.shift_ratio = bool(perturb), pick, r
        self.min_box_height, self.clip_distance = float(min_box_height), float(clip_distance)
        f64, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.float64, torch.int32, torch.int64))
        N = builder.npoints
        # ---- resident: the frames, the label table (the perturbation clips to the image: wh), the generators
        self.frames = (pts, foff, P, V2C, R0, wh)
        resident.adopt(self, lab.load(builder, dev, D, self.perturb, select_box2d, r, wh.cpu().numpy()))
        self.g_size = self.g_box3d[:, 3:6].contiguous()
        self.g_P = P.index_select(0, self.g_frame.to(torch.int64)).contiguous()
        seed = int(seed)
        self.draws_pick, self.draws_box, self.draws_sample = (DeviceDraws(seed + k, builder.device) for k in range(3))
        # ---- the batch and every intermediate
        self.points, self.seg_off, self.off, self.counts, self.slot_box, self.n_kept, self.status = \
            resident.batch_skeleton(dev, B, D, S, capacity, ps, 0)
        self.box2d, self.angle, self.corners = torch.zeros((D, 4), **f64), torch.zeros((D,), **f64), torch.zeros((D, 24), **f64)
        self.both = torch.zeros((2, D, S), **i32)               # selected, positive
        self.seg = torch.zeros((capacity + 1,), **i64)
        self.slot_label = torch.zeros((B,), **i32)
        self.t = {"raw": self.points, "off": self.off, "seg": self.seg, "choice": torch.zeros((B, N), **i32),
                  "fangle": torch.zeros((B,), **f64), "box2d": torch.zeros((B, 4), **f64), "P": torch.zeros((B, 12), **f64),
                  "corners": torch.zeros((B, 24), **f64), "heading": torch.zeros((B,), **f64), "size": torch.zeros((B, 3), **f64),
                  "coin": torch.zeros((B,), **f64), "normal": torch.zeros((B,), **f64),
                  "size_class": torch.zeros((B, 1), **i64), "B": B, "pt_stride": ps}
        if builder.one_hot:
            self.t["one_hot"] = torch.zeros((B, len(builder.classes)), dtype=torch.float32, device=dev)
        self.out = builder.alloc(B)
        if not self.pick:                                       # the first D labels, gathered once
            lab._gather_labels()

    @staticmethod
    def limits():
        """(the attempt cap of the perturbation, the largest D, the largest D * S) of the kernels."""
        return resident.limits("fcn_box2d_perturb_limits", 1) + resident.limits("fcn_frustum_train_plan_limits", 2)

    def _advance_pick(self):                                    # (the three step counters stay equal)
        p = lambda x: x.data_ptr()
        _native.check(_native.lib().fcn_box2d_perturb(p(self.gt2d), p(self.bframe), p(self.frames[5]), 0, self.F, self.shift_ratio,
                                                      self.draws_pick.seed, p(self.draws_pick.state), 1, p(self.gt2d), p(self.status),
                                                      _native.current_stream(self.device)), "fcn_box2d_perturb")

    def step(self):
        """Enqueues one batch on the current stream -- pick, gather, perturb, count, plan, fill, gather, draw, fcn_prepare_inputs --
        and nothing else: no allocation, no host read, no upload (capturable).  Returns the batch dict of InputBuilder.build(), same
        keys, shapes and dtypes, at batch size B; the same tensors every step.  self.boxes (D,4) holds the step's perturbed boxes,
        self.slot_box (B) the box of each slot, self.n_kept (1) the filled slots; check() reads the status words."""
        L, dev, bld = _native.lib(), self.device, self.builder
        B, D, S, t = self.B, self.D, self.S, self.t
        p = lambda x: x.data_ptr()
        pts, foff, P, V2C, R0, wh = self.frames
        with torch.cuda.device(dev):
            s = _native.current_stream(dev)
            self.labels.pick(self.draws_pick, self.pick, self._advance_pick, self.sampler)
            _native.check(L.fcn_box2d_perturb(p(self.gt2d), p(self.bframe), p(wh), D if self.perturb else 0, self.F, self.shift_ratio,
                                              self.draws_box.seed, p(self.draws_box.state), 1, p(self.boxes), p(self.status), s),
                          "fcn_box2d_perturb")
            args = (p(pts), p(foff), self.F, self.ps, p(P), p(V2C), p(R0), p(wh), p(self.boxes), p(self.bframe), D, S, 0,
                    self.clip_distance, p(self.gt3d))
            _native.check(L.fcn_frustum_train_count(*args, p(self.box2d), p(self.angle), p(self.both[0]), p(self.both[1]),
                                                    p(self.corners), s), "fcn_frustum_train_count")
            _native.check(L.fcn_frustum_train_plan(p(self.both[0]), p(self.both[1]), p(self.gt2d), self.min_box_height, D, S, B,
                                                   self.capacity, p(self.slot_box), p(self.seg_off), p(self.off), p(self.n_kept),
                                                   p(self.status), s), "fcn_frustum_train_plan")
            _native.check(L.fcn_frustum_train_fill(*args, p(self.seg_off), p(self.points), p(self.seg), s), "fcn_frustum_train_fill")
            torch.index_select(self.pick_idx.view(-1), 0, self.slot_box, out=self.slot_label)
            for src, dst in ((self.box2d, t["box2d"]), (self.angle, t["fangle"]), (self.corners, t["corners"])):
                torch.index_select(src, 0, self.slot_box, out=dst)
            for src, dst in ((self.g_heading, t["heading"]), (self.g_size, t["size"]), (self.g_P, t["P"]),
                             (self.g_class, t["size_class"])):
                torch.index_select(src, 0, self.slot_label, out=dst)
            if "one_hot" in t:
                torch.index_select(self.eye, 0, t["size_class"].view(-1), out=t["one_hot"])
            torch.sub(self.off[1:], self.off[:-1], out=self.counts)
            self.draws_sample.draw(self.counts, bld.npoints, bld.random_flip, bld.random_shift,
                                   out=(t["choice"], t["coin"], t["normal"]))
            return bld.launch(t, self.out)

    def check(self):
        """Reads the status words of the plan, the perturbation and the three generators (a synchronisation: not for a captured
        region); raises ValueError naming the bits set since the last check() and clears them."""
        check_status("FrameTrainSource", (self.status, self.draws_pick.status, self.draws_box.status, self.draws_sample.status),
                     STATUS_BITS, self.sampler)


# ------------------------------------------------------------------------------------------------
# The SUN-RGBD training input as ONE capturable sequence of launches (csrc/frustum_sunrgbd_plan.h)
class SunrgbdTrainSource:
    """Resident depth frames and label boxes -> the SunrgbdInputBuilder training batch at a FIXED batch size B, every step, with no
    host read and no upload: what perturb_boxes2d_sunrgbd + sunrgbd_training_candidates (with its host rng.choice per large frustum)
    + SunrgbdInputBuilder.build_device_train(draws=DeviceDraws) do behind four synchronisations, as one sequence of launches that
    can be captured into a hipGraph and draws anew on every replay (INTEGRATION.md "Capturable SUN-RGBD training input" states the
    contract).  It mirrors FrameTrainSource argument for argument: frame_points, frame_off as sunrgbd_candidates takes them; K, Rtilt
    (F,3,3); gt_box2d (G,4), gt_box3d (G,7) in upright depth with HALF extents (as sunrgbd_training_candidates takes it), box_frame
    (G), types (G names): the G labels; builder: a SunrgbdInputBuilder; B: slots of the batch; D: labels tried per step (B <= D <= G,
    D <= 2048); capacity: rows of the point buffer; seed: four DeviceDraws keyed seed (label pick), seed + 1 (box perturbation),
    seed + 2 (per-sample draws), seed + 3 (frustum subsamples), each one step further after every step(), whatever the options.
    pick=False: the first D labels in order; perturb=False: the boxes as they are -- select_box2d (G,4) then optionally gives the
    boxes that select; sub (with perturb=False and pick=False): one entry per first-D label, the subsample of that label's frustum
    (indices into its selected rows) or None, in place of the device's draw -- range-checked here against the counts of one count
    launch, and refused when `capacity` cannot hold every row (an index must never point at a row that was not stored).
    pick="epoch", rank, world: as FrameTrainSource takes them -- a rank window of the epoch's permutation (self.sampler).
    ALL pre-kept boxes (full positives >= min_positives) are filled, not only the B that end up holding a slot: the slots are decided
    after the subsample, which needs the labels of the stored rows.  So `capacity` has to hold the rows of up to D frustums:
    D times the longest frame is a sure bound; a smaller buffer works as long as check() does not report bit 2 -- rows beyond it are
    dropped (whole boxes from the end of the box order first) and every later count is the STORED count.
    Everything is validated here, once, on the host; step() validates nothing, allocates nothing, reads nothing and uploads nothing."""

    def __init__(self, frame_points, frame_off, K, Rtilt, gt_box2d, gt_box3d, box_frame, types, builder, B, D, capacity, seed,
                 perturb=True, pick=True, shift_ratio=0.1, cap=SUNRGBD_CAP, min_positives=SUNRGBD_MIN, select_box2d=None, sub=None,
                 rank=None, world=None):
        who = "SunrgbdTrainSource"
        pts, foff, F, ps, S = _frames(who, frame_points, frame_off, resident=True)
        dev = frame_points.device
        L = _native.lib()
        cal = resident.intrinsics(who, K, Rtilt, F, dev)
        lab = self.labels = LabelTable(who, gt_box2d, gt_box3d, box_frame, types, F)
        B, D, G, capacity, cap, min_positives = int(B), int(D), lab.G, int(capacity), int(cap), int(min_positives)
        max_d, max_segs, max_cap = self.limits()
        resident.check_slots(who, B, D, max_d, G)
        resident.check_segments(who, D, S, max_segs)
        if not (1 <= cap <= max_cap):
            raise ValueError("%s: cap must lie in [1, %d], got %d" % (who, max_cap, cap))
        resident.check_capacity(who, capacity)
        r = float(shift_ratio)
        if not (0.0 <= r < 1.0):
            raise ValueError("%s: shift_ratio must lie in [0, 1), got %r" % (who, shift_ratio))
        if sub is not None and (perturb or pick) and not (perturb and select_box2d is not None):   # (that refusal of load() comes first)
            raise ValueError("%s: sub goes with perturb=False and pick=False" % who)
        pick, self.sampler = resident.pick_mode(who, pick, rank, world, seed, builder.device, D, G)
        self.device, self.builder = dev, builder
        self.B, self.D, self.G, self.F, self.S, self.ps, self.capacity = B, D, G, F, S, ps, capacity
        self.perturb, self.pick, self.shift_ratio, self.cap, self.min_positives = bool(perturb), pick, r, cap, min_positives
        f64, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.float64, torch.int32, torch.int64))
        N = builder.npoints
        # ---- resident: the frames, the label table (no clip: nothing of the boxes to refuse), the generators
        self.frames = (pts, foff, cal[0], cal[1])
        resident.adopt(self, lab.load(builder, dev, D, self.perturb, select_box2d))
        self.g_size = (self.g_box3d[:, 3:6] * 2.0).contiguous()                 # box3d_size = 2l, 2w, 2h
        self.g_K = cal[0].index_select(0, self.g_frame.to(torch.int64)).contiguous()
        self.g_R = cal[1].index_select(0, self.g_frame.to(torch.int64)).contiguous()
        seed = int(seed)
        self.draws_pick, self.draws_box, self.draws_sample, self.draws_sub = (DeviceDraws(seed + k, builder.device) for k in range(4))
        # ---- the batch and every intermediate.  off holds B starts, not B + 1 bounds: a slot's rows are off[b] ... + counts[b]
        self.points, self.seg_off, _, self.counts, self.slot_box, self.n_kept, self.status = \
            resident.batch_skeleton(dev, B, D, S, capacity, ps, 0)
        self.off = torch.zeros((B,), **i64)
        self.box32, self.box64 = torch.zeros((D, 4), dtype=torch.float32, device=dev), torch.zeros((D, 4), **f64)
        self.angle, self.corners = torch.zeros((D,), **f64), torch.zeros((D, 24), **f64)
        self.both = torch.zeros((2, D, S), **i32)               # selected, positive
        self.row0 = torch.zeros((D,), **i64)
        self.cnt_stored, self.pos = torch.zeros((D,), **i32), torch.zeros((D,), **i32)
        self.plan_sub_off = torch.zeros((D + 1,), **i64)
        self.sub_off, self.sub = self.plan_sub_off, torch.zeros((D * cap,), **i32)
        self.fixed_sub = sub is not None
        self.seg = torch.zeros((capacity + 1,), **i64)
        self.slot_label, self.sub_start, self.sub_len = torch.zeros((B,), **i32), torch.zeros((B,), **i64), torch.zeros((B,), **i32)
        self.t = {"raw": self.points, "off": self.off, "seg": self.seg, "choice": torch.zeros((B, N), **i32),
                  "fangle": torch.zeros((B,), **f64), "box2d": torch.zeros((B, 4), **f64), "K": torch.zeros((B, 9), **f64),
                  "R": torch.zeros((B, 9), **f64), "corners": torch.zeros((B, 24), **f64), "heading": torch.zeros((B,), **f64),
                  "size": torch.zeros((B, 3), **f64), "coin": torch.zeros((B,), **f64), "normal": torch.zeros((B,), **f64),
                  "hshift": torch.zeros((B,), **f64), "size_class": torch.zeros((B, 1), **i64), "B": B, "pt_stride": ps}
        if builder.one_hot:
            self.t["one_hot"] = torch.zeros((B, len(builder.classes)), dtype=torch.float32, device=dev)
        self.out = builder.alloc(B)
        if not self.pick:                                       # the first D labels, gathered once
            lab._gather_labels()
        if self.fixed_sub:                                     # one count launch, read once: what the table is checked against
            with torch.cuda.device(dev):
                _native.check(L.fcn_frustum_sunrgbd_train_count(*self._args(), self.angle.data_ptr(), self.both[0].data_ptr(),
                                                                self.both[1].data_ptr(), self.corners.data_ptr(),
                                                                _native.current_stream(dev)), "fcn_frustum_sunrgbd_train_count")
            both_h = self.both.cpu().numpy().astype(np.int64)
            counts = both_h[0].sum(1)
            sub = _check_sub(who, list(sub), counts)
            rows = int(counts[both_h[1].sum(1) >= min_positives].sum())
            if rows > capacity:
                raise ValueError("%s: sub needs a capacity that holds every row of the pre-kept boxes: %d > %d" % (who, rows, capacity))
            lens = [0 if ix is None else len(ix) for ix in sub]
            flat = [ix for ix in sub if ix is not None]
            self.sub_off = resident.up(np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), dev)
            self.sub = resident.up(np.concatenate(flat).astype(np.int32), dev) if flat else torch.zeros((1,), **i32)

    @staticmethod
    def limits():
        """(the largest D, the largest D * S, the largest cap) of the kernels."""
        return resident.limits("fcn_frustum_train_plan_limits", 2) + resident.limits("fcn_draw_limits", 2)[:1]

    def _advance_pick(self):                                    # (the four step counters stay equal)
        p = lambda x: x.data_ptr()
        _native.check(_native.lib().fcn_box2d_perturb_sunrgbd(p(self.gt2d), 0, self.shift_ratio, self.draws_pick.seed,
                                                              p(self.draws_pick.state), 1, p(self.gt2d),
                                                              _native.current_stream(self.device)), "fcn_box2d_perturb_sunrgbd")

    def _args(self):
        pts, foff, K, R = self.frames
        return (pts.data_ptr(), foff.data_ptr(), self.F, self.ps, K.data_ptr(), R.data_ptr(), self.boxes.data_ptr(),
                self.bframe.data_ptr(), self.D, self.S, self.gt3d.data_ptr())

    def step(self):
        """Enqueues one batch on the current stream -- pick, gather, perturb, count, plan, fill, subsample, fcn_frustum_subset_pos,
        slots, gather, draw, fcn_prepare_inputs_sunrgbd -- and nothing else: no allocation, no host read, no upload (capturable).
        Returns the batch dict of SunrgbdInputBuilder.build(), same keys, shapes and dtypes, at batch size B; the same tensors every
        step.  self.boxes (D,4) holds the step's boxes, self.sub / self.sub_off the subsample table, self.slot_box (B) the box of
        each slot, self.n_kept (1) the filled slots; check() reads the status words."""
        L, dev, bld = _native.lib(), self.device, self.builder
        B, D, S, t = self.B, self.D, self.S, self.t
        p = lambda x: x.data_ptr()
        with torch.cuda.device(dev):
            s = _native.current_stream(dev)
            self.labels.pick(self.draws_pick, self.pick, self._advance_pick, self.sampler)
            _native.check(L.fcn_box2d_perturb_sunrgbd(p(self.gt2d), D if self.perturb else 0, self.shift_ratio, self.draws_box.seed,
                                                      p(self.draws_box.state), 1, p(self.boxes), s), "fcn_box2d_perturb_sunrgbd")
            args = self._args()
            _native.check(L.fcn_frustum_sunrgbd_train_count(*args, p(self.angle), p(self.both[0]), p(self.both[1]), p(self.corners), s),
                          "fcn_frustum_sunrgbd_train_count")
            _native.check(L.fcn_frustum_sunrgbd_train_plan(p(self.both[0]), p(self.both[1]), self.min_positives, self.cap, D, S,
                                                           self.capacity, p(self.seg_off), p(self.row0), p(self.cnt_stored),
                                                           p(self.plan_sub_off), p(self.status), s), "fcn_frustum_sunrgbd_train_plan")
            _native.check(L.fcn_frustum_sunrgbd_train_fill(*args, p(self.seg_off), p(self.points), p(self.seg), s),
                          "fcn_frustum_sunrgbd_train_fill")
            _native.check(L.fcn_frustum_subsample_draw(p(self.cnt_stored), p(self.plan_sub_off), 0 if self.fixed_sub else D, self.cap,
                                                       self.draws_sub.seed, p(self.draws_sub.state), 1, p(self.sub),
                                                       p(self.draws_sub.status), s), "fcn_frustum_subsample_draw")
            _native.check(L.fcn_frustum_subset_pos(p(self.seg), p(self.row0), p(self.cnt_stored), p(self.sub), p(self.sub_off), D,
                                                   p(self.pos), s), "fcn_frustum_subset_pos")
            _native.check(L.fcn_frustum_sunrgbd_train_slots(p(self.both[1]), p(self.pos), p(self.row0), p(self.cnt_stored),
                                                            p(self.sub_off), self.min_positives, D, S, B, self.capacity,
                                                            p(self.slot_box), p(self.n_kept), p(self.off), p(self.counts),
                                                            p(self.sub_start), p(self.sub_len), p(self.status), s),
                          "fcn_frustum_sunrgbd_train_slots")
            torch.index_select(self.pick_idx.view(-1), 0, self.slot_box, out=self.slot_label)
            self.box32.copy_(self.boxes)                        # the float32 value the reference records, widened again
            self.box64.copy_(self.box32)
            for src, dst in ((self.box64, t["box2d"]), (self.angle, t["fangle"]), (self.corners, t["corners"])):
                torch.index_select(src, 0, self.slot_box, out=dst)
            for src, dst in ((self.g_heading, t["heading"]), (self.g_size, t["size"]), (self.g_K, t["K"]), (self.g_R, t["R"]),
                             (self.g_class, t["size_class"])):
                torch.index_select(src, 0, self.slot_label, out=dst)
            if "one_hot" in t:
                torch.index_select(self.eye, 0, t["size_class"].view(-1), out=t["one_hot"])
            dd = self.draws_sample
            desc = _native.DrawDesc(B, bld.npoints, 1 if bld.random_flip else 0, 1 if bld.random_shift else 0)
            _native.check(L.fcn_draw_batch_sliced(ctypes.byref(desc), p(self.counts), p(self.sub), p(self.sub_start), p(self.sub_len),
                                                  dd.seed, p(dd.state), p(t["choice"]), p(t["coin"]), p(t["normal"]), p(t["hshift"]),
                                                  p(dd.status), s), "fcn_draw_batch_sliced")
            return bld.launch(t, self.out)

    def check(self):
        """Reads the status words of the plan, the slots and the four generators (a synchronisation: not for a captured region);
        raises ValueError naming the bits set since the last check() and clears them."""
        check_status("SunrgbdTrainSource", (self.status, self.draws_pick.status, self.draws_box.status, self.draws_sample.status,
                                            self.draws_sub.status), STATUS_BITS, self.sampler)


# ------------------------------------------------------------------------------------------------
# The KITTI first stage's INFERENCE input as ONE capturable sequence of launches (csrc/frustum_detect_plan.h)
class FrameDetectSource:
    """Resident velodyne frames and a resident table of at most D 2-D detections -> the InputBuilder inference batch at a FIXED
    batch size B1, every step, with no host read and no upload: what frustum_candidates + InputBuilder.build_device (+
    image_fov_points with fov=True) do behind their synchronisations, as one sequence of launches that can be captured into a
    hipGraph and replayed on boxes and points overwritten in place (INTEGRATION.md "Capturable inference front" states the contract).
    frame_points: a contiguous (n >= 1, >= 3) float32 device tensor, HELD, not copied -- a caller may overwrite it in place between
    steps; frame_off, calib, img_size as frustum_candidates takes them (copied to the device; S, the segments of the longest frame,
    is fixed here: frames written later must not be longer than S * fcn_frustum_select_seg() rows, nor move their offsets);
    builder: an InputBuilder; B1: slots of the batch; D: rows of the detection table (B1 <= D <= 2048; survivors beyond B1, in box
    order, are dropped and flagged); capacity: rows of the point buffer (rows beyond it are dropped and flagged); seed: keys the
    DeviceDraws of the per-sample resample, one step further after every step(); spare_group: the group of an empty slot.
    The detection table has D + 1 rows: boxes2d (D+1,4) fp64 xmin ymin xmax ymax, box_frame, box_class (index into builder.classes),
    box_group (D+1) int32, box_prob (D+1) fp32 and n_boxes (1) int32, the live rows.  A 2-D detector overwrites rows 0..n_boxes-1 and
    n_boxes in place between steps; set_boxes() fills them from host sequences.  Row D is the spare row an empty slot gathers -- a
    unit box, frame 0, class 0, spare_group, probability 0 -- written here once: leave it alone.
    fov=True: step() also selects every frame's image-FOV subset in rect camera coordinates into fov_points (n + 1, stride) /
    fov_off (F+1), as image_fov_points returns them (rows behind fov_off[F] are stale).
    Everything is validated here, once, on the host; step() validates nothing and reads nothing."""

    def __init__(self, frame_points, frame_off, calib, img_size, builder, B1, D, capacity, seed, spare_group, clip_distance=2.0,
                 clip_boxes=True, img_height_threshold=5, lidar_point_threshold=1, fov=False):
        who = "FrameDetectSource"
        resident.held(who, frame_points)
        pts, foff, F, ps, S = _frames(who, frame_points, frame_off, resident=True)
        dev = frame_points.device
        P, V2C, R0, wh = _calib(calib, img_size, F, dev)
        resident.need_device_builder(builder)
        B1, D, capacity, spare_group = int(B1), int(D), int(capacity), int(spare_group)
        max_d, max_segs = self.limits()
        resident.check_slots(who, B1, D, max_d, b="B1")
        if D * S > max_segs or (fov and F * S > max_segs):
            raise ValueError("%s: D * S = %d * %d (fov: F * S = %d * %d) segments exceed the plan's %d" % (who, D, S, F, S, max_segs))
        resident.check_capacity(who, capacity)
        if not (0 <= spare_group < 2 ** 31):
            raise ValueError("%s: spare_group must be a non-negative int32, got %d" % (who, spare_group))
        hthr, pthr, clipd = float(img_height_threshold), float(lidar_point_threshold), float(clip_distance)
        if not (np.isfinite(hthr) and np.isfinite(pthr) and np.isfinite(clipd)):
            raise ValueError("%s: thresholds and clip_distance must be finite, got %r, %r, %r" %
                             (who, img_height_threshold, lidar_point_threshold, clip_distance))
        self.device, self.builder = dev, builder
        self.B1, self.D, self.F, self.S, self.ps, self.capacity, self.spare_group = B1, D, F, S, ps, capacity, spare_group
        self.clip_distance, self.clip_boxes, self.fov = clipd, bool(clip_boxes), bool(fov)
        self.img_height_threshold, self.lidar_point_threshold = hthr, pthr
        f32, f64, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.float64, torch.int32, torch.int64))
        N, C = builder.npoints, len(builder.classes)
        # ---- resident: the frames (held), the calibration, the detection table with its spare row D
        self.frames = (pts, foff, P, V2C, R0, wh)
        self.table = DetectTable(dev, D, F, builder.classes, spare_group)
        resident.adopt(self, self.table)
        self.eye = torch.eye(C, **f32)
        self.draws = DeviceDraws(int(seed), builder.device)
        # ---- the batch and every intermediate.  The per-box outputs of the count have D + 1 rows as well: row D is what an empty
        # slot gathers, the spare row's own box and a zero angle, written here once and never by a kernel
        self.points, self.seg_off, self.off, self.counts, self.slot_box, self.n_kept, self.status = \
            resident.batch_skeleton(dev, B1, D, S, capacity, ps, D)
        self.box2d, self.angle = torch.zeros((D + 1, 4), **f64), torch.zeros((D + 1,), **f64)
        self.box2d[D] = self.boxes2d[D]
        self.seg_cnt = torch.zeros((D, S), **i32)
        self.slot_frame, self.slot_class = torch.zeros((B1,), **i32), torch.zeros((B1,), **i32)
        self.slot_group = torch.full((B1,), spare_group, **i32)
        self.t = {"raw": self.points, "off": self.off, "choice": torch.zeros((B1, N), **i32), "fangle": torch.zeros((B1,), **f64),
                  "box2d": torch.zeros((B1, 4), **f64), "P": torch.zeros((B1, 12), **f64), "B": B1, "pt_stride": ps}
        self.scalars = (torch.zeros((B1,), **f64), torch.zeros((B1,), **f64))          # the draw's coin and normal: unused
        self.out = builder.alloc_infer(B1)
        if self.fov:
            # the whole-image selection: one box (0, 0, W, H) per frame, no clipping, every box live
            n = int(pts.shape[0])
            self.fov_boxes = torch.cat([torch.zeros((F, 2), **f64), wh], 1).contiguous()
            self.fov_frame, self.fov_n = torch.arange(F, **i32), torch.full((1,), F, **i32)
            self.fov_box2d, self.fov_angle = torch.zeros((F, 4), **f64), torch.zeros((F,), **f64)
            self.fov_cnt, self.fov_seg_off = torch.zeros((F, S), **i32), torch.zeros((F * S + 1,), **i64)
            self.fov_off = torch.zeros((F + 1,), **i64)
            self.fov_points = torch.zeros((n + 1, ps), **f32)

    @staticmethod
    def limits():
        """(the largest D, the largest D * S) of the plan."""
        return resident.limits("fcn_frustum_detect_plan_limits", 2)

    def bind(self, fov_off=None, slot_frame=None, slot_class=None, slot_group=None):
        """Points outputs of step() at tensors of the caller (cascade.FrameCascade: the link's frame offsets and frustum tables):
        fov_off (F+1) int64; slot_frame, slot_class, slot_group (B1) int32 -- contiguous device tensors, written from the next
        step() on."""
        for name, t, dtype, n in (("fov_off", fov_off, torch.int64, self.F + 1), ("slot_frame", slot_frame, torch.int32, self.B1),
                                  ("slot_class", slot_class, torch.int32, self.B1), ("slot_group", slot_group, torch.int32, self.B1)):
            if t is None:
                continue
            if not (isinstance(t, torch.Tensor) and t.device == self.device and t.dtype == dtype and t.is_contiguous() and
                    tuple(t.shape) == (n,)) or (name == "fov_off" and not self.fov):
                raise ValueError("FrameDetectSource.bind: %s must be a contiguous (%d,) %s tensor on %s" % (name, n, dtype, self.device))
            setattr(self, name, t)
        return self

    def set_boxes(self, boxes2d, box_frame, types, prob, unit_group=None):
        """Fills rows 0..n-1 of the detection table and n_boxes in place from host sequences of n <= D boxes (validated here: finite
        boxes, frames in [0, F), class names of builder.classes, finite scores, groups in [0, spare_group); unit_group None: every
        box its own group, which needs n <= spare_group).  An upload: not for a captured region."""
        self.table.set_boxes("FrameDetectSource.set_boxes", boxes2d, box_frame, types, prob, unit_group)
        return self

    def step(self):
        """Enqueues one batch on the current stream -- count, plan, fill, the gathers through slot_box, the draw,
        fcn_prepare_inputs_infer and, with fov, the whole-image count, plan and fill -- and nothing else: no allocation, no host
        read, no upload (capturable).  Returns the batch dict of InputBuilder.build_device() without 'kept', at batch size B1 -- an
        empty slot holds the spare row's frustum over no rows -- plus slot_box (B1) int32 the box of each slot (D: empty), slot_frame,
        slot_class, slot_group (B1) int32 its frame, class and group (spare_group: empty) and n_kept (1) the filled slots; the same
        tensors every step.  check() reads the status words."""
        L, dev, bld = _native.lib(), self.device, self.builder
        B1, D, S, F, t, out = self.B1, self.D, self.S, self.F, self.t, self.out
        p = lambda x: x.data_ptr()
        pts, foff, P, V2C, R0, wh = self.frames
        with torch.cuda.device(dev):
            s = _native.current_stream(dev)
            args = (p(pts), p(foff), F, self.ps, p(P), p(V2C), p(R0), p(wh), p(self.boxes2d), p(self.box_frame), D, S,
                    1 if self.clip_boxes else 0, self.clip_distance, p(self.n_boxes))
            _native.check(L.fcn_frustum_detect_count(*args, p(self.box2d), p(self.angle), p(self.seg_cnt), s), "fcn_frustum_detect_count")
            _native.check(L.fcn_frustum_detect_plan(p(self.seg_cnt), p(self.box2d), p(self.box_frame), p(self.n_boxes),
                                                    self.img_height_threshold, self.lidar_point_threshold, D, S, B1, self.capacity, F,
                                                    p(self.slot_box), p(self.n_kept), p(self.seg_off), p(self.off), p(self.counts),
                                                    p(self.status), s), "fcn_frustum_detect_plan")
            _native.check(L.fcn_frustum_detect_fill(*args, p(self.seg_off), p(self.points), s), "fcn_frustum_detect_fill")
            for src, dst in ((self.angle, t["fangle"]), (self.box2d, t["box2d"]), (self.box_prob.view(D + 1, 1), out["rgb_prob"]),
                             (self.box_frame, self.slot_frame), (self.box_class, self.slot_class), (self.box_group, self.slot_group)):
                torch.index_select(src, 0, self.slot_box, out=dst)
            torch.index_select(P, 0, self.slot_frame, out=t["P"])
            if "one_hot" in out:
                torch.index_select(self.eye, 0, self.slot_class, out=out["one_hot"])
            self.draws.draw(self.counts, bld.npoints, False, False, out=(t["choice"],) + self.scalars)
            bld.launch_infer(t, out)
            if self.fov:
                fargs = (p(pts), p(foff), F, self.ps, p(P), p(V2C), p(R0), p(wh), p(self.fov_boxes), p(self.fov_frame), F, S, 0,
                         self.clip_distance, p(self.fov_n))
                _native.check(L.fcn_frustum_detect_count(*fargs, p(self.fov_box2d), p(self.fov_angle), p(self.fov_cnt), s),
                              "fcn_frustum_detect_count")
                _native.check(L.fcn_frustum_fov_plan(p(self.fov_cnt), F, S, int(pts.shape[0]), p(self.fov_seg_off), p(self.fov_off), s),
                              "fcn_frustum_fov_plan")
                _native.check(L.fcn_frustum_detect_fill(*fargs, p(self.fov_seg_off), p(self.fov_points), s), "fcn_frustum_detect_fill")
        return dict(out, slot_box=self.slot_box, slot_frame=self.slot_frame, slot_class=self.slot_class, slot_group=self.slot_group,
                    n_kept=self.n_kept)

    def check(self):
        """Reads the status words of the plan and the draws (a synchronisation: not for a captured region); raises ValueError naming
        the bits set since the last check() and clears them.  Bit 0 is the draws' own: an EMPTY slot has no row to draw from either,
        so it is set by every step with fewer survivors than slots."""
        check_status("FrameDetectSource", (self.status, self.draws.status), STATUS_BITS)


# ------------------------------------------------------------------------------------------------
# The SUN-RGBD INFERENCE input as ONE capturable sequence of launches (csrc/frustum_sunrgbd_detect_plan.h)
class SunrgbdDetectSource:
    """Resident depth frames and a resident table of at most D 2-D detections -> the SunrgbdInputBuilder inference batch at a FIXED
    batch size B, every step, with no host read and no upload: what sunrgbd_candidates (with its host rng.choice per large frustum) +
    SunrgbdInputBuilder.build_device do behind their synchronisations, as one sequence of launches that can be captured into a
    hipGraph and replayed on boxes and points overwritten in place (INTEGRATION.md "Capturable SUN-RGBD inference" states the
    contract).  It mirrors FrameDetectSource.
    frame_points: a contiguous (n >= 1, >= 3) float32 device tensor of upright-depth rows, HELD, not copied -- a caller may overwrite
    it in place between steps; frame_off, K, Rtilt as sunrgbd_candidates takes them (copied to the device; S, the segments of the
    longest frame, is fixed here: frames written later must not be longer than S * fcn_frustum_select_seg() rows, nor move their
    offsets); builder: a SunrgbdInputBuilder; B: slots of the batch; D: rows of the detection table (B <= D <= 2048; survivors beyond
    B, in box order, are dropped and flagged); capacity: rows of the point buffer (rows beyond it are dropped and flagged, and every
    later count is the STORED count); seed: two DeviceDraws keyed seed (per-sample resample) and seed + 1 (frustum subsamples), each
    one step further after every step(), whatever the options; cap / point_threshold: sunrgbd_candidates' and build_device's.
    The detection table has D + 1 rows: boxes2d (D+1,4) fp64 xmin ymin xmax ymax, box_frame, box_class (index into builder.classes)
    (D+1) int32, box_prob (D+1) fp32 and n_boxes (1) int32, the live rows.  A 2-D detector overwrites rows 0..n_boxes-1 and n_boxes in
    place between steps; set_boxes() fills them from host sequences.  Row D is the spare row an empty slot gathers -- a unit box,
    frame 0, class 0, probability 0 -- written here once: leave it alone.  There is no box_group: a box's NMS group is
    frame * C + class (C = len(builder.classes)), F * C for an empty slot.
    sub / choice (device tables, to reproduce a recorded run or to feed the existing path the same draws): sub (B * cap) int32 the
    per-slot subsample table in place of the device's draw -- slot i's `cap` indices into its stored rows at sub_off[i], the packed
    layout of the plan; choice (B, N) int32 indices into each slot's RECORD (its subsample where it has one) in place of the
    resample draw.  With either, step() clamps the composed indices to the slot's stored rows on the device (a few extra elementwise
    launches): an index never points at a row that was not stored.
    Everything is validated here, once, on the host; step() validates nothing and reads nothing."""

    def __init__(self, frame_points, frame_off, K, Rtilt, builder, B, D, capacity, seed, cap=SUNRGBD_CAP, point_threshold=SUNRGBD_MIN,
                 sub=None, choice=None):
        who = "SunrgbdDetectSource"
        resident.held(who, frame_points)
        pts, foff, F, ps, S = _frames(who, frame_points, frame_off, resident=True)
        dev = frame_points.device
        cal = resident.intrinsics(who, K, Rtilt, F, dev)
        resident.need_device_builder(builder)
        B, D, capacity, cap, point_threshold = int(B), int(D), int(capacity), int(cap), int(point_threshold)
        max_d, max_segs, max_cap = self.limits()
        N, C = builder.npoints, len(builder.classes)
        resident.check_slots(who, B, D, max_d)
        resident.check_segments(who, D, S, max_segs)
        if not (1 <= cap <= max_cap) or not (1 <= N <= max_cap):
            raise ValueError("%s: cap and the builder's npoints must lie in [1, %d], got %d, %d" % (who, max_cap, cap, N))
        resident.check_capacity(who, capacity)
        if F * C >= 2 ** 31 or abs(point_threshold) >= 2 ** 31:
            raise ValueError("%s: F * C = %d groups and point_threshold = %d must fit int32" % (who, F * C, point_threshold))
        for name, t, n in (("sub", sub, B * cap), ("choice", choice, B * N)):
            if t is not None and not (isinstance(t, torch.Tensor) and t.device == dev and t.dtype == torch.int32 and t.is_contiguous()
                                      and t.numel() == n):
                raise ValueError("%s: %s must be a contiguous int32 tensor of %d entries on %s" % (who, name, n, dev))
        self.device, self.builder = dev, builder
        self.B, self.D, self.F, self.C, self.S, self.ps, self.capacity = B, D, F, C, S, ps, capacity
        self.cap, self.point_threshold = cap, point_threshold
        f32, f64, i32, i64 = (dict(dtype=t, device=dev) for t in (torch.float32, torch.float64, torch.int32, torch.int64))
        # ---- resident: the frames (held), the calibration, the detection table with its spare row D
        self.frames = (pts, foff, cal[0], cal[1])
        self.table = DetectTable(dev, D, F, builder.classes)
        resident.adopt(self, self.table)
        self.eye = torch.eye(C, **f32)
        self.draws, self.draws_sub = DeviceDraws(int(seed), builder.device), DeviceDraws(int(seed) + 1, builder.device)
        # ---- the batch and every intermediate.  angle has D + 1 entries as well: entry D is what an empty slot gathers, zero, never
        # written by a kernel
        self.points, self.seg_off, self.off, self.counts, self.slot_box, self.n_kept, self.status = \
            resident.batch_skeleton(dev, B, D, S, capacity, ps, D)
        self.angle, self.seg_cnt = torch.zeros((D + 1,), **f64), torch.zeros((D, S), **i32)
        self.slot_frame, self.slot_class = torch.zeros((B,), **i32), torch.zeros((B,), **i32)
        self.slot_group = torch.full((B,), F * C, **i32)
        self.cnt32, self.sub_off = torch.zeros((B,), **i32), torch.zeros((B + 1,), **i64)
        self.sub_start, self.sub_len = torch.zeros((B,), **i64), torch.zeros((B,), **i32)
        self.fixed_sub, self.fixed_choice = sub is not None, choice
        self.sub = sub.view(-1) if self.fixed_sub else torch.zeros((B * cap,), **i32)
        self.t = {"raw": self.points, "off": self.off, "choice": torch.zeros((B, N), **i32), "fangle": torch.zeros((B,), **f64),
                  "box2d": torch.zeros((B, 4), **f64), "K": torch.zeros((B, 9), **f64), "R": torch.zeros((B, 9), **f64), "B": B,
                  "pt_stride": ps}
        self.scalars = tuple(torch.zeros((B,), **f64) for _ in range(3))            # the draw's coin, normal and hshift: unused
        self.out = builder.alloc_infer(B)

    @staticmethod
    def limits():
        """(the largest D, the largest D * S, the largest cap and npoints) of the kernels."""
        return resident.limits("fcn_frustum_detect_plan_limits", 2) + resident.limits("fcn_draw_limits", 2)[:1]

    def set_boxes(self, boxes2d, box_frame, types, prob):
        """Fills rows 0..n-1 of the detection table and n_boxes in place from host sequences of n <= D boxes (validated here: finite
        boxes, frames in [0, F), class names of builder.classes, finite scores).  An upload: not for a captured region."""
        self.table.set_boxes("SunrgbdDetectSource.set_boxes", boxes2d, box_frame, types, prob)
        return self

    def step(self):
        """Enqueues one batch on the current stream -- count, plan, fill, fcn_frustum_subsample_draw, the gathers through slot_box,
        fcn_draw_batch_sliced, fcn_prepare_inputs_sunrgbd_infer -- and nothing else: no allocation, no host read, no upload
        (capturable).  Returns the batch dict of SunrgbdInputBuilder.build_device() without 'kept', at batch size B -- an empty slot
        holds the spare row's frustum over no rows -- plus slot_box (B) int32 the box of each slot (D: empty), slot_frame, slot_class,
        slot_group (B) int32 its frame, class and group frame * C + class (F * C: empty) and n_kept (1) the filled slots; the same
        tensors every step.  self.sub / self.sub_off hold the step's subsample table; check() reads the status words."""
        L, dev, bld = _native.lib(), self.device, self.builder
        B, D, S, F, t, out = self.B, self.D, self.S, self.F, self.t, self.out
        p = lambda x: x.data_ptr()
        pts, foff, K, R = self.frames
        with torch.cuda.device(dev):
            s = _native.current_stream(dev)
            args = (p(pts), p(foff), F, self.ps, p(K), p(R), p(self.boxes2d), p(self.box_frame), D, S, p(self.n_boxes))
            _native.check(L.fcn_frustum_sunrgbd_detect_count(*args, p(self.angle), p(self.seg_cnt), s), "fcn_frustum_sunrgbd_detect_count")
            _native.check(L.fcn_frustum_sunrgbd_detect_plan(p(self.seg_cnt), p(self.box_frame), p(self.box_class), p(self.n_boxes),
                                                            self.point_threshold, self.cap, D, S, B, self.capacity, F, self.C,
                                                            p(self.slot_box), p(self.n_kept), p(self.seg_off), p(self.off), p(self.counts),
                                                            p(self.cnt32), p(self.sub_off), p(self.sub_start), p(self.sub_len),
                                                            p(self.slot_group), p(self.status), s), "fcn_frustum_sunrgbd_detect_plan")
            _native.check(L.fcn_frustum_sunrgbd_detect_fill(*args, p(self.seg_off), p(self.points), s), "fcn_frustum_sunrgbd_detect_fill")
            _native.check(L.fcn_frustum_subsample_draw(p(self.cnt32), p(self.sub_off), 0 if self.fixed_sub else B, self.cap,
                                                       self.draws_sub.seed, p(self.draws_sub.state), 1, p(self.sub),
                                                       p(self.draws_sub.status), s), "fcn_frustum_subsample_draw")
            for src, dst in ((self.angle, t["fangle"]), (self.boxes2d, t["box2d"]), (self.box_prob.view(D + 1, 1), out["rgb_prob"]),
                             (self.box_frame, self.slot_frame), (self.box_class, self.slot_class)):
                torch.index_select(src, 0, self.slot_box, out=dst)
            torch.index_select(K, 0, self.slot_frame, out=t["K"])
            torch.index_select(R, 0, self.slot_frame, out=t["R"])
            if "one_hot" in out:
                torch.index_select(self.eye, 0, self.slot_class, out=out["one_hot"])
            dd = self.draws
            desc = _native.DrawDesc(B, bld.npoints, 0, 0)
            _native.check(L.fcn_draw_batch_sliced(ctypes.byref(desc), p(self.counts), p(self.sub), p(self.sub_start), p(self.sub_len),
                                                  dd.seed, p(dd.state), p(t["choice"]), p(self.scalars[0]), p(self.scalars[1]),
                                                  p(self.scalars[2]), p(dd.status), s), "fcn_draw_batch_sliced")
            if self.fixed_sub or self.fixed_choice is not None:
                self._compose()
            bld.launch_infer(t, out)
        return dict(out, slot_box=self.slot_box, slot_frame=self.slot_frame, slot_class=self.slot_class, slot_group=self.slot_group,
                    n_kept=self.n_kept)

    def _compose(self):
        """The override tables into t["choice"]: a given choice indexes the slot's record, so it goes through the slot's subsample
        slice where it has one; whatever comes out is clamped to the slot's stored rows (elementwise launches, no host read)."""
        t, last = self.t, (self.counts - 1).clamp_(min=0).view(-1, 1)
        if self.fixed_choice is not None:
            ch = self.fixed_choice.view(self.B, -1).to(torch.int64)
            idx = (ch + self.sub_start.view(-1, 1)).clamp_(0, self.sub.numel() - 1)
            ch = torch.where(self.sub_len.view(-1, 1) > 0, self.sub.to(torch.int64)[idx], ch)
        else:
            ch = t["choice"].to(torch.int64)
        t["choice"].copy_(torch.minimum(ch.clamp_(min=0), last))

    def check(self):
        """Reads the status words of the plan and the two generators (a synchronisation: not for a captured region); raises
        ValueError naming the bits set since the last check() and clears them.  Bit 0 is the draws' own: an EMPTY slot has no row to
        draw from either, so it is set by every step with fewer survivors than slots."""
        check_status("SunrgbdDetectSource", (self.status, self.draws.status, self.draws_sub.status), STATUS_BITS)
