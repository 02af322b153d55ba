"""Frustum extraction on the device: LiDAR frames in velodyne coordinates + calibration + 2-D detection boxes -> the first
stage's raw frustum points and the refine stage's search set (C-ABI fcn_frustum_select_count / _fill, csrc/frustum_select.h).

Reference: kitti/prepare_data.py::extract_frustum_data_rgb_detection (:462-568) projects the whole frame to the image once per
frame in numpy (kitti_util.Calibration.project_velo_to_rect / project_rect_to_image, draw_util.get_lidar_in_image_fov) and masks
it once per detection on the host, pickling D ragged copies of the same frame for datasets/provider_sample.py;
kitti/prepare_data_refine.py:689-699 builds the rect-camera, image-FOV subset the refinement stage searches.  Here both are the
same two HIP launches over a grid of (segments, boxes); the host reads the D * S segment counts between them (they size the
point buffer) and each entry point reads box_frame and frame_off back to range-check them.  No point data crosses to the host.
No CPU fallback.
"""
import numpy as np
import torch

from . import _native
from .detect import _need_cuda


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


def frustum_candidates(frame_points, frame_off, calib, img_size, boxes2d, box_frame, clip_distance=2.0, clip_boxes=True):
    """frame_points (sum m_f, stride >= 3) float32 VELODYNE x, y, z (+ intensity, ...) of F frames packed behind each other,
    frame_off (F+1) int64 row offsets, calib {"P": (F,3,4), "V2C": (F,3,4), "R0": (F,3,3)} float64, img_size (F,2) as width,
    height, boxes2d (D,4) xmin ymin xmax ymax, box_frame (D) the frame of each box -- device tensors (everything but the points
    may be host arrays).  clip_boxes: clip every box to the image first, as the reference does.
    Returns a dict: points (sum cnt, stride) -- per box, in frame order, the frame's rows that project into it, as float32 rect
    camera x, y, z followed by the untouched columns; off (D+1) int64; box2d (D,4) fp64 the box actually used; frustum_angle
    (D) fp64; cnt (D) int32; box_frame (D) int32 -- on the device -- and counts (D) int64 on the host.  The host reads the D * S
    segment counts once, between the two launches (S = the longest frame in segments of fcn_frustum_select_seg() rows)."""
    _need_cuda(frame_points, "frustum_candidates")
    dev = frame_points.device
    pts = frame_points.detach().contiguous().float()
    if pts.dim() != 2 or pts.shape[1] < 3:
        raise ValueError("frustum_candidates: frame_points must be (n, >= 3), got %s" % (tuple(frame_points.shape),))
    foff_h = torch.as_tensor(frame_off).detach().cpu().to(torch.int64).contiguous().view(-1)      # F + 1 integers: they decide S
    foff = foff_h.to(dev, non_blocking=True)
    F, ps = int(foff_h.numel()) - 1, int(pts.shape[1])
    P, V2C, R0, wh = _calib(calib, img_size, F, dev)
    boxes = torch.as_tensor(boxes2d).to(device=dev, dtype=torch.float64).contiguous().view(-1, 4)
    bframe = torch.as_tensor(box_frame).to(device=dev, dtype=torch.int32).contiguous().view(-1)
    D = int(bframe.numel())
    if boxes.shape[0] != D:
        raise ValueError("frustum_candidates: %d boxes but %d frames" % (boxes.shape[0], D))
    L = _native.lib()
    seg = int(L.fcn_frustum_select_seg())
    longest = int((foff_h[1:] - foff_h[:-1]).max()) if F > 0 else 0
    S = max(1, -(-longest // seg))
    if pts.shape[0] == 0:
        pts = torch.zeros((1, ps), dtype=torch.float32, device=dev)        # (an address to hand in: every frame is empty)
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"box2d": torch.zeros((D, 4), **f64), "frustum_angle": torch.zeros((D,), **f64), "box_frame": bframe}
    scnt = torch.zeros((D, S), dtype=torch.int32, device=dev)
    args = (pts.data_ptr(), foff.data_ptr(), F, ps, P.data_ptr(), V2C.data_ptr(), R0.data_ptr(), wh.data_ptr(), boxes.data_ptr(),
            bframe.data_ptr(), D, S, 1 if clip_boxes else 0, float(clip_distance))
    with torch.cuda.device(dev):
        _native.check(L.fcn_frustum_select_count(*args, out["box2d"].data_ptr(), out["frustum_angle"].data_ptr(),
                                                 scnt.data_ptr(), _native.current_stream(dev)), "fcn_frustum_select_count")
        seg_counts = scnt.cpu().numpy().astype(np.int64)                    # D * S integers: the size of `points`
        seg_off = np.concatenate([[0], np.cumsum(seg_counts.reshape(-1))]).astype(np.int64)
        soff = torch.from_numpy(seg_off).to(dev, non_blocking=True)
        out["points"] = torch.empty((int(seg_off[-1]), ps), dtype=torch.float32, device=dev)
        if seg_off[-1] > 0:
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
