"""The contract of the capturable inference front (csrc/frustum_detect_plan.h; INTEGRATION.md "Capturable inference front") restated
in numpy -- NOT a port of the kernels: boolean masks for the skip rule, np.cumsum for the offsets, fancy indexing for the gathers of
frustum.FrameDetectSource.  The referee of tests/test_frustum_detect_plan_referee.py (which pins it to hand-worked cases and to the
expressions of InputBuilder.build_device and frustum.frustum_candidates), tests/test_gpu_frustum_detect.py and
tests/test_emu_frustum_detect.py."""
import numpy as np

ST_DRAW, ST_TRUNC, ST_MANY, ST_RANGE = 1, 4, 256, 1024


def plan(seg_cnt, box2d, box_frame, n_boxes, img_height_threshold, lidar_point_threshold, B1, capacity, F):
    """seg_cnt (D, S), box2d (D, 4) fp64, box_frame (D), n_boxes -> slot_box (B1) int32, n_kept, seg_off (D*S+1) int64, off (B1+1)
    int64, counts (B1) int64, status.  Rows of box2d at or beyond n_boxes, and of boxes with a frame out of range, do not matter."""
    seg_cnt = np.maximum(np.asarray(seg_cnt, dtype=np.int64), 0)
    D, S = seg_cnt.shape
    box = np.asarray(box2d, dtype=np.float64).reshape(D, 4)
    frame = np.asarray(box_frame, dtype=np.int64).reshape(D)
    status = 0
    n_boxes = int(n_boxes)
    if n_boxes < 0 or n_boxes > D:
        status |= ST_RANGE
    live = np.arange(D) < min(max(n_boxes, 0), D)
    in_range = (frame >= 0) & (frame < F)
    if (live & ~in_range).any():
        status |= ST_RANGE
    count = seg_cnt.sum(1)
    with np.errstate(invalid="ignore"):
        skip = (box[:, 3] - box[:, 1] < img_height_threshold) | (box[:, 2] - box[:, 0] < 1) | (count < lidar_point_threshold)
    survive = np.nonzero(live & in_range & ~skip & (count > 0))[0]
    if len(survive) > B1:
        status |= ST_MANY
    held = survive[:B1]
    n = len(held)
    cnt = np.zeros_like(seg_cnt)
    cnt[held] = seg_cnt[held]
    raw = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    if raw[-1] > capacity:
        status |= ST_TRUNC
    seg_off = np.minimum(raw, capacity)
    slot_box = np.full(B1, D, dtype=np.int32)
    slot_box[:n] = held
    off = np.full(B1 + 1, capacity, dtype=np.int64)
    off[:n] = seg_off[held * S]
    off[B1] = seg_off[-1]
    counts = np.zeros(B1, dtype=np.int64)
    counts[:n] = seg_off[(held + 1) * S] - seg_off[held * S]
    return slot_box, n, seg_off, off, counts, status


def fov_plan(seg_cnt, capacity):
    """seg_cnt (F, S) -> seg_off (F*S+1) int64, fov_off (F+1) int64."""
    seg_cnt = np.maximum(np.asarray(seg_cnt, dtype=np.int64), 0)
    S = seg_cnt.shape[1]
    seg_off = np.minimum(np.concatenate([[0], np.cumsum(seg_cnt.reshape(-1))]), capacity).astype(np.int64)
    return seg_off, seg_off[::S].copy()


def gathers(slot_box, box2d, angle, box_frame, box_class, box_group, box_prob, P, num_classes):
    """The source's gathers through slot_box: the per-box tables have D + 1 rows (row D: the spare row), P is (F, 12)."""
    sb = np.asarray(slot_box, dtype=np.int64)
    frame, cls = np.asarray(box_frame)[sb].astype(np.int32), np.asarray(box_class)[sb].astype(np.int32)
    return {"fangle": np.asarray(angle, dtype=np.float64)[sb], "box2d": np.asarray(box2d, dtype=np.float64)[sb],
            "P": np.asarray(P, dtype=np.float64).reshape(-1, 12)[frame], "rgb_prob": np.asarray(box_prob, dtype=np.float32)[sb].reshape(-1, 1),
            "one_hot": np.eye(num_classes, dtype=np.float32)[cls], "slot_frame": frame, "slot_class": cls,
            "slot_group": np.asarray(box_group)[sb].astype(np.int32)}
