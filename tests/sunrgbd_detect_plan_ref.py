"""The contract of capturable SUN-RGBD inference (csrc/frustum_sunrgbd_detect_plan.h, fcn_det_rows of csrc/det_eval.h; INTEGRATION.md
"Capturable SUN-RGBD inference") restated in numpy -- NOT a port of the kernels: boolean masks for the rule, np.cumsum for the
offsets, list concatenation for the tail.  The referee of tests/test_sunrgbd_detect_plan_referee.py (which pins it to hand-worked
tables, to the expressions of SunrgbdInputBuilder.build_device and to the reference's recorded run),
tests/test_gpu_sunrgbd_detect_source.py and tests/test_emu_sunrgbd_detect_source.py."""
import numpy as np

ST_DRAW, ST_TRUNC, ST_MANY, ST_RANGE, ST_OVER = 1, 4, 256, 1024, 2048
PLAN_KEYS = ("slot_box", "n_kept", "seg_off", "off", "counts", "cnt32", "sub_off", "sub_start", "sub_len", "slot_group", "status")


def plan(seg_cnt, box_frame, box_class, n_boxes, point_threshold, cap, B, capacity, F, C):
    """seg_cnt (D, S), box_frame (D), box_class (D), n_boxes -> a dict over PLAN_KEYS: slot_box (B) int32, n_kept, seg_off (D*S+1)
    int64, off (B+1) int64, counts (B) int64, cnt32 (B) int32, sub_off (B+1) int64, sub_start (B) int64, sub_len (B) int32,
    slot_group (B) int32, status.  Entries of box_frame / box_class at or beyond n_boxes do not matter."""
    seg_cnt = np.maximum(np.asarray(seg_cnt, dtype=np.int64), 0)
    D, S = seg_cnt.shape
    frame = np.asarray(box_frame, dtype=np.int64).reshape(D)
    cls = np.asarray(box_class, dtype=np.int64).reshape(D)
    status = 0
    n_boxes = int(n_boxes)
    if n_boxes < 0 or n_boxes > D:
        status |= ST_RANGE
    live = np.arange(D) < min(max(n_boxes, 0), D)
    in_range = (frame >= 0) & (frame < F) & (cls >= 0) & (cls < C)
    if (live & ~in_range).any():
        status |= ST_RANGE
    rows = np.minimum(seg_cnt.sum(1), cap)                                  # frustum.subsampled_counts
    survive = np.nonzero(live & in_range & (rows >= max(1, int(point_threshold))))[0]
    if len(survive) > B:
        status |= ST_MANY
    held = survive[:B]
    n = len(held)
    cnt = np.zeros_like(seg_cnt)
    cnt[held] = seg_cnt[held]
    raw = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    if raw[-1] > capacity:
        status |= ST_TRUNC
    seg_off = np.minimum(raw, capacity)
    slot_box = np.full(B, D, dtype=np.int32)
    slot_box[:n] = held
    off = np.full(B + 1, capacity, dtype=np.int64)
    off[:n] = seg_off[held * S]
    off[B] = seg_off[-1]
    counts = np.zeros(B, dtype=np.int64)
    counts[:n] = seg_off[(held + 1) * S] - seg_off[held * S]
    big = counts > cap                                                      # decided on the STORED rows
    sub_off = np.concatenate([[0], np.cumsum(np.where(big, cap, 0))]).astype(np.int64)
    slot_group = np.full(B, F * C, dtype=np.int32)
    slot_group[:n] = frame[held] * C + cls[held]
    return {"slot_box": slot_box, "n_kept": n, "seg_off": seg_off, "off": off, "counts": counts,
            "cnt32": np.minimum(counts, 2 ** 31 - 1).astype(np.int32), "sub_off": sub_off,
            "sub_start": np.where(big, sub_off[:B], 0).astype(np.int64), "sub_len": np.where(big, cap, 0).astype(np.int32),
            "slot_group": slot_group, "status": status}


def det_rows(keep, cnt, dets):
    """keep (G, top_k), cnt (G), dets (num_dets, 8) -> det_off (G+1) int32, rows (G*top_k) int32, scores (G*top_k) float32, n_rows,
    status."""
    keep = np.asarray(keep, dtype=np.int32)
    G, top_k = keep.shape
    cnt = np.asarray(cnt, dtype=np.int64).reshape(G)
    dets = np.asarray(dets, dtype=np.float32).reshape(-1, 8)
    c = np.clip(cnt, 0, top_k)
    det_off = np.concatenate([[0], np.cumsum(c)]).astype(np.int32)
    n = int(det_off[-1])
    rows = np.full(G * top_k, -1, dtype=np.int32)
    rows[:n] = np.concatenate([keep[g, :c[g]] for g in range(G)])
    scores = np.full(G * top_k, np.nan, dtype=np.float32)
    ok = (rows >= 0) & (rows < len(dets))
    scores[ok] = dets[rows[ok], 7]
    return det_off, rows, scores, n, (ST_OVER if (cnt == -1).any() else 0)


def corners(dets, rows):
    """Which rows of fcn_box3d_corners' output are NaN: the rows that are -1 or outside [0, num_dets)."""
    rows = np.asarray(rows)
    return (rows < 0) | (rows >= len(dets))
