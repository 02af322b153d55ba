"""The contract of the capturable two-stage inference link (csrc/cascade_plan.h; INTEGRATION.md "Capturable two-stage inference")
restated in numpy -- NOT a port of the kernels: list comprehensions over the keep lists for the candidate table, np.cumsum for the
plan.  The referee of tests/test_cascade_plan_referee.py (which pins it to the numpy of TwoStageDetector.detect and to the plan of
tests/refine_plan_ref.py), tests/test_gpu_cascade_plan.py and tests/test_emu_cascade_plan.py."""
import numpy as np

from refine_plan_ref import windows

ST_TRUNC, ST_WIDE, ST_WIDTH, ST_ROWS, ST_MANY, ST_GROUP = 4, 32, 64, 128, 256, 512


def candidates(keep, cnt, L2, unit_frame, unit_class, unit_group, dets, D):
    """keep (G, top_k), cnt (G), unit_* (B1), dets (R, 8) -> cand_row, cand_frame, cand_class, cand_group (D) int32, cand_score (D)
    float32, n_cand, status."""
    keep, cnt = np.asarray(keep, dtype=np.int64), np.asarray(cnt, dtype=np.int64)
    G, top_k = keep.shape
    B1, R = len(unit_frame), len(dets)
    status = 0
    rows = []
    for g in range(G):
        if cnt[g] < 0 or cnt[g] > top_k:
            status |= ST_GROUP
            continue
        rows += [int(r) for r in keep[g, :cnt[g]] if 0 <= r < R and r // L2 < B1]
    if len(rows) > D:
        status |= ST_ROWS
    rows = np.asarray(rows[:D], dtype=np.int64)
    n = len(rows)
    unit = rows // L2
    out = {"cand_row": np.full(D, -1, np.int32), "cand_frame": np.full(D, -1, np.int32), "cand_class": np.zeros(D, np.int32),
           "cand_group": np.full(D, G, np.int32), "cand_score": np.zeros(D, np.float32)}
    out["cand_row"][:n] = rows
    out["cand_frame"][:n] = np.asarray(unit_frame)[unit]
    out["cand_class"][:n] = np.asarray(unit_class)[unit]
    out["cand_group"][:n] = np.asarray(unit_group)[unit]
    out["cand_score"][:n] = np.asarray(dets, dtype=np.float32)[rows, 7]
    return out, n, status


def plan(seg_cnt, pred_size, strides, lpad, B, capacity):
    """-> slot_unit (B) int32, n_kept, seg_off (D*S+1) int64, off (B+1) int64, counts (B) int64, status."""
    seg_cnt = np.asarray(seg_cnt, dtype=np.int64)
    pred_size = np.asarray(pred_size, dtype=np.float64).reshape(-1, 3)
    D, S = seg_cnt.shape
    status = 0
    survive = []
    for d in range(D):
        if seg_cnt[d].sum() < 1:                                            # lidar_point_threshold = 1
            continue
        w = float(pred_size[d, 1])
        if not (w > 0.0 and np.isfinite(w)):
            status |= ST_WIDTH
        elif any(windows(w, float(s)) > float(lp) for s, lp in zip(strides, lpad)):
            status |= ST_WIDE
        else:
            survive.append(d)
    if len(survive) > B:
        status |= ST_MANY
    held = np.asarray(survive[:B], dtype=np.int64)
    n = len(held)
    cnt = np.zeros_like(seg_cnt)
    cnt[held] = np.maximum(seg_cnt[held], 0)
    raw = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    if raw[-1] > capacity:
        status |= ST_TRUNC
    seg_off = np.minimum(raw, capacity)
    slot_unit = np.full(B, D, dtype=np.int32)
    slot_unit[:n] = held
    off = np.full(B + 1, capacity, dtype=np.int64)
    off[:n] = seg_off[held * S]
    off[B] = seg_off[-1]
    counts = np.zeros(B, dtype=np.int64)
    counts[:n] = seg_off[(held + 1) * S] - seg_off[held * S]
    return slot_unit, n, seg_off, off, counts, status
