"""The contract of the capturable SUN-RGBD training input (csrc/frustum_sunrgbd_plan.h; INTEGRATION.md "Capturable SUN-RGBD training
input") restated in numpy -- NOT a port of the kernels: scalar Python floats for the perturbation, np.cumsum for the plan,
draws_ref.choice_row for the subsample, np.nonzero for the slots.  The referee of tests/test_sunrgbd_plan_referee.py (which pins it
to frustum.perturb_boxes2d_sunrgbd and the host block of frustum.sunrgbd_training_candidates), tests/test_gpu_sunrgbd_plan.py and
tests/test_emu_sunrgbd_plan.py."""
import numpy as np

import draws_ref
from frustum_plan_ref import ST_FEW, ST_TRUNC, uniforms


def perturb(seed, step, boxes, r, draw=None):
    """boxes (D,4) -> (D,4) float64: sunrgbd_utils.random_shift_box2d with the four uniforms of blocks 0 and 1 of tag 3 (cx, cy, h,
    w), Python floats (IEEE doubles, one rounding per operation), no clip, no retry.  draw(d): the four uniforms, by default the
    contract's."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    draw = draw or (lambda d: uniforms(seed, step, d, 0))
    out = np.empty_like(boxes)
    for d, (xmin, ymin, xmax, ymax) in enumerate(boxes.tolist()):
        u = draw(d)
        h, w = ymax - ymin, xmax - xmin
        cx, cy = (xmin + xmax) / 2.0, (ymin + ymax) / 2.0
        cx2 = cx + w * r * (u[0] * 2 - 1)
        cy2 = cy + h * r * (u[1] * 2 - 1)
        h2 = h * (1 + u[2] * 2 * r - r)
        w2 = w * (1 + u[3] * 2 * r - r)
        out[d] = [cx2 - w2 / 2.0, cy2 - h2 / 2.0, cx2 + w2 / 2.0, cy2 + h2 / 2.0]
    return out


def plan(seg_cnt, seg_pos, min_positives, cap, capacity):
    """-> seg_off (D*S+1) int64, row0 (D) int64, cnt_stored (D) int32, sub_off (D+1) int64, status."""
    seg_cnt = np.asarray(seg_cnt, dtype=np.int64)
    seg_pos = np.asarray(seg_pos, dtype=np.int64)
    D, S = seg_cnt.shape
    pre = seg_pos.sum(1) >= min_positives
    cnt = np.where(pre[:, None], np.maximum(seg_cnt, 0), 0)
    raw = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    seg_off = np.minimum(raw, capacity)
    row0 = seg_off[:-1:S][:D].copy() if D else np.zeros(0, dtype=np.int64)
    ends = seg_off[S::S][:D] if D else np.zeros(0, dtype=np.int64)
    cnt_stored = (ends - row0).astype(np.int32)
    sub_off = np.concatenate([[0], np.cumsum(np.where(cnt_stored > cap, cap, 0))]).astype(np.int64)
    return seg_off, row0, cnt_stored, sub_off, (ST_TRUNC if raw[-1] > capacity else 0)


def subsample(seed, step, cnt_stored, sub_off, cap, size=None):
    """The packed table fcn_frustum_subsample_draw writes under generator `seed` (the source's seed + 3) at `step`; entries outside
    every slice are -1 here (the kernel leaves them alone)."""
    sub = np.full(int(sub_off[-1]) if size is None else size, -1, dtype=np.int32)
    for d in range(len(cnt_stored)):
        if sub_off[d + 1] > sub_off[d]:
            sub[int(sub_off[d]):int(sub_off[d]) + cap] = draws_ref.choice_row(seed, step, d, int(cnt_stored[d]), cap)
    return sub


def subset_pos(seg, row0, cnt_stored, sub, sub_off):
    """fcn_frustum_subset_pos at U = D: the positives each box keeps under its slice of `sub` (all its stored rows without one)."""
    pos = np.zeros(len(row0), dtype=np.int32)
    for d in range(len(row0)):
        rows = np.asarray(seg[int(row0[d]):int(row0[d]) + int(cnt_stored[d])])
        if sub_off[d + 1] > sub_off[d]:
            rows = rows[np.asarray(sub[int(sub_off[d]):int(sub_off[d + 1])])]
        pos[d] = int((rows != 0).sum())
    return pos


def slots(seg_pos, pos, row0, cnt_stored, sub_off, min_positives, B, capacity):
    """-> slot_box (B) int32, n_kept, off (B) int64, counts (B) int64, sub_start (B) int64, sub_len (B) int32, status."""
    seg_pos = np.asarray(seg_pos, dtype=np.int64)
    survive = (seg_pos.sum(1) >= min_positives) & (np.asarray(pos) >= min_positives)
    boxes = np.nonzero(survive)[0]
    held = boxes[:B]
    n = len(held)
    slot_box = np.zeros(B, dtype=np.int32)
    off, counts = np.full(B, capacity, dtype=np.int64), np.zeros(B, dtype=np.int64)
    sub_start, sub_len = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int32)
    slot_box[:n] = held
    off[:n], counts[:n] = np.asarray(row0)[held], np.asarray(cnt_stored)[held]
    lens = (np.asarray(sub_off)[1:] - np.asarray(sub_off)[:-1])[held]
    sub_len[:n] = lens
    sub_start[:n] = np.where(lens > 0, np.asarray(sub_off)[:-1][held], 0)
    return slot_box, n, off, counts, sub_start, sub_len, (ST_FEW if len(boxes) < B else 0)
