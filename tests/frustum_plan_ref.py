"""The contract of the capturable first-stage training input (csrc/frustum_plan.h; INTEGRATION.md "Capturable first-stage training
input") restated in numpy -- NOT a port of the kernels: scalar Python floats for the perturbation, np.cumsum for the plan.  The
referee of tests/test_frustum_plan_referee.py (which pins it to frustum.perturb_boxes2d and frustum_training_candidates),
tests/test_gpu_frustum_plan.py and tests/test_emu_frustum_plan.py."""
import numpy as np

from draws_ref import _u53, philox4x32

ATTEMPTS = 32                          # fcn_box2d_perturb_limits
ST_FEW, ST_TRUNC, ST_PERTURB = 2, 4, 16


def uniforms(seed, step, d, t):
    """The four uniforms of box d's attempt t at `step`: blocks 2t and 2t + 1 of tag 3."""
    seed, step = int(seed), int(step)
    ctr = np.array([[2 * t, d, step & 0xFFFFFFFF, ((step >> 32) << 2) | 3], [2 * t + 1, d, step & 0xFFFFFFFF, ((step >> 32) << 2) | 3]],
                   dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    w = philox4x32(ctr, key).reshape(-1)
    scale = 2.0 ** -53
    return [_u53(w[2 * i], w[2 * i + 1]) * scale for i in range(4)]


def attempt(box, W, H, r, u):
    """One attempt of random_shift_box2d on (xmin, ymin, xmax, ymax) with the uniforms u (cx, cy, h, w) -> the clipped box (4
    Python floats: IEEE doubles, one rounding per operation) and whether it is valid."""
    xmin, ymin, xmax, ymax = (float(v) for v in box)
    h, w = ymax - ymin, xmax - xmin
    cx, cy = (xmin + xmax) / 2.0, (ymin + ymax) / 2.0
    cx2 = cx + w * r * (u[0] * 2 - 1)
    cy2 = cy + h * r * (u[1] * 2 - 1)
    h2 = h * (1 + u[2] * 2 * r - r)
    w2 = w * (1 + u[3] * 2 * r - r)
    clip = lambda v, hi: min(max(v, 0.0), hi)
    new = [clip(cx2 - w2 / 2.0, W - 1), clip(cy2 - h2 / 2.0, H - 1), clip(cx2 + w2 / 2.0, W - 1), clip(cy2 + h2 / 2.0, H - 1)]
    return new, new[0] < new[2] and new[1] < new[3]


def perturb(seed, step, boxes, wh, r, T=ATTEMPTS, draw=None):
    """boxes (D,4), wh (D,2) the image of each box (a row of NaN: its frame is out of range) -> (out (D,4) float64, attempt (D)
    the winning attempt or -1, fail (D) bool).  A failed box keeps its input.  draw(d, t): the four uniforms of an attempt, by
    default the contract's."""
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    wh = np.broadcast_to(np.asarray(wh, dtype=np.float64).reshape(-1, 2), (len(boxes), 2))
    draw = draw or (lambda d, t: uniforms(seed, step, d, t))
    out, used, fail = boxes.copy(), np.full(len(boxes), -1, dtype=np.int64), np.ones(len(boxes), dtype=bool)
    for d in range(len(boxes)):
        if np.isnan(wh[d]).any():
            continue
        for t in range(T):
            new, ok = attempt(boxes[d], float(wh[d, 0]), float(wh[d, 1]), r, draw(d, t))
            if ok:
                out[d], used[d], fail[d] = new, t, False
                break
    return out, used, fail


def plan(seg_cnt, seg_pos, gt2d, min_h, B, capacity):
    """-> slot_box (B) int32, seg_off (D*S+1) int64, off (B+1) int64, n_kept, status."""
    seg_cnt = np.asarray(seg_cnt, dtype=np.int64)
    seg_pos = np.asarray(seg_pos, dtype=np.int64)
    gt2d = np.asarray(gt2d, dtype=np.float64).reshape(-1, 4)
    D, S = seg_cnt.shape
    survive = ~(gt2d[:, 3] - gt2d[:, 1] < min_h) & (seg_pos.sum(1) > 0)
    boxes = np.nonzero(survive)[0]
    held = boxes[:B]
    n = len(held)
    cnt = np.zeros_like(seg_cnt)
    cnt[held] = np.maximum(seg_cnt[held], 0)
    raw = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    seg_off = np.minimum(raw, capacity)
    slot_box = np.zeros(B, dtype=np.int32)
    slot_box[:n] = held
    off = np.full(B + 1, seg_off[-1], dtype=np.int64)
    off[:n] = seg_off[held * S]
    status = (ST_FEW if len(boxes) < B else 0) | (ST_TRUNC if raw[-1] > capacity else 0)
    return slot_box, seg_off, off, n, status
