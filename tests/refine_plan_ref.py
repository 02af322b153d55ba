"""The contract of the capturable refine-stage training input (csrc/refine_plan.h; INTEGRATION.md "Capturable refine-stage training
input") restated in numpy -- NOT a port of the kernels: the Philox of tests/draws_ref.py for the jitter draw, np.cumsum and
len(np.arange(...)) for the plan.  The referee of tests/test_refine_plan_referee.py (which pins it to the host block of
cascade.refine_training_candidates and to RefineInputBuilder._lpad), tests/test_gpu_refine_plan.py and tests/test_emu_refine_plan.py."""
import numpy as np

from draws_ref import _u53, _words

ST_FEW, ST_TRUNC, ST_WIDE, ST_WIDTH = 2, 4, 32, 64


def jitter_draw(seed, step, D, A):
    """(D, A, 7) float64: unit u = d * A + a takes words 0..13 of tag 3 of row u at `step`, uniform j from words 2j, 2j + 1."""
    out = np.zeros((D, A, 7), dtype=np.float64)
    scale = 2.0 ** -53
    for u in range(D * A):
        w = _words(seed, step, u, 3, 16)
        out[u // A, u % A] = [_u53(w[2 * j], w[2 * j + 1]) * scale for j in range(7)]
    return out


def windows(w, stride):
    """len(np.arange(-w / 2, w / 2, stride)) without building the array: numpy's own length rule, ceil((stop - start) / step)."""
    return float(np.ceil((w / 2.0 - (-w / 2.0)) / stride))


def plan(seg_cnt, seg_pos, pred_size, strides, lpad, B, capacity):
    """-> slot_unit (B) int32, n_kept, seg_off (U*S+1) int64, off (B+1) int64, counts (B) int64, status."""
    seg_cnt = np.asarray(seg_cnt, dtype=np.int64)
    seg_pos = np.asarray(seg_pos, dtype=np.int64)
    pred_size = np.asarray(pred_size, dtype=np.float64).reshape(-1, 3)
    U, S = seg_cnt.shape
    status = 0
    survive = []
    for u in range(U):
        if seg_pos[u].sum() <= 0:
            continue
        w = float(pred_size[u, 1])
        if not (w > 0.0 and np.isfinite(w)):
            status |= ST_WIDTH
            continue
        if any(windows(w, float(s)) > float(lp) for s, lp in zip(strides, lpad)):
            status |= ST_WIDE
            continue
        survive.append(u)
    held = np.asarray(survive[:B], dtype=np.int64)
    n = len(held)
    cnt = np.zeros_like(seg_cnt)
    cnt[held] = np.maximum(seg_cnt[held], 0)
    raw = np.concatenate([[0], np.cumsum(cnt.reshape(-1))]).astype(np.int64)
    seg_off = np.minimum(raw, capacity)
    slot_unit = np.full(B, U, dtype=np.int32)
    slot_unit[:n] = held
    off = np.full(B + 1, capacity, dtype=np.int64)
    off[:n] = seg_off[held * S]
    off[B] = seg_off[-1]
    counts = np.zeros(B, dtype=np.int64)
    counts[:n] = seg_off[(held + 1) * S] - seg_off[held * S]
    status |= (ST_FEW if len(survive) < B else 0) | (ST_TRUNC if raw[-1] > capacity else 0)
    return slot_unit, n, seg_off, off, counts, status
