// The refinement stage's training input with NO host read between its launches: what cascade.match_detections, draw_box3d_jitter,
// the host block of cascade.refine_training_candidates (reject rule, kept list, prefix sum of the segment counts) and the host
// look-ups of RefineInputBuilder.build_device_train do per step, as launches that read nothing back -- a fixed batch of B slots at
// fixed window counts, capturable into a hipGraph (INTEGRATION.md "Capturable refine-stage training input" states the contract bit
// for bit; tests/refine_plan_ref.py restates it in numpy):
//   fcn_refine_train_match     rl_match_kernel and the count / fill of refine_label.h (seg_compact.h with RlSelect), launched without
//   fcn_refine_train_count     a read-back of the index lists: the kernels skip a candidate whose row, frame or label is
//   fcn_refine_train_fill      out of range (it is no longer REPORTED); "no frame longer than S * FS_SEG rows" is the caller's duty
//                              (checked once, where the frames are made resident);
//   fcn_box3d_jitter_draw      the (D, A, 7) uniforms rl_jitter reads, one lane per unit, on the counter-based stream of draws.h
//                              (tag 3, as fcn_box2d_perturb uses it: the two never share a key);
//   fcn_refine_train_plan      ONE workgroup between count and fill: the reject rule per unit, the units the fixed window counts
//                              cannot hold, the first B survivors IN UNIT ORDER -> slots, the exclusive prefix sum of the
//                              slot-holding units' segment counts (int64, clamped to the capacity of the point buffer), the slots'
//                              row offsets and STORED row counts.  fp_block_exscan and the ownership scheme of fp_plan_kernel
//                              (frustum_plan.h): order-preserving scans, no atomics on the data, nothing depends on scheduling.
// Status bits (one int32 word, OR-ed, never cleared here): FP_ST_FEW fewer than B survivors; FP_ST_TRUNC rows dropped because the
// total exceeds the capacity; RP_ST_WIDE a unit with positives whose predicted width needs more windows than lpad on some stride;
// RP_ST_WIDTH a unit with positives whose predicted width is not a positive finite number (bit 0 is DeviceDraws').
// rp_plan_kernel<true> is the plan of the inference link (cascade_plan.h): the same kernel, told that too few survivors is the normal
// case there and too many the one to report (RP_ST_MANY instead of FP_ST_FEW).
#pragma once
#include "draws.h"
#include "refine_label.h"
#include "frustum_plan.h"

#define RP_ST_WIDE 32                  // bit 5
#define RP_ST_WIDTH 64                 // bit 6
#define RP_ST_MANY 256                 // bit 8: more survivors than slots (the inference link alone)

struct RpJitterArgs {
    int U;
    uint64_t seed;
    const int64_t *state;
    double *jitter;                    // (U,7)
};

// unit u: blocks 0..3 of tag 3 = words w0..w15; uniform j = u53(w[2j], w[2j+1]) * 2^-53, j = 0..6 (l, h, w, cx, cy, cz, angle)
__global__ __launch_bounds__(FP_T) void rp_jitter_kernel(RpJitterArgs a)
{
    const int u = blockIdx.x * FP_T + threadIdx.x;
    if (u >= a.U) return;
    const uint64_t step = (uint64_t)a.state[0];
    const uint32_t c2 = (uint32_t)step, c3 = ((uint32_t)(step >> 32) << 2) | 3u;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const double scale = 1.0 / 9007199254740992.0;          // 2^-53
    uint32_t w[16];
#pragma unroll
    for (int blk = 0; blk < 4; ++blk) {
        uint32_t o[4];
        draw_philox((uint32_t)blk, (uint32_t)u, c2, c3, k0, k1, o);
        w[4 * blk] = o[0]; w[4 * blk + 1] = o[1]; w[4 * blk + 2] = o[2]; w[4 * blk + 3] = o[3];
    }
    double *q = a.jitter + (int64_t)u * 7;
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = draw_u53(w[2 * j], w[2 * j + 1]) * scale;
}

struct RpPlanArgs {
    const int32_t *scnt, *spos;        // (U,S)
    const double *psize;               // (U,3): l, w, h of the jittered enlarged box; row u is read only when unit u has a positive
    double stride[4];
    int32_t lpad[4];
    int U, S, B;
    int64_t cap;
    int32_t *slot_unit;                // (B)
    int32_t *n_kept;                   // (1)
    int64_t *soff;                     // (U*S+1)
    int64_t *off;                      // (B+1)
    int64_t *counts;                   // (B)
    int32_t *status;
};

template <bool DETECT> __global__ __launch_bounds__(FP_T) void rp_plan_kernel(RpPlanArgs a)
{
    __shared__ int32_t sslot[FP_MAX_D];                     // unit -> its slot, -1 without one
    __shared__ int64_t slo[FP_MAX_D], shi[FP_MAX_D];        // slot -> its clamped first row and the clamped end of its rows
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x, U = a.U, S = a.S, B = a.B;
    // ---- the reject rule, the widths and the slots: thread tid owns units [tid * EB, (tid + 1) * EB)
    const int EB = (U + FP_T - 1) / FP_T;                   // <= FP_MAX_D / FP_T = 8
    const int u0 = tid * EB < U ? tid * EB : U, u1 = u0 + EB < U ? u0 + EB : U;
    unsigned keep = 0;
    int st = 0;
    for (int u = u0; u < u1; ++u) {
        int64_t pos = 0;
        for (int s = 0; s < S; ++s) pos += a.spos[(int64_t)u * S + s];
        if (!(pos > 0)) continue;                           // the reject rule; an unmatched candidate's units count nothing
        const double w = a.psize[3 * (int64_t)u + 1];
        if (!(w > 0.0 && w <= 1.7976931348623157e308)) { st |= RP_ST_WIDTH; continue; }        // positive and finite (DBL_MAX)
        const double z1 = -w / 2.0, z2 = w / 2.0;           // as prepare_inputs_refine_kernel writes it; compared in fp64
        bool fits = true;
        for (int s = 0; s < 4; ++s)
            if (ceil((z2 - z1) / a.stride[s]) > (double)a.lpad[s]) fits = false;
        if (!fits) { st |= RP_ST_WIDE; continue; }
        keep |= 1u << (u - u0);
    }
    int64_t survivors;
    int64_t rank = fp_block_exscan((int64_t)__popc(keep), swave, tid, survivors);
    for (int u = u0; u < u1; ++u) {
        int slot = -1;
        if (keep & (1u << (u - u0))) {
            if (rank < B) { slot = (int)rank; a.slot_unit[slot] = u; }
            rank += 1;
        }
        sslot[u] = slot;
    }
    const int n = survivors < B ? (int)survivors : B;
    for (int i = n + tid; i < B; i += FP_T) a.slot_unit[i] = U;            // the spare entry of the caller's per-unit tables
    __syncthreads();
    // ---- the segment offsets: thread tid owns the flattened segments [tid * E, (tid + 1) * E)
    const int M = U * S;                                    // <= FP_MAX_SEGS
    const int E = (M + FP_T - 1) / FP_T;
    const int i0 = tid * E < M ? tid * E : M, i1 = i0 + E < M ? i0 + E : M;
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) {
        const int c = a.scnt[i];
        if (sslot[i / S] >= 0 && c > 0) sum += c;
    }
    int64_t total;
    int64_t run = fp_block_exscan(sum, swave, tid, total);
    for (int i = i0; i < i1; ++i) {
        const int slot = sslot[i / S];
        const int64_t at = run < a.cap ? run : a.cap;
        a.soff[i] = at;
        if (slot >= 0 && i % S == 0) slo[slot] = at;
        const int c = a.scnt[i];
        if (slot >= 0 && c > 0) run += c;
        if (slot >= 0 && i % S == S - 1) shi[slot] = run < a.cap ? run : a.cap;
    }
    __syncthreads();
    // ---- per slot: its first row and its STORED rows; an empty slot reads the spare row behind the buffer and holds nothing
    const int64_t end = total < a.cap ? total : a.cap;
    for (int i = tid; i < B; i += FP_T) {
        a.off[i] = i < n ? slo[i] : a.cap;
        a.counts[i] = i < n ? shi[i] - slo[i] : 0;
    }
    if (st) atomicOr(a.status, st);
    if (tid == 0) {
        a.off[B] = end;
        a.soff[M] = end;
        a.n_kept[0] = n;
        const int few = DETECT ? (survivors > B ? RP_ST_MANY : 0) : (survivors < B ? FP_ST_FEW : 0);
        const int st2 = few | (total > a.cap ? FP_ST_TRUNC : 0);
        if (st2) atomicOr(a.status, st2);
    }
}

extern "C" int fcn_refine_train_plan_limits(int *max_u, int *max_segs)
{
    if (!max_u || !max_segs) return FCN_E_BADARG;
    *max_u = FP_MAX_D;
    *max_segs = FP_MAX_SEGS;
    return 0;
}

extern "C" int fcn_refine_train_match(const float *dets, int R, const int32_t *cand_row, const int32_t *cand_frame, int D,
                                      const double *gt_box3d, int G, const int64_t *gt_off, int F, double thresh, int32_t *gt_idx,
                                      float *best_iou, void *stream)
{
    return rl_match_launch(dets, R, cand_row, cand_frame, D, gt_box3d, G, gt_off, F, thresh, gt_idx, best_iou, stream, false);
}

extern "C" int fcn_refine_train_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                      int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                      const int32_t *cand_gt, const double *gt_box3d, int G, int A, const double *jitter,
                                      double shift_ratio, int S, int32_t *seg_cnt, int32_t *seg_pos, double *pred_corners,
                                      double *pred_angle, double *pred_size, double *gt_corners, double *gt_heading,
                                      double *gt_size, void *stream)
{
    return rl_count_launch(frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, D, ratio, cand_gt, gt_box3d, G, A, jitter,
                           shift_ratio, S, seg_cnt, seg_pos, pred_corners, pred_angle, pred_size, gt_corners, gt_heading, gt_size,
                           stream, false);
}

extern "C" int fcn_refine_train_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                     int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                     const int32_t *cand_gt, const double *gt_box3d, int G, int A, const double *jitter,
                                     double shift_ratio, int S, const int64_t *seg_off, float *out_pts, void *stream)
{
    return rl_fill_launch(frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, D, ratio, cand_gt, gt_box3d, G, A, jitter,
                          shift_ratio, S, seg_off, out_pts, stream, false);
}

extern "C" int fcn_box3d_jitter_draw(int D, int A, uint64_t seed, const int64_t *state, int advance, double *jitter, void *stream)
{
    if (!state || !jitter || D < 0 || A < 1 || A > RL_MAX_A) return FCN_E_BADARG;
    if ((int64_t)D * A > FS_MAX_D) return FCN_E_LIMIT;
    if (D > 0) {
        RpJitterArgs a;
        a.U = D * A; a.seed = seed; a.state = state; a.jitter = jitter;
        hipLaunchKernelGGL(rp_jitter_kernel, dim3((a.U + FP_T - 1) / FP_T), dim3(FP_T), 0, (hipStream_t)stream, a);
        FCN_CHECK_LAUNCH();
    }
    if (advance) {                                          // state[0] + 1, in stream order behind every lane's read
        hipLaunchKernelGGL(draw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int64_t *)state);
        FCN_CHECK_LAUNCH();
    }
    return 0;
}

// the argument checks and the launch fcn_refine_train_plan and fcn_refine_detect_plan (cascade_plan.h) share
template <bool DETECT>
static inline int rp_plan_launch(const int32_t *seg_cnt, const int32_t *seg_pos, const double *pred_size, const double *stride,
                                 const int32_t *lpad, int U, int S, int B, int64_t capacity, int32_t *slot_unit, int32_t *n_kept,
                                 int64_t *seg_off, int64_t *off, int64_t *counts, int32_t *status, void *stream)
{
    if (!seg_cnt || !seg_pos || !pred_size || !stride || !lpad || !slot_unit || !n_kept || !seg_off || !off || !counts || !status)
        return FCN_E_BADARG;
    if (U < 0 || S < 1 || B < 1 || capacity < 0) return FCN_E_BADARG;
    for (int s = 0; s < 4; ++s)
        if (lpad[s] < 1 || !(stride[s] > 0.0)) return FCN_E_BADARG;
    if (U > FP_MAX_D || B > FP_MAX_D || (int64_t)U * S > FP_MAX_SEGS) return FCN_E_LIMIT;
    RpPlanArgs a;
    a.scnt = seg_cnt; a.spos = seg_pos; a.psize = pred_size;
    for (int s = 0; s < 4; ++s) { a.stride[s] = stride[s]; a.lpad[s] = lpad[s]; }
    a.U = U; a.S = S; a.B = B; a.cap = capacity;
    a.slot_unit = slot_unit; a.n_kept = n_kept; a.soff = seg_off; a.off = off; a.counts = counts; a.status = status;
    hipLaunchKernelGGL(rp_plan_kernel<DETECT>, dim3(1), dim3(FP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

extern "C" int fcn_refine_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, const double *pred_size, const double *stride,
                                     const int32_t *lpad, int U, int S, int B, int64_t capacity, int32_t *slot_unit,
                                     int32_t *n_kept, int64_t *seg_off, int64_t *off, int64_t *counts, int32_t *status,
                                     void *stream)
{
    return rp_plan_launch<false>(seg_cnt, seg_pos, pred_size, stride, lpad, U, S, B, capacity, slot_unit, n_kept, seg_off, off, counts,
                                 status, stream);
}
