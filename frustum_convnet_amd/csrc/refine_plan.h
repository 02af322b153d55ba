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
//   fcn_refine_train_plan      the plan skeleton of slot_plan.h with RpPlan<false> between count and fill: a unit is kept when it
//                              has a positive and the fixed window counts can hold its predicted width; off and the STORED row
//                              counts per slot.
// Status bits (one int32 word, OR-ed, never cleared here): FP_ST_FEW fewer than B survivors; FP_ST_TRUNC rows dropped because the
// total exceeds the capacity; RP_ST_WIDE a unit with positives whose predicted width needs more windows than lpad on some stride;
// RP_ST_WIDTH a unit with positives whose predicted width is not a positive finite number (bit 0 is DeviceDraws').
// RpPlan<true> is the plan of the inference link (cascade_plan.h): the same rule, told that too few survivors is the normal case
// there and too many the one to report (RP_ST_MANY instead of FP_ST_FEW).
#pragma once
#include "draws.h"
#include "refine_label.h"
#include "slot_plan.h"

#define RP_ST_WIDE 32                  // bit 5
#define RP_ST_WIDTH 64                 // bit 6

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
    double v[8];
    draw_uniforms<4>(draw_key(a.state, a.seed, 3u), 0u, (uint32_t)u, v);
    double *q = a.jitter + (int64_t)u * 7;
#pragma unroll
    for (int j = 0; j < 7; ++j) q[j] = v[j];
}

struct RpPlanArgs {
    SlArgs c;
    const int32_t *spos;               // (U,S)
    const double *psize;               // (U,3): l, w, h of the jittered enlarged box; row u is read only when unit u has a positive
    double stride[4];
    int32_t lpad[4];
};

template <bool DETECT> struct RpPlan {
    using Args = RpPlanArgs;
    static constexpr bool SLOTS = true, COUNTS = true, MANY = DETECT;
    __device__ static int live(const Args &a, int, int &) { return a.c.U; }
    __device__ static bool keep(const Args &a, int u, int &st)
    {
        if (!(sl_unit_sum(a.spos, u, a.c.S) > 0)) return false;     // the reject rule; an unmatched candidate's units count nothing
        const double w = a.psize[3 * (int64_t)u + 1];
        if (!(w > 0.0 && w <= 1.7976931348623157e308)) { st |= RP_ST_WIDTH; return false; }     // positive and finite (DBL_MAX)
        const double z1 = -w / 2.0, z2 = w / 2.0;           // as prepare_inputs_refine_kernel writes it; compared in fp64
        bool fits = true;
        for (int s = 0; s < 4; ++s)
            if (ceil((z2 - z1) / a.stride[s]) > (double)a.lpad[s]) fits = false;
        if (!fits) st |= RP_ST_WIDE;
        return fits;
    }
    __device__ static int filler(const Args &a) { return a.c.U; }   // the spare entry of the caller's per-unit tables
};

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
    return draw_advance(advance, state, (hipStream_t)stream);
}

// the argument checks and the launch fcn_refine_train_plan and fcn_refine_detect_plan (cascade_plan.h) share
template <bool DETECT>
static inline int rp_plan_launch(const int32_t *seg_cnt, const int32_t *seg_pos, const double *pred_size, const double *stride,
                                 const int32_t *lpad, int U, int S, int B, int64_t capacity, int32_t *slot_unit, int32_t *n_kept,
                                 int64_t *seg_off, int64_t *off, int64_t *counts, int32_t *status, void *stream)
{
    if (!seg_cnt || !seg_pos || !pred_size || !stride || !lpad || !slot_unit || !n_kept || !seg_off || !off || !counts || !status)
        return FCN_E_BADARG;
    for (int s = 0; s < 4; ++s)
        if (lpad[s] < 1 || !(stride[s] > 0.0)) return FCN_E_BADARG;
    FCN_TRY(sl_sizes(U, S, B, capacity));
    RpPlanArgs a;
    a.c = SlArgs{seg_cnt, U, S, B, capacity, slot_unit, n_kept, seg_off, off, counts, status};
    a.spos = seg_pos; a.psize = pred_size;
    for (int s = 0; s < 4; ++s) { a.stride[s] = stride[s]; a.lpad[s] = lpad[s]; }
    return sl_launch(sl_plan_kernel<RpPlan<DETECT>>, a, stream);
}

extern "C" int fcn_refine_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, const double *pred_size, const double *stride,
                                     const int32_t *lpad, int U, int S, int B, int64_t capacity, int32_t *slot_unit,
                                     int32_t *n_kept, int64_t *seg_off, int64_t *off, int64_t *counts, int32_t *status,
                                     void *stream)
{
    return rp_plan_launch<false>(seg_cnt, seg_pos, pred_size, stride, lpad, U, S, B, capacity, slot_unit, n_kept, seg_off, off, counts,
                                 status, stream);
}
