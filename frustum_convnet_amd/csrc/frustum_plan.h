// The first stage's training input with NO host read between its launches: what frustum.perturb_boxes2d, the host block of
// frustum.frustum_training_candidates (reject rule, kept list, prefix sum of the segment counts) and the host look-ups of
// InputBuilder.build_device_train do per step, as launches that read nothing back -- a fixed batch of B slots, capturable into a
// hipGraph (INTEGRATION.md "Capturable first-stage training input" states the contract bit for bit; tests/frustum_plan_ref.py
// restates it in numpy):
//   fcn_box2d_perturb          kitti/prepare_data.py::random_shift_box2d (:55-77) for D boxes, one lane per box, on the counter-based
//                              stream of draws.h (tag 3, the one tag fcn_draw_batch leaves free), with a BOUNDED retry;
//   fcn_frustum_train_count    the count / fill of frustum_label.h (seg_compact.h with FlSelect), launched without a read-back: the
//   fcn_frustum_train_fill     kernels skip a box whose frame is out of range; "no frame longer than S * FS_SEG rows" is the caller's
//                              duty (checked once, where the frames are made resident);
//   fcn_frustum_train_plan     the plan skeleton of slot_plan.h with FpPlan between the two: a box is kept when its label box is at
//                              least min_box_height high and it has a positive; off[slot] alone, no stored counts.
// Status bits (one int32 word, OR-ed, never cleared here): FP_ST_FEW fewer than B survivors; FP_ST_TRUNC rows dropped because the
// total exceeds the capacity; FP_ST_PERTURB a box without a valid draw in FP_ATTEMPTS attempts or with its frame out of range
// (bit 0 is DeviceDraws': a sample nothing could be drawn from).
#pragma once
#include "draws.h"
#include "frustum_label.h"
#include "slot_plan.h"

#define FP_ATTEMPTS 32                 // the retry bound of fcn_box2d_perturb (the reference loops for ever)
#define FP_ST_PERTURB 16               // bit 4

struct FpPerturbArgs {
    const double *boxes;               // (D,4)
    const int32_t *bframe;             // (D)
    const double *wh;                  // (F,2)
    int D, F;
    double r;
    uint64_t seed;
    const int64_t *state;
    double *out;                       // (D,4)
    int32_t *status;
};

// Arithmetic exactly as frustum.perturb_boxes2d writes it, fp64, every operation on its own (-ffp-contract=off): bit-exact
// against numpy given the same uniforms.
__global__ __launch_bounds__(FP_T) void fp_perturb_kernel(FpPerturbArgs a)
{
    const int d = blockIdx.x * FP_T + threadIdx.x;
    if (d >= a.D) return;
    const double *q = a.boxes + (int64_t)d * 4;
    const double xmin = q[0], ymin = q[1], xmax = q[2], ymax = q[3];
    double *o = a.out + (int64_t)d * 4;
    const int f = a.bframe[d];
    bool done = false;
    if (f >= 0 && f < a.F) {
        const double W = a.wh[2 * (int64_t)f], H = a.wh[2 * (int64_t)f + 1];
        const double h = ymax - ymin, w = xmax - xmin;
        const double cx = (xmin + xmax) / 2.0, cy = (ymin + ymax) / 2.0;
        const DrawKey key = draw_key(a.state, a.seed, 3u);
        const double r = a.r;
        for (int t = 0; t < FP_ATTEMPTS && !done; ++t) {
            double u[4];
            draw_uniforms<2>(key, 2u * (uint32_t)t, (uint32_t)d, u);
            const double cx2 = cx + (w * r) * (u[0] * 2.0 - 1.0);
            const double cy2 = cy + (h * r) * (u[1] * 2.0 - 1.0);
            const double h2 = h * ((1.0 + (u[2] * 2.0) * r) - r);
            const double w2 = w * ((1.0 + (u[3] * 2.0) * r) - r);
            const double x0 = fmin(fmax(cx2 - w2 / 2.0, 0.0), W - 1.0), x1 = fmin(fmax(cx2 + w2 / 2.0, 0.0), W - 1.0);
            const double y0 = fmin(fmax(cy2 - h2 / 2.0, 0.0), H - 1.0), y1 = fmin(fmax(cy2 + h2 / 2.0, 0.0), H - 1.0);
            if (x0 < x1 && y0 < y1) {
                o[0] = x0; o[1] = y0; o[2] = x1; o[3] = y1;
                done = true;
            }
        }
    }
    if (!done) {                                            // never silent, never unwritten: the input box and the flag
        o[0] = xmin; o[1] = ymin; o[2] = xmax; o[3] = ymax;
        atomicOr(a.status, FP_ST_PERTURB);
    }
}

struct FpPlanArgs {
    SlArgs c;
    const int32_t *spos;               // (D,S)
    const double *gt2d;                // (D,4)
    double min_h;
};

struct FpPlan {
    using Args = FpPlanArgs;
    static constexpr bool SLOTS = true, COUNTS = false, MANY = false;
    __device__ static int live(const Args &a, int, int &) { return a.c.U; }
    __device__ static bool keep(const Args &a, int d, int &)
    {
        const int64_t pos = sl_unit_sum(a.spos, d, a.c.S);
        const double *q = a.gt2d + (int64_t)d * 4;
        return !(q[3] - q[1] < a.min_h) && pos > 0;
    }
    __device__ static int filler(const Args &) { return 0; }   // an empty slot repeats box 0's labels over no rows
};

extern "C" int fcn_box2d_perturb_limits(int *attempts)
{
    if (!attempts) return FCN_E_BADARG;
    *attempts = FP_ATTEMPTS;
    return 0;
}

extern "C" int fcn_frustum_train_plan_limits(int *max_d, int *max_segs)
{
    if (!max_d || !max_segs) return FCN_E_BADARG;
    *max_d = FP_MAX_D;
    *max_segs = FP_MAX_SEGS;
    return 0;
}

extern "C" int fcn_box2d_perturb(const double *boxes, const int32_t *box_frame, const double *img_wh, int D, int F,
                                 double shift_ratio, uint64_t seed, const int64_t *state, int advance, double *out,
                                 int32_t *status, void *stream)
{
    if (!boxes || !box_frame || !img_wh || !state || !out || !status) return FCN_E_BADARG;
    if (D < 0 || F < 0 || !(shift_ratio >= 0.0 && shift_ratio < 1.0)) return FCN_E_BADARG;
    if (D > 0) {
        FpPerturbArgs a;
        a.boxes = boxes; a.bframe = box_frame; a.wh = img_wh; a.D = D; a.F = F; a.r = shift_ratio; a.seed = seed; a.state = state;
        a.out = out; a.status = status;
        hipLaunchKernelGGL(fp_perturb_kernel, dim3((D + FP_T - 1) / FP_T), dim3(FP_T), 0, (hipStream_t)stream, a);
        FCN_CHECK_LAUNCH();
    }
    return draw_advance(advance, state, (hipStream_t)stream);
}

extern "C" int fcn_frustum_train_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                       const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                       const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                       const double *gt_box3d, double *box2d, double *frustum_angle, int32_t *seg_cnt,
                                       int32_t *seg_pos, double *corners, void *stream)
{
    return fl_count_launch(frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, D, S, clip_boxes, clip_distance,
                           gt_box3d, box2d, frustum_angle, seg_cnt, seg_pos, corners, stream, false);
}

extern "C" int fcn_frustum_train_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                      const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                      const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                      const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg,
                                      void *stream)
{
    return fl_fill_launch(frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, D, S, clip_boxes, clip_distance,
                          gt_box3d, seg_off, out_pts, out_seg, stream, false);
}

extern "C" int fcn_frustum_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, const double *gt_box2d, double min_box_height,
                                      int D, int S, int B, int64_t capacity, int32_t *slot_box, int64_t *seg_off, int64_t *off,
                                      int32_t *n_kept, int32_t *status, void *stream)
{
    if (!seg_cnt || !seg_pos || !gt_box2d || !slot_box || !seg_off || !off || !n_kept || !status) return FCN_E_BADARG;
    FCN_TRY(sl_sizes(D, S, B, capacity));
    FpPlanArgs a;
    a.c = SlArgs{seg_cnt, D, S, B, capacity, slot_box, n_kept, seg_off, off, nullptr, status};
    a.spos = seg_pos; a.gt2d = gt_box2d; a.min_h = min_box_height;
    return sl_launch(sl_plan_kernel<FpPlan>, a, stream);
}
