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
//   fcn_frustum_train_plan     ONE workgroup between the two: the reject rule per box, the first B survivors IN BOX ORDER -> slots,
//                              the exclusive prefix sum of the slot-holding boxes' segment counts (int64, clamped to the capacity
//                              of the point buffer) and the slots' row offsets.  Order-preserving scans, no atomics on the data:
//                              the result does not depend on scheduling.
// Status bits (one int32 word, OR-ed, never cleared here): FP_ST_FEW fewer than B survivors; FP_ST_TRUNC rows dropped because the
// total exceeds the capacity; FP_ST_PERTURB a box without a valid draw in FP_ATTEMPTS attempts or with its frame out of range
// (bit 0 is DeviceDraws': a sample nothing could be drawn from).
// The plan is latency-bound (one workgroup, D * S int32): every thread owns a contiguous run of the flattened segments, sums it,
// one scan over the 256 run totals (a wave scan by __shfl_up, then the four wave totals through LDS) gives its base, and it walks
// the run again to write.
#pragma once
#include "draws.h"
#include "frustum_label.h"

#define FP_T 256
#define FP_WAVES (FP_T / 64)
#define FP_ATTEMPTS 32                 // the retry bound of fcn_box2d_perturb (the reference loops for ever)
#define FP_MAX_D 2048                  // boxes (and slots) of one plan: their slots live in LDS
#define FP_MAX_SEGS 65536              // D * S of one plan: 256 segments per thread
#define FP_ST_FEW 2                    // bit 1
#define FP_ST_TRUNC 4                  // bit 2
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
        const uint64_t step = (uint64_t)a.state[0];
        const uint32_t c2 = (uint32_t)step, c3 = ((uint32_t)(step >> 32) << 2) | 3u;
        const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
        const double scale = 1.0 / 9007199254740992.0;     // 2^-53
        const double r = a.r;
        for (int t = 0; t < FP_ATTEMPTS && !done; ++t) {
            uint32_t w0[4], w1[4];
            draw_philox(2u * (uint32_t)t, (uint32_t)d, c2, c3, k0, k1, w0);
            draw_philox(2u * (uint32_t)t + 1u, (uint32_t)d, c2, c3, k0, k1, w1);
            const double u0 = draw_u53(w0[0], w0[1]) * scale, u1 = draw_u53(w0[2], w0[3]) * scale;
            const double u2 = draw_u53(w1[0], w1[1]) * scale, u3 = draw_u53(w1[2], w1[3]) * scale;
            const double cx2 = cx + (w * r) * (u0 * 2.0 - 1.0);
            const double cy2 = cy + (h * r) * (u1 * 2.0 - 1.0);
            const double h2 = h * ((1.0 + (u2 * 2.0) * r) - r);
            const double w2 = w * ((1.0 + (u3 * 2.0) * r) - r);
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
    const int32_t *scnt, *spos;        // (D,S)
    const double *gt2d;                // (D,4)
    double min_h;
    int D, S, B;
    int64_t cap;
    int32_t *slot_box;                 // (B)
    int64_t *soff;                     // (D*S+1)
    int64_t *off;                      // (B+1)
    int32_t *n_kept;                   // (1)
    int32_t *status;
};

// exclusive scan of one value per thread over the workgroup, in thread order; total: the sum, in every thread
__device__ __forceinline__ int64_t fp_block_exscan(int64_t v, int64_t *swave, int tid, int64_t &total)
{
    const int lane = tid & 63, wave = tid >> 6;
    int64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                        // (the previous scan's readers are done with swave)
    if (lane == 63) swave[wave] = inc;
    __syncthreads();
    int64_t base = 0;
    total = 0;
    for (int w = 0; w < FP_WAVES; ++w) {
        if (w < wave) base += swave[w];
        total += swave[w];
    }
    return base + (inc - v);
}

__global__ __launch_bounds__(FP_T) void fp_plan_kernel(FpPlanArgs a)
{
    __shared__ int32_t sslot[FP_MAX_D];                     // box -> its slot, -1 without one
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x, D = a.D, S = a.S, B = a.B;
    // ---- the reject rule and the slots: thread tid owns boxes [tid * EB, (tid + 1) * EB)
    const int EB = (D + FP_T - 1) / FP_T;                   // <= FP_MAX_D / FP_T = 8
    const int d0 = tid * EB < D ? tid * EB : D, d1 = d0 + EB < D ? d0 + EB : D;
    unsigned keep = 0;
    for (int d = d0; d < d1; ++d) {
        int64_t pos = 0;
        for (int s = 0; s < S; ++s) pos += a.spos[(int64_t)d * S + s];
        const double *q = a.gt2d + (int64_t)d * 4;
        if (!(q[3] - q[1] < a.min_h) && pos > 0) keep |= 1u << (d - d0);
    }
    int64_t survivors;
    int64_t rank = fp_block_exscan((int64_t)__popc(keep), swave, tid, survivors);
    for (int d = d0; d < d1; ++d) {
        int slot = -1;
        if (keep & (1u << (d - d0))) {
            if (rank < B) { slot = (int)rank; a.slot_box[slot] = d; }
            rank += 1;
        }
        sslot[d] = slot;
    }
    const int n = survivors < B ? (int)survivors : B;
    for (int i = n + tid; i < B; i += FP_T) a.slot_box[i] = 0;
    __syncthreads();
    // ---- the segment offsets: thread tid owns the flattened segments [tid * E, (tid + 1) * E)
    const int M = D * S;                                    // <= FP_MAX_SEGS
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
        if (slot >= 0 && i % S == 0) a.off[slot] = at;
        const int c = a.scnt[i];
        if (slot >= 0 && c > 0) run += c;
    }
    const int64_t end = total < a.cap ? total : a.cap;
    for (int i = n + tid; i <= B; i += FP_T) a.off[i] = end;
    if (tid == 0) {
        a.soff[M] = end;
        a.n_kept[0] = n;
        const int st = (survivors < B ? FP_ST_FEW : 0) | (total > a.cap ? FP_ST_TRUNC : 0);
        if (st) atomicOr(a.status, st);
    }
}

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
    if (advance) {                                          // state[0] + 1, in stream order behind every lane's read
        hipLaunchKernelGGL(draw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (int64_t *)state);
        FCN_CHECK_LAUNCH();
    }
    return 0;
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
    if (D < 0 || S < 1 || B < 1 || capacity < 0) return FCN_E_BADARG;
    if (D > FP_MAX_D || B > FP_MAX_D || (int64_t)D * S > FP_MAX_SEGS) return FCN_E_LIMIT;
    FpPlanArgs a;
    a.scnt = seg_cnt; a.spos = seg_pos; a.gt2d = gt_box2d; a.min_h = min_box_height; a.D = D; a.S = S; a.B = B; a.cap = capacity;
    a.slot_box = slot_box; a.soff = seg_off; a.off = off; a.n_kept = n_kept; a.status = status;
    hipLaunchKernelGGL(fp_plan_kernel, dim3(1), dim3(FP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}
