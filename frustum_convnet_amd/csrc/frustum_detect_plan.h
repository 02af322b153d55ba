// The front of two-stage INFERENCE with NO host read between its launches: what frustum.frustum_candidates (two range-checking
// read-backs, the D * S segment counts read for the prefix sum), InputBuilder.build_device (the D clipped boxes read for the skip
// rule, the kept list) and frustum.image_fov_points (the same again for the second stage's search set) do on the host, as launches
// that read nothing back -- a table of at most D 2-D detections, a fixed first-stage batch of B1 slots, capturable into a hipGraph
// (INTEGRATION.md "Capturable inference front" states the contract bit for bit; tests/frustum_detect_plan_ref.py restates it in
// numpy):
//   fcn_frustum_detect_count   the count / fill of frustum_select.h (seg_compact.h with the FsGeo policy, the row loop unchanged),
//   fcn_frustum_detect_fill    launched without a read-back: the kernels skip a box whose frame is out of range and a box at or
//                              beyond the device-resident box count n_boxes (its counts are zero, nothing of it is read or stored);
//                              "no frame longer than S * FS_SEG rows" is the caller's duty (checked once, where the frames are made
//                              resident);
//   fcn_frustum_detect_plan    ONE workgroup between the two: InputBuilder.build_device's skip rule per box in its own fp64
//                              expression, the first B1 survivors IN BOX ORDER -> slots, the exclusive prefix sum of the
//                              slot-holding boxes' segment counts (int64, clamped to the capacity of the point buffer), the slots'
//                              row offsets and STORED row counts.  fp_block_exscan and the ownership scheme of fp_plan_kernel
//                              (frustum_plan.h): order-preserving scans, no atomics on the data, nothing depends on scheduling;
//   fcn_frustum_fov_plan       the same kernel under a template parameter for the whole-image selection of the second stage's search
//                              set (one box (0, 0, W, H) per frame, no clipping): no reject rule and no slots, the prefix sum of the
//                              (F, S) counts and every S-th entry of it as the frames' offsets.  The capacity handed in is the row
//                              count of the frame buffer: a subset of a frame is no longer than the frame, so the clamp never cuts
//                              -- it is kept because it is what bounds the fill's stores whatever the counts hold.
// Status bits of the plan (one int32 word, OR-ed, never cleared here): FP_ST_TRUNC rows dropped because the total exceeds the
// capacity; RP_ST_MANY more survivors than slots; FD_ST_RANGE n_boxes outside [0, D] (taken as 0 / D) or a box below n_boxes whose
// frame is outside [0, F) (the box is ignored, never dereferenced).  Fewer survivors than slots is the normal case at inference: no
// bit (bit 0 is DeviceDraws': an empty slot has no row to draw from).
#pragma once
#include "frustum_select.h"
#include "refine_plan.h"

#define FD_ST_RANGE 1024               // bit 10

struct FdArgs {
    ScArgs c;
    FsGeo g;
    const int32_t *nbox;               // (1) the boxes of the table that are live
};

// FsSelect behind the device-resident box count: the geometry, the predicate and the header are frustum_select.h's
struct FdSelect : FsSelect {
    using Args = FdArgs;
    __device__ __forceinline__ bool setup(const FdArgs &a, int d, int64_t &p0, int64_t &m)
    {
        return d < a.nbox[0] && fs_setup(a.g, d, b, p0, m);
    }
    __device__ __forceinline__ void header(const FdArgs &a, int d, int tid) const { box_angle(a.g, d, tid); }
};

struct FdPlanArgs {
    const int32_t *scnt;               // (U,S)
    const double *box2d;               // (U,4) the clipped boxes the count wrote; row d is read only when box d is live
    const int32_t *bframe;             // (U)
    const int32_t *nbox;               // (1)
    double min_h, min_pts;
    int U, S, B, F;
    int64_t cap;
    int32_t *slot_box;                 // (B)
    int32_t *n_kept;                   // (1)
    int64_t *soff;                     // (U*S+1)
    int64_t *off;                      // (B+1); FOV: (U+1)
    int64_t *counts;                   // (B)
    int32_t *status;
};

// FOV: every unit holds its rows, off[u] is unit u's first row -- no rule, no slots, no status
template <bool FOV> __global__ __launch_bounds__(FP_T) void fd_plan_kernel(FdPlanArgs a)
{
    __shared__ int32_t sslot[FOV ? 1 : FP_MAX_D];           // box -> its slot, -1 without one
    __shared__ int64_t slo[FOV ? 1 : FP_MAX_D], shi[FOV ? 1 : FP_MAX_D];       // slot -> its clamped first row and clamped end
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x, U = a.U, S = a.S, B = a.B;
    int n = 0, st = 0;
    int64_t survivors = 0;
    if constexpr (!FOV) {
        // ---- the skip rule and the slots: thread tid owns boxes [tid * EB, (tid + 1) * EB)
        int nb = a.nbox[0];
        if (nb < 0 || nb > U) {
            if (tid == 0) st |= FD_ST_RANGE;
            nb = nb < 0 ? 0 : U;
        }
        const int EB = (U + FP_T - 1) / FP_T;               // <= FP_MAX_D / FP_T = 8
        const int u0 = tid * EB < U ? tid * EB : U, u1 = u0 + EB < U ? u0 + EB : U;
        unsigned keep = 0;
        for (int u = u0; u < u1 && u < nb; ++u) {
            const int f = a.bframe[u];
            if (f < 0 || f >= a.F) { st |= FD_ST_RANGE; continue; }
            int64_t cnt = 0;
            for (int s = 0; s < S; ++s) {
                const int c = a.scnt[(int64_t)u * S + s];
                if (c > 0) cnt += c;
            }
            // InputBuilder.build_device: skip = (ymax - ymin < img_height_threshold) | (xmax - xmin < 1) | (count <
            // lidar_point_threshold); kept = ~skip & (count > 0) -- the same comparisons, fp64, on the box the count wrote
            const double *q = a.box2d + (int64_t)u * 4;
            const bool skip = (q[3] - q[1] < a.min_h) || (q[2] - q[0] < 1.0) || ((double)cnt < a.min_pts);
            if (!skip && cnt > 0) keep |= 1u << (u - u0);
        }
        int64_t rank = fp_block_exscan((int64_t)__popc(keep), swave, tid, survivors);
        for (int u = u0; u < u1; ++u) {
            int slot = -1;
            if (keep & (1u << (u - u0))) {
                if (rank < B) { slot = (int)rank; a.slot_box[slot] = u; }
                rank += 1;
            }
            sslot[u] = slot;
        }
        n = survivors < B ? (int)survivors : B;
        for (int i = n + tid; i < B; i += FP_T) a.slot_box[i] = U;             // the spare row of the caller's per-box tables
        __syncthreads();
    }
    // ---- the segment offsets: thread tid owns the flattened segments [tid * E, (tid + 1) * E)
    const int M = U * S;                                    // <= FP_MAX_SEGS
    const int E = (M + FP_T - 1) / FP_T;
    const int i0 = tid * E < M ? tid * E : M, i1 = i0 + E < M ? i0 + E : M;
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) {
        const int c = a.scnt[i];
        if ((FOV || sslot[i / S] >= 0) && c > 0) sum += c;
    }
    int64_t total;
    int64_t run = fp_block_exscan(sum, swave, tid, total);
    for (int i = i0; i < i1; ++i) {
        const int slot = FOV ? 0 : sslot[i / S];
        const int64_t at = run < a.cap ? run : a.cap;
        a.soff[i] = at;
        if constexpr (FOV) {
            if (i % S == 0) a.off[i / S] = at;
        } else {
            if (slot >= 0 && i % S == 0) slo[slot] = at;
        }
        const int c = a.scnt[i];
        if (slot >= 0 && c > 0) run += c;
        if constexpr (!FOV)
            if (slot >= 0 && i % S == S - 1) shi[slot] = run < a.cap ? run : a.cap;
    }
    const int64_t end = total < a.cap ? total : a.cap;
    if constexpr (FOV) {
        if (tid == 0) { a.off[U] = end; a.soff[M] = end; }
    } else {
        __syncthreads();
        // ---- per slot: its first row and its STORED rows; an empty slot reads the spare row behind the buffer and holds nothing
        for (int i = tid; i < B; i += FP_T) {
            a.off[i] = i < n ? slo[i] : a.cap;
            a.counts[i] = i < n ? shi[i] - slo[i] : 0;
        }
        if (tid == 0) {
            a.off[B] = end;
            a.soff[M] = end;
            a.n_kept[0] = n;
            st |= (survivors > B ? RP_ST_MANY : 0) | (total > a.cap ? FP_ST_TRUNC : 0);
        }
        if (st) atomicOr(a.status, st);
    }
}

extern "C" int fcn_frustum_detect_plan_limits(int *max_d, int *max_segs)
{
    if (!max_d || !max_segs) return FCN_E_BADARG;
    *max_d = FP_MAX_D;
    *max_segs = FP_MAX_SEGS;
    return 0;
}

// ---- count / fill: FsSelect behind n_boxes, without the read-backs
extern "C" int fcn_frustum_detect_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                        const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                        const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                        const int32_t *n_boxes, double *box2d, double *frustum_angle, int32_t *seg_cnt, void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, nullptr, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !n_boxes || !box2d || !frustum_angle)
        return FCN_E_BADARG;
    FdArgs a;
    fs_args(a.c, a.g, frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, S, clip_boxes, clip_distance);
    a.nbox = n_boxes;
    a.g.box2d = box2d; a.g.angle = frustum_angle; a.c.scnt = seg_cnt;
    return sc_launch<FdSelect, false>(a, D, nullptr, 0, D, nullptr, F, (hipStream_t)stream, false);
}

extern "C" int fcn_frustum_detect_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                       const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                       const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                       const int32_t *n_boxes, const int64_t *seg_off, float *out_pts, void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !n_boxes || !seg_off || !out_pts)
        return FCN_E_BADARG;
    FdArgs a;
    fs_args(a.c, a.g, frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, S, clip_boxes, clip_distance);
    a.nbox = n_boxes;
    a.c.soff = seg_off; a.c.out = out_pts;
    return sc_launch<FdSelect, true>(a, D, nullptr, 0, D, nullptr, F, (hipStream_t)stream, false);
}

// ---- the plans
extern "C" int fcn_frustum_detect_plan(const int32_t *seg_cnt, const double *box2d, const int32_t *box_frame, const int32_t *n_boxes,
                                       double img_height_threshold, double lidar_point_threshold, int D, int S, int B1,
                                       int64_t capacity, int F, int32_t *slot_box, int32_t *n_kept, int64_t *seg_off, int64_t *off,
                                       int64_t *counts, int32_t *status, void *stream)
{
    if (!seg_cnt || !box2d || !box_frame || !n_boxes || !slot_box || !n_kept || !seg_off || !off || !counts || !status)
        return FCN_E_BADARG;
    if (D < 0 || S < 1 || B1 < 1 || capacity < 0 || F < 0) return FCN_E_BADARG;
    if (img_height_threshold != img_height_threshold || lidar_point_threshold != lidar_point_threshold) return FCN_E_BADARG;
    if (D > FP_MAX_D || B1 > FP_MAX_D || (int64_t)D * S > FP_MAX_SEGS) return FCN_E_LIMIT;
    FdPlanArgs a;
    a.scnt = seg_cnt; a.box2d = box2d; a.bframe = box_frame; a.nbox = n_boxes;
    a.min_h = img_height_threshold; a.min_pts = lidar_point_threshold;
    a.U = D; a.S = S; a.B = B1; a.F = F; a.cap = capacity;
    a.slot_box = slot_box; a.n_kept = n_kept; a.soff = seg_off; a.off = off; a.counts = counts; a.status = status;
    hipLaunchKernelGGL(fd_plan_kernel<false>, dim3(1), dim3(FP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

extern "C" int fcn_frustum_fov_plan(const int32_t *seg_cnt, int F, int S, int64_t capacity, int64_t *seg_off, int64_t *fov_off,
                                    void *stream)
{
    if (!seg_cnt || !seg_off || !fov_off) return FCN_E_BADARG;
    if (F < 0 || S < 1 || capacity < 0) return FCN_E_BADARG;
    if ((int64_t)F * S > FP_MAX_SEGS) return FCN_E_LIMIT;
    FdPlanArgs a = FdPlanArgs();
    a.scnt = seg_cnt; a.U = F; a.S = S; a.F = F; a.cap = capacity; a.soff = seg_off; a.off = fov_off;
    hipLaunchKernelGGL(fd_plan_kernel<true>, dim3(1), dim3(FP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}
