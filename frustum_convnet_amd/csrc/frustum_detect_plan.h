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
//   fcn_frustum_detect_plan    the plan skeleton of slot_plan.h with FdPlan between the two: InputBuilder.build_device's skip rule
//                              per box in its own fp64 expression, on the boxes that are live and whose frame is in range; off and
//                              the STORED row counts per slot;
//   fcn_frustum_fov_plan       the skeleton with FdFov for the whole-image selection of the second stage's search set (one box
//                              (0, 0, W, H) per frame, no clipping): no rule and no slots, the prefix sum of the (F, S) counts and
//                              every S-th entry of it as the frames' offsets.  The capacity handed in is the row count of the frame
//                              buffer: a subset of a frame is no longer than the frame, so the clamp never cuts -- it is kept because
//                              it is what bounds the fill's stores whatever the counts hold.
// Status bits of the plan (one int32 word, OR-ed, never cleared here): FP_ST_TRUNC rows dropped because the total exceeds the
// capacity; RP_ST_MANY more survivors than slots; FD_ST_RANGE n_boxes outside [0, D] (taken as 0 / D) or a box below n_boxes whose
// frame is outside [0, F) (the box is ignored, never dereferenced).  Fewer survivors than slots is the normal case at inference: no
// bit (bit 0 is DeviceDraws': an empty slot has no row to draw from).
#pragma once
#include "frustum_select.h"
#include "slot_plan.h"

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
    SlArgs c;
    const double *box2d;               // (D,4) the clipped boxes the count wrote; row d is read only when box d is live
    const int32_t *bframe;             // (D)
    const int32_t *nbox;               // (1)
    double min_h, min_pts;
    int F;
};

struct FdPlan {
    using Args = FdPlanArgs;
    static constexpr bool SLOTS = true, COUNTS = true, MANY = true;
    __device__ static int live(const Args &a, int tid, int &st)
    {
        const int nb = a.nbox[0];
        if (nb >= 0 && nb <= a.c.U) return nb;
        if (tid == 0) st |= FD_ST_RANGE;
        return nb < 0 ? 0 : a.c.U;
    }
    __device__ static bool keep(const Args &a, int u, int &st)
    {
        const int f = a.bframe[u];
        if (f < 0 || f >= a.F) { st |= FD_ST_RANGE; return false; }
        int64_t cnt = 0;
        for (int s = 0; s < a.c.S; ++s) {
            const int c = a.c.scnt[(int64_t)u * a.c.S + s];
            if (c > 0) cnt += c;
        }
        // InputBuilder.build_device: skip = (ymax - ymin < img_height_threshold) | (xmax - xmin < 1) | (count <
        // lidar_point_threshold); kept = ~skip & (count > 0) -- the same comparisons, fp64, on the box the count wrote
        const double *q = a.box2d + (int64_t)u * 4;
        const bool skip = (q[3] - q[1] < a.min_h) || (q[2] - q[0] < 1.0) || ((double)cnt < a.min_pts);
        return !skip && cnt > 0;
    }
    __device__ static int filler(const Args &a) { return a.c.U; }   // the spare row of the caller's per-box tables
};

// every frame holds its rows and is its own slot: off[f] is frame f's first row
struct FdFov {
    struct Args {
        SlArgs c;
    };
    static constexpr bool SLOTS = false, COUNTS = false;
};

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
    if (F < 0 || img_height_threshold != img_height_threshold || lidar_point_threshold != lidar_point_threshold) return FCN_E_BADARG;
    FCN_TRY(sl_sizes(D, S, B1, capacity));
    FdPlanArgs a;
    a.c = SlArgs{seg_cnt, D, S, B1, capacity, slot_box, n_kept, seg_off, off, counts, status};
    a.box2d = box2d; a.bframe = box_frame; a.nbox = n_boxes;
    a.min_h = img_height_threshold; a.min_pts = lidar_point_threshold; a.F = F;
    return sl_launch(sl_plan_kernel<FdPlan>, a, stream);
}

extern "C" int fcn_frustum_fov_plan(const int32_t *seg_cnt, int F, int S, int64_t capacity, int64_t *seg_off, int64_t *fov_off,
                                    void *stream)
{
    if (!seg_cnt || !seg_off || !fov_off) return FCN_E_BADARG;
    if (F < 0 || S < 1 || capacity < 0) return FCN_E_BADARG;
    if ((int64_t)F * S > FP_MAX_SEGS) return FCN_E_LIMIT;
    FdFov::Args a;                                          // not sl_sizes: F alone has no limit here, nothing per frame lives in LDS
    a.c = SlArgs{seg_cnt, F, S, F, capacity, nullptr, nullptr, seg_off, fov_off, nullptr, nullptr};
    return sl_launch(sl_plan_kernel<FdFov>, a, stream);
}
