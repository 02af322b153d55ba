// The training side of refine_select.h: first-stage detections + the frame's LABEL boxes -> the refinement stage's training
// records, on the device.  The reference does this on the host (kitti/prepare_data_refine.py::extract_frustum_det_data :406-592):
// per detection the 3-D IoU against every label box of the frame (rbbox_iou_3d, boost polygon clipping), the best one when it
// reaches the threshold (:493-499), the box enlarged by 1.2 and, per augmentX copy, jittered by random_shift_rotate_box3d
// (:203-236, the copies CHAIN: copy a perturbs the result of copy a - 1, :513-519), the frame's points inside it and, among
// those, the points inside the label box through two Delaunay hulls (:527-535); a copy without a positive is rejected (:547).
// Three launches do it:
//   rl_match_kernel   one wave per candidate, the lanes stride over the frame's label boxes: the 3-D IoU of the centre forms
//                     with fcn_iou_from_params (box_iou.h, the float32 clip core), a wave reduction that keeps the largest IoU
//                     and, among equals, the lowest row; gt_idx = -1 when the frame has no label box or !(best >= thresh).
//                     rbbox_iou_3d's standup-box prefilter (ops/pybind11/rbbox_iou.py:179-184) is not restated: it zeroes only
//                     pairs whose axis-aligned hulls are disjoint, and the clip gives those pairs an IoU of 0 anyway.
//   count             the count of seg_compact.h with RlSelect, grid (S, U) over units u = d * A + a (candidate d, copy a):
//                     seg_cnt[u * S + s] = the rows of segment s inside the jittered enlarged box, seg_pos[u * S + s] = those of
//                     them inside the label box; workgroup s == 0 also writes both boxes' corners / heading / size.
//   fill              after the caller's ONE cumulative sum over the (U * S) counts: the selected rows, bit-exact copies of all
//                     pt_stride floats in ascending frame order, bounded by seg_off.
// The segments, the quarters, the ballot + prefix-popcount compaction and the host side are seg_compact.h's; the enlarged box
// (rs_setup), the closed-box predicate (rs_inside: fp64 from the fp32 row, a non-finite row never inside) and the corner order
// (rs_corner) are refine_select.h's.  One RsBox per unit selects (enlarged, jittered), a second one (the label box, NOT enlarged)
// counts the positives among the selected rows.  The per-point label itself is not emitted (RlSelect::SEG is false):
// datasets/provider_sample_refine.py never reads it (:250) and fcn_prepare_inputs_refine has no input for it; only its sum decides
// (the reject rule).
// A unit replays jitter steps 0..a of its candidate from jitter[d, 0..a, :] (seven uniform draws per step in the reference's
// order l, h, w, cx, cy, cz, angle), every product grouped as Python groups it, the floored modulo as fmod + one conditional
// add.  All deciding arithmetic is fp64, every sum left to right (the library is built with -ffp-contract=off).
#pragma once
#include "refine_select.h"
#ifndef FCN_HD
#define FCN_HD __device__ __forceinline__
#endif
#include "box_iou.h"

#define RL_MAX_A 64

struct RlArgs {
    ScArgs c;
    RsGeo r;                           // frames, dets, candidate lists, ratio (refine_select.h)
    const int32_t *cgt;                // (D) row of gt, < 0: the unit is empty
    const double *gt;                  // (G,7) tx, ty, tz, l, w, h, ry (t the bottom centre)
    const double *jitter;              // (D,A,7) or nullptr
    int G, A;
    double shift;
    double *pcorners, *pangle, *psize, *gcorners, *ghead, *gsize;      // count only
};

// random_shift_rotate_box3d (:203-236) with r = shift and the seven draws q[0..6]: the box keeps its meaning, every field follows
__device__ __forceinline__ void rl_jitter(RsBox &b, const double *q, double r)
{
    const double l1 = b.l + b.l * r * (q[0] * 2.0 - 1.0);
    const double h1 = b.h + b.h * r * (q[1] * 2.0 - 1.0);
    const double w1 = b.w + b.w * r * (q[2] * 2.0 - 1.0);
    const double cx1 = b.cx + b.l * r * (q[3] * 2.0 - 1.0);
    const double cy1 = b.cy + b.h * r * (q[4] * 2.0 - 1.0);
    const double cz1 = b.cz + b.w * r * (q[5] * 2.0 - 1.0);
    const double two_pi = 2.0 * M_PI;
    double ang = (b.ry + M_PI) + r * (q[6] * 2.0 - 1.0) * M_PI;
    ang = fmod(ang, two_pi);                               // Python's %: the sign of the divisor
    if (ang < 0.0) ang += two_pi;
    b.l = l1; b.h = h1; b.w = w1; b.cx = cx1; b.cy = cy1; b.cz = cz1; b.ry = ang - M_PI;
}

// label row -> its box in centre form (extract_boxes :42-46), not enlarged
__device__ __forceinline__ void rl_label_box(const double *q, RsBox &g)
{
    g.l = q[3]; g.w = q[4]; g.h = q[5];
    g.cx = q[0]; g.cy = q[1] - g.h / 2.0; g.cz = q[2];
    g.ry = q[6];
    g.c = cos(g.ry); g.s = sin(g.ry);
    g.hl = g.l / 2.0; g.hh = g.h / 2.0; g.hw = g.w / 2.0;
}

// unit u -> its jittered enlarged box b, its label box g and its frame's rows [p0, p0 + m); false: the unit is empty (no label
// matched) or its candidate's row / frame / label is out of range -- nothing of it is read
__device__ __forceinline__ bool rl_setup(const RlArgs &a, int u, RsBox &b, RsBox &g, int64_t &p0, int64_t &m)
{
    const int d = u / a.A, copy = u - d * a.A;
    const int gi = a.cgt[d];
    if (gi < 0 || gi >= a.G) return false;
    if (!rs_setup(a.r, d, b, p0, m)) return false;
    if (a.jitter) {
        for (int k = 0; k <= copy; ++k) rl_jitter(b, a.jitter + ((int64_t)d * a.A + k) * 7, a.shift);
        b.c = cos(b.ry); b.s = sin(b.ry);
        b.hl = b.l / 2.0; b.hh = b.h / 2.0; b.hw = b.w / 2.0;
    }
    rl_label_box(a.gt + (int64_t)gi * 7, g);
    return true;
}

struct RlSelect {
    using Args = RlArgs;
    static constexpr bool WHOLE = false, POS = true, SEG = false;
    RsBox b, g;
    __device__ __forceinline__ bool setup(const RlArgs &a, int u, int64_t &p0, int64_t &m) { return rl_setup(a, u, b, g, p0, m); }
    __device__ __forceinline__ void header(const RlArgs &a, int u, int tid) const
    {
        if (tid < 8) rs_corner(b, tid, a.pcorners + ((int64_t)u * 8 + tid) * 3);
        else if (tid < 16) rs_corner(g, tid - 8, a.gcorners + ((int64_t)u * 8 + (tid - 8)) * 3);
        if (tid == 0) {
            a.pangle[u] = b.ry;
            a.psize[3 * (int64_t)u] = b.l; a.psize[3 * (int64_t)u + 1] = b.w; a.psize[3 * (int64_t)u + 2] = b.h;
            a.ghead[u] = g.ry;
            a.gsize[3 * (int64_t)u] = g.l; a.gsize[3 * (int64_t)u + 1] = g.w; a.gsize[3 * (int64_t)u + 2] = g.h;
        }
    }
    __device__ __forceinline__ bool select(const float4 &v, float4 &o) const
    {
        o = v;                             // the row is stored as it is
        return rs_inside(b, v.x, v.y, v.z);
    }
    __device__ __forceinline__ bool positive(const float4 &v, const float4 &) const { return rs_inside(g, v.x, v.y, v.z); }
};

// ---- the match
#define RL_MT 256

struct RlMatchArgs {
    const float *dets;                 // (R,8)
    const int32_t *crow, *cframe;      // (D)
    const double *gt;                  // (G,7)
    const int64_t *goff;               // (F+1)
    int R, D, G, F;
    double thresh;
    int32_t *gidx;
    float *best;
};

__global__ __launch_bounds__(RL_MT) void rl_match_kernel(RlMatchArgs a)
{
    const int lane = threadIdx.x & 63;
    const int d = blockIdx.x * (RL_MT / 64) + (threadIdx.x >> 6);
    if (d >= a.D) return;                      // (wave-uniform)
    const int row = a.crow[d], f = a.cframe[d];
    if (row < 0 || row >= a.R || f < 0 || f >= a.F) {
        if (lane == 0) { a.gidx[d] = -1; a.best[d] = 0.f; }
        return;
    }
    const float *q = a.dets + (int64_t)row * 8;
    // centre form (tx, ty - h/2, tz, l, w, h, ry) in fp64 from the fp32 row; the label box is taken RELATIVE to this centre (in
    // fp64) before the float32 clip core sees it: overlaps do not depend on where the pair stands
    const double dl = q[3], dw = q[4], dh = q[5], dry = q[6];
    const double dcx = q[0], dcy = (double)q[1] - dh / 2.0, dcz = q[2];
    const float dco = (float)cos(dry), dsi = (float)sin(dry);
    int64_t g0 = a.goff[f], g1 = a.goff[f + 1];
    if (g0 < 0) g0 = 0;
    if (g1 > a.G) g1 = a.G;
    float best = -1.f;
    int bidx = 0x7fffffff;
    for (int64_t j = g0 + lane; j < g1; j += 64) {
        const double *t = a.gt + j * 7;
        const double gh = t[5], gry = t[6];
        float i2, i3;
        fcn_iou_from_params(0.f, 0.f, 0.f, (float)dl, (float)dw, (float)dh, dco, dsi, (float)(t[0] - dcx),
                            (float)((t[1] - gh / 2.0) - dcy), (float)(t[2] - dcz), (float)t[3], (float)t[4], (float)gh,
                            (float)cos(gry), (float)sin(gry), &i2, &i3);
        if (i3 > best) { best = i3; bidx = (int)j; }          // j ascends per lane: the first maximum is kept
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bidx, o, 64);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    if (lane == 0) {
        const bool any = bidx != 0x7fffffff;                                // false: the frame has no label box
        a.gidx[d] = (!any || !((double)best >= a.thresh)) ? -1 : bidx;      // the negated form: a NaN matches nothing
        a.best[d] = any ? best : 0.f;
    }
}

// What the entries below and the no-read entries of refine_plan.h (fcn_refine_train_match / _count / _fill) share: the argument
// checks, the kernels' arguments and the launch.  read_lists: read the index lists back first (sc_read_lists: a synchronisation)
// and report a candidate out of range or a frame longer than S segments; without it nothing is read and 0 is returned once the
// launch is enqueued -- the kernels skip a candidate whose row, frame or label is out of range either way, the length condition
// is the caller's then.
static inline int rl_match_launch(const float *dets, int R, const int32_t *cand_row, const int32_t *cand_frame, int D,
                                  const double *gt_box3d, int G, const int64_t *gt_off, int F, double thresh, int32_t *gt_idx,
                                  float *best_iou, void *stream, bool read_lists)
{
    if (D < 0 || F < 0 || R < 0 || G < 0) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!gt_idx || !best_iou) return FCN_E_BADARG;
    if (F == 0) {
        hipError_t e = hipMemsetAsync(gt_idx, 0xff, (size_t)D * sizeof(int32_t), (hipStream_t)stream);       // -1
        if (e == hipSuccess) e = hipMemsetAsync(best_iou, 0, (size_t)D * sizeof(float), (hipStream_t)stream);
        return (int)e;
    }
    if (!dets || !cand_row || !cand_frame || !gt_off || (G > 0 && !gt_box3d)) return FCN_E_BADARG;
    bool ok = true, fits = true;
    if (read_lists) {
        ok = false;
        const ScList lists[2] = {{cand_row, R, false}, {cand_frame, F, false}};
        FCN_TRY(sc_read_lists(lists, 2, D, nullptr, F, 1, (hipStream_t)stream, &ok, &fits));
    }
    RlMatchArgs a;
    a.dets = dets; a.crow = cand_row; a.cframe = cand_frame; a.gt = gt_box3d; a.goff = gt_off;
    a.R = R; a.D = D; a.G = G; a.F = F; a.thresh = thresh; a.gidx = gt_idx; a.best = best_iou;
    hipLaunchKernelGGL(rl_match_kernel, dim3((D + RL_MT / 64 - 1) / (RL_MT / 64)), dim3(RL_MT), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}

extern "C" int fcn_refine_match(const float *dets, int R, const int32_t *cand_row, const int32_t *cand_frame, int D,
                                const double *gt_box3d, int G, const int64_t *gt_off, int F, double thresh, int32_t *gt_idx,
                                float *best_iou, void *stream)
{
    return rl_match_launch(dets, R, cand_row, cand_frame, D, gt_box3d, G, gt_off, F, thresh, gt_idx, best_iou, stream, true);
}

// ---- count / fill
static inline bool rl_sizes_ok(int F, int pt_stride, int R, int D, int G, int A, int S)
{
    if (pt_stride < 3 || D < 0 || F < 0 || R < 0 || G < 0 || S < 1 || A < 1 || A > RL_MAX_A) return false;
    return (int64_t)D * A <= FS_MAX_D;         // units are the grid's y dimension
}

// Read back when asked: cand_row, cand_frame and, what these two calls add, cand_gt (no entry >= G; a negative one marks an empty
// unit and is no error) and frame_off.
template <bool FILL>
static inline int rl_launch(RlArgs &a, const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                            const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, const int32_t *cand_gt,
                            const double *gt_box3d, int G, int A, const double *jitter, double shift_ratio, int S, void *stream,
                            bool read_lists)
{
    a.c.pts = frame_pts; a.c.ps = pt_stride; a.c.S = S;
    a.r.foff = frame_off; a.r.dets = dets; a.r.crow = cand_row; a.r.cframe = cand_frame; a.r.F = F; a.r.R = R; a.r.ratio = ratio;
    a.cgt = cand_gt; a.gt = gt_box3d; a.jitter = jitter; a.G = G; a.A = A; a.shift = shift_ratio;
    const ScList lists[3] = {{cand_row, R, false}, {cand_frame, F, false}, {cand_gt, G, true}};
    return sc_launch<RlSelect, FILL>(a, D * A, lists, 3, D, frame_off, F, (hipStream_t)stream, read_lists);
}

static inline int rl_count_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                  int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                  const int32_t *cand_gt, const double *gt_box3d, int G, int A, const double *jitter,
                                  double shift_ratio, int S, int32_t *seg_cnt, int32_t *seg_pos, double *pred_corners,
                                  double *pred_angle, double *pred_size, double *gt_corners, double *gt_heading,
                                  double *gt_size, void *stream, bool read_lists)
{
    if (!rl_sizes_ok(F, pt_stride, R, D, G, A, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt || !seg_pos || (!jitter && A != 1)) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, seg_pos, (size_t)D * A * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !cand_gt || !gt_box3d || !pred_corners || !pred_angle ||
        !pred_size || !gt_corners || !gt_heading || !gt_size)
        return FCN_E_BADARG;
    RlArgs a = RlArgs();
    a.c.scnt = seg_cnt; a.c.spos = seg_pos; a.pcorners = pred_corners; a.pangle = pred_angle; a.psize = pred_size;
    a.gcorners = gt_corners; a.ghead = gt_heading; a.gsize = gt_size;
    return rl_launch<false>(a, frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, D, ratio, cand_gt, gt_box3d, G, A,
                            jitter, shift_ratio, S, stream, read_lists);
}

static inline int rl_fill_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                 int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                 const int32_t *cand_gt, const double *gt_box3d, int G, int A, const double *jitter,
                                 double shift_ratio, int S, const int64_t *seg_off, float *out_pts, void *stream, bool read_lists)
{
    if (!rl_sizes_ok(F, pt_stride, R, D, G, A, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!jitter && A != 1) return FCN_E_BADARG;
    if (F == 0) return 0;
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !cand_gt || !gt_box3d || !seg_off || !out_pts)
        return FCN_E_BADARG;
    RlArgs a = RlArgs();
    a.c.soff = seg_off; a.c.out = out_pts;
    return rl_launch<true>(a, frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, D, ratio, cand_gt, gt_box3d, G, A,
                           jitter, shift_ratio, S, stream, read_lists);
}

extern "C" int fcn_refine_label_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                      int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                      const int32_t *cand_gt, const double *gt_box3d, int G, int A, const double *jitter,
                                      double shift_ratio, int S, int32_t *seg_cnt, int32_t *seg_pos, double *pred_corners,
                                      double *pred_angle, double *pred_size, double *gt_corners, double *gt_heading,
                                      double *gt_size, void *stream)
{
    return rl_count_launch(frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, D, ratio, cand_gt, gt_box3d, G, A, jitter,
                           shift_ratio, S, seg_cnt, seg_pos, pred_corners, pred_angle, pred_size, gt_corners, gt_heading, gt_size,
                           stream, true);
}

extern "C" int fcn_refine_label_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                     int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                     const int32_t *cand_gt, const double *gt_box3d, int G, int A, const double *jitter,
                                     double shift_ratio, int S, const int64_t *seg_off, float *out_pts, void *stream)
{
    return rl_fill_launch(frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, D, ratio, cand_gt, gt_box3d, G, A, jitter,
                          shift_ratio, S, seg_off, out_pts, stream, true);
}
