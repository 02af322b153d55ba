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
//   rl_count_kernel   grid (S, U) over units u = d * A + a (candidate d, copy a) and the segments of frustum_select.h:
//                     seg_cnt[u * S + s] = the rows of segment s inside the jittered enlarged box, seg_pos[u * S + s] = those of
//                     them inside the label box; workgroup s == 0 also writes both boxes' corners / heading / size.
//   rl_fill_kernel    after the caller's ONE cumulative sum over the (U * S) counts: the selected rows, bit-exact copies of all
//                     pt_stride floats in ascending frame order, bounded by seg_off as fl_fill_kernel bounds its stores.
// The segments, the quarters (fs_quarter) and the ballot + prefix-popcount compaction are frustum_select.h's; the enlarged box
// (rs_setup), the closed-box predicate (rs_inside: fp64 from the fp32 row, a non-finite row never inside) and the corner order
// (rs_corner) are refine_select.h's.  One RsBox per unit selects (enlarged, jittered), a second one (the label box, NOT enlarged)
// counts the positives among the selected rows.  The per-point label itself is not emitted: datasets/provider_sample_refine.py
// never reads it (:250) and fcn_prepare_inputs_refine has no input for it; only its sum decides (the reject rule).
// A unit replays jitter steps 0..a of its candidate from jitter[d, 0..a, :] (seven uniform draws per step in the reference's
// order l, h, w, cx, cy, cz, angle), every product grouped as Python groups it, the floored modulo as fmod + one conditional
// add.  All deciding arithmetic is fp64, every sum left to right (the library is built with -ffp-contract=off).  No workgroup
// waits for another; there are no atomics.
#pragma once
#include "refine_select.h"
#include "frustum_select.h"
#ifndef FCN_HD
#define FCN_HD __device__ __forceinline__
#endif
#include "box_iou.h"

#define RL_MAX_A 64

struct RlArgs {
    RsArgs r;                          // frames, dets, candidate lists, ratio (refine_select.h); r.out: fill only
    const int32_t *cgt;                // (D) row of gt, < 0: the unit is empty
    const double *gt;                  // (G,7) tx, ty, tz, l, w, h, ry (t the bottom centre)
    const double *jitter;              // (D,A,7) or nullptr
    const int64_t *soff;               // (U*S+1), fill only
    int G, A, S;
    double shift;
    int32_t *scnt, *spos;              // (U,S), count only
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

// the row's x, y, z (V4: all four floats, which the fill stores back as they are)
template <bool V4> __device__ __forceinline__ void rl_load(const RsArgs &a, int64_t row, float4 &v)
{
    if constexpr (V4) {
        v = *(const float4 *)(a.pts + row * 4);
    } else {
        const float *p = a.pts + row * a.ps;
        v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = 0.f;
    }
}

template <bool V4> __global__ __launch_bounds__(FS_T) void rl_count_kernel(RlArgs a)
{
    __shared__ int wcnt[FS_WAVES], wpos[FS_WAVES];
    const int s = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RsBox b, g;
    int64_t p0, m;
    if (!rl_setup(a, u, b, g, p0, m)) {        // (workgroup-uniform)
        if (tid == 0) { a.scnt[(int64_t)u * a.S + s] = 0; a.spos[(int64_t)u * a.S + s] = 0; }
        return;
    }
    if (s == 0) {
        if (tid < 8) rs_corner(b, tid, a.pcorners + ((int64_t)u * 8 + tid) * 3);
        else if (tid < 16) rs_corner(g, tid - 8, a.gcorners + ((int64_t)u * 8 + (tid - 8)) * 3);
        if (tid == 0) {
            a.pangle[u] = b.ry;
            a.psize[3 * (int64_t)u] = b.l; a.psize[3 * (int64_t)u + 1] = b.w; a.psize[3 * (int64_t)u + 2] = b.h;
            a.ghead[u] = g.ry;
            a.gsize[3 * (int64_t)u] = g.l; a.gsize[3 * (int64_t)u + 1] = g.w; a.gsize[3 * (int64_t)u + 2] = g.h;
        }
    }
    int64_t lo, hi;
    fs_quarter(m, s, wave, lo, hi);
    int c = 0, p = 0;
    float4 v;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        rl_load<V4>(a.r, p0 + i, v);
        if (rs_inside(b, v.x, v.y, v.z)) { c += 1; p += rs_inside(g, v.x, v.y, v.z) ? 1 : 0; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o, 64); p += __shfl_xor(p, o, 64); }
    if (lane == 0) { wcnt[wave] = c; wpos[wave] = p; }
    __syncthreads();
    if (tid == 0) {
        int tc = 0, tp = 0;
        for (int w = 0; w < FS_WAVES; ++w) { tc += wcnt[w]; tp += wpos[w]; }
        a.scnt[(int64_t)u * a.S + s] = tc;
        a.spos[(int64_t)u * a.S + s] = tp;
    }
}

template <bool V4> __global__ __launch_bounds__(FS_T) void rl_fill_kernel(RlArgs a)
{
    __shared__ int wcnt[FS_WAVES];
    const int s = blockIdx.x, u = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RsBox b, g;
    int64_t p0, m;
    if (!rl_setup(a, u, b, g, p0, m)) return;
    int64_t lo, hi;
    fs_quarter(m, s, wave, lo, hi);
    int c = 0;
    float4 v;
    for (int64_t i = lo + lane; i < hi; i += 64) {
        rl_load<V4>(a.r, p0 + i, v);
        c += rs_inside(b, v.x, v.y, v.z) ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int64_t run = 0;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    // the caller's offsets bound the writes: rows beyond this workgroup's slice of out_pts are dropped, never stored
    const int64_t o0 = a.soff[(int64_t)u * a.S + s];
    int64_t cap = a.soff[(int64_t)u * a.S + s + 1] - o0;
    if (o0 < 0) cap = 0;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        bool in = false;
        if (i < hi) {
            rl_load<V4>(a.r, p0 + i, v);
            in = rs_inside(b, v.x, v.y, v.z);
        }
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        const int64_t pos = run + (int64_t)__popcll(mask & lt_mask);
        if (in && pos < cap) {
            if constexpr (V4) {
                *(float4 *)(a.r.out + (o0 + pos) * 4) = v;
            } else {
                const uint32_t *src = (const uint32_t *)(a.r.pts + (p0 + i) * a.r.ps);
                uint32_t *dst = (uint32_t *)(a.r.out + (o0 + pos) * a.r.ps);
                for (int k = 0; k < a.r.ps; ++k) dst[k] = src[k];
            }
        }
        run += (int64_t)__popcll(mask);
    }
}

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
// checks, the kernels' arguments and the launch.  read_lists: read the index lists back first (rs_candidates_in_range, rl_read_lists:
// a synchronisation) and report a candidate out of range or a frame longer than S segments; without it nothing is read and 0 is
// returned once the launch is enqueued -- the kernels skip a candidate whose row, frame or label is out of range either way, the
// length condition is the caller's then.
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
    bool ok = true;
    if (read_lists) {
        ok = false;
        FCN_TRY(rs_candidates_in_range(cand_row, cand_frame, D, R, F, (hipStream_t)stream, &ok));
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
// As rs_candidates_in_range for what these two calls add: cand_gt (D) and frame_off (F+1) are read back before the launch.
// *ok: no cand_gt is >= G (a negative one marks an empty unit and is no error); *fits: no frame is longer than S * FS_SEG rows.
static inline int rl_read_lists(const int32_t *cgt, const int64_t *foff, int D, int G, int F, int S, hipStream_t stream, bool *ok,
                                bool *fits)
{
    std::unique_ptr<int64_t[]> ho(new (std::nothrow) int64_t[(size_t)F + 1]);      // (nothing may throw through the C-ABI)
    std::unique_ptr<int32_t[]> hg(new (std::nothrow) int32_t[(size_t)D]);
    if (!ho || !hg) return 2;                                                      // hipErrorOutOfMemory
#ifdef FCN_HOST_EMU
    memcpy(hg.get(), cgt, (size_t)D * 4);
    memcpy(ho.get(), foff, ((size_t)F + 1) * 8);
#else
    hipError_t e = hipMemcpyAsync(hg.get(), cgt, (size_t)D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ho.get(), foff, ((size_t)F + 1) * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return (int)e;
#endif
    *ok = true; *fits = true;
    for (int d = 0; d < D; ++d)
        if (hg[d] >= G) *ok = false;
    for (int f = 0; f < F; ++f)
        if (ho[f + 1] - ho[f] > (int64_t)S * FS_SEG) *fits = false;
    return 0;
}

static inline bool rl_sizes_ok(int F, int pt_stride, int R, int D, int G, int A, int S)
{
    if (pt_stride < 3 || D < 0 || F < 0 || R < 0 || G < 0 || S < 1 || A < 1 || A > RL_MAX_A) return false;
    return (int64_t)D * A <= FS_MAX_D;         // units are the grid's y dimension
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
    const int U = D * A;
    if (F == 0) {
        hipError_t e = hipMemsetAsync(seg_cnt, 0, (size_t)U * S * sizeof(int32_t), (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(seg_pos, 0, (size_t)U * S * sizeof(int32_t), (hipStream_t)stream);
        return (int)e;
    }
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !cand_gt || !gt_box3d || !pred_corners || !pred_angle ||
        !pred_size || !gt_corners || !gt_heading || !gt_size)
        return FCN_E_BADARG;
    bool ok = true, ok_gt = true, fits = true;
    if (read_lists) {
        ok = false; ok_gt = false; fits = false;
        FCN_TRY(rs_candidates_in_range(cand_row, cand_frame, D, R, F, (hipStream_t)stream, &ok));
        FCN_TRY(rl_read_lists(cand_gt, frame_off, D, G, F, S, (hipStream_t)stream, &ok_gt, &fits));
    }
    if (!fits) return FCN_E_BADARG;
    RlArgs a;
    a.r.pts = frame_pts; a.r.foff = frame_off; a.r.dets = dets; a.r.crow = cand_row; a.r.cframe = cand_frame; a.r.ooff = nullptr;
    a.r.F = F; a.r.ps = pt_stride; a.r.R = R; a.r.ratio = ratio;
    a.r.corners = nullptr; a.r.angle = nullptr; a.r.size = nullptr; a.r.cnt = nullptr; a.r.out = nullptr;
    a.cgt = cand_gt; a.gt = gt_box3d; a.jitter = jitter; a.soff = nullptr; a.G = G; a.A = A; a.S = S; a.shift = shift_ratio;
    a.scnt = seg_cnt; a.spos = seg_pos; a.pcorners = pred_corners; a.pangle = pred_angle; a.psize = pred_size;
    a.gcorners = gt_corners; a.ghead = gt_heading; a.gsize = gt_size;
    if (rs_vec4(frame_pts, nullptr, pt_stride))
        hipLaunchKernelGGL(rl_count_kernel<true>, dim3(S, U), dim3(FS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(rl_count_kernel<false>, dim3(S, U), dim3(FS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return (ok && ok_gt) ? 0 : FCN_E_BADARG;
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
    bool ok = true, ok_gt = true, fits = true;
    if (read_lists) {
        ok = false; ok_gt = false; fits = false;
        FCN_TRY(rs_candidates_in_range(cand_row, cand_frame, D, R, F, (hipStream_t)stream, &ok));
        FCN_TRY(rl_read_lists(cand_gt, frame_off, D, G, F, S, (hipStream_t)stream, &ok_gt, &fits));
    }
    if (!fits) return FCN_E_BADARG;
    RlArgs a;
    a.r.pts = frame_pts; a.r.foff = frame_off; a.r.dets = dets; a.r.crow = cand_row; a.r.cframe = cand_frame; a.r.ooff = nullptr;
    a.r.F = F; a.r.ps = pt_stride; a.r.R = R; a.r.ratio = ratio;
    a.r.corners = nullptr; a.r.angle = nullptr; a.r.size = nullptr; a.r.cnt = nullptr; a.r.out = out_pts;
    a.cgt = cand_gt; a.gt = gt_box3d; a.jitter = jitter; a.soff = seg_off; a.G = G; a.A = A; a.S = S; a.shift = shift_ratio;
    a.scnt = nullptr; a.spos = nullptr; a.pcorners = nullptr; a.pangle = nullptr; a.psize = nullptr;
    a.gcorners = nullptr; a.ghead = nullptr; a.gsize = nullptr;
    if (rs_vec4(frame_pts, out_pts, pt_stride))
        hipLaunchKernelGGL(rl_fill_kernel<true>, dim3(S, D * A), dim3(FS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(rl_fill_kernel<false>, dim3(S, D * A), dim3(FS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return (ok && ok_gt) ? 0 : FCN_E_BADARG;
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
