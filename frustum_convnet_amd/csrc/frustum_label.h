// The training side of frustum_select.h: LiDAR frames + calibration + 2-D boxes + one GROUND-TRUTH 3-D box beside each 2-D box ->
// the first stage's raw frustum points WITH their foreground labels and the box corners, on the device.  The reference does this
// on the host in numpy (kitti/prepare_data.py::extract_frustum_data :260-391): per ground-truth box it masks the frame, labels the
// selected points through a Delaunay hull of the box's corners (extract_pc_in_box3d :31-41 on compute_box_3d's corners,
// kitti_util.py:324-359) and rejects boxes without a labelled point (:354).  Here the two launches of frustum_select.h gain the
// label: the same grid of (S, D) workgroups, the same segments, quarters, ballot + prefix-popcount compaction and the SAME
// selection predicate (fs_select through fs_test) -- the device helpers of frustum_select.h are used as they are:
//   fl_count_kernel   seg_cnt[d * S + s] as fs_count_kernel, seg_pos[d * S + s] = the selected rows of the segment inside the 3-D
//                     box; workgroup s == 0 also writes box2d, frustum_angle and the eight corners (compute_box_3d's order);
//   fl_fill_kernel    as fs_fill_kernel, plus out_seg (int64, 1 inside the box, else 0) at the position of every row it stores:
//                     seg_off bounds both stores.
// The in-box predicate (fl_inside) is analytic, one function for both kernels, in fp64 on the row's rect coordinates AFTER their
// rounding to float32 (the reference tests the float32 pc_rect), every sum left to right: with c = cos(ry), s = sin(ry),
// dx = x - tx, dy = y - ty, dz = z - tz: ax = c * dx - s * dz, az = s * dx + c * dz (the row in the box's own axes); inside iff
// |ax| <= l / 2, |az| <= w / 2 and -h <= dy <= 0 (t is the bottom centre, y points down).  A face counts as inside.  It runs on
// selected rows only.  No workgroup waits for another; there are no atomics.
#pragma once
#include "frustum_select.h"

struct FlArgs {
    FsArgs s;                          // everything the selection needs (frustum_select.h)
    const double *gt;                  // (D,7) tx, ty, tz, l, w, h, ry in rect camera coordinates
    int32_t *spos;                     // (D,S), count only
    double *corners;                   // (D,24), count only
    int64_t *oseg;                     // fill only
};

struct FlBox {
    double tx, ty, tz, hl, hw, h, c, s;
};

__device__ __forceinline__ void fl_setup(const FlArgs &a, int d, FlBox &g)
{
    const double *q = a.gt + (int64_t)d * 7;
    g.tx = q[0]; g.ty = q[1]; g.tz = q[2];
    g.hl = q[3] / 2.0; g.hw = q[4] / 2.0; g.h = q[5];
    g.c = cos(q[6]); g.s = sin(q[6]);
}

// THE in-box predicate of both kernels; x, y, z: the row's rect coordinates as the float32 the fill stores
__device__ __forceinline__ bool fl_inside(const FlBox &g, float xf, float yf, float zf)
{
    const double dx = (double)xf - g.tx, dy = (double)yf - g.ty, dz = (double)zf - g.tz;
    const double ax = g.c * dx - g.s * dz;
    const double az = g.s * dx + g.c * dz;
    return fabs(ax) <= g.hl && fabs(az) <= g.hw && dy >= -g.h && dy <= 0.0;
}

// compute_box_3d: roty(ry) . (x_k, y_k, z_k) + t with x_k = +-l/2, y_k = 0 / -h, z_k = +-w/2 in its order; o: (8,3)
__device__ __forceinline__ void fl_corners(const FlBox &g, double *o)
{
    for (int k = 0; k < 8; ++k) {
        const double xc = (k & 2) ? -g.hl : g.hl;                          // l/2, l/2, -l/2, -l/2
        const double yc = (k & 4) ? -g.h : 0.0;                            // 0 x 4, -h x 4
        const double zc = ((k & 3) == 0 || (k & 3) == 3) ? g.hw : -g.hw;   // w/2, -w/2, -w/2, w/2
        o[3 * k] = (g.c * xc + g.s * zc) + g.tx;
        o[3 * k + 1] = yc + g.ty;
        o[3 * k + 2] = ((-g.s) * xc + g.c * zc) + g.tz;
    }
}

template <bool V4> __global__ __launch_bounds__(FS_T) void fl_count_kernel(FlArgs a)
{
    __shared__ int wcnt[FS_WAVES], wpos[FS_WAVES];
    const int s = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FsBox b;
    int64_t p0, m;
    if (!fs_setup(a.s, d, b, p0, m)) {         // (workgroup-uniform)
        if (tid == 0) { a.s.scnt[(int64_t)d * a.s.S + s] = 0; a.spos[(int64_t)d * a.s.S + s] = 0; }
        return;
    }
    FlBox g;
    fl_setup(a, d, g);
    if (s == 0 && tid == 0) {
        double *o = a.s.box2d + (int64_t)d * 4;
        o[0] = b.xmin; o[1] = b.ymin; o[2] = b.xmax; o[3] = b.ymax;
        const double cu = (b.xmin + b.xmax) / 2.0;                         // (as fs_count_kernel)
        const double xr = ((cu - b.p[2]) * 20.0) / b.p[0] + b.p[3] / (-b.p[0]);
        a.s.angle[d] = -atan2(20.0, xr);
        fl_corners(g, a.corners + (int64_t)d * 24);
    }
    int64_t lo, hi;
    fs_quarter(m, s, wave, lo, hi);
    int c = 0, p = 0;
    float4 v;
    for (int64_t i = lo + lane; i < hi; i += 64)
        if (fs_test<V4>(a.s, b, p0 + i, v)) { c += 1; p += fl_inside(g, v.x, v.y, v.z) ? 1 : 0; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { c += __shfl_xor(c, o, 64); p += __shfl_xor(p, o, 64); }
    if (lane == 0) { wcnt[wave] = c; wpos[wave] = p; }
    __syncthreads();
    if (tid == 0) {
        int tc = 0, tp = 0;
        for (int w = 0; w < FS_WAVES; ++w) { tc += wcnt[w]; tp += wpos[w]; }
        a.s.scnt[(int64_t)d * a.s.S + s] = tc;
        a.spos[(int64_t)d * a.s.S + s] = tp;
    }
}

template <bool V4> __global__ __launch_bounds__(FS_T) void fl_fill_kernel(FlArgs a)
{
    __shared__ int wcnt[FS_WAVES];
    const int s = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FsBox b;
    int64_t p0, m;
    if (!fs_setup(a.s, d, b, p0, m)) return;
    FlBox g;
    fl_setup(a, d, g);
    int64_t lo, hi;
    fs_quarter(m, s, wave, lo, hi);
    const int c = fs_wave_count<V4>(a.s, b, p0, lo, hi, lane);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int64_t run = 0;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    // the caller's offsets bound BOTH stores: a row beyond this workgroup's slice is dropped from out_pts and out_seg alike
    const int64_t o0 = a.s.soff[(int64_t)d * a.s.S + s];
    int64_t cap = a.s.soff[(int64_t)d * a.s.S + s + 1] - o0;
    if (o0 < 0) cap = 0;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        float4 v;
        const bool in = i < hi && fs_test<V4>(a.s, b, p0 + i, v);
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        const int64_t pos = run + (int64_t)__popcll(mask & lt_mask);
        if (in && pos < cap) {
            if constexpr (V4) {
                *(float4 *)(a.s.out + (o0 + pos) * 4) = v;
            } else {
                const uint32_t *src = (const uint32_t *)(a.s.pts + (p0 + i) * a.s.ps);
                float *dst = a.s.out + (o0 + pos) * a.s.ps;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z;
                for (int k = 3; k < a.s.ps; ++k) ((uint32_t *)dst)[k] = src[k];
            }
            a.oseg[o0 + pos] = fl_inside(g, v.x, v.y, v.z) ? 1 : 0;
        }
        run += (int64_t)__popcll(mask);
    }
}

// What the entries below and the no-read pair of frustum_plan.h (fcn_frustum_train_count / _fill) share: the argument checks, the
// kernels' arguments and the launch.  read_lists: read box_frame and frame_off back first (fs_read_lists: a synchronisation) and
// report an out-of-range frame or a frame longer than S segments; without it nothing is read and 0 is returned once the launch is
// enqueued -- the kernels skip a box whose frame is out of range either way, the length condition is the caller's then.
static inline int fl_count_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                  const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                  const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                  const double *gt_box3d, double *box2d, double *frustum_angle, int32_t *seg_cnt,
                                  int32_t *seg_pos, double *corners, void *stream, bool read_lists)
{
    if (pt_stride < 3 || D < 0 || F < 0 || S < 1 || D > FS_MAX_D) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt || !seg_pos) return FCN_E_BADARG;
    if (F == 0) {
        hipError_t e = hipMemsetAsync(seg_cnt, 0, (size_t)D * S * sizeof(int32_t), (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(seg_pos, 0, (size_t)D * S * sizeof(int32_t), (hipStream_t)stream);
        return (int)e;
    }
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !gt_box3d || !box2d || !frustum_angle ||
        !corners)
        return FCN_E_BADARG;
    bool ok = true, fits = true;
    if (read_lists) {
        ok = false; fits = false;
        FCN_TRY(fs_read_lists(box_frame, frame_off, D, F, S, (hipStream_t)stream, &ok, &fits));
    }
    if (!fits) return FCN_E_BADARG;
    FlArgs a;
    a.s.pts = frame_pts; a.s.foff = frame_off; a.s.P = P; a.s.V2C = V2C; a.s.R0 = R0; a.s.wh = img_wh; a.s.boxes = boxes;
    a.s.bframe = box_frame; a.s.soff = nullptr; a.s.F = F; a.s.ps = pt_stride; a.s.D = D; a.s.S = S; a.s.clip = clip_boxes;
    a.s.clipd = clip_distance; a.s.box2d = box2d; a.s.angle = frustum_angle; a.s.scnt = seg_cnt; a.s.out = nullptr;
    a.gt = gt_box3d; a.spos = seg_pos; a.corners = corners; a.oseg = nullptr;
    if (fs_vec4(frame_pts, nullptr, pt_stride))
        hipLaunchKernelGGL(fl_count_kernel<true>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(fl_count_kernel<false>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}

static inline int fl_fill_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                 const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                 const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                 const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg, void *stream,
                                 bool read_lists)
{
    if (pt_stride < 3 || D < 0 || F < 0 || S < 1 || D > FS_MAX_D) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !gt_box3d || !seg_off || !out_pts ||
        !out_seg)
        return FCN_E_BADARG;
    bool ok = true, fits = true;
    if (read_lists) {
        ok = false; fits = false;
        FCN_TRY(fs_read_lists(box_frame, frame_off, D, F, S, (hipStream_t)stream, &ok, &fits));
    }
    if (!fits) return FCN_E_BADARG;
    FlArgs a;
    a.s.pts = frame_pts; a.s.foff = frame_off; a.s.P = P; a.s.V2C = V2C; a.s.R0 = R0; a.s.wh = img_wh; a.s.boxes = boxes;
    a.s.bframe = box_frame; a.s.soff = seg_off; a.s.F = F; a.s.ps = pt_stride; a.s.D = D; a.s.S = S; a.s.clip = clip_boxes;
    a.s.clipd = clip_distance; a.s.box2d = nullptr; a.s.angle = nullptr; a.s.scnt = nullptr; a.s.out = out_pts;
    a.gt = gt_box3d; a.spos = nullptr; a.corners = nullptr; a.oseg = out_seg;
    if (fs_vec4(frame_pts, out_pts, pt_stride))
        hipLaunchKernelGGL(fl_fill_kernel<true>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(fl_fill_kernel<false>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}

extern "C" int fcn_frustum_label_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                       const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                       const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                       const double *gt_box3d, double *box2d, double *frustum_angle, int32_t *seg_cnt,
                                       int32_t *seg_pos, double *corners, void *stream)
{
    return fl_count_launch(frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, D, S, clip_boxes, clip_distance,
                           gt_box3d, box2d, frustum_angle, seg_cnt, seg_pos, corners, stream, true);
}

extern "C" int fcn_frustum_label_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                      const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                      const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                      const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg,
                                      void *stream)
{
    return fl_fill_launch(frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, D, S, clip_boxes, clip_distance,
                          gt_box3d, seg_off, out_pts, out_seg, stream, true);
}
