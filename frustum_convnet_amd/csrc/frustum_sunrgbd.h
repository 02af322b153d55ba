// The SUN-RGBD side of frustum_select.h / frustum_label.h: upright-depth frames (x, y, z + rgb) + the per-frame camera matrix K
// and tilt rotation Rtilt + 2-D boxes (+ one label 3-D box beside each 2-D box) -> the five-scale model's raw frustum points in
// upright CAMERA coordinates (with their foreground labels and the box corners), on the device.  The reference does this on the
// host in numpy, scanning the whole frame once per box (sunrgbd/prepare_data.py::extract_frustum_data :132-267,
// extract_frustum_data_from_rgb_detection :270-381 with sunrgbd_utils.SUNRGBD_Calibration).  Here it is the two launches of
// seg_compact.h over a grid of (S, D) workgroups; only the geometry is new (SrSelect<LAB>, LAB: with the label box):
//   count   seg_cnt[d * S + s] (and, labelled, seg_pos[d * S + s]); workgroup s == 0 also writes the frustum angle of the box
//           centre (and the eight corners in compute_box_3d's order, flipped to upright camera);
//   fill    after the caller's cumulative sum over the (D * S) counts: the selected rows in ascending frame order as (x, -z, y) of
//           the input row -- an exact swap and negation -- then columns 3.. bit for bit (and out_seg).
// ONE selection predicate (sr_select), in fp64 from the fp32 row, every sum left to right (-ffp-contract=off):
//   d = Rtilt^T . (x, y, z), c = (d0, -d2, d1), i = K . c, u = i0 / i2, v = i1 / i2; selected iff xmin <= u < xmax, ymin <= v < ymax.
// No image-bounds test, no clip distance, no guard on i2: the reference has none (:191-192).  A row with a non-finite x, y or z is
// never selected.  Boxes are used as given.
// ONE in-box predicate (sr_inside), closed, on the input row in upright depth: with c = cos(-heading), s = sin(-heading),
// dx = x - cx, dy = y - cy, dz = z - cz: ax = c * dx + s * dy, ay = -s * dx + c * dy; inside iff |ax| <= l, |ay| <= w, |dz| <= h
// (l, w, h are the label file's HALF extents).
#pragma once
#include "frustum_select.h"

struct SrArgs {
    ScArgs c;                          // c.pts: (sum m_f, ps) upright depth x, y, z, then r, g, b, ...
    const int64_t *foff;               // (F+1)
    const double *K, *Rt;              // (F,9) (F,9) row-major
    const double *boxes;               // (D,4)
    const int32_t *bframe;             // (D)
    const double *gt;                  // (D,7) cx cy cz l w h heading, labelled only
    int F;
    double *angle;                     // count only
    double *corners;                   // (D,24), labelled count only
};

struct SrBox {
    double k[9], r[9];
    double xmin, ymin, xmax, ymax;
};

struct SrGt {
    double cx, cy, cz, l, w, h, c, s;
};

// box d -> its frame's calibration, the box and the frame's rows [p0, p0 + m); false: the frame is out of range (nothing of it is read)
__device__ __forceinline__ bool sr_setup(const SrArgs &a, int d, SrBox &b, int64_t &p0, int64_t &m)
{
    const int f = a.bframe[d];
    if (f < 0 || f >= a.F) return false;
    for (int i = 0; i < 9; ++i) { b.k[i] = a.K[(int64_t)f * 9 + i]; b.r[i] = a.Rt[(int64_t)f * 9 + i]; }
    const double *q = a.boxes + (int64_t)d * 4;
    b.xmin = q[0]; b.ymin = q[1]; b.xmax = q[2]; b.ymax = q[3];
    p0 = a.foff[f];
    m = a.foff[f + 1] - p0;
    if (m < 0) m = 0;
    return true;
}

__device__ __forceinline__ void sr_gt(const SrArgs &a, int d, SrGt &g)
{
    const double *q = a.gt + (int64_t)d * 7;
    g.cx = q[0]; g.cy = q[1]; g.cz = q[2]; g.l = q[3]; g.w = q[4]; g.h = q[5];
    const double t = -q[6];                                                // rotz(-1 * heading_angle)
    g.c = cos(t); g.s = sin(t);
}

// THE selection predicate of both kernels
__device__ __forceinline__ bool sr_select(const SrBox &b, float xf, float yf, float zf)
{
    if (!(sc_finite(xf) && sc_finite(yf) && sc_finite(zf))) return false;
    const double x = xf, y = yf, z = zf;
    const double d0 = b.r[0] * x + b.r[3] * y + b.r[6] * z;               // Rtilt^T
    const double d1 = b.r[1] * x + b.r[4] * y + b.r[7] * z;
    const double d2 = b.r[2] * x + b.r[5] * y + b.r[8] * z;
    const double c0 = d0, c1 = -d2, c2 = d1;                              // flip_axis_to_camera
    const double i0 = b.k[0] * c0 + b.k[1] * c1 + b.k[2] * c2;
    const double i1 = b.k[3] * c0 + b.k[4] * c1 + b.k[5] * c2;
    const double i2 = b.k[6] * c0 + b.k[7] * c1 + b.k[8] * c2;
    const double u = i0 / i2, v = i1 / i2;
    return u >= b.xmin && u < b.xmax && v >= b.ymin && v < b.ymax;
}

// THE in-box predicate of both labelled kernels; x, y, z: the INPUT row (upright depth)
__device__ __forceinline__ bool sr_inside(const SrGt &g, float xf, float yf, float zf)
{
    const double dx = (double)xf - g.cx, dy = (double)yf - g.cy, dz = (double)zf - g.cz;
    const double ax = g.c * dx + g.s * dy;
    const double ay = (-g.s) * dx + g.c * dy;
    return fabs(ax) <= g.l && fabs(ay) <= g.w && fabs(dz) <= g.h;
}

// project_image_to_upright_camera of (box centre, depth 20) -> -atan2(z, x) of the upright camera point
__device__ __forceinline__ double sr_angle(const SrBox &b)
{
    const double cu = (b.xmin + b.xmax) / 2.0, cv = (b.ymin + b.ymax) / 2.0;
    const double X = ((cu - b.k[2]) * 20.0) / b.k[0];
    const double Y = ((cv - b.k[5]) * 20.0) / b.k[4];
    const double e0 = X, e1 = 20.0, e2 = -Y;                               // flip_axis_to_depth
    const double ud0 = b.r[0] * e0 + b.r[1] * e1 + b.r[2] * e2;
    const double ud1 = b.r[3] * e0 + b.r[4] * e1 + b.r[5] * e2;
    return -atan2(ud1, ud0);                                               // upright camera (ud0, -ud2, ud1)
}

// compute_box_3d (sunrgbd_utils.py:257-263): rotz(-heading) . (x_k, y_k, z_k) + centroid, flipped to upright camera; o: (8,3)
__device__ __forceinline__ void sr_corners(const SrGt &g, double *o)
{
    for (int k = 0; k < 8; ++k) {
        const double xc = ((k & 3) == 1 || (k & 3) == 2) ? g.l : -g.l;     // -l, l, l, -l
        const double yc = (k & 2) ? -g.w : g.w;                            // w, w, -w, -w
        const double zc = (k & 4) ? -g.h : g.h;                            // h x 4, -h x 4
        const double X = (g.c * xc + (-g.s) * yc) + g.cx;
        const double Y = (g.s * xc + g.c * yc) + g.cy;
        const double Z = zc + g.cz;
        o[3 * k] = X; o[3 * k + 1] = -Z; o[3 * k + 2] = Y;
    }
}

template <bool LAB> struct SrSelect {
    using Args = SrArgs;
    static constexpr bool WHOLE = false, POS = LAB, SEG = LAB;
    SrBox b;
    SrGt g;
    __device__ __forceinline__ bool setup(const SrArgs &a, int d, int64_t &p0, int64_t &m)
    {
        if (!sr_setup(a, d, b, p0, m)) return false;
        if constexpr (LAB) sr_gt(a, d, g);
        return true;
    }
    __device__ __forceinline__ void header(const SrArgs &a, int d, int tid) const
    {
        if (tid != 0) return;
        a.angle[d] = sr_angle(b);
        if constexpr (LAB) sr_corners(g, a.corners + (int64_t)d * 24);
    }
    __device__ __forceinline__ bool select(const float4 &v, float4 &o) const
    {
        o = make_float4(v.x, -v.z, v.y, v.w);  // upright depth -> upright camera: (x, -z, y), the xyz bits are the input's
        return sr_select(b, v.x, v.y, v.z);
    }
    __device__ __forceinline__ bool positive(const float4 &v, const float4 &) const { return sr_inside(g, v.x, v.y, v.z); }
};

// what the four entry points share after the refusals of frustum_select.h: the kernels' arguments and the launch (sc_launch;
// read_lists = false is the no-read pair of frustum_sunrgbd_plan.h)
static inline void sr_args(SrArgs &a, const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                           const double *Rtilt, const double *boxes, const int32_t *box_frame, int S)
{
    a = SrArgs();
    a.c.pts = frame_pts; a.c.ps = pt_stride; a.c.S = S;
    a.foff = frame_off; a.K = K; a.Rt = Rtilt; a.boxes = boxes; a.bframe = box_frame; a.F = F;
}

template <bool LAB, bool FILL> static inline int sr_launch(const SrArgs &a, int D, hipStream_t stream, bool read_lists)
{
    const ScList lists[1] = {{a.bframe, a.F, false}};
    return sc_launch<SrSelect<LAB>, FILL>(a, D, lists, 1, D, a.foff, a.F, stream, read_lists);
}

extern "C" int fcn_frustum_sunrgbd_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                         const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                         double *frustum_angle, int32_t *seg_cnt, void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, nullptr, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !K || !Rtilt || !boxes || !box_frame || !frustum_angle) return FCN_E_BADARG;
    SrArgs a;
    sr_args(a, frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, S);
    a.angle = frustum_angle; a.c.scnt = seg_cnt;
    return sr_launch<false, false>(a, D, (hipStream_t)stream, true);
}

extern "C" int fcn_frustum_sunrgbd_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                        const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                        const int64_t *seg_off, float *out_pts, void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !K || !Rtilt || !boxes || !box_frame || !seg_off || !out_pts) return FCN_E_BADARG;
    SrArgs a;
    sr_args(a, frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, S);
    a.c.soff = seg_off; a.c.out = out_pts;
    return sr_launch<false, true>(a, D, (hipStream_t)stream, true);
}

// What the labelled entries below and the no-read pair of frustum_sunrgbd_plan.h (fcn_frustum_sunrgbd_train_count / _fill) share:
// the argument checks, the kernels' arguments and the launch.
static inline int sr_label_count_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                        const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                        const double *gt_box3d, double *frustum_angle, int32_t *seg_cnt, int32_t *seg_pos,
                                        double *corners, void *stream, bool read_lists)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt || !seg_pos) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, seg_pos, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !K || !Rtilt || !boxes || !box_frame || !gt_box3d || !frustum_angle || !corners)
        return FCN_E_BADARG;
    SrArgs a;
    sr_args(a, frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, S);
    a.gt = gt_box3d; a.angle = frustum_angle; a.c.scnt = seg_cnt; a.c.spos = seg_pos; a.corners = corners;
    return sr_launch<true, false>(a, D, (hipStream_t)stream, read_lists);
}

static inline int sr_label_fill_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                       const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                       const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg,
                                       void *stream, bool read_lists)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !K || !Rtilt || !boxes || !box_frame || !gt_box3d || !seg_off || !out_pts || !out_seg)
        return FCN_E_BADARG;
    SrArgs a;
    sr_args(a, frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, S);
    a.gt = gt_box3d; a.c.soff = seg_off; a.c.out = out_pts; a.c.oseg = out_seg;
    return sr_launch<true, true>(a, D, (hipStream_t)stream, read_lists);
}

extern "C" int fcn_frustum_sunrgbd_label_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride,
                                               const double *K, const double *Rtilt, const double *boxes, const int32_t *box_frame,
                                               int D, int S, const double *gt_box3d, double *frustum_angle, int32_t *seg_cnt,
                                               int32_t *seg_pos, double *corners, void *stream)
{
    return sr_label_count_launch(frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, D, S, gt_box3d, frustum_angle, seg_cnt,
                                 seg_pos, corners, stream, true);
}

extern "C" int fcn_frustum_sunrgbd_label_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride,
                                              const double *K, const double *Rtilt, const double *boxes, const int32_t *box_frame,
                                              int D, int S, const double *gt_box3d, const int64_t *seg_off, float *out_pts,
                                              int64_t *out_seg, void *stream)
{
    return sr_label_fill_launch(frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, D, S, gt_box3d, seg_off, out_pts,
                                out_seg, stream, true);
}

// The positives a unit keeps after the reference's 2048-row subsample (prepare_data.py:219-226): pos[u] = the sum of
// seg[off[u] + sub[j]] over j in [sub_off[u], sub_off[u + 1]); a unit without a subsample (an empty range) sums all its cnt[u] rows.
// One workgroup per unit.  An index outside [0, cnt[u]) is skipped, never dereferenced (the host range-checks sub before upload).
__global__ __launch_bounds__(FS_T) void sr_subset_pos_kernel(const int64_t *seg, const int64_t *off, const int32_t *cnt,
                                                             const int32_t *sub, const int64_t *sub_off, int32_t *pos)
{
    __shared__ int wsum[FS_WAVES];
    const int u = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t o0 = off[u], j0 = sub_off[u], j1 = sub_off[u + 1];
    const int n = cnt[u];
    int p = 0;
    if (j1 > j0) {
        for (int64_t j = j0 + tid; j < j1; j += FS_T) {
            const int k = sub[j];
            if (k >= 0 && k < n) p += seg[o0 + k] != 0 ? 1 : 0;
        }
    } else {
        for (int k = tid; k < n; k += FS_T) p += seg[o0 + k] != 0 ? 1 : 0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) p += __shfl_xor(p, o, 64);
    if (lane == 0) wsum[wave] = p;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < FS_WAVES; ++w) t += wsum[w];
        pos[u] = t;
    }
}

extern "C" int fcn_frustum_subset_pos(const int64_t *seg, const int64_t *off, const int32_t *cnt, const int32_t *sub,
                                      const int64_t *sub_off, int U, int32_t *pos, void *stream)
{
    if (U < 0 || U > 0x7fffffff / 2) return FCN_E_BADARG;
    if (U == 0) return 0;
    if (!seg || !off || !cnt || !sub || !sub_off || !pos) return FCN_E_BADARG;
    hipLaunchKernelGGL(sr_subset_pos_kernel, dim3(U), dim3(FS_T), 0, (hipStream_t)stream, seg, off, cnt, sub, sub_off, pos);
    FCN_CHECK_LAUNCH();
    return 0;
}
