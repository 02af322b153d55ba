// The front of the pipeline, on the device: LiDAR frames in velodyne coordinates + per-frame calibration + 2-D detection boxes ->
// the first stage's raw frustum points in rect camera coordinates.  The reference does this on the host in numpy
// (kitti/prepare_data.py::extract_frustum_data_rgb_detection :462-568 with kitti_util.Calibration.project_velo_to_rect /
// project_rect_to_image / project_image_to_rect and draw_util.get_lidar_in_image_fov :12-23), once per detection over the whole
// frame.  Here the two launches of seg_compact.h do it over a grid of (S, D) workgroups (a KITTI sweep has ~120 000 points: one
// workgroup per box, as refine_select.h has it, would walk ~470 dependent iterations per pass):
//   count   seg_cnt[d * S + s] = the selected rows of the segment; workgroup s == 0 also writes the box actually used (clipped to
//           the image when asked: :523-524) and the frustum angle of its centre (:537-543);
//   fill    after the caller's ONE cumulative sum over the flattened (D * S) counts (seg_off; every S-th entry is a box's
//           offset): the selected rows in ascending frame order -- (float) rect x, y, z, then columns 3.. of the input row bit
//           for bit (column 3 is the intensity).
// The scan, the compaction and the host side are seg_compact.h's; this header is the geometry (FsSelect).
// Both kernels decide with ONE predicate (fs_select), in fp64 from the fp32 row, every sum evaluated left to right (the library is
// built with -ffp-contract=off): ref = V2C . (x, y, z, 1), rect = R0 . ref, img = P . (rect, 1), u = img_0 / img_2, v = img_1 / img_2;
// selected iff xmin <= u < xmax, ymin <= v < ymax, 0 <= u < W, 0 <= v < H and (double)x > clip_distance -- the VELODYNE x
// (get_lidar_in_image_fov :16-18).  A row with a non-finite x, y or z is never selected; img_2 has no guard of its own (the
// reference has none).
#pragma once
#include "seg_compact.h"

struct FsGeo {
    const int64_t *foff;               // (F+1)
    const double *P, *V2C, *R0, *wh;   // (F,12) (F,12) (F,9) (F,2)
    const double *boxes;               // (D,4)
    const int32_t *bframe;             // (D)
    int F, clip;
    double clipd;
    double *box2d, *angle;             // count only
};

struct FsArgs {
    ScArgs c;                          // c.pts: (sum m_f, ps) velodyne x, y, z, intensity, ...
    FsGeo g;
};

struct FsBox {
    double v[12], r[9], p[12];         // V2C, R0, P of the box's frame
    double xmin, ymin, xmax, ymax, W, H, clipd;
};

// box d -> its frame's calibration, the box actually used and the frame's rows [p0, p0 + m); false: the frame is out of range
// (nothing of it is read)
__device__ __forceinline__ bool fs_setup(const FsGeo &a, int d, FsBox &b, int64_t &p0, int64_t &m)
{
    const int f = a.bframe[d];
    if (f < 0 || f >= a.F) return false;
    for (int i = 0; i < 12; ++i) { b.v[i] = a.V2C[(int64_t)f * 12 + i]; b.p[i] = a.P[(int64_t)f * 12 + i]; }
    for (int i = 0; i < 9; ++i) b.r[i] = a.R0[(int64_t)f * 9 + i];
    b.W = a.wh[2 * (int64_t)f]; b.H = a.wh[2 * (int64_t)f + 1];
    b.clipd = a.clipd;
    const double *q = a.boxes + (int64_t)d * 4;
    b.xmin = q[0]; b.ymin = q[1]; b.xmax = q[2]; b.ymax = q[3];
    if (a.clip) {                      // np.clip(box[[0, 2]], 0, W - 1), np.clip(box[[1, 3]], 0, H - 1)
        b.xmin = fmin(fmax(b.xmin, 0.0), b.W - 1.0); b.xmax = fmin(fmax(b.xmax, 0.0), b.W - 1.0);
        b.ymin = fmin(fmax(b.ymin, 0.0), b.H - 1.0); b.ymax = fmin(fmax(b.ymax, 0.0), b.H - 1.0);
    }
    p0 = a.foff[f];
    m = a.foff[f + 1] - p0;
    if (m < 0) m = 0;
    return true;
}

// THE predicate of both kernels; r0..r2: the row in rect camera coordinates (fp64)
__device__ __forceinline__ bool fs_select(const FsBox &b, float xf, float yf, float zf, double &r0, double &r1, double &r2)
{
    r0 = 0.0; r1 = 0.0; r2 = 0.0;
    if (!(sc_finite(xf) && sc_finite(yf) && sc_finite(zf))) return false;
    const double x = xf, y = yf, z = zf;
    const double f0 = b.v[0] * x + b.v[1] * y + b.v[2] * z + b.v[3];
    const double f1 = b.v[4] * x + b.v[5] * y + b.v[6] * z + b.v[7];
    const double f2 = b.v[8] * x + b.v[9] * y + b.v[10] * z + b.v[11];
    r0 = b.r[0] * f0 + b.r[1] * f1 + b.r[2] * f2;
    r1 = b.r[3] * f0 + b.r[4] * f1 + b.r[5] * f2;
    r2 = b.r[6] * f0 + b.r[7] * f1 + b.r[8] * f2;
    const double i0 = b.p[0] * r0 + b.p[1] * r1 + b.p[2] * r2 + b.p[3];
    const double i1 = b.p[4] * r0 + b.p[5] * r1 + b.p[6] * r2 + b.p[7];
    const double i2 = b.p[8] * r0 + b.p[9] * r1 + b.p[10] * r2 + b.p[11];
    const double u = i0 / i2, v = i1 / i2;
    return u >= b.xmin && u < b.xmax && v >= b.ymin && v < b.ymax && u >= 0.0 && u < b.W && v >= 0.0 && v < b.H && x > b.clipd;
}

// the unlabelled geometry; frustum_label.h adds the label to it
struct FsSelect {
    using Args = FsArgs;
    static constexpr bool WHOLE = false, POS = false, SEG = false;
    FsBox b;
    __device__ __forceinline__ bool setup(const FsArgs &a, int d, int64_t &p0, int64_t &m) { return fs_setup(a.g, d, b, p0, m); }
    // the box actually used and the frustum angle of its centre
    __device__ __forceinline__ void box_angle(const FsGeo &a, int d, int tid) const
    {
        if (tid != 0) return;
        double *o = a.box2d + (int64_t)d * 4;
        o[0] = b.xmin; o[1] = b.ymin; o[2] = b.xmax; o[3] = b.ymax;
        // project_image_to_rect of (box centre u, ., depth 20): x = ((u - c_u) * 20) / f_u + b_x with b_x = P[0,3] / (-f_u)
        const double cu = (b.xmin + b.xmax) / 2.0;
        const double xr = ((cu - b.p[2]) * 20.0) / b.p[0] + b.p[3] / (-b.p[0]);
        a.angle[d] = -atan2(20.0, xr);
    }
    __device__ __forceinline__ void header(const FsArgs &a, int d, int tid) const { box_angle(a.g, d, tid); }
    __device__ __forceinline__ bool select(const float4 &v, float4 &o) const
    {
        double r0, r1, r2;
        const bool in = fs_select(b, v.x, v.y, v.z, r0, r1, r2);
        o = v;
        if (in) { o.x = (float)r0; o.y = (float)r1; o.z = (float)r2; }     // the reference stores pc_rect as float32
        return in;
    }
};

extern "C" int fcn_frustum_select_seg(void) { return FS_SEG; }

// what the sized frustum entries (here, frustum_label.h, frustum_sunrgbd.h) refuse first
static inline bool fs_sizes_ok(int F, int pt_stride, int D, int S)
{
    return !(pt_stride < 3 || D < 0 || F < 0 || S < 1 || D > FS_MAX_D);
}

static inline void fs_args(ScArgs &c, FsGeo &g, const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                           const double *V2C, const double *R0, const double *img_wh, const double *boxes, const int32_t *box_frame,
                           int S, int clip_boxes, double clip_distance)
{
    c = ScArgs(); g = FsGeo();
    c.pts = frame_pts; c.ps = pt_stride; c.S = S;
    g.foff = frame_off; g.P = P; g.V2C = V2C; g.R0 = R0; g.wh = img_wh; g.boxes = boxes; g.bframe = box_frame;
    g.F = F; g.clip = clip_boxes; g.clipd = clip_distance;
}

// The return code reports boxes whose frame is out of range and frames longer than S segments: box_frame (D) and frame_off (F+1) are
// read back before the launch (sc_read_lists).
extern "C" int fcn_frustum_select_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                        const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                        const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                        double *box2d, double *frustum_angle, int32_t *seg_cnt, void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, nullptr, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !box2d || !frustum_angle)
        return FCN_E_BADARG;
    FsArgs a;
    fs_args(a.c, a.g, frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, S, clip_boxes, clip_distance);
    a.g.box2d = box2d; a.g.angle = frustum_angle; a.c.scnt = seg_cnt;
    const ScList lists[1] = {{box_frame, F, false}};
    return sc_launch<FsSelect, false>(a, D, lists, 1, D, frame_off, F, (hipStream_t)stream, true);
}

extern "C" int fcn_frustum_select_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                       const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                       const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                       const int64_t *seg_off, float *out_pts, void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !seg_off || !out_pts)
        return FCN_E_BADARG;
    FsArgs a;
    fs_args(a.c, a.g, frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, S, clip_boxes, clip_distance);
    a.c.soff = seg_off; a.c.out = out_pts;
    const ScList lists[1] = {{box_frame, F, false}};
    return sc_launch<FsSelect, true>(a, D, lists, 1, D, frame_off, F, (hipStream_t)stream, true);
}
