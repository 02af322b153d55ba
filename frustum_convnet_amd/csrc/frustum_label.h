// The training side of frustum_select.h: LiDAR frames + calibration + 2-D boxes + one GROUND-TRUTH 3-D box beside each 2-D box ->
// the first stage's raw frustum points WITH their foreground labels and the box corners, on the device.  The reference does this
// on the host in numpy (kitti/prepare_data.py::extract_frustum_data :260-391): per ground-truth box it masks the frame, labels the
// selected points through a Delaunay hull of the box's corners (extract_pc_in_box3d :31-41 on compute_box_3d's corners,
// kitti_util.py:324-359) and rejects boxes without a labelled point (:354).  Here the two launches of seg_compact.h gain the label
// (FlSelect: FsSelect of frustum_select.h -- the SAME selection predicate -- plus the label box):
//   count   seg_cnt[d * S + s] as frustum_select.h, seg_pos[d * S + s] = the selected rows of the segment inside the 3-D box;
//           workgroup s == 0 also writes box2d, frustum_angle and the eight corners (compute_box_3d's order);
//   fill    as frustum_select.h, plus out_seg (int64, 1 inside the box, else 0) at the position of every row it stores: seg_off
//           bounds both stores.
// The in-box predicate (fl_inside) is analytic, one function for both kernels, in fp64 on the row's rect coordinates AFTER their
// rounding to float32 (the reference tests the float32 pc_rect), every sum left to right: with c = cos(ry), s = sin(ry),
// dx = x - tx, dy = y - ty, dz = z - tz: ax = c * dx - s * dz, az = s * dx + c * dz (the row in the box's own axes); inside iff
// |ax| <= l / 2, |az| <= w / 2 and -h <= dy <= 0 (t is the bottom centre, y points down).  A face counts as inside.  It runs on
// selected rows only.
#pragma once
#include "frustum_select.h"

struct FlArgs {
    ScArgs c;
    FsGeo g;                           // everything the selection needs (frustum_select.h)
    const double *gt;                  // (D,7) tx, ty, tz, l, w, h, ry in rect camera coordinates
    double *corners;                   // (D,24), count only
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

struct FlSelect {
    using Args = FlArgs;
    static constexpr bool WHOLE = false, POS = true, SEG = true;
    FsSelect f;
    FlBox g;
    __device__ __forceinline__ bool setup(const FlArgs &a, int d, int64_t &p0, int64_t &m)
    {
        if (!fs_setup(a.g, d, f.b, p0, m)) return false;
        fl_setup(a, d, g);
        return true;
    }
    __device__ __forceinline__ void header(const FlArgs &a, int d, int tid) const
    {
        f.box_angle(a.g, d, tid);
        if (tid == 0) fl_corners(g, a.corners + (int64_t)d * 24);
    }
    __device__ __forceinline__ bool select(const float4 &v, float4 &o) const { return f.select(v, o); }
    __device__ __forceinline__ bool positive(const float4 &, const float4 &o) const { return fl_inside(g, o.x, o.y, o.z); }
};

// What the entries below and the no-read pair of frustum_plan.h (fcn_frustum_train_count / _fill) share: the argument checks, the
// kernels' arguments and the launch.  read_lists: read box_frame and frame_off back first (a synchronisation) and report an
// out-of-range frame or a frame longer than S segments; without it nothing is read (sc_launch).
static inline int fl_count_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                  const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                  const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                  const double *gt_box3d, double *box2d, double *frustum_angle, int32_t *seg_cnt,
                                  int32_t *seg_pos, double *corners, void *stream, bool read_lists)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt || !seg_pos) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, seg_pos, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !gt_box3d || !box2d || !frustum_angle ||
        !corners)
        return FCN_E_BADARG;
    FlArgs a;
    fs_args(a.c, a.g, frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, S, clip_boxes, clip_distance);
    a.g.box2d = box2d; a.g.angle = frustum_angle; a.c.scnt = seg_cnt; a.c.spos = seg_pos;
    a.gt = gt_box3d; a.corners = corners;
    const ScList lists[1] = {{box_frame, F, false}};
    return sc_launch<FlSelect, false>(a, D, lists, 1, D, frame_off, F, (hipStream_t)stream, read_lists);
}

static inline int fl_fill_launch(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                 const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                 const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                 const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg, void *stream,
                                 bool read_lists)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !gt_box3d || !seg_off || !out_pts ||
        !out_seg)
        return FCN_E_BADARG;
    FlArgs a;
    fs_args(a.c, a.g, frame_pts, frame_off, F, pt_stride, P, V2C, R0, img_wh, boxes, box_frame, S, clip_boxes, clip_distance);
    a.c.soff = seg_off; a.c.out = out_pts; a.c.oseg = out_seg;
    a.gt = gt_box3d; a.corners = nullptr;
    const ScList lists[1] = {{box_frame, F, false}};
    return sc_launch<FlSelect, true>(a, D, lists, 1, D, frame_off, F, (hipStream_t)stream, read_lists);
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
