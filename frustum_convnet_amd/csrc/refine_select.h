// The link between the two stages of the cascade, on the device: first-stage detections -> the raw points of the refinement
// stage.  The reference does this on the host (kitti/prepare_data_refine.py::extract_frustum_data_rgb_detection :649-773):
// every predicted box is enlarged by `ratio` (:724-727), the frame's LiDAR points inside it are found with
// scipy.spatial.Delaunay(corners).find_simplex (extract_pc_in_box3d) and pickled with the enlarged box's corners / size /
// heading for datasets/provider_sample_refine.py.  Here the two launches of seg_compact.h do it, one workgroup per candidate box
// (RsSelect::WHOLE: the whole frame is one segment):
//   count   the enlarged box's corners (order of compute_box_3d_obj_array :56-79, roty(ry)), heading and size in fp64 like the
//           pickled records, and the number of frame points inside;
//   fill    after the caller's cumulative sum of the counts: the selected rows, bit-exact copies of all pt_stride floats, in
//           ascending frame order (a stable compaction).
// The scan, the compaction and the host side are seg_compact.h's; this header is the geometry.  Both kernels decide with ONE
// predicate (rs_inside), in fp64 from the fp32 inputs: a closed box, |x'| <= l/2, |dy| <= h/2, |z'| <= w/2 with (x', z') = p - centre
// rotated back by ry (the Delaunay test of the reference has a tolerance at the faces instead); a point with a non-finite
// coordinate is never inside.
#pragma once
#include "seg_compact.h"

struct RsGeo {
    const int64_t *foff;       // (F+1)
    const float *dets;         // (R, 8): tx, ty, tz, l, w, h, ry, score
    const int32_t *crow, *cframe;
    int F, R;
    double ratio;
};

struct RsArgs {
    ScArgs c;                  // c.soff: out_off (D+1); c.scnt: cnt (D)
    RsGeo r;
    double *corners, *angle, *size;    // count only
};

struct RsBox {
    double cx, cy, cz, c, s, hl, hh, hw;      // centre, cos / sin of ry, half extents of the ENLARGED box
    double ry, l, w, h;
};

// candidate d -> its enlarged box and its frame's rows [p0, p0 + m); false: the candidate's row or frame is out of range (nothing
// of it is read).  prepare_data_refine.py:715-727: centre (tx, ty - h/2, tz) from the un-enlarged height, then l, w, h times ratio.
__device__ __forceinline__ bool rs_setup(const RsGeo &a, int d, RsBox &b, int64_t &p0, int64_t &m)
{
    const int row = a.crow[d], f = a.cframe[d];
    if (row < 0 || row >= a.R || f < 0 || f >= a.F) return false;
    const float *q = a.dets + (int64_t)row * 8;
    const double l = q[3], w = q[4], h = q[5];
    b.cx = q[0]; b.cy = (double)q[1] - h / 2.0; b.cz = q[2];
    b.ry = q[6];
    b.c = cos(b.ry); b.s = sin(b.ry);
    b.l = l * a.ratio; b.w = w * a.ratio; b.h = h * a.ratio;
    b.hl = b.l / 2.0; b.hh = b.h / 2.0; b.hw = b.w / 2.0;
    p0 = a.foff[f];
    m = a.foff[f + 1] - p0;
    if (m < 0) m = 0;
    return true;
}

// THE inside test of both kernels
__device__ __forceinline__ bool rs_inside(const RsBox &b, float x, float y, float z)
{
    if (!(sc_finite(x) && sc_finite(y) && sc_finite(z))) return false;
    const double dx = (double)x - b.cx, dy = (double)y - b.cy, dz = (double)z - b.cz;
    const double lx = b.c * dx - b.s * dz, lz = b.s * dx + b.c * dz;
    return fabs(lx) <= b.hl && fabs(dy) <= b.hh && fabs(lz) <= b.hw;
}

// corner k of the box -> o[0..2].  compute_box_3d_obj_array: x = l/2 * (+ + - - + + - -), y = h/2 * (+ + + + - - - -),
// z = w/2 * (+ - - + + - - +); roty(ry)
__device__ __forceinline__ void rs_corner(const RsBox &b, int k, double *o)
{
    const double x = (k & 2) ? -b.hl : b.hl, y = (k & 4) ? -b.hh : b.hh, z = ((k + 1) & 2) ? -b.hw : b.hw;
    o[0] = (b.c * x + b.s * z) + b.cx;
    o[1] = y + b.cy;
    o[2] = (-b.s * x + b.c * z) + b.cz;
}

struct RsSelect {
    using Args = RsArgs;
    static constexpr bool WHOLE = true, POS = false, SEG = false;
    RsBox b;
    __device__ __forceinline__ bool setup(const RsArgs &a, int d, int64_t &p0, int64_t &m) { return rs_setup(a.r, d, b, p0, m); }
    __device__ __forceinline__ void header(const RsArgs &a, int d, int tid) const
    {
        if (tid < 8) rs_corner(b, tid, a.corners + ((int64_t)d * 8 + tid) * 3);
        if (tid == 0) {
            a.angle[d] = b.ry;
            a.size[3 * d] = b.l; a.size[3 * d + 1] = b.w; a.size[3 * d + 2] = b.h;
        }
    }
    __device__ __forceinline__ bool select(const float4 &v, float4 &o) const
    {
        o = v;                             // the row is stored as it is
        return rs_inside(b, v.x, v.y, v.z);
    }
};

// The return code reports candidates whose row / frame is out of range: the two lists (2 * D integers) are read back before the
// launch (sc_read_lists).
static inline void rs_args(RsArgs &a, const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                           const int32_t *cand_row, const int32_t *cand_frame, double ratio)
{
    a = RsArgs();
    a.c.pts = frame_pts; a.c.ps = pt_stride; a.c.S = 1;
    a.r.foff = frame_off; a.r.dets = dets; a.r.crow = cand_row; a.r.cframe = cand_frame; a.r.F = F; a.r.R = R; a.r.ratio = ratio;
}

extern "C" int fcn_refine_select_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                       int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                       double *pred_corners, double *pred_angle, double *pred_size, int32_t *cnt, void *stream)
{
    if (pt_stride < 3 || D < 0 || F < 0 || R < 0) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!cnt) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(cnt, nullptr, (size_t)D, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !pred_corners || !pred_angle || !pred_size)
        return FCN_E_BADARG;
    RsArgs a;
    rs_args(a, frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, ratio);
    a.corners = pred_corners; a.angle = pred_angle; a.size = pred_size; a.c.scnt = cnt;
    const ScList lists[2] = {{cand_row, R, false}, {cand_frame, F, false}};
    return sc_launch<RsSelect, false>(a, D, lists, 2, D, nullptr, F, (hipStream_t)stream, true);
}

extern "C" int fcn_refine_select_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                      int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                      const int64_t *out_off, float *out_pts, void *stream)
{
    if (pt_stride < 3 || D < 0 || F < 0 || R < 0) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !out_off || !out_pts) return FCN_E_BADARG;
    RsArgs a;
    rs_args(a, frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, ratio);
    a.c.soff = out_off; a.c.out = out_pts;
    const ScList lists[2] = {{cand_row, R, false}, {cand_frame, F, false}};
    return sc_launch<RsSelect, true>(a, D, lists, 2, D, nullptr, F, (hipStream_t)stream, true);
}
