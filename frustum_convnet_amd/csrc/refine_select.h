// The link between the two stages of the cascade, on the device: first-stage detections -> the raw points of the refinement
// stage.  The reference does this on the host (kitti/prepare_data_refine.py::extract_frustum_data_rgb_detection :649-773):
// every predicted box is enlarged by `ratio` (:724-727), the frame's LiDAR points inside it are found with
// scipy.spatial.Delaunay(corners).find_simplex (extract_pc_in_box3d) and pickled with the enlarged box's corners / size /
// heading for datasets/provider_sample_refine.py.  Here two memory-bound launches do it, one workgroup per candidate box:
//   rs_count_kernel   the enlarged box's corners (order of compute_box_3d_obj_array :56-79, roty(ry)), heading and size in fp64
//                     like the pickled records, and the number of frame points inside;
//   rs_fill_kernel    after the caller's cumulative sum of the counts: the selected rows, bit-exact copies of all pt_stride floats,
//                     in ascending frame order (a stable compaction).
// A workgroup's four waves take one contiguous quarter of the frame each (a multiple of 64 points), so ordered output needs no
// barrier inside the scan: every wave counts its quarter, one exclusive scan over the four counts gives its base, and the fill
// walks the quarter again with __ballot + prefix popcount behind a running offset.  Both kernels decide with ONE predicate
// (rs_inside), in fp64 from the fp32 inputs: a closed box, |x'| <= l/2, |dy| <= h/2, |z'| <= w/2 with (x', z') = p - centre rotated
// back by ry (the Delaunay test of the reference has a tolerance at the faces instead); a point with a non-finite coordinate is
// never inside.  No workgroup waits for another.
#pragma once
#include <memory>
#include <new>

#include "fcn_common.h"

#define RS_T 256
#define RS_WAVES (RS_T / 64)

struct RsArgs {
    const float *pts;          // (sum m_f, ps)
    const int64_t *foff;       // (F+1)
    const float *dets;         // (R, 8): tx, ty, tz, l, w, h, ry, score
    const int32_t *crow, *cframe;
    const int64_t *ooff;       // (D+1), fill only
    int F, ps, R;
    double ratio;
    double *corners, *angle, *size;    // count only
    int32_t *cnt;
    float *out;                // fill only
};

struct RsBox {
    double cx, cy, cz, c, s, hl, hh, hw;      // centre, cos / sin of ry, half extents of the ENLARGED box
    double ry, l, w, h;
};

// candidate d -> its enlarged box and its frame's rows [p0, p0 + m); false: the candidate's row or frame is out of range (nothing
// of it is read).  prepare_data_refine.py:715-727: centre (tx, ty - h/2, tz) from the un-enlarged height, then l, w, h times ratio.
__device__ __forceinline__ bool rs_setup(const RsArgs &a, int d, RsBox &b, int64_t &p0, int64_t &m)
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

__device__ __forceinline__ bool rs_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// THE inside test of both kernels
__device__ __forceinline__ bool rs_inside(const RsBox &b, float x, float y, float z)
{
    if (!(rs_finite(x) && rs_finite(y) && rs_finite(z))) return false;
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

// V4: pt_stride == 4 and 16-byte aligned rows -- one 16-byte load per point, which the fill stores back as it is
template <bool V4> __device__ __forceinline__ bool rs_test(const RsArgs &a, const RsBox &b, int64_t row, float4 &v)
{
    if constexpr (V4) {
        v = *(const float4 *)(a.pts + row * 4);
        return rs_inside(b, v.x, v.y, v.z);
    } else {
        const float *p = a.pts + row * a.ps;
        return rs_inside(b, p[0], p[1], p[2]);
    }
}

// this wave's quarter [lo, hi) of a frame of m points
__device__ __forceinline__ void rs_quarter(int64_t m, int wave, int64_t &lo, int64_t &hi)
{
    const int64_t seg = (((m + RS_WAVES - 1) / RS_WAVES) + 63) & ~(int64_t)63;
    lo = seg * wave < m ? seg * wave : m;
    hi = lo + seg < m ? lo + seg : m;
}

// points of [lo, hi) inside the box: the same value in every lane
template <bool V4> __device__ __forceinline__ int rs_wave_count(const RsArgs &a, const RsBox &b, int64_t p0, int64_t lo, int64_t hi, int lane)
{
    int c = 0;
    float4 v;
    for (int64_t i = lo + lane; i < hi; i += 64) c += rs_test<V4>(a, b, p0 + i, v) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
}

template <bool V4> __global__ __launch_bounds__(RS_T) void rs_count_kernel(RsArgs a)
{
    __shared__ int wcnt[RS_WAVES];
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RsBox b;
    int64_t p0, m;
    if (!rs_setup(a, d, b, p0, m)) {           // (workgroup-uniform)
        if (tid == 0) a.cnt[d] = 0;
        return;
    }
    if (tid < 8) rs_corner(b, tid, a.corners + ((int64_t)d * 8 + tid) * 3);
    if (tid == 0) {
        a.angle[d] = b.ry;
        a.size[3 * d] = b.l; a.size[3 * d + 1] = b.w; a.size[3 * d + 2] = b.h;
    }
    int64_t lo, hi;
    rs_quarter(m, wave, lo, hi);
    const int c = rs_wave_count<V4>(a, b, p0, lo, hi, lane);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < RS_WAVES; ++w) t += wcnt[w];
        a.cnt[d] = t;
    }
}

template <bool V4> __global__ __launch_bounds__(RS_T) void rs_fill_kernel(RsArgs a)
{
    __shared__ int wcnt[RS_WAVES];
    const int d = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    RsBox b;
    int64_t p0, m;
    if (!rs_setup(a, d, b, p0, m)) return;
    int64_t lo, hi;
    rs_quarter(m, wave, lo, hi);
    const int c = rs_wave_count<V4>(a, b, p0, lo, hi, lane);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int64_t run = 0;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    // the caller's offsets bound the writes: rows beyond this candidate's slice of out_pts are dropped, never stored
    const int64_t o0 = a.ooff[d], cap = a.ooff[d + 1] - o0;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        float4 v;
        const bool in = i < hi && rs_test<V4>(a, b, p0 + i, v);
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        const int64_t pos = run + (int64_t)__popcll(mask & lt_mask);
        if (in && pos < cap) {
            if constexpr (V4) {
                *(float4 *)(a.out + (o0 + pos) * 4) = v;
            } else {
                const uint32_t *src = (const uint32_t *)(a.pts + (p0 + i) * a.ps);
                uint32_t *dst = (uint32_t *)(a.out + (o0 + pos) * a.ps);
                for (int k = 0; k < a.ps; ++k) dst[k] = src[k];
            }
        }
        run += (int64_t)__popcll(mask);
    }
}

// The return code reports candidates whose row / frame is out of range, which only the device arrays know: the two lists (2 * D
// integers) are read back before the launch.  That is a stream synchronisation -- the entry points are not capturable into a
// hipGraph; their caller reads the counts on the host between the two anyway.
static inline int rs_candidates_in_range(const int32_t *crow, const int32_t *cframe, int D, int R, int F, hipStream_t stream, bool *ok)
{
    std::unique_ptr<int32_t[]> h(new (std::nothrow) int32_t[(size_t)2 * D]);     // (nothing may throw through the C-ABI)
    if (!h) return 2;                                                               // hipErrorOutOfMemory
#ifdef FCN_HOST_EMU
    // the host emulation of tests/ has no copy engine: its "device" arrays are host memory
    memcpy(h.get(), crow, (size_t)D * 4);
    memcpy(h.get() + D, cframe, (size_t)D * 4);
#else
    hipError_t e = hipMemcpyAsync(h.get(), crow, (size_t)D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h.get() + D, cframe, (size_t)D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return (int)e;
#endif
    *ok = true;
    for (int d = 0; d < D; ++d)
        if (h[d] < 0 || h[d] >= R || h[D + d] < 0 || h[D + d] >= F) *ok = false;
    return 0;
}

static inline bool rs_vec4(const float *pts, const float *out, int ps)
{
    return ps == 4 && (((uintptr_t)pts | (uintptr_t)out) & 15) == 0;
}

extern "C" int fcn_refine_select_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                       int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                       double *pred_corners, double *pred_angle, double *pred_size, int32_t *cnt, void *stream)
{
    if (pt_stride < 3 || D < 0 || F < 0 || R < 0) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!cnt) return FCN_E_BADARG;
    if (F == 0) {
        hipError_t e = hipMemsetAsync(cnt, 0, (size_t)D * sizeof(int32_t), (hipStream_t)stream);
        return (int)e;
    }
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !pred_corners || !pred_angle || !pred_size)
        return FCN_E_BADARG;
    bool ok = false;
    FCN_TRY(rs_candidates_in_range(cand_row, cand_frame, D, R, F, (hipStream_t)stream, &ok));
    RsArgs a;
    a.pts = frame_pts; a.foff = frame_off; a.dets = dets; a.crow = cand_row; a.cframe = cand_frame; a.ooff = nullptr;
    a.F = F; a.ps = pt_stride; a.R = R; a.ratio = ratio;
    a.corners = pred_corners; a.angle = pred_angle; a.size = pred_size; a.cnt = cnt; a.out = nullptr;
    if (rs_vec4(frame_pts, nullptr, pt_stride))
        hipLaunchKernelGGL(rs_count_kernel<true>, dim3(D), dim3(RS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(rs_count_kernel<false>, dim3(D), dim3(RS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}

extern "C" int fcn_refine_select_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                      int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio,
                                      const int64_t *out_off, float *out_pts, void *stream)
{
    if (pt_stride < 3 || D < 0 || F < 0 || R < 0) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !out_off || !out_pts) return FCN_E_BADARG;
    bool ok = false;
    FCN_TRY(rs_candidates_in_range(cand_row, cand_frame, D, R, F, (hipStream_t)stream, &ok));
    RsArgs a;
    a.pts = frame_pts; a.foff = frame_off; a.dets = dets; a.crow = cand_row; a.cframe = cand_frame; a.ooff = out_off;
    a.F = F; a.ps = pt_stride; a.R = R; a.ratio = ratio;
    a.corners = nullptr; a.angle = nullptr; a.size = nullptr; a.cnt = nullptr; a.out = out_pts;
    if (rs_vec4(frame_pts, out_pts, pt_stride))
        hipLaunchKernelGGL(rs_fill_kernel<true>, dim3(D), dim3(RS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(rs_fill_kernel<false>, dim3(D), dim3(RS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}
