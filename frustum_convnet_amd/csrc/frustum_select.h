// The front of the pipeline, on the device: LiDAR frames in velodyne coordinates + per-frame calibration + 2-D detection boxes ->
// the first stage's raw frustum points in rect camera coordinates.  The reference does this on the host in numpy
// (kitti/prepare_data.py::extract_frustum_data_rgb_detection :462-568 with kitti_util.Calibration.project_velo_to_rect /
// project_rect_to_image / project_image_to_rect and draw_util.get_lidar_in_image_fov :12-23), once per detection over the whole
// frame.  Here two memory-bound launches do it over a grid of (S, D) workgroups, workgroup (s, d) scanning SEGMENT s -- rows
// [s * FS_SEG, min((s + 1) * FS_SEG, m)) -- of box d's frame (a KITTI sweep has ~120 000 points: one workgroup per box, as
// refine_select.h has it, would walk ~470 dependent iterations per pass):
//   fs_count_kernel   seg_cnt[d * S + s] = the selected rows of the segment; workgroup s == 0 also writes the box actually used
//                     (clipped to the image when asked: :523-524) and the frustum angle of its centre (:537-543);
//   fs_fill_kernel    after the caller's ONE cumulative sum over the flattened (D * S) counts (seg_off: every workgroup's base and
//                     cap; every S-th entry is a box's offset): the selected rows in ascending frame order -- (float) rect x, y, z,
//                     then columns 3.. of the input row bit for bit (column 3 is the intensity).
// Inside a workgroup everything is as in refine_select.h: the four waves take a contiguous quarter of the segment each (a multiple
// of 64 rows), one exclusive scan over the four counts gives a wave its base, and the fill walks the quarter again with __ballot +
// prefix popcount behind a running offset.  No workgroup waits for another; there are no atomics.
// Both kernels decide with ONE predicate (fs_select), in fp64 from the fp32 row, every sum evaluated left to right (the library is
// built with -ffp-contract=off): ref = V2C . (x, y, z, 1), rect = R0 . ref, img = P . (rect, 1), u = img_0 / img_2, v = img_1 / img_2;
// selected iff xmin <= u < xmax, ymin <= v < ymax, 0 <= u < W, 0 <= v < H and (double)x > clip_distance -- the VELODYNE x
// (get_lidar_in_image_fov :16-18).  A row with a non-finite x, y or z is never selected; img_2 has no guard of its own (the
// reference has none).
#pragma once
#include <memory>
#include <new>

#include "fcn_common.h"

#define FS_T 256
#define FS_WAVES (FS_T / 64)
#define FS_SEG 4096                    // rows per segment: a multiple of FS_T
static_assert(FS_SEG % FS_T == 0, "a segment is a whole number of workgroup strides");

struct FsArgs {
    const float *pts;                  // (sum m_f, ps) velodyne x, y, z, intensity, ...
    const int64_t *foff;               // (F+1)
    const double *P, *V2C, *R0, *wh;   // (F,12) (F,12) (F,9) (F,2)
    const double *boxes;               // (D,4)
    const int32_t *bframe;             // (D)
    const int64_t *soff;               // (D*S+1), fill only
    int F, ps, D, S, clip;
    double clipd;
    double *box2d, *angle;             // count only
    int32_t *scnt;                     // count only
    float *out;                        // fill only
};

struct FsBox {
    double v[12], r[9], p[12];         // V2C, R0, P of the box's frame
    double xmin, ymin, xmax, ymax, W, H, clipd;
};

// box d -> its frame's calibration, the box actually used and the frame's rows [p0, p0 + m); false: the frame is out of range
// (nothing of it is read)
__device__ __forceinline__ bool fs_setup(const FsArgs &a, int d, FsBox &b, int64_t &p0, int64_t &m)
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

__device__ __forceinline__ bool fs_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// THE predicate of both kernels; r0..r2: the row in rect camera coordinates (fp64)
__device__ __forceinline__ bool fs_select(const FsBox &b, float xf, float yf, float zf, double &r0, double &r1, double &r2)
{
    r0 = 0.0; r1 = 0.0; r2 = 0.0;
    if (!(fs_finite(xf) && fs_finite(yf) && fs_finite(zf))) return false;
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

// V4: pt_stride == 4 and 16-byte aligned rows -- one 16-byte load per point.  v: the output row's first four floats when selected
template <bool V4> __device__ __forceinline__ bool fs_test(const FsArgs &a, const FsBox &b, int64_t row, float4 &v)
{
    double r0, r1, r2;
    bool in;
    if constexpr (V4) {
        v = *(const float4 *)(a.pts + row * 4);
        in = fs_select(b, v.x, v.y, v.z, r0, r1, r2);
    } else {
        const float *p = a.pts + row * a.ps;
        in = fs_select(b, p[0], p[1], p[2], r0, r1, r2);
    }
    if (in) { v.x = (float)r0; v.y = (float)r1; v.z = (float)r2; }      // the reference stores pc_rect as float32
    return in;
}

// segment s of a frame of m rows -> [lo, hi) (empty beyond the frame), then this wave's quarter [qlo, qhi) of it
__device__ __forceinline__ void fs_quarter(int64_t m, int s, int wave, int64_t &qlo, int64_t &qhi)
{
    const int64_t lo = (int64_t)s * FS_SEG < m ? (int64_t)s * FS_SEG : m;
    const int64_t hi = lo + FS_SEG < m ? lo + FS_SEG : m;
    const int64_t n = hi - lo;
    const int64_t q = (((n + FS_WAVES - 1) / FS_WAVES) + 63) & ~(int64_t)63;
    qlo = lo + (q * wave < n ? q * wave : n);
    qhi = qlo + q < hi ? qlo + q : hi;
}

// selected rows of [lo, hi): the same value in every lane
template <bool V4> __device__ __forceinline__ int fs_wave_count(const FsArgs &a, const FsBox &b, int64_t p0, int64_t lo, int64_t hi, int lane)
{
    int c = 0;
    float4 v;
    for (int64_t i = lo + lane; i < hi; i += 64) c += fs_test<V4>(a, b, p0 + i, v) ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    return c;
}

template <bool V4> __global__ __launch_bounds__(FS_T) void fs_count_kernel(FsArgs a)
{
    __shared__ int wcnt[FS_WAVES];
    const int s = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FsBox b;
    int64_t p0, m;
    if (!fs_setup(a, d, b, p0, m)) {           // (workgroup-uniform)
        if (tid == 0) a.scnt[(int64_t)d * a.S + s] = 0;
        return;
    }
    if (s == 0 && tid == 0) {
        double *o = a.box2d + (int64_t)d * 4;
        o[0] = b.xmin; o[1] = b.ymin; o[2] = b.xmax; o[3] = b.ymax;
        // project_image_to_rect of (box centre u, ., depth 20): x = ((u - c_u) * 20) / f_u + b_x with b_x = P[0,3] / (-f_u)
        const double cu = (b.xmin + b.xmax) / 2.0;
        const double xr = ((cu - b.p[2]) * 20.0) / b.p[0] + b.p[3] / (-b.p[0]);
        a.angle[d] = -atan2(20.0, xr);
    }
    int64_t lo, hi;
    fs_quarter(m, s, wave, lo, hi);
    const int c = fs_wave_count<V4>(a, b, p0, lo, hi, lane);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < FS_WAVES; ++w) t += wcnt[w];
        a.scnt[(int64_t)d * a.S + s] = t;
    }
}

template <bool V4> __global__ __launch_bounds__(FS_T) void fs_fill_kernel(FsArgs a)
{
    __shared__ int wcnt[FS_WAVES];
    const int s = blockIdx.x, d = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    FsBox b;
    int64_t p0, m;
    if (!fs_setup(a, d, b, p0, m)) return;
    int64_t lo, hi;
    fs_quarter(m, s, wave, lo, hi);
    const int c = fs_wave_count<V4>(a, b, p0, lo, hi, lane);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int64_t run = 0;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    // the caller's offsets bound the writes: rows beyond this workgroup's slice of out_pts are dropped, never stored
    const int64_t o0 = a.soff[(int64_t)d * a.S + s];
    int64_t cap = a.soff[(int64_t)d * a.S + s + 1] - o0;
    if (o0 < 0) cap = 0;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        float4 v;
        const bool in = i < hi && fs_test<V4>(a, b, p0 + i, v);
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        const int64_t pos = run + (int64_t)__popcll(mask & lt_mask);
        if (in && pos < cap) {
            if constexpr (V4) {
                *(float4 *)(a.out + (o0 + pos) * 4) = v;
            } else {
                const uint32_t *src = (const uint32_t *)(a.pts + (p0 + i) * a.ps);
                float *dst = a.out + (o0 + pos) * a.ps;
                dst[0] = v.x; dst[1] = v.y; dst[2] = v.z;
                for (int k = 3; k < a.ps; ++k) ((uint32_t *)dst)[k] = src[k];
            }
        }
        run += (int64_t)__popcll(mask);
    }
}

// The return code reports boxes whose frame is out of range and frames longer than S segments, which only the device arrays
// know: box_frame (D) and frame_off (F+1) are read back before the launch.  That is a stream synchronisation -- the entry points
// are not capturable into a hipGraph; their caller reads the counts on the host between the two anyway.
// *ok: every box's frame is in range; *fits: no frame is longer than S * FS_SEG rows.
static inline int fs_read_lists(const int32_t *bframe, const int64_t *foff, int D, int F, int S, hipStream_t stream, bool *ok, bool *fits)
{
    std::unique_ptr<int64_t[]> ho(new (std::nothrow) int64_t[(size_t)F + 1]);      // (nothing may throw through the C-ABI)
    std::unique_ptr<int32_t[]> hb(new (std::nothrow) int32_t[(size_t)D]);
    if (!ho || !hb) return 2;                                                      // hipErrorOutOfMemory
#ifdef FCN_HOST_EMU
    // the host emulation of tests/ has no copy engine: its "device" arrays are host memory
    memcpy(hb.get(), bframe, (size_t)D * 4);
    memcpy(ho.get(), foff, ((size_t)F + 1) * 8);
#else
    hipError_t e = hipMemcpyAsync(hb.get(), bframe, (size_t)D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ho.get(), foff, ((size_t)F + 1) * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return (int)e;
#endif
    *ok = true; *fits = true;
    for (int d = 0; d < D; ++d)
        if (hb[d] < 0 || hb[d] >= F) *ok = false;
    for (int f = 0; f < F; ++f)
        if (ho[f + 1] - ho[f] > (int64_t)S * FS_SEG) *fits = false;
    return 0;
}

static inline bool fs_vec4(const float *pts, const float *out, int ps)
{
    return ps == 4 && (((uintptr_t)pts | (uintptr_t)out) & 15) == 0;
}

#define FS_MAX_D 65535                 // boxes are the grid's y dimension

extern "C" int fcn_frustum_select_seg(void) { return FS_SEG; }

extern "C" int fcn_frustum_select_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                        const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                        const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                        double *box2d, double *frustum_angle, int32_t *seg_cnt, void *stream)
{
    if (pt_stride < 3 || D < 0 || F < 0 || S < 1 || D > FS_MAX_D) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt) return FCN_E_BADARG;
    if (F == 0) {
        hipError_t e = hipMemsetAsync(seg_cnt, 0, (size_t)D * S * sizeof(int32_t), (hipStream_t)stream);
        return (int)e;
    }
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !box2d || !frustum_angle)
        return FCN_E_BADARG;
    bool ok = false, fits = false;
    FCN_TRY(fs_read_lists(box_frame, frame_off, D, F, S, (hipStream_t)stream, &ok, &fits));
    if (!fits) return FCN_E_BADARG;
    FsArgs a;
    a.pts = frame_pts; a.foff = frame_off; a.P = P; a.V2C = V2C; a.R0 = R0; a.wh = img_wh; a.boxes = boxes; a.bframe = box_frame;
    a.soff = nullptr; a.F = F; a.ps = pt_stride; a.D = D; a.S = S; a.clip = clip_boxes; a.clipd = clip_distance;
    a.box2d = box2d; a.angle = frustum_angle; a.scnt = seg_cnt; a.out = nullptr;
    if (fs_vec4(frame_pts, nullptr, pt_stride))
        hipLaunchKernelGGL(fs_count_kernel<true>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(fs_count_kernel<false>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}

extern "C" int fcn_frustum_select_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                                       const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                                       const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance,
                                       const int64_t *seg_off, float *out_pts, void *stream)
{
    if (pt_stride < 3 || D < 0 || F < 0 || S < 1 || D > FS_MAX_D) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !P || !V2C || !R0 || !img_wh || !boxes || !box_frame || !seg_off || !out_pts)
        return FCN_E_BADARG;
    bool ok = false, fits = false;
    FCN_TRY(fs_read_lists(box_frame, frame_off, D, F, S, (hipStream_t)stream, &ok, &fits));
    if (!fits) return FCN_E_BADARG;
    FsArgs a;
    a.pts = frame_pts; a.foff = frame_off; a.P = P; a.V2C = V2C; a.R0 = R0; a.wh = img_wh; a.boxes = boxes; a.bframe = box_frame;
    a.soff = seg_off; a.F = F; a.ps = pt_stride; a.D = D; a.S = S; a.clip = clip_boxes; a.clipd = clip_distance;
    a.box2d = nullptr; a.angle = nullptr; a.scnt = nullptr; a.out = out_pts;
    if (fs_vec4(frame_pts, out_pts, pt_stride))
        hipLaunchKernelGGL(fs_fill_kernel<true>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(fs_fill_kernel<false>, dim3(S, D), dim3(FS_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}
