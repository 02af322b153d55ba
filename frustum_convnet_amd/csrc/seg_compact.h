// The scan-and-compact skeleton of the input side: "of a frame's rows, the ones a per-unit geometry selects, in ascending frame
// order" -- stated once for refine_select.h, frustum_select.h, frustum_label.h, frustum_sunrgbd.h and refine_label.h, which keep
// only their geometry (a POLICY, below) and their entry points.  Two memory-bound launches over a grid of (S, units) workgroups,
// workgroup (s, u) scanning SEGMENT s -- rows [s * FS_SEG, min((s + 1) * FS_SEG, m)) -- of unit u's frame:
//   sc_count_kernel   seg_cnt[u * S + s] = the selected rows of the segment (and, P::POS, seg_pos[u * S + s] = the positives among
//                     them); workgroup s == 0 also writes the unit's own outputs (P::header: box, angle, corners, sizes);
//   sc_fill_kernel    after the caller's ONE cumulative sum over the flattened (units * S) counts (seg_off: every workgroup's base
//                     and cap): the selected rows in ascending frame order -- columns 0..2 as the policy stores them, columns 3..
//                     of the input row bit for bit -- and, P::SEG, out_seg (int64, 1 for a positive, else 0) beside every stored row.
// Inside a workgroup the four waves take a contiguous quarter of the segment each (a multiple of 64 rows: it fixes the row order),
// every wave counts its quarter, one exclusive scan over the four counts gives a wave its base, and the fill walks the quarter
// again with __ballot + prefix popcount behind a running offset.  The caller's offsets bound every store: a row beyond the
// workgroup's slice is dropped, never stored; a negative base grants nothing.  No workgroup waits for another; there are no atomics.
// P::WHOLE (the cascade link): one segment covers the whole frame, the grid is (units) and S is not read.
//
// A policy P is a struct holding the unit's state (calibration, boxes: wave-uniform, so it lives in scalar registers) with
//   P::Args                        the kernels' argument; its member c (ScArgs) is what the skeleton itself reads
//   P::WHOLE, P::POS, P::SEG       (static constexpr bool) see above
//   bool setup(a, u, p0, m)        unit u -> the state and its frame's rows [p0, p0 + m); workgroup-uniform; false: the unit is out
//                                  of range or empty -- nothing of it is read, its counts are zero and nothing is stored
//   void header(a, u, tid)         the unit's own outputs, called by the count workgroup with s == 0
//   bool select(v, o)              THE selection predicate of both kernels; v: the row's x, y, z (and column 3) as loaded, o: the
//                                  stored row's first four floats when selected
//   bool positive(v, o)            (P::POS or P::SEG) THE label predicate of both kernels, on selected rows only
// Everything is resolved at compile time (templates, if constexpr): there is no mode inside the row loop.
#pragma once
#include <memory>
#include <new>

#include "fcn_common.h"

#define FS_T 256
#define FS_WAVES (FS_T / 64)
#define FS_SEG 4096                    // rows per segment: a multiple of FS_T
static_assert(FS_SEG % FS_T == 0, "a segment is a whole number of workgroup strides");
#define FS_MAX_D 65535                 // units are the grid's y dimension

struct ScArgs {
    const float *pts;                  // (sum m_f, ps) x, y, z, ...
    int ps, S;
    const int64_t *soff;               // (units*S+1), fill only
    int32_t *scnt, *spos;              // (units,S), count only (spos: P::POS only)
    float *out;                        // fill only
    int64_t *oseg;                     // fill only, P::SEG only
};

__device__ __forceinline__ bool sc_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// V4: pt_stride == 4 and 16-byte aligned rows -- one 16-byte load and one 16-byte store per point
static inline bool sc_vec4(const float *pts, const float *out, int ps)
{
    return ps == 4 && (((uintptr_t)pts | (uintptr_t)out) & 15) == 0;
}

// this wave's quarter [qlo, qhi) of the rows [lo, hi)
__device__ __forceinline__ void sc_quarter(int64_t lo, int64_t hi, int wave, int64_t &qlo, int64_t &qhi)
{
    const int64_t n = hi - lo;
    const int64_t q = (((n + FS_WAVES - 1) / FS_WAVES) + 63) & ~(int64_t)63;
    qlo = lo + (q * wave < n ? q * wave : n);
    qhi = qlo + q < hi ? qlo + q : hi;
}

// segment s of a frame of m rows (empty beyond the frame; WHOLE: all of it) -> this wave's quarter of it
template <bool WHOLE> __device__ __forceinline__ void sc_wave_rows(int64_t m, int s, int wave, int64_t &qlo, int64_t &qhi)
{
    if constexpr (WHOLE) {
        sc_quarter(0, m, wave, qlo, qhi);
    } else {
        const int64_t lo = (int64_t)s * FS_SEG < m ? (int64_t)s * FS_SEG : m;
        const int64_t hi = lo + FS_SEG < m ? lo + FS_SEG : m;
        sc_quarter(lo, hi, wave, qlo, qhi);
    }
}

template <class P, bool V4> __device__ __forceinline__ bool sc_test(const ScArgs &c, const P &g, int64_t row, float4 &v, float4 &o)
{
    if constexpr (V4) {
        v = *(const float4 *)(c.pts + row * 4);
    } else {
        const float *p = c.pts + row * c.ps;
        v.x = p[0]; v.y = p[1]; v.z = p[2]; v.w = 0.f;
    }
    return g.select(v, o);
}

// selected rows of [lo, hi) (and, POS, the positives among them): the same values in every lane
template <class P, bool V4, bool POS>
__device__ __forceinline__ void sc_wave_count(const ScArgs &c, const P &g, int64_t p0, int64_t lo, int64_t hi, int lane, int &n, int &np)
{
    n = 0; np = 0;
    float4 v, o;
    for (int64_t i = lo + lane; i < hi; i += 64)
        if (sc_test<P, V4>(c, g, p0 + i, v, o)) {
            n += 1;
            if constexpr (POS) np += g.positive(v, o) ? 1 : 0;
        }
#pragma unroll
    for (int k = 32; k > 0; k >>= 1) {
        n += __shfl_xor(n, k, 64);
        if constexpr (POS) np += __shfl_xor(np, k, 64);
    }
}

template <class P, bool V4> __global__ __launch_bounds__(FS_T) void sc_count_kernel(typename P::Args a)
{
    __shared__ int wcnt[P::POS ? 2 * FS_WAVES : FS_WAVES];      // the waves' counts, then (P::POS) their positives
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = P::WHOLE ? 0 : blockIdx.x, u = P::WHOLE ? blockIdx.x : blockIdx.y;
    const int64_t slot = P::WHOLE ? (int64_t)u : (int64_t)u * a.c.S + s;
    P g;
    int64_t p0, m;
    if (!g.setup(a, u, p0, m)) {               // (workgroup-uniform)
        if (tid == 0) {
            a.c.scnt[slot] = 0;
            if constexpr (P::POS) a.c.spos[slot] = 0;
        }
        return;
    }
    if (s == 0) g.header(a, u, tid);
    int64_t lo, hi;
    sc_wave_rows<P::WHOLE>(m, s, wave, lo, hi);
    int n, np;
    sc_wave_count<P, V4, P::POS>(a.c, g, p0, lo, hi, lane, n, np);
    if (lane == 0) {
        wcnt[wave] = n;
        if constexpr (P::POS) wcnt[FS_WAVES + wave] = np;
    }
    __syncthreads();
    if (tid == 0) {
        int tc = 0, tp = 0;
        for (int w = 0; w < FS_WAVES; ++w) {
            tc += wcnt[w];
            if constexpr (P::POS) tp += wcnt[FS_WAVES + w];
        }
        a.c.scnt[slot] = tc;
        if constexpr (P::POS) a.c.spos[slot] = tp;
    }
}

template <class P, bool V4> __global__ __launch_bounds__(FS_T) void sc_fill_kernel(typename P::Args a)
{
    __shared__ int wcnt[FS_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = P::WHOLE ? 0 : blockIdx.x, u = P::WHOLE ? blockIdx.x : blockIdx.y;
    const int64_t slot = P::WHOLE ? (int64_t)u : (int64_t)u * a.c.S + s;
    P g;
    int64_t p0, m;
    if (!g.setup(a, u, p0, m)) return;         // (workgroup-uniform)
    int64_t lo, hi;
    sc_wave_rows<P::WHOLE>(m, s, wave, lo, hi);
    int n, np;
    sc_wave_count<P, V4, false>(a.c, g, p0, lo, hi, lane, n, np);
    if (lane == 0) wcnt[wave] = n;
    __syncthreads();
    int64_t run = 0;
    for (int w = 0; w < wave; ++w) run += wcnt[w];
    // the caller's offsets bound EVERY store: a row beyond this workgroup's slice is dropped from out_pts and out_seg alike
    const int64_t o0 = a.c.soff[slot];
    int64_t cap = a.c.soff[slot + 1] - o0;
    if (o0 < 0) cap = 0;
    const unsigned long long lt_mask = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        float4 v, o;
        // (every lane reaches the ballot; the skip below is on a wave-uniform mask)
        const bool in = i < hi && sc_test<P, V4>(a.c, g, p0 + i, v, o);
        const unsigned long long mask = __ballot(in);
        if (mask == 0ull) continue;
        const int64_t pos = run + (int64_t)__popcll(mask & lt_mask);
        if (in && pos < cap) {
            if constexpr (V4) {
                *(float4 *)(a.c.out + (o0 + pos) * 4) = o;
            } else {
                const uint32_t *src = (const uint32_t *)(a.c.pts + (p0 + i) * a.c.ps);
                float *dst = a.c.out + (o0 + pos) * a.c.ps;
                dst[0] = o.x; dst[1] = o.y; dst[2] = o.z;
                for (int k = 3; k < a.c.ps; ++k) ((uint32_t *)dst)[k] = src[k];
            }
            if constexpr (P::SEG) a.c.oseg[o0 + pos] = g.positive(v, o) ? 1 : 0;
        }
        run += (int64_t)__popcll(mask);
    }
}

// ---- the host side
// The return codes report what only the device arrays know: index lists with an entry out of range and frames longer than S
// segments.  They are read back before the launch -- a stream synchronisation: an entry point that reads is not capturable into a
// hipGraph; its caller reads the counts on the host between count and fill anyway.
struct ScList {
    const int32_t *idx;                // (D)
    int lim;                           // in range: idx[d] < lim and ...
    bool neg_ok;                       // ... idx[d] >= 0, unless a negative entry has a meaning of its own
};

// *ok: every entry of every list is in range; *fits: no frame is longer than S * FS_SEG rows (foff == nullptr: not asked)
static inline int sc_read_lists(const ScList *lists, int nl, int D, const int64_t *foff, int F, int S, hipStream_t stream, bool *ok,
                                bool *fits)
{
    const size_t no = foff ? (size_t)F + 1 : 0;
    std::unique_ptr<int64_t[]> ho(new (std::nothrow) int64_t[no + 1]);             // (nothing may throw through the C-ABI)
    std::unique_ptr<int32_t[]> hi(new (std::nothrow) int32_t[(size_t)nl * D + 1]);
    if (!ho || !hi) return 2;                                                      // hipErrorOutOfMemory
#ifdef FCN_HOST_EMU
    // the host emulation of tests/ has no copy engine: its "device" arrays are host memory
    for (int l = 0; l < nl; ++l) memcpy(hi.get() + (size_t)l * D, lists[l].idx, (size_t)D * 4);
    if (foff) memcpy(ho.get(), foff, no * 8);
#else
    hipError_t e = hipSuccess;
    for (int l = 0; l < nl && e == hipSuccess; ++l)
        e = hipMemcpyAsync(hi.get() + (size_t)l * D, lists[l].idx, (size_t)D * 4, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && foff) e = hipMemcpyAsync(ho.get(), foff, no * 8, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return (int)e;
#endif
    *ok = true; *fits = true;
    for (int l = 0; l < nl; ++l)
        for (int d = 0; d < D; ++d) {
            const int32_t v = hi[(size_t)l * D + d];
            if (v >= lists[l].lim || (v < 0 && !lists[l].neg_ok)) *ok = false;
        }
    if (foff)
        for (int f = 0; f < F; ++f)
            if (ho[f + 1] - ho[f] > (int64_t)S * FS_SEG) *fits = false;
    return 0;
}

// What every entry point does once its arguments are checked: read the lists back when asked (read_lists; without it nothing is
// read and 0 is returned once the launch is enqueued -- the kernels skip a unit that is out of range either way, the length
// condition is the caller's then), refuse a frame that does not fit, launch, and report a list out of range AFTER the launch.
// sc_launch<P, false> is the count's launcher, sc_launch<P, true> the fill's.
template <class P, bool FILL>
static inline int sc_launch(const typename P::Args &a, int units, const ScList *lists, int nl, int D, const int64_t *foff, int F,
                            hipStream_t stream, bool read_lists)
{
    bool ok = true, fits = true;
    if (read_lists) {
        ok = false; fits = false;
        FCN_TRY(sc_read_lists(lists, nl, D, foff, F, a.c.S, stream, &ok, &fits));
    }
    if (!fits) return FCN_E_BADARG;
    const dim3 grid = P::WHOLE ? dim3(units) : dim3(a.c.S, units);
    const bool v4 = sc_vec4(a.c.pts, FILL ? a.c.out : nullptr, a.c.ps);
    if constexpr (FILL) {
        if (v4) hipLaunchKernelGGL((sc_fill_kernel<P, true>), grid, dim3(FS_T), 0, stream, a);
        else hipLaunchKernelGGL((sc_fill_kernel<P, false>), grid, dim3(FS_T), 0, stream, a);
    } else {
        if (v4) hipLaunchKernelGGL((sc_count_kernel<P, true>), grid, dim3(FS_T), 0, stream, a);
        else hipLaunchKernelGGL((sc_count_kernel<P, false>), grid, dim3(FS_T), 0, stream, a);
    }
    FCN_CHECK_LAUNCH();
    return ok ? 0 : FCN_E_BADARG;
}

// the F == 0 form of a count: every count is zero, nothing is launched
static inline int sc_zero_counts(int32_t *scnt, int32_t *spos, size_t n, hipStream_t stream)
{
    hipError_t e = hipMemsetAsync(scnt, 0, n * sizeof(int32_t), stream);
    if (e == hipSuccess && spos) e = hipMemsetAsync(spos, 0, n * sizeof(int32_t), stream);
    return (int)e;
}
