// Single-launch inference forward of one PointNet scale (kernel K6): entries -> pooled features.
//
// With running statistics the three BatchNorms are affine maps known before the launch, so they fold into the weights and the
// grid-wide boundaries of the layered forward (batch sums between the layers) are gone:
//   pn_infer_fold_kernel  one small launch for all scales of a forward: s_l = gamma_l * rsqrt(running_var_l + eps),
//                         t_l = beta_l - running_mean_l * s_l (formed in fp64, rounded once -- the values the layered eval path uses);
//                         W1' = diag(s_1) W1 with t_1 as plain fp32 rows (a0, a1, a2, t1); W2' = diag(s_2) W2, W3' = diag(s_3) W3
//                         in the kb-major MFMA operand order of the forward GEMMs (pn_pack.h: F2, F3); t_2, t_3 (in the bf16 modes
//                         the images hold W2, W3 as the layered path rounds them and s_2, s_3 go to the epilogues as fp32
//                         vectors -- ones in split mode); and the zero fill
//                         of every scale's feature buffer, in stream order ahead of every tile.  Reads the running statistics only.
//   pn_infer_kernel       one launch per scale, a workgroup (4 waves, 2 x 2) per live 64-row tile of entries:
//                           h1 = relu(W1' u + t_1)   three FMAs per element straight into the A image of GEMM 2 (one 32-deep chunk)
//                           h2 = relu(h1 W2'^T + t_2) kept in LDS as the kb-major A image of GEMM 3 (all C2 / 32 chunks)
//                           h3 = relu(h2 W3'^T + t_3) max-reduced per window over the accumulators
//                         Weights stream from L2 in the pre-encoded order; activations never leave the CU.  Every value is >= +0.0
//                         after the ReLU and non-negative floats order like their bit patterns: the rows of a window meet in an LDS
//                         table [window slot][column] (32-bit unsigned max) and leave as one 32-bit unsigned atomic max per non-zero
//                         (window, column) into the zero-filled features -- a window may continue in a neighbouring tile, zeros need
//                         no publishing, empty windows (cnt == 0) keep the fill value, and a maximum does not depend on order: the
//                         output is bit-identical from run to run.
// LDS per workgroup (static): h2 image C2/32 x 8448 B (16.5 / 33 / 66 KiB for C2 = 64 / 128 / 256) + 24.5 KiB of operand staging
// (A chunk of GEMM 2 + one 128-column weight chunk; the epilogue patches and the pooling table alias it) -> 3 / 2 / 1 workgroups
// per CU.  A 128-row tile of the widest scale would need 132 + 33 KiB: 64 rows for every scale.
#pragma once
#include <type_traits>

#include "gemm_tile.h"
#include "pn_pack.h"

#define PNI_TM 64                  // rows of a workgroup's tile
#define PNI_T 256                  // threads
#define PNI_MAXC2 256              // widest h2 image kept in LDS

__device__ __forceinline__ void pni_max_u32(unsigned *p, unsigned v, bool wg)
{
#ifdef FCN_HOST_EMU
    unsigned o = __atomic_load_n(p, __ATOMIC_SEQ_CST);
    while (o < v && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
#else
    // (two call sites with constant scopes: ds_max_u32 on the table, global_atomic_umax on the features)
    if (wg) __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// relu with a canonical +0.0 for everything that is not positive (-0.0 and NaN included: their bit patterns would win an unsigned max)
__device__ __forceinline__ float pni_relu(float y) { return y > 0.f ? y : 0.f; }

// ------------------------------------------------------------------------------------------------ fold
struct PniFoldScale {
    const float *W[3], *gamma[3], *beta[3], *rmean[3], *rvar[3];
    float *w1f, *wenc, *shift, *feat;
    int64_t nfeat;
    int C1, C2, C3, precision;
};
struct PniFoldAll {
    PniFoldScale s[8];
    float eps;
};

__device__ __forceinline__ void pni_bn_fold(const PniFoldScale &S, int layer, int c, float eps, float &fs, float &ft)
{
    // (the arithmetic of the layered path's consumer-side finalisation, fwd_bn_in: the same scale / shift bit for bit)
    const double rstd = fcn_rsqrt64((double)S.rvar[layer][c] + (double)eps);
    const double sc = (double)S.gamma[layer][c] * rstd;
    fs = (float)sc;
    ft = (float)((double)S.beta[layer][c] - (double)S.rmean[layer][c] * sc);
}

// item t of a folded forward image: (chunk, k-block, output column n) -> both planes of s[n] * W[n][32c + 8kb + 0..7]
// (SCALED = false: the plain weight -- the bf16 modes, see pn_infer_fold_kernel)
template <int MM, bool SCALED>
__device__ __forceinline__ void pni_pack_item(const PniFoldScale &S, int layer, int COUT, int CIN, float eps, int t, u32x4 *__restrict__ img)
{
    const int n = t % COUT, r = t / COUT, kb = r & 3, c = r >> 2;
    float fs = 1.f, ft;
    if constexpr (SCALED) pni_bn_fold(S, layer, n, eps, fs, ft);
    const float *W = S.W[layer];
    const v4f a = ldg4(W + (int64_t)n * CIN + c * KC + 8 * kb), b = ldg4(W + (int64_t)n * CIN + c * KC + 8 * kb + 4);
    const float x[8] = {fs * a.x, fs * a.y, fs * a.z, fs * a.w, fs * b.x, fs * b.y, fs * b.z, fs * b.w};
    u32x4 hi, lo;
    enc8<MM>(x, hi, lo);
    img[((int64_t)c * 8 + kb) * COUT + n] = hi;
    img[((int64_t)c * 8 + 4 + kb) * COUT + n] = lo;
}

__global__ __launch_bounds__(PNI_T) void pn_infer_fold_kernel(PniFoldAll a)
{
    // the scale is workgroup-uniform: static indices only (a dynamically indexed kernel argument goes through scratch)
    PniFoldScale S = a.s[0];
#pragma unroll
    for (int q = 1; q < 8; ++q)
        if ((int)blockIdx.y == q) S = a.s[q];
    const int first = blockIdx.x * PNI_T + threadIdx.x, step = gridDim.x * PNI_T;
    const int n2 = S.C2 * S.C1 / 8, n3 = S.C3 * S.C2 / 8;
    u32x4 *F2 = (u32x4 *)S.wenc, *F3 = (u32x4 *)(S.wenc + (int64_t)S.C2 * S.C1);
    const bool split = S.precision == FCN_PREC_SPLIT;
    for (int t = first; t < n2 + n3; t += step) {
        const bool l3 = t >= n2;
        const int v = l3 ? t - n2 : t, layer = l3 ? 2 : 1;
        const int COUT = l3 ? S.C3 : S.C2, CIN = l3 ? S.C2 : S.C1;
        if (split) pni_pack_item<MM_F16X3, true>(S, layer, COUT, CIN, a.eps, v, l3 ? F3 : F2);
        else pni_pack_item<MM_BF16X1, false>(S, layer, COUT, CIN, a.eps, v, l3 ? F3 : F2);
    }
    for (int c = first; c < S.C1; c += step) {
        float fs, ft;
        pni_bn_fold(S, 0, c, a.eps, fs, ft);
        const v4f r = {fs * S.W[0][3 * c], fs * S.W[0][3 * c + 1], fs * S.W[0][3 * c + 2], ft};
        *(v4f *)(S.w1f + 4 * c) = r;
    }
    for (int c = first; c < S.C2 + S.C3; c += step) {
        float fs, ft;
        if (c < S.C2) pni_bn_fold(S, 1, c, a.eps, fs, ft);
        else pni_bn_fold(S, 2, c - S.C2, a.eps, fs, ft);
        S.shift[c] = ft;
        // the scale the epilogues apply to the accumulator: 1 where it sits in the weights (split mode: fma(1, y, t) = y + t exactly).
        // The bf16 modes keep it OUT of the 8-bit-significand operand: their weight images are then the layered path's own, bit for
        // bit, and the result agrees with the layered bf16-operand forward up to fp32 summation order -- rounding s * W instead of W
        // re-draws every weight's bf16 rounding, and behind a channel with a tiny running variance (scale ~300) ONE re-drawn weight
        // moves the largest outputs by 2^-9 of their magnitude
        S.shift[S.C2 + S.C3 + c] = split ? 1.f : fs;
    }
    // the pooling publishes into zero-filled features: the fill sits in stream order ahead of every tile of every scale
    if (((uintptr_t)S.feat & 15) == 0) {
        const int64_t n4 = S.nfeat / 4;
        for (int64_t i = first; i < n4; i += step) *(v4f *)(S.feat + 4 * i) = zero4();
        for (int64_t i = 4 * n4 + first; i < S.nfeat; i += step) S.feat[i] = 0.f;
    } else {
        for (int64_t i = first; i < S.nfeat; i += step) S.feat[i] = 0.f;
    }
}

static inline bool pni_desc_ok(const fcn_pn_desc *d, int *rc)
{
    *rc = FCN_E_BADARG;
    if (!d || d->training != FCN_BN_RUNNING) return false;
    // (FCN_PREC_F32 is not offered: the fp32 MFMA runs at the vector rate and is the layered path's A/B reference mode)
    if (d->precision != FCN_PREC_SPLIT && d->precision != FCN_PREC_BF16 && d->precision != FCN_PREC_BF16_OPS) return false;
    if (d->B <= 0 || d->L <= 0 || d->K <= 0 || d->nvec < 0) return false;
    if (d->C1 <= 0 || d->C2 <= 0 || d->C3 <= 0 || d->C1 % 64 || d->C2 % 64 || d->C3 % 64 || d->C1 > 512 || d->C2 > 512) return false;
    *rc = FCN_E_LIMIT;
    if (d->C2 > PNI_MAXC2 || d->L > 8192 || d->K > 1024) return false;
    if ((int64_t)d->B * d->L * d->K >= (int64_t)1 << 31) return false;
    *rc = 0;
    return true;
}
static inline int64_t pni_feat_floats(const fcn_pn_desc *d)
{
    return d->nlc ? (int64_t)d->B * d->L * d->C3 : (int64_t)d->B * (d->C3 + d->nvec) * d->L;
}

extern "C" int fcn_pn_infer_fold(int nscale, const fcn_pn_desc *const *d, const fcn_pn_params *const *p,
                                 const fcn_pn_infer_ws *const *iws, float *const *feat, void *stream)
{
    if (nscale < 1 || nscale > 8 || !d || !p || !iws || !feat) return FCN_E_BADARG;
    PniFoldAll a;
    int64_t maxwork = 1;
    for (int s = 0; s < 8; ++s) {
        const int q = s < nscale ? s : 0;
        int rc;
        if (!pni_desc_ok(d[q], &rc)) return rc;
        if (!p[q] || !iws[q] || !feat[q] || !iws[q]->w1f || !iws[q]->wenc || !iws[q]->shift) return FCN_E_BADARG;
        if (((uintptr_t)iws[q]->w1f & 15) || ((uintptr_t)iws[q]->wenc & 15) || ((uintptr_t)iws[q]->shift & 15)) return FCN_E_BADARG;
        if (d[q]->eps != d[0]->eps) return FCN_E_BADARG;
        PniFoldScale &S = a.s[s];
        for (int l = 0; l < 3; ++l) {
            S.W[l] = p[q]->W[l]; S.gamma[l] = p[q]->gamma[l]; S.beta[l] = p[q]->beta[l];
            S.rmean[l] = p[q]->running_mean[l]; S.rvar[l] = p[q]->running_var[l];
            if (!S.W[l] || !S.gamma[l] || !S.beta[l] || !S.rmean[l] || !S.rvar[l]) return FCN_E_BADARG;
        }
        if (((uintptr_t)S.W[1] & 15) || ((uintptr_t)S.W[2] & 15)) return FCN_E_BADARG;
        S.w1f = iws[q]->w1f; S.wenc = iws[q]->wenc; S.shift = iws[q]->shift; S.feat = feat[q];
        S.nfeat = pni_feat_floats(d[q]);
        S.C1 = d[q]->C1; S.C2 = d[q]->C2; S.C3 = d[q]->C3; S.precision = d[q]->precision;
        const int64_t work = (int64_t)(S.C2 * S.C1 + S.C3 * S.C2) / 8 + S.nfeat / 4;
        if (s < nscale && work > maxwork) maxwork = work;
    }
    a.eps = d[0]->eps;
    // a few items per thread: the scale with the most work sets the grid, the others finish early
    hipLaunchKernelGGL(pn_infer_fold_kernel, dim3((unsigned)((maxwork + 4 * PNI_T - 1) / (4 * PNI_T)), nscale), dim3(PNI_T), 0,
                       (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------ infer
struct PniArgs {
    const float4 *ent;         // (B, cap) rows (ux, uy, uz, w)
    const int32_t *woff;       // (B, L+1)
    const int32_t *ewin;       // (B, cap) window of each row
    const int32_t *tiles;      // live-tile list (128-row tiles: two workgroups each)
    const int32_t *cnt;        // (B, L) hits per window; 0: the window's single stand-in row publishes nothing
    const v4f *w1f;            // [C1] (a0, a1, a2, t1)
    const u32x4 *F2, *F3;      // folded forward images
    const float *t2, *t3;
    const float *s2, *s3;      // epilogue scales (ones in split mode: the scale is in the weights)
    const float *one_hot;      // (B, nvec) or nullptr
    float *feat;
    int32_t *flags;
    int L, cap, tps, C1, C2, C3, nvec, nlc;
};

template <int MM, int C2T>
__global__ __launch_bounds__(PNI_T) void pn_infer_kernel(PniArgs a)
{
    constexpr int TM = PNI_TM, NTHR = PNI_T;
    constexpr int LDRA = KbTile<TM>::LDR;
    constexpr int AU4 = KbTile<TM>::U4;                       // u32x4 of one 32-deep chunk of a TM-row image
    constexpr int STG = AU4 + KbTile<128>::U4;                // staging: A chunk of GEMM 2 + the widest weight chunk
    static_assert(STG * 4 >= (NTHR / 64) * EP_FLOATS, "the waves' epilogue patches alias the staging buffers");
    __shared__ u32x4 stg[STG];
    __shared__ u32x4 h2img[(C2T / KC) * AU4];
    __shared__ int winS[TM];
    __shared__ float keepS[TM];

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l31 = lane & 31, lh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int xt = fcn_xcd_tile(blockIdx.x, 2 * a.tiles[0]);
    if (xt < 0) return;
    const int lt = xt >> 1, sub = xt & 1;
    const int code = a.tiles[4 + lt];
    const int b = code / a.tps, t = code % a.tps;
    const int L = a.L;
    const int nent = a.woff[(int64_t)b * (L + 1) + L];
    const int row0 = t * 128 + sub * TM;
    const int nvalid = min(TM, nent - row0);
    if (nvalid <= 0) return;
    const int64_t grow0 = (int64_t)b * a.cap + row0;
    const int C3 = a.C3, CT = C3 + a.nvec;

    // the one-hot rows of the reference layout: the frustum's first tile writes them (every frustum has one: an empty window still
    // holds a stand-in row)
    if (!a.nlc && a.nvec > 0 && row0 == 0)
        for (int i = tid; i < a.nvec * L; i += NTHR) {
            const int v = i / L, l = i % L;
            a.feat[((int64_t)b * CT + C3 + v) * L + l] = a.one_hot[(int64_t)b * a.nvec + v];
        }
    if (tid < TM) {
        int pw = -1;
        bool live = false;
        if (tid < nvalid) {
            pw = a.ewin[grow0 + tid];
            live = a.cnt[(int64_t)b * L + pw] > 0;
        }
        winS[tid] = pw;
        keepS[tid] = live ? 1.f : 0.f;
    }
    const int r0 = tid % TM;
    const bool r0valid = r0 < nvalid;
    float ux = 0.f, uy = 0.f, uz = 0.f;
    if (r0valid) {
        const float4 e = a.ent[grow0 + r0];
        ux = e.x; uy = e.y; uz = e.z;
    }
    __syncthreads();

    u32x4 *Ab = stg, *Bb = stg + AU4;
    bool bad = false;
    auto publish = [&](int l, int col, unsigned bits) __attribute__((always_inline)) {
        float *dst = a.nlc ? a.feat + ((int64_t)b * L + l) * C3 + col : a.feat + ((int64_t)b * CT + col) * L + l;
        pni_max_u32((unsigned *)dst, bits, false);
    };

    // one block of 64 * NT output columns of layer LAYER (2: h2 into its LDS image, 3: h3 into the window maxima)
    auto run_block = [&](auto ntc, auto layerc, const int n0) __attribute__((always_inline)) {
        constexpr int NT = decltype(ntc)::value, LAYER = decltype(layerc)::value;
        constexpr int TN = 64 * NT, LDRB = KbTile<TN>::LDR;
        constexpr int NB = TN * 8 / NTHR;                     // u32x4 of the encoded weight per thread per chunk
        const u32x4 *Wenc = LAYER == 2 ? a.F2 : a.F3;
        const int CIN = LAYER == 2 ? a.C1 : a.C2, COUT = LAYER == 2 ? a.C2 : a.C3;
        u32x4 rw[NB];
        const u32x4 *wsrc = Wenc + n0 + (tid % TN) + (int64_t)(tid / TN) * COUT;      // item f = tid + NTHR*i: column f % TN, (plane, k-block) f / TN
        auto load_chunk = [&](int c) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < NB; ++i) rw[i] = ldgu4(wsrc + ((int64_t)c * 8 + i * (NTHR / TN)) * COUT);
        };
        load_chunk(0);
        f32x16 acc[1][NT];
        acc_zero<1, NT>(acc);
        const int nchunk = CIN / KC;
        for (int c = 0; c < nchunk; ++c) {
            if constexpr (LAYER == 2) {
                // h1 of this thread's row, the wave's k-block of the chunk (wave-uniform channel index: the folded rows of conv1
                // come through the scalar cache)
                const int kb = wave;
                float z[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const v4f al = a.w1f[c * KC + 8 * kb + j];
                    const float zz = fmaf(al.x, ux, fmaf(al.y, uy, fmaf(al.z, uz, al.w)));
                    z[j] = r0valid ? pni_relu(zz) : 0.f;
                }
                u32x4 hi, lo;
                enc8<MM>(z, hi, lo);
                Ab[kb * LDRA + r0] = hi;
                Ab[(4 + kb) * LDRA + r0] = lo;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const int f = tid + NTHR * i;
                Bb[(f / TN) * LDRB + (f % TN)] = rw[i];       // (plane, k-block) row f / TN of the image
            }
            __syncthreads();
            if (c + 1 < nchunk) load_chunk(c + 1);
            mma_chunk_kb<MM, 1, NT, LDRA, LDRB>(LAYER == 2 ? Ab : h2img + c * AU4, Bb, wm * 32, wn * 32 * NT, acc);
            __syncthreads();
        }
        // (the staging buffers are free after the last barrier: the patches / the table alias them)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) bad |= !(fabsf(acc[0][nt][reg]) < 3.0e38f);
        if constexpr (LAYER == 2) {
            float *patch = (float *)stg + wave * EP_FLOATS;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                ep_put(patch, acc[0][nt], l31, lh);
                __builtin_amdgcn_wave_barrier();
                const int cbase = n0 + wn * 32 * NT + nt * 32;          // = one 32-deep chunk of GEMM 3's reduction
                u32x4 *img = h2img + (cbase / KC) * AU4;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int idx = lane + 64 * q, row = wm * 32 + (idx >> 3), kq = idx & 7;
                    const v4f v = ep_get(patch, lane, q);
                    const v4f t4 = *(const v4f *)(a.t2 + cbase + 4 * kq), s4 = *(const v4f *)(a.s2 + cbase + 4 * kq);
                    kb_store4<MM, LDRA>(img, row, kq, pni_relu(fmaf(s4.x, v.x, t4.x)), pni_relu(fmaf(s4.y, v.y, t4.y)),
                                        pni_relu(fmaf(s4.z, v.z, t4.z)), pni_relu(fmaf(s4.w, v.w, t4.w)));
                }
                __builtin_amdgcn_wave_barrier();
            }
            __syncthreads();          // h2 complete for every wave; the patches are done before the next block stages
        } else {
            constexpr int NSLOT = (STG * 4 / TN) < TM ? (STG * 4 / TN) : TM;      // window slots of the table (windows past it: direct atomics)
            unsigned *tab = (unsigned *)stg;
            const int win0 = winS[0];
            const int ns = min(winS[nvalid - 1] - win0 + 1, NSLOT);
            for (int i = tid; i < ns * TN; i += NTHR) tab[i] = 0u;
            __syncthreads();
            {
                // a lane's segment = its rows of one window, all NT columns of the lane at once (rows ascend with reg: windows are
                // runs of rows)
                float t3v[NT], s3v[NT], best[NT];
                int cur = -1;
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    t3v[nt] = a.t3[n0 + wn * 32 * NT + nt * 32 + l31];
                    s3v[nt] = a.s3[n0 + wn * 32 * NT + nt * 32 + l31];
                    best[nt] = 0.f;
                }
                auto flush = [&]() __attribute__((always_inline)) {
                    if (cur < 0) return;
                    const int slot = cur - win0;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const unsigned bits = __float_as_uint(best[nt]);
                        if (bits == 0u) continue;
                        const int col = wn * 32 * NT + nt * 32 + l31;
                        if (slot < NSLOT) pni_max_u32(&tab[slot * TN + col], bits, true);
                        else publish(cur, n0 + col, bits);
                    }
                };
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int row = wm * 32 + acc_row(reg, lh);
                    const int w = winS[row];
                    if (w != cur) {
                        flush();
                        cur = w;
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt) best[nt] = 0.f;
                    }
                    const bool keep = keepS[row] != 0.f;
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        const float y = fmaf(s3v[nt], acc[0][nt][reg], t3v[nt]);
                        const float v = (keep && y > 0.f) ? y : 0.f;
                        best[nt] = v > best[nt] ? v : best[nt];
                    }
                }
                flush();
            }
            __syncthreads();
            for (int i = tid; i < ns * TN; i += NTHR) {
                const unsigned bits = tab[i];
                if (bits != 0u) publish(win0 + i / TN, n0 + i % TN, bits);
            }
            __syncthreads();          // the table is read before the next block stages over it
        }
    };

    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    typedef std::integral_constant<int, 3> I3;
    {
        int n0 = 0;
        for (; n0 + 128 <= a.C2; n0 += 128) run_block(I2(), I2(), n0);
        if (n0 < a.C2) run_block(I1(), I2(), n0);
    }
    {
        int n0 = 0;
        for (; n0 + 128 <= C3; n0 += 128) run_block(I2(), I3(), n0);
        if (n0 < C3) run_block(I1(), I3(), n0);
    }
    // fp16 operand parts overflow at |x| >= 65504 (inf - inf = NaN in the products, which the ReLU would turn into a silent zero):
    // a non-finite GEMM output raises the sticky flag in every instantiation (the layered forward raises it in split mode only)
    if (a.flags && __ballot(bad) != 0ull && lane == 0) atomicOr(a.flags, FCN_FLAG_NONFINITE);
}

template <int MM>
static int pni_launch(const PniArgs &a, int B, hipStream_t st)
{
    const unsigned grid = (2u * (unsigned)(B * a.tps) + 7u) / 8u * 8u;
    if (a.C2 <= 64) hipLaunchKernelGGL((pn_infer_kernel<MM, 64>), dim3(grid), dim3(PNI_T), 0, st, a);
    else if (a.C2 <= 128) hipLaunchKernelGGL((pn_infer_kernel<MM, 128>), dim3(grid), dim3(PNI_T), 0, st, a);
    else hipLaunchKernelGGL((pn_infer_kernel<MM, PNI_MAXC2>), dim3(grid), dim3(PNI_T), 0, st, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

extern "C" int fcn_pn_infer(const fcn_pn_desc *d, const int32_t *cnt, const float *one_hot, const fcn_pn_ws *ws,
                            const fcn_pn_infer_ws *iws, float *feat, void *stream)
{
    int rc;
    if (!pni_desc_ok(d, &rc)) return rc;
    if (!cnt || !ws || !iws || !feat || !ws->woff || !ws->ent || !ws->ewin || !ws->tiles) return FCN_E_BADARG;
    if (!iws->w1f || !iws->wenc || !iws->shift) return FCN_E_BADARG;
    if (((uintptr_t)iws->w1f & 15) || ((uintptr_t)iws->wenc & 15) || ((uintptr_t)iws->shift & 15) || ((uintptr_t)ws->ent & 15)) return FCN_E_BADARG;
    if (d->nvec > 0 && !one_hot && !d->nlc) return FCN_E_BADARG;
    PniArgs a;
    a.ent = (const float4 *)ws->ent; a.woff = ws->woff; a.ewin = ws->ewin; a.tiles = ws->tiles; a.cnt = cnt;
    a.w1f = (const v4f *)iws->w1f; a.F2 = (const u32x4 *)iws->wenc; a.F3 = (const u32x4 *)(iws->wenc + (int64_t)d->C2 * d->C1);
    a.t2 = iws->shift; a.t3 = iws->shift + d->C2;
    a.s2 = iws->shift + d->C2 + d->C3; a.s3 = a.s2 + d->C2;
    a.one_hot = one_hot; a.feat = feat; a.flags = ws->flags;
    a.L = d->L; a.cap = d->L * d->K; a.tps = (a.cap + 127) / 128;
    a.C1 = d->C1; a.C2 = d->C2; a.C3 = d->C3; a.nvec = d->nlc ? 0 : d->nvec; a.nlc = d->nlc;
    if (d->precision == FCN_PREC_SPLIT) return pni_launch<MM_F16X3>(a, d->B, (hipStream_t)stream);
    return pni_launch<MM_BF16X1>(a, d->B, (hipStream_t)stream);
}
