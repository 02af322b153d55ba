// The batch builders' random draws on the device (fcn_draw_batch): what inputs.draw() / draw_sunrgbd() / draw_refine() do per
// sample on the host with numpy -- np.random.choice(n, N, n < N), a flip coin, a depth-shift normal and, for SUN-RGBD, a
// height-shift uniform (datasets/provider_sample.py:165-168, :225, :238; provider_sample_sunrgbd.py:144, :211, :224, :228) -- as
// ONE launch that writes the four arrays fcn_prepare_inputs* reads.  The stream is NOT numpy's Mersenne Twister: the contract is
// the counter-based one below (INTEGRATION.md "Random draws on the device"), restated in numpy by tests/draws_ref.py.
//
//   generator  Philox4x32-10, key = (seed lo, seed hi), counter = (i, b, step lo, ((step >> 32) << 2) | tag); b the sample row,
//              step the device-resident counter state[0], tag the stream: 0 permutation keys, 1 indices with replacement, 2 scalars
//   n >= N     row j's 32-bit key k_j = word j & 3 of block j >> 2 (tag 0); composite C_j = (k_j << 32) | j; choice[b, :] = the j of
//              the N smallest composites in ascending order (a uniform N-subset in uniform order up to key ties, which the index
//              breaks: the distance to the ideal distribution is at most about (N + 1)^2 / 2^33)
//   0 < n < N  choice[b, i] = (w * n) >> 32, w = word i & 3 of block i >> 2 (tag 1); relative bias at most n / 2^32
//   scalars    blocks 0 and 1 of tag 2: coin from words 0, 1; u1 from 2, 3; u2 from 4, 5; hshift from 6, 7; 53-bit uniforms,
//              normal = sqrt(-2 ln u1) cos(2 pi u2) in fp64
// One workgroup of 256 threads per sample row; three paths chosen per row:
//   (A) n < N                 direct
//   (B) N <= n <= SORT_CAP    every composite into LDS, bitonic sort on uint64 padded with ~0, the first N written
//   (C) n > SORT_CAP          MSB-first radix select on the composite: a digit histogram in LDS per pass with Philox recomputed
//                             (no n keys in HBM), until the composites below the threshold bin and inside it number at most
//                             SORT_CAP; those are compacted into LDS (LDS atomics hand out the slots; the sort that follows makes
//                             their order irrelevant), sorted, and the first N written.  Composites are unique, so the refinement
//                             ends for any bin occupancy: after 64 bits a bin holds one row.
// A second one-thread launch leaves state[0] + 1 behind, in stream order after every row has read the counter: a captured pair
// of launches draws anew on every replay.
#pragma once
#include "fcn_common.h"

#define DRAW_T 256
#define DRAW_MAX_N 2048
#define DRAW_SORT_CAP 4096
#define DRAW_DIGIT_BITS 8

struct DrawArgs {
    int B, N, flip, shift;
    const int64_t *counts;
    const int32_t *sub;        // optional composition: where sub_off[b + 1] > sub_off[b] the row draws from that many and writes
    const int64_t *sub_off;    // sub[sub_off[b] + c] (SUN-RGBD's 2048-row subsample of a frustum)
    uint64_t seed;
    const int64_t *state;
    int32_t *choice;
    double *coin, *normal, *hshift;
    int32_t *status;
    // the two other forms of the same kernel (draw_batch_kernel's MODE)
    const int64_t *slice_start = nullptr;  // DRAW_SLICED: row b's slice of sub is sub[slice_start[b] ..+ slice_len[b]) (B entries each,
    const int32_t *slice_len = nullptr;    //              no packing assumed); slice_len[b] <= 0: no subsample
    const int32_t *cnt32 = nullptr;        // DRAW_SUBSAMPLE: row b draws from cnt32[b] rows and writes choice[out_off[b] + i], i < N, only
    const int64_t *out_off = nullptr;      //              where out_off[b + 1] > out_off[b]; no scalars
};

#define DRAW_ROWS 0                    // fcn_draw_batch: one row of choice per sample, subsample slices packed behind sub_off (B+1)
#define DRAW_SLICED 1                  // fcn_draw_batch_sliced: the same, slices given as start + length per row
#define DRAW_SUBSAMPLE 2               // fcn_frustum_subsample_draw: the frustum subsamples themselves (tag 0 only)

// The high half of a 32 x 32 product is written as a 64-bit product's upper word: the host build of the tests has no __umulhi.
__device__ __forceinline__ void draw_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                            uint32_t (&o)[4])
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// 53 random bits as an integer-valued double in [0, 2^53)
__device__ __forceinline__ double draw_u53(uint32_t hi, uint32_t lo)
{
    return (double)(hi >> 5) * 67108864.0 + (double)(lo >> 6);
}

// the counter's upper words and the key of stream `tag` at the device-resident step
struct DrawKey {
    uint32_t c2, c3, k0, k1;
};

__device__ __forceinline__ DrawKey draw_key(const int64_t *state, uint64_t seed, uint32_t tag)
{
    const uint64_t step = (uint64_t)state[0];
    return {(uint32_t)step, ((uint32_t)(step >> 32) << 2) | tag, (uint32_t)seed, (uint32_t)(seed >> 32)};
}

// blocks blk0 .. blk0 + NB - 1 of row `row`: 2 * NB uniforms in [0, 1), u[2 i + j] = u53(words 2 j, 2 j + 1 of block blk0 + i) * 2^-53
template <int NB> __device__ __forceinline__ void draw_uniforms(const DrawKey &k, uint32_t blk0, uint32_t row, double (&u)[2 * NB])
{
    const double scale = 1.0 / 9007199254740992.0;         // 2^-53
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        uint32_t w[4];
        draw_philox(blk0 + (uint32_t)i, row, k.c2, k.c3, k.k0, k.k1, w);
        u[2 * i] = draw_u53(w[0], w[1]) * scale;
        u[2 * i + 1] = draw_u53(w[2], w[3]) * scale;
    }
}

template <int DIGIT_BITS, int SORT_CAP, int MODE = DRAW_ROWS>
__global__ __launch_bounds__(DRAW_T) void draw_batch_kernel(DrawArgs a)
{
    static_assert(SORT_CAP >= 2 && (SORT_CAP & (SORT_CAP - 1)) == 0, "the bitonic sort pads to a power of two");
    static_assert(DIGIT_BITS >= 1 && DIGIT_BITS <= 8 && 64 % DIGIT_BITS == 0, "digits tile the 64-bit composite");
    constexpr int NBIN = 1 << DIGIT_BITS;
    __shared__ uint64_t skey[SORT_CAP];
    __shared__ unsigned shist[NBIN];
    __shared__ uint64_t sprefix;
    __shared__ unsigned sbelow, sinbin, scnt;
    const int b = blockIdx.x, tid = threadIdx.x, N = a.N;
    const uint64_t step = (uint64_t)a.state[0];
    const uint32_t c2 = (uint32_t)step, c3 = (uint32_t)(step >> 32) << 2;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    uint32_t w[4];

    if (MODE != DRAW_SUBSAMPLE && tid == 0) {                  // ---- the row's scalars (tag 2)
        const double scale = 1.0 / 9007199254740992.0;         // 2^-53
        uint32_t v[4];
        draw_philox(0u, (uint32_t)b, c2, c3 | 2u, k0, k1, w);
        draw_philox(1u, (uint32_t)b, c2, c3 | 2u, k0, k1, v);
        a.coin[b] = a.flip ? draw_u53(w[0], w[1]) * scale : 0.0;
        double nrm = 0.0, hs = 0.5;
        if (a.shift) {
            const double u1 = (draw_u53(w[2], w[3]) + 1.0) * scale, u2 = draw_u53(v[0], v[1]) * scale;
            nrm = sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
            hs = draw_u53(v[2], v[3]) * scale;
        }
        a.normal[b] = nrm;
        if (a.hshift) a.hshift[b] = hs;
    }

    int64_t n64;
    const int32_t *sub = nullptr;
    int32_t *row;
    if constexpr (MODE == DRAW_SUBSAMPLE) {
        const int64_t o0 = a.out_off[b];
        if (a.out_off[b + 1] <= o0) return;                    // (workgroup-uniform) no subsample for this box
        n64 = a.cnt32[b];
        row = a.choice + o0;
    } else {
        n64 = a.counts[b];
        if constexpr (MODE == DRAW_SLICED) {
            const int32_t len = a.slice_len[b];
            if (len > 0) { n64 = len; sub = a.sub + a.slice_start[b]; }
        } else if (a.sub) {
            const int64_t s0 = a.sub_off[b], s1 = a.sub_off[b + 1];
            if (s1 > s0) { n64 = s1 - s0; sub = a.sub + s0; }
        }
        row = a.choice + (int64_t)b * N;
    }
    if (n64 <= 0 || n64 >= 2147483648LL) {                     // ---- nothing to draw from: zeros (never unwritten) and the flag
        for (int c = tid; c < N; c += DRAW_T) row[c] = 0;
        if (tid == 0) atomicOr(a.status, 1);
        return;
    }
    const uint32_t n = (uint32_t)n64;

    if (n < (uint32_t)N) {                                     // ---- (A) with replacement
        const bool vec = ((uintptr_t)row & 15) == 0;
        for (int i = tid; 4 * i < N; i += DRAW_T) {
            draw_philox((uint32_t)i, (uint32_t)b, c2, c3 | 1u, k0, k1, w);
            int32_t v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t r = (uint32_t)(((uint64_t)w[k] * n) >> 32);
                v[k] = sub ? sub[r] : (int32_t)r;
            }
            if (vec && 4 * i + 3 < N) {
                *(int4 *)(row + 4 * i) = make_int4(v[0], v[1], v[2], v[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (4 * i + k < N) row[4 * i + k] = v[k];
            }
        }
        return;
    }

    const uint32_t nblk = (n + 3u) >> 2;                       // Philox blocks that cover the n keys
    uint32_t m;                                                // composites in LDS
    if (n <= (uint32_t)SORT_CAP) {                             // ---- (B) all of them
        for (uint32_t i = tid; i < nblk; i += DRAW_T) {
            draw_philox(i, (uint32_t)b, c2, c3, k0, k1, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = 4u * i + k;
                if (j < n) skey[j] = ((uint64_t)w[k] << 32) | j;
            }
        }
        m = n;
    } else {                                                   // ---- (C) radix select, most significant digit first
        // invariant: `below` composites have their top `bits` bits < prefix (all of them are drawn, below < N), `inbin` have
        // them == prefix, and below + inbin >= N
        uint64_t prefix = 0;
        uint32_t below = 0, inbin = n;
        int bits = 0;
        while (below + inbin > (uint32_t)SORT_CAP) {           // (workgroup-uniform: the three values come from LDS)
            for (int t = tid; t < NBIN; t += DRAW_T) shist[t] = 0;
            __syncthreads();
            const int sh = 64 - bits - DIGIT_BITS;
            for (uint32_t i = tid; i < nblk; i += DRAW_T) {
                draw_philox(i, (uint32_t)b, c2, c3, k0, k1, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t j = 4u * i + k;
                    const uint64_t C = ((uint64_t)w[k] << 32) | j;
                    if (j < n && (bits == 0 || (C >> (64 - bits)) == prefix)) atomicAdd(&shist[(unsigned)(C >> sh) & (NBIN - 1)], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {                                    // the bin that holds the N-th smallest
                const uint32_t need = (uint32_t)N - below;
                uint32_t cum = 0;
                int t = 0;
                for (; t < NBIN - 1; ++t) {
                    if (cum + shist[t] >= need) break;
                    cum += shist[t];
                }
                sprefix = (prefix << DIGIT_BITS) | (uint64_t)t;
                sbelow = below + cum;
                sinbin = shist[t];
            }
            __syncthreads();
            prefix = sprefix; below = sbelow; inbin = sinbin;
            bits += DIGIT_BITS;
            if (bits >= 64) break;                             // a bin of one row (composites are unique)
        }
        if (tid == 0) scnt = 0;
        __syncthreads();
        const int sh = 64 - bits;                              // bits >= DIGIT_BITS here: n > SORT_CAP ran the loop once
        for (uint32_t i = tid; i < nblk; i += DRAW_T) {
            draw_philox(i, (uint32_t)b, c2, c3, k0, k1, w);
            uint64_t cand[4];
            unsigned mine = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = 4u * i + k;
                const uint64_t C = ((uint64_t)w[k] << 32) | j;
                if (j < n && (C >> sh) <= prefix) cand[mine++] = C;
            }
            if (mine) {
                const unsigned pos = atomicAdd(&scnt, mine);
                for (unsigned q = 0; q < mine; ++q)
                    if (pos + q < (unsigned)SORT_CAP) skey[pos + q] = cand[q];
            }
        }
        m = below + inbin;
        if (m > (uint32_t)SORT_CAP) m = SORT_CAP;              // (cannot happen: below < N <= SORT_CAP and the loop's exit)
    }
    uint32_t P = 1;
    while (P < m) P <<= 1;
    for (uint32_t j = m + tid; j < P; j += DRAW_T) skey[j] = ~0ull;
    __syncthreads();
    // ---- bitonic sort, ascending: pair t of a step is (i, i | j) with bit j of i clear.  The pairs of a step are disjoint, so a
    // thread reads all of its pairs before it writes any: one LDS round trip per step instead of one per pair (the compiler
    // cannot prove that and would order every read behind the previous pair's writes)
    constexpr int PAIRS = (SORT_CAP / 2 + DRAW_T - 1) / DRAW_T;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            uint64_t x[PAIRS], y[PAIRS];
#pragma unroll
            for (int q = 0; q < PAIRS; ++q) {
                const uint32_t t = tid + q * DRAW_T;
                if (t < (P >> 1)) {
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    x[q] = skey[i]; y[q] = skey[i | j];
                }
            }
#pragma unroll
            for (int q = 0; q < PAIRS; ++q) {
                const uint32_t t = tid + q * DRAW_T;
                if (t < (P >> 1)) {
                    const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    if ((x[q] > y[q]) == ((i & k) == 0)) { skey[i] = y[q]; skey[i | j] = x[q]; }
                }
            }
            __syncthreads();
        }
    }
    for (int c = tid; c < N; c += DRAW_T) {
        const uint32_t j = (uint32_t)skey[c];
        row[c] = sub ? sub[j] : (int32_t)j;
    }
}

// state[0] + 1, in stream order behind the rows' reads
static __global__ void draw_advance_kernel(int64_t *state)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) state[0] = state[0] + 1;
}

static inline int draw_advance(int advance, const int64_t *state, hipStream_t stream)
{
    if (advance) {
        hipLaunchKernelGGL(draw_advance_kernel, dim3(1), dim3(64), 0, stream, (int64_t *)state);
        FCN_CHECK_LAUNCH();
    }
    return 0;
}

template <int DIGIT_BITS, int SORT_CAP, int MODE = DRAW_ROWS>
static inline int draw_batch_launch(const DrawArgs &a, hipStream_t stream, bool advance = true)
{
    if (a.B <= 0 || a.N <= 0) return FCN_E_BADARG;
    if (a.N > SORT_CAP) return FCN_E_LIMIT;
    hipLaunchKernelGGL((draw_batch_kernel<DIGIT_BITS, SORT_CAP, MODE>), dim3(a.B), dim3(DRAW_T), 0, stream, a);
    FCN_CHECK_LAUNCH();
    return draw_advance(advance, a.state, stream);
}

#ifndef FCN_DRAWS_NO_ENTRY
extern "C" int fcn_draw_limits(int *max_n, int *sort_cap)
{
    if (!max_n || !sort_cap) return FCN_E_BADARG;
    *max_n = DRAW_MAX_N;
    *sort_cap = DRAW_SORT_CAP;
    return 0;
}

extern "C" int fcn_draw_batch(const fcn_draw_desc *d, const int64_t *counts, const int32_t *sub, const int64_t *sub_off,
                              uint64_t seed, int64_t *state, int32_t *choice, double *coin, double *normal, double *hshift,
                              int32_t *status, void *stream)
{
    if (!d || !counts || !state || !choice || !coin || !normal || !status) return FCN_E_BADARG;
    if ((sub == nullptr) != (sub_off == nullptr)) return FCN_E_BADARG;
    if (d->B <= 0 || d->N <= 0) return FCN_E_BADARG;
    if (d->N > DRAW_MAX_N) return FCN_E_LIMIT;
    DrawArgs a;
    a.B = d->B; a.N = d->N; a.flip = d->random_flip != 0; a.shift = d->random_shift != 0;
    a.counts = counts; a.sub = sub; a.sub_off = sub_off; a.seed = seed; a.state = state; a.choice = choice;
    a.coin = coin; a.normal = normal; a.hshift = hshift; a.status = status;
    return draw_batch_launch<DRAW_DIGIT_BITS, DRAW_SORT_CAP>(a, (hipStream_t)stream);
}
#endif
