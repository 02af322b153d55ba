// Epoch-exact label sampling on the device (fcn_epoch_pick): what the reference's DataLoader(shuffle=True, drop_last=True) does for
// the training sources (train/train_net_det.py:262-269) -- a fresh permutation of the G records per epoch, every record at most once
// per epoch, the tail that fills no batch dropped -- as ONE launch per step with 16 bytes of state and no G-sized table anywhere
// (INTEGRATION.md "Epoch-exact label sampling" states the contract; tests/draws_ref.choice_row(seed, e, 0, G, G) is perm_e).
//
//   permutation  perm_e = the j of the G composites C_j = (k_j << 32) | j in ascending order, k_j = word j & 3 of Philox block
//                j >> 2 at counter (block, 0, e lo, ((e >> 32) << 2) | 0), key (seed lo, seed hi): draws.h's tag-0 order of row 0
//                with the epoch as the step
//   window       state = (epoch e, turn t); pick[i] = perm_e[r0 + i], i < D, r0 = (t * world + rank) * D
//   advance      T = G / (D * world) turns per epoch (integer division: the tail of G - T * D * world labels is dropped); the
//                state left behind is (e, t + 1) if t + 1 < T, else (e + 1, 0)
//   failure      G <= 0, G >= 2^31, D * world > G, e < 0, t < 0 or t >= T: pick all zeros, status bit 0, the state as it was
// One workgroup of 256 threads; two paths:
//   (B) G <= SORT_CAP   every composite into LDS, bitonic sort on uint64 padded with ~0, ranks r0 .. r0 + D - 1 written
//   (C) G > SORT_CAP    a rank-window select with Philox recomputed in every pass (no G keys in HBM), in two steps:
//                       1. r0 > 0: an MSB-first radix walk towards the composite of rank r0 -- a digit histogram in LDS per pass,
//                          the bin that holds rank r0 refined -- until the composites below the bin number exactly r0: then
//                          lo = the bin's smallest possible composite separates the ranks < r0 from the ranks >= r0.  At most
//                          64 / DIGIT_BITS passes: after 64 bits a bin holds one composite (they are unique), the one of rank r0.
//                       2. draws.h's select of the D smallest among the composites >= lo: refine until the composites below the
//                          threshold bin and inside it number at most SORT_CAP, compact them into LDS, sort, the first D written.
// Every loop condition is workgroup-uniform: the values it tests come from LDS behind a barrier (or from the state, which every
// thread read alike).
// The state is advanced in THIS launch, behind a barrier of the same workgroup: every thread reads state[0..1] into registers on
// entry, the sort's barriers and one more lie between those reads and the one store by thread 0 at the very end, and there is no
// second workgroup.  A captured launch therefore moves on at every replay, as draw_advance_kernel's second launch does for draws.h.
#pragma once
#include "draws.h"

struct EpochArgs {
    const int64_t *count;      // (1) device: G
    int D, rank, world, advance;
    uint64_t seed;
    int64_t *state;            // (2) device: epoch, turn
    int32_t *pick;             // (D)
    int32_t *status;
};

template <int DIGIT_BITS, int SORT_CAP>
__global__ __launch_bounds__(DRAW_T) void epoch_pick_kernel(EpochArgs a)
{
    static_assert(SORT_CAP >= 2 && (SORT_CAP & (SORT_CAP - 1)) == 0, "the bitonic sort pads to a power of two");
    static_assert(DIGIT_BITS >= 1 && DIGIT_BITS <= 8 && 64 % DIGIT_BITS == 0, "digits tile the 64-bit composite");
    constexpr int NBIN = 1 << DIGIT_BITS;
    __shared__ uint64_t skey[SORT_CAP];
    __shared__ unsigned shist[NBIN];
    __shared__ uint64_t sprefix;
    __shared__ unsigned sbelow, sinbin, scnt;
    const int tid = threadIdx.x, D = a.D;
    const int64_t G = a.count[0], e = a.state[0], t = a.state[1];     // (every thread: the state is read before it is written)
    const int64_t DW = (int64_t)D * a.world;
    const int64_t T = (G > 0 && G < 2147483648LL) ? G / DW : 0;
    if (T <= 0 || e < 0 || t < 0 || t >= T) {                  // ---- (workgroup-uniform) no window: zeros, the flag, the state kept
        for (int c = tid; c < D; c += DRAW_T) a.pick[c] = 0;
        if (tid == 0) atomicOr(a.status, 1);
        return;
    }
    const uint32_t n = (uint32_t)G;
    const uint32_t r0 = (uint32_t)((t * a.world + a.rank) * D);         // r0 + D <= T * D * world <= G
    const uint32_t c2 = (uint32_t)(uint64_t)e, c3 = (uint32_t)((uint64_t)e >> 32) << 2;
    const uint32_t k0 = (uint32_t)a.seed, k1 = (uint32_t)(a.seed >> 32);
    const uint32_t nblk = (n + 3u) >> 2;                       // Philox blocks that cover the n keys
    uint32_t w[4];
    uint32_t m, base;                                          // composites in LDS; the window's first rank among them
    if (n <= (uint32_t)SORT_CAP) {                             // ---- (B) all of them
        for (uint32_t i = tid; i < nblk; i += DRAW_T) {
            draw_philox(i, 0u, c2, c3, k0, k1, w);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = 4u * i + k;
                if (j < n) skey[j] = ((uint64_t)w[k] << 32) | j;
            }
        }
        m = n;
        base = r0;
    } else {                                                   // ---- (C)
        // step 1.  invariant: `below` composites have their top `bits` bits < prefix, below <= r0, and the composite of rank r0
        // has them == prefix
        uint64_t prefix = 0;
        uint32_t below = 0;
        int bits = 0;
        while (below < r0) {                                   // (workgroup-uniform: below comes from LDS, r0 from the state)
            for (int q = tid; q < NBIN; q += DRAW_T) shist[q] = 0;
            __syncthreads();
            const int sh = 64 - bits - DIGIT_BITS;
            for (uint32_t i = tid; i < nblk; i += DRAW_T) {
                draw_philox(i, 0u, c2, c3, k0, k1, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t j = 4u * i + k;
                    const uint64_t C = ((uint64_t)w[k] << 32) | j;
                    if (j < n && (bits == 0 || (C >> (64 - bits)) == prefix)) atomicAdd(&shist[(unsigned)(C >> sh) & (NBIN - 1)], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {                                    // the bin that holds rank r0
                const uint32_t need = r0 - below;              // its rank among the bin's composites, from 0
                uint32_t cum = 0;
                int q = 0;
                for (; q < NBIN - 1; ++q) {
                    if (cum + shist[q] > need) break;
                    cum += shist[q];
                }
                sprefix = (prefix << DIGIT_BITS) | (uint64_t)q;
                sbelow = below + cum;
            }
            __syncthreads();
            prefix = sprefix; below = sbelow;
            bits += DIGIT_BITS;
            if (bits >= 64) break;                             // a bin of one composite: the one of rank r0, so below == r0
        }
        const uint64_t lo = bits ? prefix << (64 - bits) : 0;  // C >= lo  <=>  rank(C) >= r0
        // step 2.  among the composites >= lo: `below` of them have their top `bits` bits < prefix (all of them are in the window,
        // below < D), `inbin` have them == prefix, and below + inbin >= D
        prefix = 0; below = 0; bits = 0;
        uint32_t inbin = n - r0;
        while (below + inbin > (uint32_t)SORT_CAP) {           // (workgroup-uniform: the values come from LDS)
            for (int q = tid; q < NBIN; q += DRAW_T) shist[q] = 0;
            __syncthreads();
            const int sh = 64 - bits - DIGIT_BITS;
            for (uint32_t i = tid; i < nblk; i += DRAW_T) {
                draw_philox(i, 0u, c2, c3, k0, k1, w);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t j = 4u * i + k;
                    const uint64_t C = ((uint64_t)w[k] << 32) | j;
                    if (j < n && C >= lo && (bits == 0 || (C >> (64 - bits)) == prefix))
                        atomicAdd(&shist[(unsigned)(C >> sh) & (NBIN - 1)], 1u);
                }
            }
            __syncthreads();
            if (tid == 0) {                                    // the bin that holds the window's last rank
                const uint32_t need = (uint32_t)D - below;
                uint32_t cum = 0;
                int q = 0;
                for (; q < NBIN - 1; ++q) {
                    if (cum + shist[q] >= need) break;
                    cum += shist[q];
                }
                sprefix = (prefix << DIGIT_BITS) | (uint64_t)q;
                sbelow = below + cum;
                sinbin = shist[q];
            }
            __syncthreads();
            prefix = sprefix; below = sbelow; inbin = sinbin;
            bits += DIGIT_BITS;
            if (bits >= 64) break;                             // a bin of one composite
        }
        if (tid == 0) scnt = 0;
        __syncthreads();
        for (uint32_t i = tid; i < nblk; i += DRAW_T) {
            draw_philox(i, 0u, c2, c3, k0, k1, w);
            uint64_t cand[4];
            unsigned mine = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t j = 4u * i + k;
                const uint64_t C = ((uint64_t)w[k] << 32) | j;
                if (j < n && C >= lo && (bits == 0 || (C >> (64 - bits)) <= prefix)) cand[mine++] = C;
            }
            if (mine) {
                const unsigned pos = atomicAdd(&scnt, mine);
                for (unsigned q = 0; q < mine; ++q)
                    if (pos + q < (unsigned)SORT_CAP) skey[pos + q] = cand[q];
            }
        }
        m = below + inbin;
        if (m > (uint32_t)SORT_CAP) m = SORT_CAP;              // (cannot happen: below < D <= SORT_CAP and the loop's exit)
        base = 0;
    }
    uint32_t P = 1;
    while (P < m) P <<= 1;
    for (uint32_t j = m + tid; j < P; j += DRAW_T) skey[j] = ~0ull;
    __syncthreads();
    // ---- bitonic sort, ascending, as in draw_batch_kernel: a thread reads all of its disjoint pairs of a step before it writes any
    constexpr int PAIRS = (SORT_CAP / 2 + DRAW_T - 1) / DRAW_T;
    for (uint32_t k = 2; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            uint64_t x[PAIRS], y[PAIRS];
#pragma unroll
            for (int q = 0; q < PAIRS; ++q) {
                const uint32_t p = tid + q * DRAW_T;
                if (p < (P >> 1)) {
                    const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    x[q] = skey[i]; y[q] = skey[i | j];
                }
            }
#pragma unroll
            for (int q = 0; q < PAIRS; ++q) {
                const uint32_t p = tid + q * DRAW_T;
                if (p < (P >> 1)) {
                    const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                    if ((x[q] > y[q]) == ((i & k) == 0)) { skey[i] = y[q]; skey[i | j] = x[q]; }
                }
            }
            __syncthreads();
        }
    }
    for (int c = tid; c < D; c += DRAW_T) a.pick[c] = (int32_t)(uint32_t)skey[base + c];    // base + D <= m
    if (a.advance) {                                           // ---- the next turn, behind every thread's read of the state
        __syncthreads();
        if (tid == 0) {
            if (t + 1 < T) {
                a.state[1] = t + 1;
            } else {
                a.state[0] = e + 1;
                a.state[1] = 0;
            }
        }
    }
}

template <int DIGIT_BITS, int SORT_CAP> static inline int epoch_pick_launch(const EpochArgs &a, hipStream_t stream)
{
    if (!a.count || !a.state || !a.pick || !a.status) return FCN_E_BADARG;
    if (a.D < 1 || a.world < 1 || a.rank < 0 || a.rank >= a.world) return FCN_E_BADARG;
    if (a.D > SORT_CAP) return FCN_E_LIMIT;
    hipLaunchKernelGGL((epoch_pick_kernel<DIGIT_BITS, SORT_CAP>), dim3(1), dim3(DRAW_T), 0, stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

#ifndef FCN_DRAWS_NO_ENTRY
extern "C" int fcn_epoch_pick_limits(int *max_d, int *sort_cap)
{
    if (!max_d || !sort_cap) return FCN_E_BADARG;
    *max_d = DRAW_MAX_N;
    *sort_cap = DRAW_SORT_CAP;
    return 0;
}

extern "C" int fcn_epoch_pick(const int64_t *count, int D, int rank, int world, uint64_t seed, int64_t *state, int advance,
                              int32_t *pick, int32_t *status, void *stream)
{
    if (!count || !state || !pick || !status || D < 1 || world < 1 || rank < 0 || rank >= world) return FCN_E_BADARG;
    if (D > DRAW_MAX_N) return FCN_E_LIMIT;
    EpochArgs a;
    a.count = count; a.D = D; a.rank = rank; a.world = world; a.advance = advance != 0; a.seed = seed; a.state = state;
    a.pick = pick; a.status = status;
    return epoch_pick_launch<DRAW_DIGIT_BITS, DRAW_SORT_CAP>(a, (hipStream_t)stream);
}
#endif
