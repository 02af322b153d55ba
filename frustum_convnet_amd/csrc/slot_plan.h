// The plan skeleton of the input side: the ONE latency-bound workgroup every capturable sequence puts between its count and fill
// launches -- "of U units with S segment counts each, the units a rule keeps, the first B of them IN UNIT ORDER -> slots, and the
// exclusive prefix sum of the row-holding units' counts (int64, clamped to the capacity of the point buffer)" -- stated once for
// frustum_plan.h, frustum_sunrgbd_plan.h, refine_plan.h, cascade_plan.h and frustum_detect_plan.h, which keep only their rule (a
// POLICY, below), their argument structs and their entry points.  Three steps, each a function of callables:
//   sl_run       thread tid owns the contiguous run [lo, hi) of n items: ceil(n / FP_T) each, the last threads' runs short or empty;
//   sl_assign    every thread applies the rule to its run of units, one scan over the 256 kept counts (fp_block_exscan: a wave scan by
//                __shfl_up, then the four wave totals through LDS) gives its first rank, and it walks the run again: a kept unit's
//                rank is its slot while rank < B; the slots behind the last survivor are handed to the caller's filler;
//   sl_offsets   the same over the flattened U * S counts: every thread sums its run's counts of the units that hold rows (c > 0
//                only), one scan gives its base, and it walks the run again writing soff[i] = min(run, cap) and handing every unit's
//                clamped first row and clamped end to the caller; soff[U * S] is the clamped total.
// Order-preserving scans, no atomics on the data: nothing depends on scheduling.  The status word is OR-ed, never cleared here.
//
// sl_plan_kernel<P> is the kernel of the plans that go from counts to slots and offsets in one launch (the SUN-RGBD plan and slots
// kernels, with a draw between them, and the candidate table of the cascade link are built from the steps alone).  A policy P has
//   P::Args                     the kernel's argument; its member c (SlArgs) is what the skeleton itself reads and writes
//   P::SLOTS                    (static constexpr bool) the units go through a rule and the kept ones get slots; false: every unit
//                               holds its rows and is its own slot (B = U), nothing but soff and off is written, no status is touched
//   P::COUNTS                   (SLOTS only) off[i] and counts[i] per slot: its clamped first row and its STORED rows, an empty slot
//                               reading the spare row `cap` over no rows, off[B] the clamped total; false: off[slot] alone, and
//                               off[n..B] the clamped total
//   P::MANY                     (SLOTS only) more survivors than slots is what is reported (RP_ST_MANY: inference, where fewer is the
//                               normal case); false: fewer is (FP_ST_FEW: training)
//   int live(a, tid, st)        (SLOTS only) the units [0, live) are put to the rule, the rest are dropped unread
//   bool keep(a, u, st)         (SLOTS only) THE rule on unit u; st: status bits to OR in
//   int filler(a)               (SLOTS only) slot_unit of an empty slot
// Everything is resolved at compile time (templates, if constexpr), and an LDS array a policy does not use is not allocated.
#pragma once
#include "fcn_common.h"

#define FP_T 256
#define FP_WAVES (FP_T / 64)
#define FP_MAX_D 2048                  // units (and slots) of one plan: their slots live in LDS
#define FP_MAX_SEGS 65536              // U * S of one plan: 256 segments per thread
#define FP_ST_FEW 2                    // bit 1: fewer survivors than slots
#define FP_ST_TRUNC 4                  // bit 2: rows dropped because the total exceeds the capacity
#define RP_ST_MANY 256                 // bit 8: more survivors than slots

struct SlArgs {
    const int32_t *scnt;               // (U,S)
    int U, S, B;
    int64_t cap;
    int32_t *slot_unit;                // (B)
    int32_t *n_kept;                   // (1)
    int64_t *soff;                     // (U*S+1)
    int64_t *off;                      // (B+1)
    int64_t *counts;                   // (B), P::COUNTS only
    int32_t *status;
};

// exclusive scan of one value per thread over the workgroup, in thread order; total: the sum, in every thread
__device__ __forceinline__ int64_t fp_block_exscan(int64_t v, int64_t *swave, int tid, int64_t &total)
{
    const int lane = tid & 63, wave = tid >> 6;
    int64_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int64_t t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    __syncthreads();                                        // (the previous scan's readers are done with swave)
    if (lane == 63) swave[wave] = inc;
    __syncthreads();
    int64_t base = 0;
    total = 0;
    for (int w = 0; w < FP_WAVES; ++w) {
        if (w < wave) base += swave[w];
        total += swave[w];
    }
    return base + (inc - v);
}

__device__ __forceinline__ void sl_run(int n, int tid, int &lo, int &hi)
{
    const int e = (n + FP_T - 1) / FP_T;
    lo = tid * e < n ? tid * e : n;
    hi = lo + e < n ? lo + e : n;
}

// unit u's S entries of a (U, S) table, summed as they are
__device__ __forceinline__ int64_t sl_unit_sum(const int32_t *v, int u, int S)
{
    int64_t sum = 0;
    for (int s = 0; s < S; ++s) sum += v[(int64_t)u * S + s];
    return sum;
}

// kept(u): the rule; place(u, slot): once per unit, slot -1 without one; empty(i): once per slot i in [n, B).  U <= FP_MAX_D, so a
// run is at most 8 units.  Returns n = min(survivors, B).
template <class Kept, class Place, class Empty>
__device__ __forceinline__ int sl_assign(int U, int B, int64_t *swave, int tid, int64_t &survivors, Kept kept, Place place, Empty empty)
{
    int u0, u1;
    sl_run(U, tid, u0, u1);
    unsigned keep = 0;
    for (int u = u0; u < u1; ++u)
        if (kept(u)) keep |= 1u << (u - u0);
    int64_t rank = fp_block_exscan((int64_t)__popc(keep), swave, tid, survivors);
    for (int u = u0; u < u1; ++u) {
        int slot = -1;
        if (keep & (1u << (u - u0))) {
            if (rank < B) slot = (int)rank;
            rank += 1;
        }
        place(u, slot);
    }
    const int n = survivors < B ? (int)survivors : B;
    for (int i = n + tid; i < B; i += FP_T) empty(i);
    return n;
}

// slot_of(u): >= 0 when unit u holds its rows; first(u, slot, at) / last(u, slot, end): once per unit, its clamped first row and
// the clamped end of its rows.  U * S <= FP_MAX_SEGS.  Returns the unclamped total.
template <class SlotOf, class First, class Last>
__device__ __forceinline__ int64_t sl_offsets(const int32_t *scnt, int U, int S, int64_t cap, int64_t *soff, int64_t *swave, int tid,
                                              SlotOf slot_of, First first, Last last)
{
    const int M = U * S;
    int i0, i1;
    sl_run(M, tid, i0, i1);
    int64_t sum = 0;
    for (int i = i0; i < i1; ++i) {
        const int c = scnt[i];
        if (slot_of(i / S) >= 0 && c > 0) sum += c;
    }
    int64_t total;
    int64_t run = fp_block_exscan(sum, swave, tid, total);
    for (int i = i0; i < i1; ++i) {
        const int u = i / S, slot = slot_of(u);
        const int64_t at = run < cap ? run : cap;
        soff[i] = at;
        if (i % S == 0) first(u, slot, at);
        const int c = scnt[i];
        if (slot >= 0 && c > 0) run += c;
        if (i % S == S - 1) last(u, slot, run < cap ? run : cap);
    }
    if (tid == 0) soff[M] = total < cap ? total : cap;
    return total;
}

template <class P> __global__ __launch_bounds__(FP_T) void sl_plan_kernel(typename P::Args a)
{
    __shared__ int32_t sslot[P::SLOTS ? FP_MAX_D : 1];      // unit -> its slot, -1 without one
    __shared__ int64_t slo[P::COUNTS ? FP_MAX_D : 1], shi[P::COUNTS ? FP_MAX_D : 1];   // slot -> its clamped first row and end
    __shared__ int64_t swave[FP_WAVES];
    const SlArgs &c = a.c;
    const int tid = threadIdx.x, U = c.U, B = c.B;
    int n = U, st = 0;
    int64_t survivors = 0;
    if constexpr (P::SLOTS) {
        const int live = P::live(a, tid, st);
        const int filler = P::filler(a);
        n = sl_assign(U, B, swave, tid, survivors, [&](int u) { return u < live && P::keep(a, u, st); },
                      [&](int u, int slot) {
                          if (slot >= 0) c.slot_unit[slot] = u;
                          sslot[u] = slot;
                      },
                      [&](int i) { c.slot_unit[i] = filler; });
        __syncthreads();
    }
    const int64_t total = sl_offsets(c.scnt, U, c.S, c.cap, c.soff, swave, tid,
                                     [&](int u) {
                                         if constexpr (P::SLOTS) return (int)sslot[u];
                                         else return u;
                                     },
                                     [&](int, int slot, int64_t at) {
                                         if (slot < 0) return;
                                         if constexpr (P::COUNTS) slo[slot] = at;
                                         else c.off[slot] = at;
                                     },
                                     [&](int, int slot, int64_t end) {
                                         if constexpr (P::COUNTS)
                                             if (slot >= 0) shi[slot] = end;
                                     });
    const int64_t end = total < c.cap ? total : c.cap;
    if constexpr (P::COUNTS) {
        __syncthreads();
        for (int i = tid; i < B; i += FP_T) {
            c.off[i] = i < n ? slo[i] : c.cap;
            c.counts[i] = i < n ? shi[i] - slo[i] : 0;
        }
        if (tid == 0) c.off[B] = end;
    } else {
        for (int i = n + tid; i <= B; i += FP_T) c.off[i] = end;
    }
    if constexpr (P::SLOTS) {
        if (tid == 0) {
            c.n_kept[0] = n;
            st |= (P::MANY ? (survivors > B ? RP_ST_MANY : 0) : (survivors < B ? FP_ST_FEW : 0)) | (total > c.cap ? FP_ST_TRUNC : 0);
        }
        if (st) atomicOr(c.status, st);
    }
}

// the size checks the plan entries share (an entry without slots: B = 1)
static inline int sl_sizes(int U, int S, int B, int64_t capacity)
{
    if (U < 0 || S < 1 || B < 1 || capacity < 0) return FCN_E_BADARG;
    if (U > FP_MAX_D || B > FP_MAX_D || (int64_t)U * S > FP_MAX_SEGS) return FCN_E_LIMIT;
    return 0;
}

// one workgroup
template <class A> static inline int sl_launch(void (*kernel)(A), const A &a, void *stream)
{
    hipLaunchKernelGGL(kernel, dim3(1), dim3(FP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}
