// SUN-RGBD INFERENCE with NO host read between its launches: what frustum.sunrgbd_candidates (two range-checking read-backs, the
// D * S segment counts read for the prefix sum, a host rng.choice per frustum over `cap` rows) and SunrgbdInputBuilder.build_device
// (the kept list from the host counts) do on the host, as launches that read nothing back -- a table of at most D 2-D detections, a
// fixed batch of B slots, capturable into a hipGraph (INTEGRATION.md "Capturable SUN-RGBD inference" states the contract bit for
// bit; tests/sunrgbd_detect_plan_ref.py restates it in numpy):
//   fcn_frustum_sunrgbd_detect_count  the count / fill of frustum_sunrgbd.h (seg_compact.h with SrSelect<false>: geometry, predicate
//   fcn_frustum_sunrgbd_detect_fill   and row loop unchanged), launched as fcn_frustum_detect_count / _fill launch frustum_select.h:
//                                     without a read-back, the kernels skipping a box whose frame is out of range and a box at or
//                                     beyond the device-resident box count n_boxes (its counts are zero, nothing of it is read or
//                                     stored); "no frame longer than S * FS_SEG rows" is the caller's duty (checked once, where the
//                                     frames are made resident);
//   fcn_frustum_sunrgbd_detect_plan   ONE workgroup between the two, built from the steps of slot_plan.h (sl_plan_kernel<P> itself
//                                     does not fit: a policy has no per-slot outputs of its own, and the subsample offsets need a
//                                     third scan behind the slots' STORED counts): sl_assign under build_device's rule
//                                     min(count, cap) >= max(1, point_threshold) on the boxes that are live and whose frame and
//                                     class are in range, sl_offsets over the slot-holding boxes' segment counts, then per slot
//                                     off, the stored rows, the (frame, class) group and -- one fp_block_exscan over the slots --
//                                     its slice of the subsample table.
// The subsample table is laid out PER SLOT, packed: slot i's slice is sub[sub_off[i] .. sub_off[i + 1]), `cap` entries where the
// slot stored more than `cap` rows, else empty -- at most B * cap entries, and (cnt32, sub_off, B) is what fcn_frustum_subsample_draw
// takes as (cnt_stored, sub_off, D), unchanged; (sub_start, sub_len) is what fcn_draw_batch_sliced takes.  Every count behind the
// plan is the STORED count: no index ever points at a row that was not stored.  Order-preserving scans, no atomics on the data.
// Status bits (one int32 word, OR-ed, never cleared here): FP_ST_TRUNC rows dropped because the total exceeds the capacity;
// RP_ST_MANY more survivors than slots; FD_ST_RANGE n_boxes outside [0, D] (taken as 0 / D) or a live box whose frame is outside
// [0, F) or whose class is outside [0, C) (the box is ignored, never dereferenced).  Fewer survivors than slots sets no bit.
#pragma once
#include "frustum_sunrgbd_plan.h"
#include "frustum_detect_plan.h"

struct SdArgs : SrArgs {
    const int32_t *nbox;               // (1) the boxes of the table that are live
};

// SrSelect<false> behind the device-resident box count: the geometry, the predicate and the header are frustum_sunrgbd.h's
struct SdSelect : SrSelect<false> {
    using Args = SdArgs;
    __device__ __forceinline__ bool setup(const SdArgs &a, int d, int64_t &p0, int64_t &m)
    {
        return d < a.nbox[0] && sr_setup(a, d, b, p0, m);
    }
};

struct SdPlanArgs {
    SlArgs c;
    const int32_t *bframe, *bclass;    // (D) each; entry d is read only when box d is live
    const int32_t *nbox;               // (1)
    int min_pts, sub_cap, F, C;
    int32_t *cnt32;                    // (B) the stored rows again, as fcn_frustum_subsample_draw reads them
    int64_t *sub_off;                  // (B+1)
    int64_t *sub_start;                // (B)
    int32_t *sub_len;                  // (B)
    int32_t *slot_group;               // (B)
};

__global__ __launch_bounds__(FP_T) void sd_plan_kernel(SdPlanArgs a)
{
    __shared__ int32_t sslot[FP_MAX_D];                     // box -> its slot, -1 without one
    __shared__ int64_t slo[FP_MAX_D], shi[FP_MAX_D];        // slot -> its clamped first row and end
    __shared__ int64_t swave[FP_WAVES];
    const SlArgs &c = a.c;
    const int tid = threadIdx.x, D = c.U, B = c.B;
    int st = 0;
    int live = a.nbox[0];
    if (live < 0 || live > D) {
        if (tid == 0) st |= FD_ST_RANGE;
        live = live < 0 ? 0 : D;
    }
    const int bar = a.min_pts > 1 ? a.min_pts : 1;
    int64_t survivors;
    const int n = sl_assign(D, B, swave, tid, survivors,
                            [&](int d) {
                                if (d >= live) return false;
                                const int f = a.bframe[d], k = a.bclass[d];
                                if (f < 0 || f >= a.F || k < 0 || k >= a.C) { st |= FD_ST_RANGE; return false; }
                                int64_t cnt = 0;
                                for (int s = 0; s < c.S; ++s) {
                                    const int v = c.scnt[(int64_t)d * c.S + s];
                                    if (v > 0) cnt += v;
                                }
                                // SunrgbdInputBuilder.build_device: rows = min(count, cap); kept = rows >= max(1, point_threshold)
                                return (cnt < a.sub_cap ? cnt : (int64_t)a.sub_cap) >= bar;
                            },
                            [&](int d, int slot) {
                                if (slot >= 0) {
                                    c.slot_unit[slot] = d;
                                    a.slot_group[slot] = a.bframe[d] * a.C + a.bclass[d];
                                }
                                sslot[d] = slot;
                            },
                            [&](int i) { c.slot_unit[i] = D; a.slot_group[i] = a.F * a.C; });   // the spare row, the spare group
    __syncthreads();
    const int64_t total = sl_offsets(c.scnt, D, c.S, c.cap, c.soff, swave, tid, [&](int d) { return (int)sslot[d]; },
                                     [&](int, int slot, int64_t at) { if (slot >= 0) slo[slot] = at; },
                                     [&](int, int slot, int64_t end) { if (slot >= 0) shi[slot] = end; });
    __syncthreads();
    // ---- per slot: off, the STORED rows, and the slice of the subsample table of a slot that stored more than sub_cap rows
    int i0, i1;
    sl_run(B, tid, i0, i1);
    int64_t mine = 0;
    for (int i = i0; i < i1; ++i) {
        const int64_t rows = i < n ? shi[i] - slo[i] : 0;
        c.off[i] = i < n ? slo[i] : c.cap;                  // an empty slot reads the spare row `capacity` over no rows
        c.counts[i] = rows;
        a.cnt32[i] = rows < 0x7fffffff ? (int32_t)rows : 0x7fffffff;
        if (rows > a.sub_cap) mine += a.sub_cap;
    }
    int64_t all;
    int64_t at = fp_block_exscan(mine, swave, tid, all);
    for (int i = i0; i < i1; ++i) {
        const bool sub = i < n && shi[i] - slo[i] > a.sub_cap;
        a.sub_off[i] = at;
        a.sub_start[i] = sub ? at : 0;
        a.sub_len[i] = sub ? a.sub_cap : 0;
        if (sub) at += a.sub_cap;
    }
    if (tid == 0) {
        a.sub_off[B] = all;
        c.off[B] = total < c.cap ? total : c.cap;
        c.n_kept[0] = n;
        st |= (survivors > B ? RP_ST_MANY : 0) | (total > c.cap ? FP_ST_TRUNC : 0);
    }
    if (st) atomicOr(c.status, st);
}

// ---- count / fill: SrSelect<false> behind n_boxes, without the read-backs
extern "C" int fcn_frustum_sunrgbd_detect_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride,
                                                const double *K, const double *Rtilt, const double *boxes, const int32_t *box_frame,
                                                int D, int S, const int32_t *n_boxes, double *frustum_angle, int32_t *seg_cnt,
                                                void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, nullptr, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !K || !Rtilt || !boxes || !box_frame || !n_boxes || !frustum_angle) return FCN_E_BADARG;
    SdArgs a;
    sr_args(a, frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, S);
    a.nbox = n_boxes;
    a.angle = frustum_angle; a.c.scnt = seg_cnt;
    return sc_launch<SdSelect, false>(a, D, nullptr, 0, D, nullptr, F, (hipStream_t)stream, false);
}

extern "C" int fcn_frustum_sunrgbd_detect_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride,
                                               const double *K, const double *Rtilt, const double *boxes, const int32_t *box_frame,
                                               int D, int S, const int32_t *n_boxes, const int64_t *seg_off, float *out_pts,
                                               void *stream)
{
    if (!fs_sizes_ok(F, pt_stride, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !K || !Rtilt || !boxes || !box_frame || !n_boxes || !seg_off || !out_pts) return FCN_E_BADARG;
    SdArgs a;
    sr_args(a, frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, S);
    a.nbox = n_boxes;
    a.c.soff = seg_off; a.c.out = out_pts;
    return sc_launch<SdSelect, true>(a, D, nullptr, 0, D, nullptr, F, (hipStream_t)stream, false);
}

// ---- the plan
extern "C" int fcn_frustum_sunrgbd_detect_plan(const int32_t *seg_cnt, const int32_t *box_frame, const int32_t *box_class,
                                               const int32_t *n_boxes, int point_threshold, int cap, int D, int S, int B,
                                               int64_t capacity, int F, int C, int32_t *slot_box, int32_t *n_kept, int64_t *seg_off,
                                               int64_t *off, int64_t *counts, int32_t *cnt32, int64_t *sub_off, int64_t *sub_start,
                                               int32_t *sub_len, int32_t *slot_group, int32_t *status, void *stream)
{
    if (!seg_cnt || !box_frame || !box_class || !n_boxes || !slot_box || !n_kept || !seg_off || !off || !counts || !cnt32 || !sub_off ||
        !sub_start || !sub_len || !slot_group || !status)
        return FCN_E_BADARG;
    if (cap < 1 || F < 0 || C < 1 || (int64_t)F * C > 0x7fffffff) return FCN_E_BADARG;
    FCN_TRY(sl_sizes(D, S, B, capacity));
    SdPlanArgs a;
    a.c = SlArgs{seg_cnt, D, S, B, capacity, slot_box, n_kept, seg_off, off, counts, status};
    a.bframe = box_frame; a.bclass = box_class; a.nbox = n_boxes;
    a.min_pts = point_threshold; a.sub_cap = cap; a.F = F; a.C = C;
    a.cnt32 = cnt32; a.sub_off = sub_off; a.sub_start = sub_start; a.sub_len = sub_len; a.slot_group = slot_group;
    return sl_launch(sd_plan_kernel, a, stream);
}
