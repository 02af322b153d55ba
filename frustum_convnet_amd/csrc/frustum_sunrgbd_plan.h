// The SUN-RGBD training input with NO host read between its launches: what frustum.perturb_boxes2d_sunrgbd, the host block of
// frustum.sunrgbd_training_candidates (full-positive bar, prefix sum of the segment counts, rng.choice of every frustum over `cap`
// rows, post-subsample bar, kept list) and the host look-ups of SunrgbdInputBuilder.build_device_train do per step, as launches
// that read nothing back -- a fixed batch of B slots, capturable into a hipGraph (INTEGRATION.md "Capturable SUN-RGBD training
// input" states the contract bit for bit; tests/sunrgbd_plan_ref.py restates it in numpy):
//   fcn_box2d_perturb_sunrgbd        sunrgbd/sunrgbd_utils.py::random_shift_box2d (:208-221) for D boxes, one lane per box, on tag 3 of
//                                    the draws' counter layout (fcn_box2d_perturb's stream): no clip, no retry, nothing can fail;
//   fcn_frustum_sunrgbd_train_count  the labelled count / fill of frustum_sunrgbd.h (seg_compact.h with SrSelect<true>), launched without
//   fcn_frustum_sunrgbd_train_fill   a read-back: the kernels skip a box whose frame is out of range; "no frame longer than
//                                    S * FS_SEG rows" is the caller's duty (checked once, where the frames are made resident);
//   fcn_frustum_sunrgbd_train_plan   ONE workgroup between the two, built from the steps of slot_plan.h: the full-positive bar per box
//                                    (pre-kept, no slots yet), sl_offsets over the pre-kept boxes' segment counts, the rows of each
//                                    box that fit under the clamp (cnt_stored) and the offsets of the subsample table;
//   fcn_frustum_subsample_draw       draw_batch_kernel of draws.h in its DRAW_SUBSAMPLE form: for every box of more than `cap` STORED
//                                    rows the row-d choice of fcn_draw_batch at N = cap, n = cnt_stored[d] (the whole-row LDS sort and
//                                    the radix select are that kernel's: there is one selection);
//   fcn_frustum_sunrgbd_train_slots  ONE workgroup behind fcn_frustum_subset_pos: sl_assign under the post-subsample bar, and per
//                                    slot what fcn_draw_batch_sliced and fcn_prepare_inputs_sunrgbd read;
//   fcn_draw_batch_sliced            draw_batch_kernel in its DRAW_SLICED form: fcn_draw_batch with a (start, length) pair per row in
//                                    place of the packed sub_off.
// From the plan on every count is cnt_stored: no index ever points at a row that was not stored.  Order-preserving scans, no atomics
// on the data: the result does not depend on scheduling.  Status bits (one int32 word, OR-ed, never cleared here): FP_ST_FEW fewer
// than B survivors; FP_ST_TRUNC rows dropped because the total exceeds the capacity (bit 0 is the draws'; bit 4 is never set here).
#pragma once
#include "draws.h"
#include "slot_plan.h"
#include "frustum_sunrgbd.h"

struct SpPerturbArgs {
    const double *boxes;               // (D,4)
    int D;
    double r;
    uint64_t seed;
    const int64_t *state;
    double *out;                       // (D,4)
};

// Arithmetic exactly as frustum.perturb_boxes2d_sunrgbd writes it, fp64, every operation on its own (-ffp-contract=off): bit-exact
// against Python floats given the same uniforms.
__global__ __launch_bounds__(FP_T) void sp_perturb_kernel(SpPerturbArgs a)
{
    const int d = blockIdx.x * FP_T + threadIdx.x;
    if (d >= a.D) return;
    const double *q = a.boxes + (int64_t)d * 4;
    const double xmin = q[0], ymin = q[1], xmax = q[2], ymax = q[3];
    const double h = ymax - ymin, w = xmax - xmin;
    const double cx = (xmin + xmax) / 2.0, cy = (ymin + ymax) / 2.0;
    const double r = a.r;
    double u[4];
    draw_uniforms<2>(draw_key(a.state, a.seed, 3u), 0u, (uint32_t)d, u);
    const double cx2 = cx + (w * r) * (u[0] * 2.0 - 1.0);
    const double cy2 = cy + (h * r) * (u[1] * 2.0 - 1.0);
    const double h2 = h * ((1.0 + (u[2] * 2.0) * r) - r);
    const double w2 = w * ((1.0 + (u[3] * 2.0) * r) - r);
    double *o = a.out + (int64_t)d * 4;
    o[0] = cx2 - w2 / 2.0; o[1] = cy2 - h2 / 2.0; o[2] = cx2 + w2 / 2.0; o[3] = cy2 + h2 / 2.0;
}

struct SpPlanArgs {
    const int32_t *scnt, *spos;        // (D,S)
    int min_pos, cap, D, S;
    int64_t capacity;
    int64_t *soff;                     // (D*S+1)
    int64_t *row0;                     // (D)
    int32_t *cnt_stored;               // (D)
    int64_t *sub_off;                  // (D+1)
    int32_t *status;
};

__global__ __launch_bounds__(FP_T) void sp_plan_kernel(SpPlanArgs a)
{
    __shared__ int32_t skeep[FP_MAX_D];                     // box -> pre-kept: 0, else -1 (sl_offsets' "slot")
    __shared__ int64_t sstart[FP_MAX_D + 1];                // box -> its first row (clamped); [D] the clamped total
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x, D = a.D;
    int d0, d1;
    sl_run(D, tid, d0, d1);
    for (int d = d0; d < d1; ++d) skeep[d] = sl_unit_sum(a.spos, d, a.S) >= a.min_pos ? 0 : -1;     // the full-positive bar
    __syncthreads();
    const int64_t total = sl_offsets(a.scnt, D, a.S, a.capacity, a.soff, swave, tid, [&](int d) { return (int)skeep[d]; },
                                     [&](int d, int, int64_t at) { a.row0[d] = at; sstart[d] = at; }, [](int, int, int64_t) {});
    if (tid == 0) {
        sstart[D] = total < a.capacity ? total : a.capacity;
        if (total > a.capacity) atomicOr(a.status, FP_ST_TRUNC);
    }
    __syncthreads();
    // ---- the rows each box stored and the subsample table's offsets: boxes [d0, d1) again
    int64_t mine = 0;
    for (int d = d0; d < d1; ++d) {
        const int32_t c = (int32_t)(sstart[d + 1] - sstart[d]);     // a dropped box starts where the next one does: 0
        a.cnt_stored[d] = c;
        if (c > a.cap) mine += a.cap;
    }
    int64_t all;
    int64_t at = fp_block_exscan(mine, swave, tid, all);
    for (int d = d0; d < d1; ++d) {
        a.sub_off[d] = at;
        if ((int32_t)(sstart[d + 1] - sstart[d]) > a.cap) at += a.cap;
    }
    if (tid == 0) a.sub_off[D] = all;
}

struct SpSlotsArgs {
    const int32_t *spos;               // (D,S)
    const int32_t *pos;                // (D) the positives after the subsample
    const int64_t *row0;               // (D)
    const int32_t *cnt_stored;         // (D)
    const int64_t *sub_off;            // (D+1)
    int min_pos, D, S, B;
    int64_t capacity;
    int32_t *slot_box;                 // (B)
    int32_t *n_kept;                   // (1)
    int64_t *off;                      // (B)
    int64_t *counts;                   // (B)
    int64_t *sub_start;                // (B)
    int32_t *sub_len;                  // (B)
    int32_t *status;
};

__global__ __launch_bounds__(FP_T) void sp_slots_kernel(SpSlotsArgs a)
{
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x;
    int64_t survivors;
    const int n = sl_assign(a.D, a.B, swave, tid, survivors,
                            [&](int d) { return sl_unit_sum(a.spos, d, a.S) >= a.min_pos && a.pos[d] >= a.min_pos; },
                            [&](int d, int i) {
                                if (i < 0) return;
                                const int64_t s0 = a.sub_off[d], s1 = a.sub_off[d + 1];
                                a.slot_box[i] = d;
                                a.off[i] = a.row0[d];
                                a.counts[i] = a.cnt_stored[d];
                                a.sub_start[i] = s1 > s0 ? s0 : 0;
                                a.sub_len[i] = s1 > s0 ? (int32_t)(s1 - s0) : 0;
                            },
                            [&](int i) {                    // an empty slot: box 0's labels over no rows, reading the spare row
                                a.slot_box[i] = 0; a.off[i] = a.capacity; a.counts[i] = 0; a.sub_start[i] = 0; a.sub_len[i] = 0;
                            });
    if (tid == 0) {
        a.n_kept[0] = n;
        if (survivors < a.B) atomicOr(a.status, FP_ST_FEW);
    }
}

extern "C" int fcn_box2d_perturb_sunrgbd(const double *boxes, int D, double shift_ratio, uint64_t seed, const int64_t *state,
                                         int advance, double *out, void *stream)
{
    if (!boxes || !state || !out) return FCN_E_BADARG;
    if (D < 0 || !(shift_ratio >= 0.0 && shift_ratio < 1.0)) return FCN_E_BADARG;
    if (D > 0) {
        SpPerturbArgs a;
        a.boxes = boxes; a.D = D; a.r = shift_ratio; a.seed = seed; a.state = state; a.out = out;
        hipLaunchKernelGGL(sp_perturb_kernel, dim3((D + FP_T - 1) / FP_T), dim3(FP_T), 0, (hipStream_t)stream, a);
        FCN_CHECK_LAUNCH();
    }
    return draw_advance(advance, state, (hipStream_t)stream);
}

extern "C" int fcn_frustum_sunrgbd_train_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride,
                                               const double *K, const double *Rtilt, const double *boxes, const int32_t *box_frame,
                                               int D, int S, const double *gt_box3d, double *frustum_angle, int32_t *seg_cnt,
                                               int32_t *seg_pos, double *corners, void *stream)
{
    return sr_label_count_launch(frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, D, S, gt_box3d, frustum_angle, seg_cnt,
                                 seg_pos, corners, stream, false);
}

extern "C" int fcn_frustum_sunrgbd_train_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride,
                                              const double *K, const double *Rtilt, const double *boxes, const int32_t *box_frame,
                                              int D, int S, const double *gt_box3d, const int64_t *seg_off, float *out_pts,
                                              int64_t *out_seg, void *stream)
{
    return sr_label_fill_launch(frame_pts, frame_off, F, pt_stride, K, Rtilt, boxes, box_frame, D, S, gt_box3d, seg_off, out_pts,
                                out_seg, stream, false);
}

extern "C" int fcn_frustum_sunrgbd_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, int min_positives, int cap, int D, int S,
                                              int64_t capacity, int64_t *seg_off, int64_t *row0, int32_t *cnt_stored,
                                              int64_t *sub_off, int32_t *status, void *stream)
{
    if (!seg_cnt || !seg_pos || !seg_off || !row0 || !cnt_stored || !sub_off || !status) return FCN_E_BADARG;
    if (cap < 1) return FCN_E_BADARG;
    FCN_TRY(sl_sizes(D, S, 1, capacity));
    SpPlanArgs a;
    a.scnt = seg_cnt; a.spos = seg_pos; a.min_pos = min_positives; a.cap = cap; a.D = D; a.S = S; a.capacity = capacity;
    a.soff = seg_off; a.row0 = row0; a.cnt_stored = cnt_stored; a.sub_off = sub_off; a.status = status;
    return sl_launch(sp_plan_kernel, a, stream);
}

extern "C" int fcn_frustum_subsample_draw(const int32_t *cnt_stored, const int64_t *sub_off, int D, int cap, uint64_t seed,
                                          int64_t *state, int advance, int32_t *sub, int32_t *status, void *stream)
{
    if (!cnt_stored || !sub_off || !state || !sub || !status) return FCN_E_BADARG;
    if (D < 0 || cap < 1) return FCN_E_BADARG;
    if (cap > DRAW_MAX_N) return FCN_E_LIMIT;
    if (D > 0) {
        DrawArgs a;
        a.B = D; a.N = cap; a.flip = 0; a.shift = 0; a.counts = nullptr; a.sub = nullptr; a.sub_off = nullptr; a.seed = seed;
        a.state = state; a.choice = sub; a.coin = nullptr; a.normal = nullptr; a.hshift = nullptr; a.status = status;
        a.cnt32 = cnt_stored; a.out_off = sub_off;
        FCN_TRY((draw_batch_launch<DRAW_DIGIT_BITS, DRAW_SORT_CAP, DRAW_SUBSAMPLE>(a, (hipStream_t)stream, false)));
    }
    return draw_advance(advance, state, (hipStream_t)stream);
}

extern "C" int fcn_frustum_sunrgbd_train_slots(const int32_t *seg_pos, const int32_t *pos, const int64_t *row0,
                                               const int32_t *cnt_stored, const int64_t *sub_off, int min_positives, int D, int S,
                                               int B, int64_t capacity, int32_t *slot_box, int32_t *n_kept, int64_t *off,
                                               int64_t *counts, int64_t *sub_start, int32_t *sub_len, int32_t *status, void *stream)
{
    if (!seg_pos || !pos || !row0 || !cnt_stored || !sub_off || !slot_box || !n_kept || !off || !counts || !sub_start || !sub_len ||
        !status)
        return FCN_E_BADARG;
    FCN_TRY(sl_sizes(D, S, B, capacity));
    SpSlotsArgs a;
    a.spos = seg_pos; a.pos = pos; a.row0 = row0; a.cnt_stored = cnt_stored; a.sub_off = sub_off; a.min_pos = min_positives;
    a.D = D; a.S = S; a.B = B; a.capacity = capacity; a.slot_box = slot_box; a.n_kept = n_kept; a.off = off; a.counts = counts;
    a.sub_start = sub_start; a.sub_len = sub_len; a.status = status;
    return sl_launch(sp_slots_kernel, a, stream);
}

extern "C" int fcn_draw_batch_sliced(const fcn_draw_desc *d, const int64_t *counts, const int32_t *sub, const int64_t *sub_start,
                                     const int32_t *sub_len, uint64_t seed, int64_t *state, int32_t *choice, double *coin,
                                     double *normal, double *hshift, int32_t *status, void *stream)
{
    if (!d || !counts || !sub || !sub_start || !sub_len || !state || !choice || !coin || !normal || !status) return FCN_E_BADARG;
    if (d->B <= 0 || d->N <= 0) return FCN_E_BADARG;
    if (d->N > DRAW_MAX_N) return FCN_E_LIMIT;
    DrawArgs a;
    a.B = d->B; a.N = d->N; a.flip = d->random_flip != 0; a.shift = d->random_shift != 0;
    a.counts = counts; a.sub = sub; a.sub_off = nullptr; a.seed = seed; a.state = state; a.choice = choice;
    a.coin = coin; a.normal = normal; a.hshift = hshift; a.status = status; a.slice_start = sub_start; a.slice_len = sub_len;
    return draw_batch_launch<DRAW_DIGIT_BITS, DRAW_SORT_CAP, DRAW_SLICED>(a, (hipStream_t)stream);
}
