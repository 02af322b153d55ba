// Two-stage INFERENCE with NO host read between its launches: what TwoStageDetector.detect does on the host between the first
// stage's NMS and the second stage's forward -- the keep lists flattened into a candidate table, the D point counts read for the
// reject rule and the prefix sum, the D predicted widths read for the window counts -- as launches that read nothing back: a fixed
// number of candidates D, a fixed batch of B slots at fixed window counts, capturable into a hipGraph (INTEGRATION.md "Capturable
// two-stage inference" states the contract bit for bit; tests/cascade_plan_ref.py restates it in numpy):
//   fcn_cascade_candidates     ONE workgroup: keep (G, top_k) / cnt (G) of fcn_rotate_nms_3d -> the first D kept rows, groups
//                              ascending and keep order inside a group, with the frame, class and group of the frustum each row came
//                              from (row / L2) and its score.  An order-preserving scan over the groups' valid entries
//                              (fp_block_exscan, slot_plan.h): no atomics on the data, nothing depends on scheduling.
//   fcn_refine_detect_count    the count / fill of refine_select.h on the SEGMENTED (S, D) grid of seg_compact.h -- CdSelect is
//   fcn_refine_detect_fill     RsSelect with WHOLE = false: the same geometry, predicate and header, the same row loop -- launched
//                              without a read-back of the candidate lists: the kernels skip a candidate whose row or frame is out of
//                              range (the filler rows of the table included); "no frame longer than S * FS_SEG rows" is the caller's
//                              duty (checked once, where the frames are made resident);
//   fcn_refine_detect_plan     the plan skeleton of slot_plan.h with RpPlan<true> (refine_plan.h) between the two, the positives
//                              being the counts themselves: the reference's lidar_point_threshold = 1
//                              (prepare_data_refine.py:739-741) as the reject rule.
// Status bits (one int32 word, OR-ed, never cleared here): CD_ST_ROWS more kept rows than D; RP_ST_MANY more surviving candidates
// than B; CD_ST_GROUP a group that overflowed the NMS (cnt = -1) or reports cnt > top_k, passed on to nobody; FP_ST_TRUNC, RP_ST_WIDE
// and RP_ST_WIDTH as the training plan sets them (bit 0 is DeviceDraws').
#pragma once
#include "refine_select.h"
#include "refine_plan.h"

#define CD_ST_ROWS 128                 // bit 7
#define CD_ST_GROUP 512                // bit 9
#define CD_MAX_G 65536                 // groups of one call: 256 per thread

struct CdCandArgs {
    const int32_t *keep, *cnt;         // (G, top_k), (G)
    const int32_t *uframe, *uclass, *ugroup;       // (B1)
    const float *dets;                 // (R, 8)
    int G, top_k, L2, B1, R, D;
    int32_t *crow, *cframe, *cclass, *cgroup;      // (D)
    float *cscore;                     // (D)
    int32_t *n_cand, *status;
};

// the entries of group g that are passed on: none of a group whose count is no count; false: the group is flagged
__device__ __forceinline__ bool cd_group(const CdCandArgs &a, int g, int &c)
{
    c = a.cnt[g];
    if (c < 0 || c > a.top_k) { c = 0; return false; }
    return true;
}

// a keep entry that is a row of dets and comes from a frustum of the batch
__device__ __forceinline__ bool cd_entry(const CdCandArgs &a, int row) { return row >= 0 && row < a.R && row / a.L2 < a.B1; }

__global__ __launch_bounds__(FP_T) void cd_candidates_kernel(CdCandArgs a)
{
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x, G = a.G, D = a.D;
    // the groups of this thread's run: count their valid entries, scan, walk them again to write
    int g0, g1;
    sl_run(G, tid, g0, g1);
    int64_t sum = 0;
    int st = 0;
    for (int g = g0; g < g1; ++g) {
        int c;
        if (!cd_group(a, g, c)) st |= CD_ST_GROUP;
        for (int k = 0; k < c; ++k) sum += cd_entry(a, a.keep[(int64_t)g * a.top_k + k]) ? 1 : 0;
    }
    int64_t total;
    int64_t run = fp_block_exscan(sum, swave, tid, total);
    for (int g = g0; g < g1 && run < D; ++g) {
        int c;
        cd_group(a, g, c);
        for (int k = 0; k < c && run < D; ++k) {
            const int row = a.keep[(int64_t)g * a.top_k + k];
            if (!cd_entry(a, row)) continue;
            const int u = row / a.L2;
            a.crow[run] = row;
            a.cframe[run] = a.uframe[u];
            a.cclass[run] = a.uclass[u];
            a.cgroup[run] = a.ugroup[u];
            a.cscore[run] = a.dets[(int64_t)row * 8 + 7];
            run += 1;
        }
    }
    // the filler behind the kept rows: a candidate the count skips, of the spare group G
    const int n = total < D ? (int)total : D;
    for (int i = n + tid; i < D; i += FP_T) {
        a.crow[i] = -1; a.cframe[i] = -1; a.cclass[i] = 0; a.cgroup[i] = G; a.cscore[i] = 0.f;
    }
    if (st) atomicOr(a.status, st);
    if (tid == 0) {
        a.n_cand[0] = n;
        if (total > D) atomicOr(a.status, CD_ST_ROWS);
    }
}

extern "C" int fcn_cascade_candidates(const int32_t *keep, const int32_t *cnt, int G, int top_k, int L2, const int32_t *unit_frame,
                                      const int32_t *unit_class, const int32_t *unit_group, int B1, const float *dets, int R, int D,
                                      int32_t *cand_row, int32_t *cand_frame, int32_t *cand_class, int32_t *cand_group,
                                      float *cand_score, int32_t *n_cand, int32_t *status, void *stream)
{
    if (!keep || !cnt || !unit_frame || !unit_class || !unit_group || !dets || !cand_row || !cand_frame || !cand_class ||
        !cand_group || !cand_score || !n_cand || !status)
        return FCN_E_BADARG;
    if (G < 1 || top_k < 1 || L2 < 1 || B1 < 1 || R < 1 || D < 1) return FCN_E_BADARG;
    if (G > CD_MAX_G || D > FP_MAX_D) return FCN_E_LIMIT;
    CdCandArgs a;
    a.keep = keep; a.cnt = cnt; a.uframe = unit_frame; a.uclass = unit_class; a.ugroup = unit_group; a.dets = dets;
    a.G = G; a.top_k = top_k; a.L2 = L2; a.B1 = B1; a.R = R; a.D = D;
    a.crow = cand_row; a.cframe = cand_frame; a.cclass = cand_class; a.cgroup = cand_group; a.cscore = cand_score;
    a.n_cand = n_cand; a.status = status;
    return sl_launch(cd_candidates_kernel, a, stream);
}

// ---- count / fill: RsSelect on the segmented grid
struct CdSelect : RsSelect {
    static constexpr bool WHOLE = false;
};

static inline bool cd_sizes_ok(int F, int pt_stride, int R, int D, int S)
{
    return pt_stride >= 3 && D >= 0 && D <= FS_MAX_D && F >= 0 && R >= 0 && S >= 1;        // candidates are the grid's y dimension
}

extern "C" int fcn_refine_detect_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                       int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, int S,
                                       int32_t *seg_cnt, double *pred_corners, double *pred_angle, double *pred_size, void *stream)
{
    if (!cd_sizes_ok(F, pt_stride, R, D, S)) return FCN_E_BADARG;
    if (D == 0) return 0;
    if (!seg_cnt) return FCN_E_BADARG;
    if (F == 0) return sc_zero_counts(seg_cnt, nullptr, (size_t)D * S, (hipStream_t)stream);
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !pred_corners || !pred_angle || !pred_size)
        return FCN_E_BADARG;
    RsArgs a;
    rs_args(a, frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, ratio);
    a.c.S = S;
    a.corners = pred_corners; a.angle = pred_angle; a.size = pred_size; a.c.scnt = seg_cnt;
    return sc_launch<CdSelect, false>(a, D, nullptr, 0, D, nullptr, F, (hipStream_t)stream, false);
}

extern "C" int fcn_refine_detect_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets,
                                      int R, const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, int S,
                                      const int64_t *seg_off, float *out_pts, void *stream)
{
    if (!cd_sizes_ok(F, pt_stride, R, D, S)) return FCN_E_BADARG;
    if (D == 0 || F == 0) return 0;
    if (!frame_pts || !frame_off || !dets || !cand_row || !cand_frame || !seg_off || !out_pts) return FCN_E_BADARG;
    RsArgs a;
    rs_args(a, frame_pts, frame_off, F, pt_stride, dets, R, cand_row, cand_frame, ratio);
    a.c.S = S;
    a.c.soff = seg_off; a.c.out = out_pts;
    return sc_launch<CdSelect, true>(a, D, nullptr, 0, D, nullptr, F, (hipStream_t)stream, false);
}

// ---- the plan: the training plan's rule with the counts as the positives
extern "C" int fcn_refine_detect_plan(const int32_t *seg_cnt, const double *pred_size, const double *stride, const int32_t *lpad,
                                      int D, int S, int B, int64_t capacity, int32_t *slot_unit, int32_t *n_kept, int64_t *seg_off,
                                      int64_t *off, int64_t *counts, int32_t *status, void *stream)
{
    return rp_plan_launch<true>(seg_cnt, seg_cnt, pred_size, stride, lpad, D, S, B, capacity, slot_unit, n_kept, seg_off, off, counts,
                                status, stream);
}
