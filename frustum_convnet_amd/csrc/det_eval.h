// SUN-RGBD evaluation behind the NMS, on the device (included at the end of box_iou.hip):
//   box3d_corners_kernel   datasets/data_utils.py:44-70 compute_box_3d of the kept rows (train/test_net_det_sunrgbd.py:94-99)
//   det_match_kernel       the matching loop of train/sunrgbd_eval/eval_det.py:134-159 (eval_det_cls): every detection against
//                          every label box of its image and class, greedy in descending score
//   det_ap_kernel          the curve and the area of :161-169 + voc_ap (:41-72, use_07_metric=False)
//   det_rows_kernel        the keep lists of the NMS packed group after group (what SunrgbdDetector.detect_frames does on the host
//                          behind a read-back of keep / cnt), for the capturable chain of evaluate.SunrgbdFrameChain
// The reference does all of it in Python, one boost / scipy polygon clip per (detection, label) pair on the host; here the
// corners, the overlaps and the flags stay in HBM and the host reads the AP table.  The clip core is box_iou.h.
//
// Order-free form of the greedy walk.  The reference sorts a class's detections by descending score and walks them once; a
// detection only ever looks at ITS best label jmax (first maximum under strict >), so two detections interact only when they
// share (image, class) and jmax.  Walking in descending score, the first detection with ovmax > thresh on a label takes it and
// every later one with the same jmax is a false positive -- also when a second label would qualify.  Hence
//   tp[d] = ovmax[d] > thresh  and no detection e of the same group with jmax[e] == jmax[d], ovmax[e] > thresh that comes
//           before d in (score descending, input index ascending)
// which needs no sort and no sequential walk: one pairwise pass inside the group.  Equal scores: the lower input index comes
// first (np.argsort in the reference is unstable there; this is the documented rule).
#pragma once
#include "slot_plan.h"

#define DEV_T 256
#define DR_MAX_G (FP_T * 256)          // groups of one fcn_det_rows: 256 per thread
#define DR_ST_OVER 2048                // bit 11: a group's cnt is -1 (the NMS met more than 4096 candidates: no keep list)

// The (BEV IoU, 3-D IoU) of rbbox_iou_3d_pair (box_ops.h:173-260) from two (8,3) corner arrays in the order of compute_box_3d:
// BEV polygon = corners 6,7,4,5 (x,z), y extents from corners 0 and 4.  What eval_det.py:84-86 get_iou_cc asks per pair.
struct DetPoly {
    float x[4], z[4], ytop, ybot;
};
__device__ __forceinline__ void det_poly_load(const float *c, DetPoly &p)
{
    const int ord[4] = {6, 7, 4, 5};
#pragma unroll
    for (int k = 0; k < 4; ++k) { p.x[k] = c[ord[k] * 3]; p.z[k] = c[ord[k] * 3 + 2]; }
    p.ytop = c[1];
    p.ybot = c[13];
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void box3d_corners_kernel(const float *__restrict__ dets, int R, const int32_t *__restrict__ rows,
                                                            int n, float *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = rows ? rows[i] : i;
    float *o = out + (int64_t)i * 24;
    if (r < 0 || r >= R) {                                                 // (an unused keep slot, -1): never dereferenced
        for (int k = 0; k < 24; ++k) o[k] = __builtin_nanf("");
        return;
    }
    const float *d = dets + (int64_t)r * 8;
    const float co = cosf(d[6]), si = sinf(d[6]);
    const float hl = d[3] / 2.f, hw = d[4] / 2.f, hh = d[5] / 2.f;
    // x = +l/2 +l/2 -l/2 -l/2 (twice), y = +h/2 x 4, -h/2 x 4, z = +w/2 -w/2 -w/2 +w/2 (twice); roty: X = c x + s z, Z = -s x + c z
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float x = (k & 2) ? -hl : hl;
        const float y = (k & 4) ? -hh : hh;
        const float z = ((k & 3) == 1 || (k & 3) == 2) ? -hw : hw;
        o[k * 3] = co * x + si * z + d[0];
        o[k * 3 + 1] = y + d[1];
        o[k * 3 + 2] = -si * x + co * z + d[2];
    }
}

extern "C" int fcn_box3d_corners(const float *dets, int num_dets, const int32_t *rows, int n, float *corners, void *stream)
{
    if (n < 0 || num_dets < 0) return FCN_E_BADARG;
    if (n == 0) return 0;
    if (!corners || (num_dets > 0 && !dets)) return FCN_E_BADARG;
    if (!rows && n > num_dets) return FCN_E_BADARG;
    hipLaunchKernelGGL(box3d_corners_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, dets, num_dets, rows, n,
                       corners);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
struct DetMatchArgs {
    const int32_t *det_off, *gt_off;   // (G+1) each: the detections / label boxes of group g are rows [off[g], off[g+1])
    const float *det_c, *score;        // (nd,8,3), (nd)
    const float *gt_c;                 // (ng,8,3)
    int nd, ng;
    float thresh;
    int32_t *tp;                       // (nd)
    float *ovmax;                      // (nd): -inf in a group without a label box (eval_det.py:141)
    int32_t *jmax;                     // (nd): index of the best label INSIDE its group (the reference's j), -1 without one
};

// One workgroup per (image, class) group; both loops stride over the workgroup, so nd and ng of a group are unbounded.  The
// offsets are clamped to [0, nd] / [0, ng]: a bad offset array reads and writes nothing outside the buffers.
__global__ __launch_bounds__(DEV_T) void det_match_kernel(DetMatchArgs a)
{
    const int g = blockIdx.x, tid = threadIdx.x;
    const int d0 = max(0, min(a.nd, a.det_off[g])), d1 = max(d0, min(a.nd, a.det_off[g + 1]));
    const int g0 = max(0, min(a.ng, a.gt_off[g])), g1 = max(g0, min(a.ng, a.gt_off[g + 1]));
    // pass 1: ovmax / jmax of every detection (first maximum under strict >)
    for (int d = d0 + tid; d < d1; d += DEV_T) {
        DetPoly p;
        det_poly_load(a.det_c + (int64_t)d * 24, p);
        float best = -INFINITY;
        int bj = -1;
        for (int j = g0; j < g1; ++j) {
            DetPoly q;
            det_poly_load(a.gt_c + (int64_t)j * 24, q);
            float i2, i3;
            fcn_iou_from_polys(p.x, p.z, p.ytop, p.ybot, q.x, q.z, q.ytop, q.ybot, &i2, &i3);
            if (i3 > best) { best = i3; bj = j - g0; }
        }
        a.ovmax[d] = best;
        a.jmax[d] = bj;
    }
    __syncthreads();                                                       // (the group's ovmax / jmax are this workgroup's own stores)
    // pass 2: the greedy walk in its order-free form (see the head of this file)
    for (int d = d0 + tid; d < d1; d += DEV_T) {
        const float ov = a.ovmax[d], s = a.score[d];
        const int j = a.jmax[d];
        int t = (j >= 0 && ov > a.thresh) ? 1 : 0;
        for (int e = d0; t && e < d1; ++e) {
            if (e == d || a.jmax[e] != j || !(a.ovmax[e] > a.thresh)) continue;
            const float se = a.score[e];
            if (se > s || (se == s && e < d)) t = 0;                       // e takes the label first
        }
        a.tp[d] = t;
    }
}

extern "C" int fcn_det_match(const int32_t *det_off, const int32_t *gt_off, int G, const float *det_corners, const float *scores,
                             int nd, const float *gt_corners, int ng, float thresh, int32_t *tp, float *ovmax, int32_t *jmax,
                             void *stream)
{
    if (G < 0 || nd < 0 || ng < 0 || !(thresh == thresh)) return FCN_E_BADARG;
    if (G > 0 && (!det_off || !gt_off)) return FCN_E_BADARG;
    if (nd > 0 && (!det_corners || !scores || !tp || !ovmax || !jmax)) return FCN_E_BADARG;
    if (ng > 0 && !gt_corners) return FCN_E_BADARG;
    if (G == 0 || nd == 0) return 0;
    DetMatchArgs a;
    a.det_off = det_off; a.gt_off = gt_off; a.det_c = det_corners; a.score = scores; a.gt_c = gt_corners; a.nd = nd; a.ng = ng;
    a.thresh = thresh; a.tp = tp; a.ovmax = ovmax; a.jmax = jmax;
    hipLaunchKernelGGL(det_match_kernel, dim3(G), dim3(DEV_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
struct DetApArgs {
    const int32_t *tp;                 // (nd)
    const float *score;                // (nd)
    const int32_t *cls;                // (nd): class of each detection, in [0, C)
    const int32_t *npos;               // (C): label boxes of each class (> 0: the caller's duty, npos is host knowledge)
    int nd;
    int32_t *rank;                     // (nd): place of detection d among its class by (score descending, index ascending)
    double *rec, *prec;                // (nd): class c's curve at [base_c, base_c + n_c), base_c = detections of classes < c
    double *ap;                        // (C)
};

// One workgroup per class.  Counts are int32, the curve and the area fp64.
__global__ __launch_bounds__(DEV_T) void det_ap_kernel(DetApArgs a)
{
    __shared__ int si[DEV_T], sj[DEV_T];
    __shared__ double sd[DEV_T];
    const int c = blockIdx.x, tid = threadIdx.x, nd = a.nd;
    // ---- where the class's curve lives and how long it is
    int lt = 0, eq = 0;
    for (int d = tid; d < nd; d += DEV_T) {
        const int k = a.cls[d];
        lt += (k < c) ? 1 : 0;
        eq += (k == c) ? 1 : 0;
    }
    si[tid] = lt;
    sj[tid] = eq;
    __syncthreads();
    for (int o = DEV_T / 2; o > 0; o >>= 1) {
        if (tid < o) { si[tid] += si[tid + o]; sj[tid] += sj[tid + o]; }
        __syncthreads();
    }
    const int base = si[0], n = sj[0];                                     // base + n <= nd whatever cls holds
    __syncthreads();
    // ---- rank by pairwise count, tp into rank order (staged in rec as 0 / 1)
    for (int d = tid; d < nd; d += DEV_T) {
        if (a.cls[d] != c) continue;
        const float s = a.score[d];
        int r = 0;
        for (int e = 0; e < nd; ++e) {
            if (a.cls[e] != c) continue;
            const float se = a.score[e];
            r += (se > s || (se == s && e < d)) ? 1 : 0;
        }
        a.rank[d] = r;
        a.rec[base + r] = a.tp[d] != 0 ? 1.0 : 0.0;                        // r < n: at most n - 1 others come before d
    }
    __syncthreads();
    // ---- cumulative tp over the whole class: chunks of the workgroup's width with a carry
    const double np = (double)a.npos[c];
    int carry = 0;
    for (int k0 = 0; k0 < n; k0 += DEV_T) {
        const int k = k0 + tid;
        si[tid] = (k < n && a.rec[base + k] > 0.5) ? 1 : 0;
        __syncthreads();
        for (int o = 1; o < DEV_T; o <<= 1) {
            const int t = tid >= o ? si[tid - o] : 0;
            __syncthreads();
            si[tid] += t;
            __syncthreads();
        }
        const int tpc = carry + si[tid];                                   // tp + fp = k + 1
        if (k < n) {
            a.rec[base + k] = (double)tpc / np;
            a.prec[base + k] = (double)tpc / fmax((double)(k + 1), 2.220446049250313e-16);
        }
        carry += si[DEV_T - 1];
        __syncthreads();
    }
    // ---- precision envelope (reverse running maximum, sentinel 0 behind the end) and sum of (delta rec) * envelope
    double run = 0.0, acc = 0.0;
    for (int k0 = ((n - 1) / DEV_T) * DEV_T; n > 0 && k0 >= 0; k0 -= DEV_T) {
        const int k = k0 + tid;
        sd[tid] = k < n ? a.prec[base + k] : 0.0;
        __syncthreads();
        for (int o = 1; o < DEV_T; o <<= 1) {
            const double t = tid + o < DEV_T ? sd[tid + o] : 0.0;
            __syncthreads();
            sd[tid] = fmax(sd[tid], t);
            __syncthreads();
        }
        if (k < n) {
            const double env = fmax(sd[tid], run);
            const double r1 = a.rec[base + k], r0 = k > 0 ? a.rec[base + k - 1] : 0.0;
            acc += (r1 - r0) * env;
        }
        run = fmax(run, sd[0]);
        __syncthreads();
    }
    sd[tid] = acc;
    __syncthreads();
    for (int o = DEV_T / 2; o > 0; o >>= 1) {
        if (tid < o) sd[tid] += sd[tid + o];
        __syncthreads();
    }
    if (tid == 0) a.ap[c] = sd[0];                                         // a class without a detection: 0, as voc_ap([], [])
}

extern "C" int fcn_det_ap(const int32_t *tp, const float *scores, const int32_t *det_class, int nd, const int32_t *npos, int C,
                          int32_t *rank, double *rec, double *prec, double *ap, void *stream)
{
    if (nd < 0 || C < 0) return FCN_E_BADARG;
    if (C > 0 && (!npos || !ap)) return FCN_E_BADARG;
    if (nd > 0 && (!tp || !scores || !det_class || !rank || !rec || !prec)) return FCN_E_BADARG;
    if (C == 0) return 0;
    DetApArgs a;
    a.tp = tp; a.score = scores; a.cls = det_class; a.npos = npos; a.nd = nd; a.rank = rank; a.rec = rec; a.prec = prec;
    a.ap = ap;
    hipLaunchKernelGGL(det_ap_kernel, dim3(C), dim3(DEV_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The tail of a capturable detection chain, one workgroup behind fcn_rotate_nms_3d: keep (G, top_k) / cnt (G) -> the kept rows group
// after group in keep order, their scores, and the groups' offsets -- what SunrgbdDetector.detect_frames builds on the host from a
// read-back of keep / cnt.  The steps of slot_plan.h: every thread owns a run of groups (sl_run), one fp_block_exscan over the runs'
// clamped counts gives its base, the offsets go to det_off; behind a barrier the whole workgroup walks the G * top_k keep entries
// (coalesced) and stores entry (g, j), j < c_g, at det_off[g] + j.  Order-preserving, no atomics on the data.
struct DetRowsArgs {
    const int32_t *keep, *cnt;         // (G, top_k), (G)
    const float *dets;                 // (num_dets, 8)
    int G, top_k, num_dets;
    int32_t *det_off;                  // (G+1)
    int32_t *rows;                     // (G*top_k)
    float *scores;                     // (G*top_k)
    int32_t *n_rows, *status;          // (1) each
};

__global__ __launch_bounds__(FP_T) void det_rows_kernel(DetRowsArgs a)
{
    __shared__ int64_t swave[FP_WAVES];
    const int tid = threadIdx.x, G = a.G, K = a.top_k;
    int g0, g1;
    sl_run(G, tid, g0, g1);
    int64_t mine = 0;
    bool over = false;
    for (int g = g0; g < g1; ++g) {
        const int c = a.cnt[g];
        over = over || c == -1;
        mine += c < 0 ? 0 : (c > K ? K : c);
    }
    int64_t total;
    int64_t at = fp_block_exscan(mine, swave, tid, total);
    for (int g = g0; g < g1; ++g) {
        const int c = a.cnt[g];
        a.det_off[g] = (int32_t)at;
        at += c < 0 ? 0 : (c > K ? K : c);
    }
    if (tid == 0) { a.det_off[G] = (int32_t)total; a.n_rows[0] = (int32_t)total; }
    if (over) atomicOr(a.status, DR_ST_OVER);
    __syncthreads();                                                       // (det_off: this workgroup's own stores)
    const int64_t E = (int64_t)G * K;
    for (int64_t e = tid; e < E; e += FP_T) {
        const int g = (int)(e / K), j = (int)(e % K);
        const int c = a.cnt[g];
        if (j >= (c < 0 ? 0 : (c > K ? K : c))) continue;
        const int r = a.keep[e];
        const int64_t o = (int64_t)a.det_off[g] + j;
        a.rows[o] = r;
        a.scores[o] = (r >= 0 && r < a.num_dets) ? a.dets[(int64_t)r * 8 + 7] : __builtin_nanf("");   // never dereferenced
    }
    for (int64_t e = total + tid; e < E; e += FP_T) { a.rows[e] = -1; a.scores[e] = __builtin_nanf(""); }
}

extern "C" int fcn_det_rows(const int32_t *keep, const int32_t *cnt, int G, int top_k, const float *dets, int num_dets,
                            int32_t *det_off, int32_t *rows, float *scores, int32_t *n_rows, int32_t *status, void *stream)
{
    if (!keep || !cnt || !det_off || !rows || !scores || !n_rows || !status) return FCN_E_BADARG;
    if (G < 1 || top_k < 1 || num_dets < 0 || (num_dets > 0 && !dets)) return FCN_E_BADARG;
    if (G > DR_MAX_G || top_k > 4096 || (int64_t)G * top_k > 0x7fffffff) return FCN_E_LIMIT;
    DetRowsArgs a;
    a.keep = keep; a.cnt = cnt; a.dets = dets; a.G = G; a.top_k = top_k; a.num_dets = num_dets; a.det_off = det_off; a.rows = rows;
    a.scores = scores; a.n_rows = n_rows; a.status = status;
    return sl_launch(det_rows_kernel, a, stream);
}
