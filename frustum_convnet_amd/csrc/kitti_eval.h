// KITTI evaluation behind the NMS, on the device (included at the end of box_iou.hip):
//   kitti_label_rows_kernel   the label-format row of every kept detection, train/test_net_det.py:88-105,284-293 with compute_alpha
//                             of datasets/provider_sample.py:389-394
//   kitti_overlaps_kernel     imageBoxOverlap / groundBoxOverlap / box3DOverlap of every (detection, label) pair of a frame, once
//                             (train/kitti_eval/evaluate_object_3d_offline.cpp:229-346) + the host-side rules of :158-172
//   kitti_pass_a_kernel       cleanData (:383-456) + computeStatistics(compute_fp = false) (:458-555): the true positives' scores
//   kitti_thresholds_kernel   getThresholds (:348-381)
//   kitti_pass_b_kernel       cleanData + computeStatistics(compute_fp = true) for all threshold slots of a list in one launch
//   kitti_curves_kernel       precision / AOS, the suffix maximum and the 11-point AP (:680-699, :716-720)
// The reference writes text files and shells out to a program that clips every pair with boost polygons up to 42 times; here a
// pair is clipped once (box_iou.h), in fp32, and everything behind it stays in HBM until the table.  Lines cited without a file
// are evaluate_object_3d_offline.cpp.
//
// Indices.  A "list" k = (metric * 3 + class) * 3 + difficulty, 27 of them; metric 0 image, 1 ground, 2 3-D; class 0 car,
// 1 pedestrian, 2 cyclist.  Label types: 0 Car, 1 Pedestrian, 2 Cyclist, 3 Van, 4 Person_sitting, 5 DontCare, 6 anything else.
//
// The walks stay sequential where the reference's carry state (assigned_detection): pass A walks the labels of a frame in input
// order with one wave searching the detections of each; pass B gives every threshold slot a lane that walks :479-591 as written.
// The per-slot assigned flags are bits of a caller-owned workspace, so no count of a frame is bounded by a wave or by LDS.
//
// A quirk kept as the reference has it: cleanData marks a detection below the minimum height as "ignored" (1) BEFORE it looks at
// its class (:449-454), so a short detection of another class is a candidate of every class's walk (it can only ever be
// "assigned", never a true or false positive).
#pragma once

#define KEV_T 64                       // one wave per (frame, list)
#define KEV_SLOTS 41                   // N_SAMPLE_PTS
#define KEV_LISTS 27
#define KEV_SORT_T 1024                // the rank sort of a list is O(n^2) compares: the widest workgroup there is

struct KittiScene {
    const int32_t *det_off, *gt_off, *pair_off;   // (F+1) each, on the device
    int F;
    const float *det;                  // (nd,13) alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry, score
    const int32_t *det_class;          // (nd) 0 / 1 / 2, anything else: a class that is not evaluated
    int nd;
    const float *gt;                   // (ng,14) truncation, occlusion, alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry
    const int32_t *gt_type;            // (ng)
    int ng;
    float *ov;                         // (npairs,3): pair (d, g) of frame f at pair_off[f] + (d - det_off[f]) * ng_f + (g - gt_off[f])
    int npairs;
};

struct KittiFrame {
    int d0, d1, g0, g1, ngf;
    int64_t p0;
};

// The rows of frame f, clamped to the buffers: a bad offset array reads and writes nothing outside them.  A frame whose pairs
// would not fit into ov is treated as empty.
__device__ __forceinline__ KittiFrame kitti_frame(const KittiScene &s, int f)
{
    KittiFrame r;
    r.d0 = max(0, min(s.nd, s.det_off[f]));
    r.d1 = max(r.d0, min(s.nd, s.det_off[f + 1]));
    r.g0 = max(0, min(s.ng, s.gt_off[f]));
    r.g1 = max(r.g0, min(s.ng, s.gt_off[f + 1]));
    r.ngf = r.g1 - r.g0;
    r.p0 = (int64_t)max(0, min(s.npairs, s.pair_off[f]));
    if (r.p0 + (int64_t)(r.d1 - r.d0) * r.ngf > (int64_t)s.npairs) { r.d1 = r.d0; r.g1 = r.g0; r.ngf = 0; }
    return r;
}

__device__ __forceinline__ double kitti_min_overlap(int cls) { return cls == 0 ? 0.7 : 0.5; }            // :56, every metric

// cleanData's verdict on a label (:386-429): 0 counted, 1 ignored (neighbour class, or too hard for the level), -1 another class
__device__ __forceinline__ int kitti_ignored_gt(const float *g, int type, int cls, int dl)
{
    const int min_h[3] = {40, 25, 25}, max_occ[3] = {0, 1, 2};
    const double max_tr[3] = {0.15, 0.3, 0.5};
    const int valid = type == cls ? 1 : ((cls == 1 && type == 4) || (cls == 0 && type == 3)) ? 0 : -1;
    const double height = (double)g[6] - (double)g[4];
    const bool ignore = (int)g[1] > max_occ[dl] || (double)g[0] > max_tr[dl] || height < (double)min_h[dl];
    if (valid == 1 && !ignore) return 0;
    if (valid == 0 || (ignore && valid == 1)) return 1;
    return -1;
}

// ... and on a detection (:437-455): the height is truncated to int32 before the comparison, and compared before the class
__device__ __forceinline__ int kitti_ignored_det(const float *d, int dcls, int cls, int dl)
{
    const int min_h[3] = {40, 25, 25};
    const int height = (int)fabs((double)d[2] - (double)d[4]);
    if (height < min_h[dl]) return 1;
    return dcls == cls ? 0 : -1;
}

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void kitti_label_rows_kernel(const float *__restrict__ dets, int R, const int32_t *__restrict__ rows,
                                                               int n, const float *__restrict__ boxes, int NB,
                                                               const int32_t *__restrict__ row_box, float *__restrict__ table,
                                                               int32_t *__restrict__ ok)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = rows ? rows[i] : i, b = row_box[i];
    float *o = table + (int64_t)i * 13;
    if (r < 0 || r >= R || b < 0 || b >= NB) {                             // (an unused keep slot): never dereferenced
        for (int k = 0; k < 13; ++k) o[k] = __builtin_nanf("");
        ok[i] = 0;
        return;
    }
    const float *d = dets + (int64_t)r * 8, *q = boxes + (int64_t)b * 4;
    // compute_alpha in fp64 (an angle of up to 3 pi / 2 + ry leaves fp32 arithmetic no room under 1e-6); np.sign(0) = 0
    const double beta = atan2((double)d[2], (double)d[0]);
    const double sg = beta > 0.0 ? 1.0 : (beta < 0.0 ? -1.0 : 0.0);
    o[0] = (float)(-sg * 3.141592653589793 / 2.0 + beta + (double)d[6]);
    o[1] = q[0]; o[2] = q[1]; o[3] = q[2]; o[4] = q[3];
    o[5] = d[5]; o[6] = d[4]; o[7] = d[3];                                 // h, w, l
    o[8] = d[0]; o[9] = d[1]; o[10] = d[2]; o[11] = d[6]; o[12] = d[7];
    ok[i] = (d[5] < 0.01f || d[4] < 0.01f || d[3] < 0.01f) ? 0 : 1;       // test_net_det.py:290
}

extern "C" int fcn_kitti_label_rows(const float *dets, int num_dets, const int32_t *rows, int n, const float *boxes2d, int num_boxes,
                                    const int32_t *row_box, float *table, int32_t *ok, void *stream)
{
    if (n < 0 || num_dets < 0 || num_boxes < 0) return FCN_E_BADARG;
    if (n == 0) return 0;
    if (!table || !ok || !row_box || (num_dets > 0 && !dets) || (num_boxes > 0 && !boxes2d)) return FCN_E_BADARG;
    if (!rows && n > num_dets) return FCN_E_BADARG;
    hipLaunchKernelGGL(kitti_label_rows_kernel, dim3((n + 127) / 128), dim3(128), 0, (hipStream_t)stream, dets, num_dets, rows, n,
                       boxes2d, num_boxes, row_box, table, ok);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// One workgroup per frame, the pairs strided over it.  Criterion -1 (union) for ordinary labels, criterion 0 (over the detection's
// own area / volume) for DontCare: the only criterion the protocol ever asks of such a pair (:582).  The ground rectangles are
// built about the DETECTION's centre, so the clip works on coordinates of the size of the boxes at any depth.
// flags (10) int32, OR-ed: [metric * 3 + class] = the class is evaluated for the metric (:162-170), [9] = some alpha is -10 (:158).
__global__ __launch_bounds__(DEV_T) void kitti_overlaps_kernel(KittiScene s, int32_t *__restrict__ flags)
{
    const int f = blockIdx.x, tid = threadIdx.x;
    const KittiFrame fr = kitti_frame(s, f);
    const int64_t np = (int64_t)(fr.d1 - fr.d0) * fr.ngf;
    for (int64_t p = tid; p < np; p += DEV_T) {
        const int dj = (int)(p / fr.ngf), gi = (int)(p % fr.ngf);
        const float *d = s.det + (int64_t)(fr.d0 + dj) * 13, *g = s.gt + (int64_t)(fr.g0 + gi) * 14;
        const bool dc = s.gt_type[fr.g0 + gi] == 5;
        float *o = s.ov + (fr.p0 + p) * 3;
        // image (:229-263)
        {
            const float w = fminf(d[3], g[5]) - fmaxf(d[1], g[3]), h = fminf(d[4], g[6]) - fmaxf(d[2], g[4]);
            float v = 0.f;
            if (!(w <= 0.f || h <= 0.f)) {
                const float inter = w * h, a = (d[3] - d[1]) * (d[4] - d[2]), b = (g[5] - g[3]) * (g[6] - g[4]);
                v = dc ? inter / a : inter / (a + b - inter);
            }
            o[0] = v;
        }
        // ground (:296-316) and 3-D (:319-346): toPolygon's rectangle is fcn_bev_rect's
        float ax[4], az[4], bx[4], bz[4];
        fcn_bev_rect(0.f, 0.f, d[7], d[6], cosf(d[11]), sinf(d[11]), ax, az);
        fcn_bev_rect(g[10] - d[8], g[12] - d[10], g[9], g[8], cosf(g[13]), sinf(g[13]), bx, bz);
        const float inter = fcn_quad_intersection_area(ax, az, bx, bz);
        float aa = 0.5f * fcn_quad_area2(ax, az), ab = 0.5f * fcn_quad_area2(bx, bz);
        aa = aa < 0.f ? -aa : aa;
        ab = ab < 0.f ? -ab : ab;
        const float ymax = fminf(d[9], g[11]), ymin = fmaxf(d[9] - d[5], g[11] - g[7]);
        const float ivol = inter * fmaxf(0.f, ymax - ymin);
        const float dvol = d[5] * d[7] * d[6], gvol = g[7] * g[9] * g[8];
        o[1] = dc ? inter / aa : inter / (aa + ab - inter);
        o[2] = dc ? ivol / dvol : ivol / (dvol + gvol - ivol);
    }
    for (int j = fr.d0 + tid; j < fr.d1; j += DEV_T) {
        const float *d = s.det + (int64_t)j * 13;
        const int c = s.det_class[j];
        if (d[0] == -10.f) atomicOr(flags + 9, 1);
        if (c < 0 || c > 2) continue;
        if (d[1] >= 0.f) atomicOr(flags + c, 1);
        if (d[8] != -1000.f) atomicOr(flags + 3 + c, 1);
        if (d[9] != -1000.f) atomicOr(flags + 6 + c, 1);
    }
}

static int kitti_scene_bad(const KittiScene &s)
{
    if (s.F < 0 || s.nd < 0 || s.ng < 0 || s.npairs < 0) return 1;
    if (s.F > 0 && (!s.det_off || !s.gt_off || !s.pair_off)) return 1;
    if (s.nd > 0 && (!s.det || !s.det_class)) return 1;
    if (s.ng > 0 && (!s.gt || !s.gt_type)) return 1;
    if (s.npairs > 0 && !s.ov) return 1;
    return 0;
}

#define KITTI_SCENE_PARAMS                                                                                                          \
    const int32_t *det_off, const int32_t *gt_off, const int32_t *pair_off, int F, const float *det_table, const int32_t *det_class, \
        int nd, const float *gt_table, const int32_t *gt_type, int ng, float *ov, int npairs
#define KITTI_SCENE_FILL(s)                                                                                                      \
    KittiScene s;                                                                                                                \
    s.det_off = det_off; s.gt_off = gt_off; s.pair_off = pair_off; s.F = F; s.det = det_table; s.det_class = det_class; s.nd = nd; \
    s.gt = gt_table; s.gt_type = gt_type; s.ng = ng; s.ov = ov; s.npairs = npairs

extern "C" int fcn_kitti_overlaps(KITTI_SCENE_PARAMS, int32_t *flags, void *stream)
{
    KITTI_SCENE_FILL(s);
    if (kitti_scene_bad(s) || !flags) return FCN_E_BADARG;
    hipError_t e = hipMemsetAsync(flags, 0, 10 * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (F == 0 || nd == 0) return 0;
    hipLaunchKernelGGL(kitti_overlaps_kernel, dim3(F), dim3(DEV_T), 0, (hipStream_t)stream, s, flags);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Pass A.  grid (F, 27), one wave each.  assigned: (27, nd, 2) int32 workspace, word 0 used here (zeroed by the wave that owns the
// rows).  tp_score (27, ng) float32 with tp_count (27): a list never holds more true positives than there are labels.  n_gt (27).
__global__ __launch_bounds__(KEV_T) void kitti_pass_a_kernel(KittiScene s, int class_mask, int32_t *__restrict__ assigned,
                                                             float *__restrict__ tp_score, int32_t *__restrict__ tp_count,
                                                             int32_t *__restrict__ n_gt)
{
    const int f = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    const int m = k / 9, cls = (k / 3) % 3, dl = k % 3;
    if (!((class_mask >> cls) & 1)) return;
    const KittiFrame fr = kitti_frame(s, f);
    int32_t *asg = assigned + (int64_t)k * s.nd * 2;
    for (int j = fr.d0 + tid; j < fr.d1; j += KEV_T) asg[(int64_t)j * 2] = 0;
    __syncthreads();
    const double minov = kitti_min_overlap(cls);
    int ngt = 0;
    for (int g = fr.g0; g < fr.g1; ++g) {
        const int ig = kitti_ignored_gt(s.gt + (int64_t)g * 14, s.gt_type[g], cls, dl);
        ngt += ig == 0 ? 1 : 0;
        if (ig == -1) continue;                                            // (wave-uniform)
        // the unassigned candidate with the highest score; among equal scores the first index (:508 is a strict >)
        float best = -10000000.f;                                          // NO_DETECTION
        int bj = -1;
        for (int j = fr.d0 + tid; j < fr.d1; j += KEV_T) {
            const float *d = s.det + (int64_t)j * 13;
            if (kitti_ignored_det(d, s.det_class[j], cls, dl) == -1 || asg[(int64_t)j * 2] != 0) continue;
            const float o = s.ov[(fr.p0 + (int64_t)(j - fr.d0) * fr.ngf + (g - fr.g0)) * 3 + m];
            if ((double)o > minov && d[12] > best) { best = d[12]; bj = j; }
        }
        for (int w = 1; w < KEV_T; w <<= 1) {
            const float ob = __shfl_xor(best, w);
            const int oj = __shfl_xor(bj, w);
            if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj < bj))) { best = ob; bj = oj; }
        }
        if (bj >= 0 && tid == 0) {
            const int idt = kitti_ignored_det(s.det + (int64_t)bj * 13, s.det_class[bj], cls, dl);
            if (ig == 0 && idt == 0) {                                     // a true positive (:542-554)
                const int at = atomicAdd(tp_count + k, 1);
                if (at < s.ng) tp_score[(int64_t)k * s.ng + at] = best;
            }
            asg[(int64_t)bj * 2] = 1;
        }
        __syncthreads();                                                   // (the flag is read by the whole wave at the next label)
    }
    if (tid == 0 && ngt > 0) atomicAdd(n_gt + k, ngt);
}

extern "C" int fcn_kitti_pass_a(KITTI_SCENE_PARAMS, int class_mask, int32_t *assigned, float *tp_score, int32_t *tp_count,
                                int32_t *n_gt, void *stream)
{
    KITTI_SCENE_FILL(s);
    if (kitti_scene_bad(s) || !tp_count || !n_gt || (nd > 0 && !assigned) || (ng > 0 && !tp_score)) return FCN_E_BADARG;
    hipError_t e = hipMemsetAsync(tp_count, 0, KEV_LISTS * sizeof(int32_t), (hipStream_t)stream);
    if (e == hipSuccess) e = hipMemsetAsync(n_gt, 0, KEV_LISTS * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (F == 0 || ng == 0) return 0;
    hipLaunchKernelGGL(kitti_pass_a_kernel, dim3(F, KEV_LISTS), dim3(KEV_T), 0, (hipStream_t)stream, s, class_mask, assigned, tp_score,
                       tp_count, n_gt);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// getThresholds.  One workgroup per list: a rank sort (descending; equal scores keep their order, which no output can see) into
// sorted (27, ng), then one lane walks the recall steps in fp64 as :358-379 do.  thresholds (27, 41) fp64 (0 behind the count),
// num_thresholds (27).
__global__ __launch_bounds__(KEV_SORT_T) void kitti_thresholds_kernel(const float *__restrict__ tp_score,
                                                                      const int32_t *__restrict__ tp_count,
                                                                      const int32_t *__restrict__ n_gt, int ng,
                                                                      float *__restrict__ sorted, double *__restrict__ thresholds,
                                                                      int32_t *__restrict__ num_thresholds)
{
    const int k = blockIdx.x, tid = threadIdx.x;
    const int n = max(0, min(ng, tp_count[k]));
    const float *v = tp_score + (int64_t)k * ng;
    float *out = sorted + (int64_t)k * ng;
    for (int i = tid; i < n; i += KEV_SORT_T) {
        const float x = v[i];
        int r = 0;
        for (int e = 0; e < n; ++e) {
            const float y = v[e];
            r += (y > x || (y == x && e < i)) ? 1 : 0;
        }
        out[r] = x;                                                        // r < n: at most n - 1 others come before i
    }
    __syncthreads();
    if (tid != 0) return;
    const double n_groundtruth = (double)n_gt[k];
    double current_recall = 0;
    int T = 0;
    for (int i = 0; i < n; ++i) {
        const double l_recall = (double)(i + 1) / n_groundtruth;
        const double r_recall = i < n - 1 ? (double)(i + 2) / n_groundtruth : l_recall;
        if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
        if (T < KEV_SLOTS) thresholds[k * KEV_SLOTS + T++] = (double)out[i];
        current_recall += 1.0 / (41.0 - 1.0);
    }
    num_thresholds[k] = T;
    for (int t = T; t < KEV_SLOTS; ++t) thresholds[k * KEV_SLOTS + t] = 0.0;
}

extern "C" int fcn_kitti_thresholds(const float *tp_score, const int32_t *tp_count, const int32_t *n_gt, int ng, float *sorted,
                                    double *thresholds, int32_t *num_thresholds, void *stream)
{
    if (ng < 0 || !tp_count || !n_gt || !thresholds || !num_thresholds || (ng > 0 && (!tp_score || !sorted))) return FCN_E_BADARG;
    hipLaunchKernelGGL(kitti_thresholds_kernel, dim3(KEV_LISTS), dim3(KEV_SORT_T), 0, (hipStream_t)stream, tp_score, tp_count, n_gt,
                       ng, sorted, thresholds, num_thresholds);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Pass B.  grid (F, 27), one wave each, lane t = threshold slot t of the list (slots >= T idle).  Every lane walks :479-591 as
// written; its assigned flags are bit t of the (27, nd, 2) int32 words.  counts (3, 27, 41) int32: tp, fp, fn, summed with
// atomics.  sim (F, 9, 41) fp64: the frame's sum of (1 + cos(delta alpha)) / 2 over its true positives in label order, image
// metric only; slots < T are written, the others never read.
__global__ __launch_bounds__(KEV_T) void kitti_pass_b_kernel(KittiScene s, int class_mask, const double *__restrict__ thresholds,
                                                             const int32_t *__restrict__ num_thresholds,
                                                             int32_t *__restrict__ assigned, int32_t *__restrict__ counts,
                                                             double *__restrict__ sim)
{
    const int f = blockIdx.x, k = blockIdx.y, t = threadIdx.x;
    const int m = k / 9, cls = (k / 3) % 3, dl = k % 3;
    if (!((class_mask >> cls) & 1)) return;
    const KittiFrame fr = kitti_frame(s, f);
    int32_t *asg = assigned + (int64_t)k * s.nd * 2;
    // the words are shared by the lanes (one bit each) and set with atomics, which act in L2: they are zeroed and read there too
    for (int64_t j = (int64_t)fr.d0 * 2 + t; j < (int64_t)fr.d1 * 2; j += KEV_T)
        __hip_atomic_store(asg + j, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (t >= max(0, min(KEV_SLOTS, num_thresholds[k]))) return;
    const double thr = thresholds[k * KEV_SLOTS + t], minov = kitti_min_overlap(cls);
    const int word = t >> 5, bit = 1 << (t & 31);
    int tp = 0, fp = 0, fn = 0;
    double similarity = 0.0;
    for (int g = fr.g0; g < fr.g1; ++g) {
        const float *gt = s.gt + (int64_t)g * 14;
        const int ig = kitti_ignored_gt(gt, s.gt_type[g], cls, dl);
        if (ig == -1) continue;
        int det_idx = -1, det_ign = 0;
        bool found = false, assigned_ignored_det = false;
        double max_overlap = 0;
        for (int j = fr.d0; j < fr.d1; ++j) {
            const float *d = s.det + (int64_t)j * 13;
            const int idt = kitti_ignored_det(d, s.det_class[j], cls, dl);
            if (idt == -1) continue;
            if (__hip_atomic_load(asg + (int64_t)j * 2 + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) continue;
            if ((double)d[12] < thr) continue;
            const double o = (double)s.ov[(fr.p0 + (int64_t)(j - fr.d0) * fr.ngf + (g - fr.g0)) * 3 + m];
            if (o > minov && (o > max_overlap || assigned_ignored_det) && idt == 0) {
                max_overlap = o; det_idx = j; det_ign = 0; found = true; assigned_ignored_det = false;
            } else if (o > minov && !found && idt == 1) {
                det_idx = j; det_ign = 1; found = true; assigned_ignored_det = true;
            }
        }
        if (!found) {
            fn += ig == 0 ? 1 : 0;
            continue;
        }
        if (!(ig == 1 || det_ign == 1)) {
            ++tp;
            if (m == 0) similarity += (1.0 + cos((double)gt[2] - (double)s.det[(int64_t)det_idx * 13])) / 2.0;
        }
        atomicOr(asg + (int64_t)det_idx * 2 + word, bit);
    }
    // :561-591: what is left unassigned of the class is a false positive, unless a DontCare area holds it
    for (int j = fr.d0; j < fr.d1; ++j) {
        const float *d = s.det + (int64_t)j * 13;
        if (kitti_ignored_det(d, s.det_class[j], cls, dl) != 0 || (double)d[12] < thr) continue;
        if (__hip_atomic_load(asg + (int64_t)j * 2 + word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit) continue;
        ++fp;
        for (int g = fr.g0; g < fr.g1; ++g) {
            if (s.gt_type[g] != 5) continue;
            if ((double)s.ov[(fr.p0 + (int64_t)(j - fr.d0) * fr.ngf + (g - fr.g0)) * 3 + m] > minov) { --fp; break; }
        }
    }
    if (tp) atomicAdd(counts + k * KEV_SLOTS + t, tp);
    if (fp) atomicAdd(counts + (KEV_LISTS + k) * KEV_SLOTS + t, fp);
    if (fn) atomicAdd(counts + (2 * KEV_LISTS + k) * KEV_SLOTS + t, fn);
    if (m == 0) sim[((int64_t)f * 9 + (cls * 3 + dl)) * KEV_SLOTS + t] = similarity;
}

extern "C" int fcn_kitti_pass_b(KITTI_SCENE_PARAMS, int class_mask, const double *thresholds, const int32_t *num_thresholds,
                                int32_t *assigned, int32_t *counts, double *sim, void *stream)
{
    KITTI_SCENE_FILL(s);
    if (kitti_scene_bad(s) || !thresholds || !num_thresholds || !counts || (nd > 0 && !assigned) || (F > 0 && !sim)) return FCN_E_BADARG;
    hipError_t e = hipMemsetAsync(counts, 0, 3 * KEV_LISTS * KEV_SLOTS * sizeof(int32_t), (hipStream_t)stream);
    if (e != hipSuccess) return (int)e;
    if (F == 0) return 0;
    hipLaunchKernelGGL(kitti_pass_b_kernel, dim3(F, KEV_LISTS), dim3(KEV_T), 0, (hipStream_t)stream, s, class_mask, thresholds,
                       num_thresholds, assigned, counts, sim);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// Curves and AP.  One wave per list.  precision (27, 41), aos (9, 41), ap (27), aos_ap (9), all fp64.  The orientation sums are
// reduced over the frames in frame order by one lane per slot: two runs give the same bits.  The suffix maximum is
// std::max_element's (the first of the largest under <, over all 41 entries: the zeros behind the count take part, a NaN from
// 0 / 0 at the front of a range stays).  AP = sum of entries 0, 4, .., 40 / 11 * 100 in fp64 (the reference sums them in float for
// printing only: 11 * 2^-24 * 100 < 7e-5 away).  A class that is not evaluated (flags, class_mask) has NaN rows; AOS is NaN
// throughout when any alpha is -10.
__global__ __launch_bounds__(KEV_T) void kitti_curves_kernel(const int32_t *__restrict__ counts, const int32_t *__restrict__ num_thresholds,
                                                             const double *__restrict__ sim, int F, const int32_t *__restrict__ flags,
                                                             int class_mask, double *__restrict__ precision, double *__restrict__ aos,
                                                             double *__restrict__ ap, double *__restrict__ aos_ap)
{
    __shared__ double raw[2][KEV_SLOTS], fil[2][KEV_SLOTS];
    const int k = blockIdx.x, i = threadIdx.x;
    const int m = k / 9, cls = (k / 3) % 3, cd = k % 9;
    const int T = max(0, min(KEV_SLOTS, num_thresholds[k]));
    const bool evaluated = ((class_mask >> cls) & 1) && flags[m * 3 + cls] != 0;
    const bool with_aos = m == 0 && evaluated && flags[9] == 0;
    const double nan = __builtin_nan("");
    if (i < KEV_SLOTS) {
        double p = 0.0, a = 0.0;
        if (i < T) {
            const int tp = counts[k * KEV_SLOTS + i], fp = counts[(KEV_LISTS + k) * KEV_SLOTS + i];
            p = (double)tp / (double)(tp + fp);
            if (m == 0) {
                // frame order, one chain of additions; the loads of sixteen frames are issued ahead of their additions (the loop is
                // bound by load latency), which changes neither the order nor the bits
                const double *sp = sim + (int64_t)cd * KEV_SLOTS + i;
                const int64_t step = 9 * KEV_SLOTS;
                double sum = 0.0, v[16];
                int f = 0;
                for (; f + 16 <= F; f += 16) {
#pragma unroll
                    for (int q = 0; q < 16; ++q) v[q] = sp[(f + q) * step];
#pragma unroll
                    for (int q = 0; q < 16; ++q) sum += v[q];
                }
                for (; f < F; ++f) sum += sp[f * step];
                a = sum / (double)(tp + fp);
            }
        }
        raw[0][i] = p;
        raw[1][i] = a;
    }
    __syncthreads();
    if (i < KEV_SLOTS) {
        for (int q = 0; q < 2; ++q) {
            double v = raw[q][i];
            if (i < T) {
                int best = i;
                for (int j = i + 1; j < KEV_SLOTS; ++j)
                    if (raw[q][best] < raw[q][j]) best = j;
                v = raw[q][best];
            }
            fil[q][i] = v;
        }
        precision[k * KEV_SLOTS + i] = evaluated ? fil[0][i] : nan;
        if (m == 0) aos[cd * KEV_SLOTS + i] = with_aos ? fil[1][i] : nan;
    }
    __syncthreads();
    if (i == 0) {
        double sp = 0.0, sa = 0.0;
        for (int j = 0; j < KEV_SLOTS; j += 4) { sp += fil[0][j]; sa += fil[1][j]; }
        ap[k] = evaluated ? sp / 11.0 * 100.0 : nan;
        if (m == 0) aos_ap[cd] = with_aos ? sa / 11.0 * 100.0 : nan;
    }
}

extern "C" int fcn_kitti_curves(const int32_t *counts, const int32_t *num_thresholds, const double *sim, int F, const int32_t *flags,
                                int class_mask, double *precision, double *aos, double *ap, double *aos_ap, void *stream)
{
    if (F < 0 || !counts || !num_thresholds || !flags || !precision || !aos || !ap || !aos_ap || (F > 0 && !sim)) return FCN_E_BADARG;
    hipLaunchKernelGGL(kitti_curves_kernel, dim3(KEV_LISTS), dim3(KEV_T), 0, (hipStream_t)stream, counts, num_thresholds, sim, F,
                       flags, class_mask, precision, aos, ap, aos_ap);
    FCN_CHECK_LAUNCH();
    return 0;
}
