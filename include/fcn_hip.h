/*
 * fcn_hip.h -- C-ABI of libfcn_hip.so: the MI355X (gfx950) implementation of Frustum ConvNet's
 * per-frustum hot path.  Plain pointers + sizes + a HIP stream; no torch types, no hidden
 * allocation, no implicit synchronisation, no global state.  Every function enqueues work on
 * `stream` (a hipStream_t passed as void*) and returns 0 or a non-zero code (hipError_t value, or
 * FCN_E_* below); it is safe to call while the stream is being captured into a hipGraph.
 *
 * What each entry point replaces in the reference (paths relative to the reference repo):
 *
 *   fcn_query_depth_point_f32   query_depth_point_forward(), PYBIND11 "forward"
 *                               ops/query_depth_point/query_depth_point_cuda.cpp:25-50 and the launcher +
 *                               kernel ops/query_depth_point/query_depth_point_cuda_kernel.cu:16-86
 *   fcn_pn_compact / fcn_pn_forward / fcn_pn_backward
 *                               the torch ops behind PointNetModule.forward + the max over K in
 *                               PointNetFeat.forward: gather, centre subtract, 3 x [Conv2d 1x1, BatchNorm2d,
 *                               ReLU], (cnt>0) mask, torch.max(.,-1), one-hot concat
 *                               models/det_base.py:75-101,134-157 (+ autograd of the same)
 *   fcn_pn_infer_fold / fcn_pn_infer
 *                               the same forward under model.eval() in one launch per scale (BatchNorm folded)
 *   fcn_convnet_forward/backward ConvFeatNet.forward + cls_out/reg_out (cuDNN/ATen in the reference),
 *                               models/det_base.py:196-224,367-368 (+ autograd of the same)
 *   fcn_convnet_pack / _forward2 the same forward with the weight re-packing split off and per-feature-map start events
 *   fcn_det_loss_tail[_rows]    the ~150 torch ops of the train-loss tail, models/det_base.py:373-476
 *   fcn_adam_step_f32           optim.Adam.step() of the step loop, train/train_net_det.py:131-133,321-339
 *   fcn_sgd_step_f32            optim.SGD.step() (momentum) of the same loop's 'sgd' branch, train/train_net_det.py:325-327
 *   fcn_prepare_inputs          the per-sample numpy work of the data loader + collate,
 *                               datasets/provider_sample.py:137-262,270-327,396-397
 *   fcn_prepare_inputs_refine   the same for the refinement stage, datasets/provider_sample_refine.py:176-419
 *   fcn_prepare_inputs_sunrgbd  the same for the SUN-RGBD loader, datasets/provider_sample_sunrgbd.py:116-326
 *   fcn_det_iou_metrics         the IoU metrics of models/det_base.py:480-503 (D2H + boost clipping every step in the reference)
 *   fcn_box3d_iou_pair_f32      rbbox_iou_3d_pair, ops/pybind11/box_ops.h:173-260 (boost polygon clipping on the host)
 *   fcn_decode_detections       the numpy decode loop of train/test_net_det.py:254-293 + from_prediction_to_label_format
 *   fcn_rotate_nms_3d           rotate_nms_3d_cc, ops/pybind11/rbbox_iou.py:294-311 + nms_cpu.h:148-240
 *   fcn_decode_detections_rule  the same loop with the SUN-RGBD rule of train/test_net_det_sunrgbd.py:208-252
 *   fcn_box3d_corners           compute_box_3d, datasets/data_utils.py:44-70
 *   fcn_det_match, fcn_det_ap   eval_det_cls + voc_ap, train/sunrgbd_eval/eval_det.py:41-72,89-169
 *   fcn_kitti_label_rows        write_detection_results + compute_alpha, train/test_net_det.py:88-105, provider_sample.py:389-394
 *   fcn_kitti_overlaps, _pass_a, _thresholds, _pass_b, _curves
 *                               the official KITTI evaluator, train/kitti_eval/evaluate_object_3d_offline.cpp
 *   fcn_stamp                   (measurement aid, no reference counterpart)
 *   fcn_stream_capture_id       (graph-capture bookkeeping of the Python layer, no reference counterpart)
 *
 * Buffers are caller-owned.  "ws" buffers are scratch the caller provides (sizes documented per call).
 */
#ifndef FCN_HIP_H
#define FCN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FCN_E_BADARG 10001   /* unsupported shape / null pointer */
#define FCN_E_LIMIT  10002   /* size beyond a documented limit   */

/* Matrix-core operand precision of the GEMM kernels (fcn_pn_desc.precision / fcn_cn_desc.precision).  Storage, BatchNorm
 * statistics and accumulation are fp32 in every mode.
 *   FCN_PREC_SPLIT  default, the parity mode: every fp32 operand is split into two 16-bit parts and a product is formed
 *                   from three 16-bit MFMAs (fp16 parts in the forward GEMMs, bf16 parts in the backward GEMMs) -- fp32-class
 *                   results (logits within 1e-4 of the fp32 reference) at 5.3x the fp32 matrix rate of gfx950.  Forward
 *                   operands (activations after BN+ReLU, weights) must stay below 65504 in magnitude.
 *   FCN_PREC_F32    exact fp32 MFMA (v_mfma_f32_32x32x2_f32): the reference mode for A/B comparisons.
 *   FCN_PREC_BF16   throughput mode of BASELINE config 2 (bf16 activations + GEMM inputs): single bf16 MFMA per product, fp32
 *                   accumulate, and the BIG intermediate tensors -- the PointNet's per-entry y2 / y3 / dy3 / dz2, the streams that
 *                   reach HBM -- STORED as bf16 in the first half of their (fp32-sized) buffers; BatchNorm sums, pooled features,
 *                   logits and all parameter gradients stay fp32 (logits within a few 1e-2 relative of the fp32 reference;
 *                   grouping indices unaffected).  The FCN's y / dz arenas (a few thousand rows per layer, L2-resident) stay
 *                   fp32 in this mode since round 6: bf16 arenas made every fcn_convnet_* launch 22-49 % slower and saved no
 *                   memory time (fcn_net.hip, CN_MM_OF).
 *   FCN_PREC_BF16_OPS  the same operands with fp32 storage everywhere (rounds 1-2's bf16 mode). */
#define FCN_PREC_SPLIT 0
#define FCN_PREC_F32   1
#define FCN_PREC_BF16  2
#define FCN_PREC_BF16_OPS 3

/* Version / build probe: returns 950 (the only arch this library is built for). */
int fcn_arch(void);

/* ---------------------------------------------------------------------------------------------
 * Sliding-frustum grouping.  Bit-exact restatement of query_depth_point_cuda_kernel.cu:16-65.
 *   pts_z : z of point 0 of sample 0; element stride pt_stride floats, sample stride pt_bstride floats
 *           ((B,3,N) layout: xyz+2*N, 1, 3*N;  (B,N,3) layout: xyz+2, 3, 3*N) -- never transposed on device
 *   ctr_z : same for the m window centres
 *   idx   : (b,m,nsample) int64, fully written (padding with first hit; zeros for empty windows)
 *   cnt   : (b,m) int32
 * ------------------------------------------------------------------------------------------- */
int fcn_query_depth_point_f32(const float *pts_z, int64_t pt_stride, int64_t pt_bstride,
                              const float *ctr_z, int64_t ct_stride, int64_t ct_bstride,
                              int b, int n, int m, float dis_z, int nsample,
                              int64_t *idx, int32_t *cnt, void *stream);

/* The same operator for ALL scales of one batch in ONE launch (the scales of PointNetFeat.forward share the point cloud and differ
 * in window centres, half height and nsample: models/det_base.py:126-157 calls query_depth_point once per scale).  Arrays of
 * nscale <= 8 entries; outputs exactly those of nscale calls of fcn_query_depth_point_f32. */
int fcn_query_depth_point_multi_f32(int nscale, const float *pts_z, int64_t pt_stride, int64_t pt_bstride,
                                    const float *const *ctr_z, const int64_t *ct_stride, const int64_t *ct_bstride,
                                    int b, int n, const int32_t *m, const float *dis_z, const int32_t *nsample,
                                    int64_t *const *idx, int32_t *const *cnt, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One PointNet scale (PointNetModule + max over K), "entry space" dataflow: every distinct
 * (window, point) pair is evaluated once and carries its multiplicity as a weight.
 * Channel widths C1,C2,C3 must be multiples of 64; L <= 8192; K <= 1024.
 * ------------------------------------------------------------------------------------------- */
/* BatchNorm modes (fcn_pn_desc.training, fcn_cn_desc.training):
 *   FCN_BN_TRAIN    batch statistics; the running statistics (running_mean, running_var, num_batches_tracked) are updated;
 *                   the forward saves what the backward reads.
 *   FCN_BN_RUNNING  running statistics, nothing saved: inference.  Every backward entry returns FCN_E_BADARG.
 *   FCN_BN_FROZEN   running statistics, which are never written, and the forward saves what the backward reads (the
 *                   reference's model.eval() fine-tune, torchvision's FrozenBatchNorm).  The backward differentiates through the
 *                   running statistics: dy = gamma * rstd_running * dz (no batch-mean terms), dgamma = sum dz * xhat,
 *                   dbeta = sum dz.  fcn_pn_group_compact[2] folds BN1 from the running statistics, fcn_pn_forward /
 *                   fcn_convnet_pack / fcn_convnet_forward[2] take the training forward's launches without the batch sums,
 *                   every fcn_pn_backward* / fcn_convnet_backward accepts it, in all four FCN_PREC_* modes.
 * Any other value: FCN_E_BADARG from every entry point that reads the descriptor's mode. */
#define FCN_BN_RUNNING 0
#define FCN_BN_TRAIN   1
#define FCN_BN_FROZEN  2

typedef struct fcn_pn_desc {
    int32_t B, N, L, K;          /* frustums, points per frustum, windows, nsample        */
    int32_t C1, C2, C3;          /* MLP widths                                              */
    int32_t nvec;                /* one-hot width appended after pooling (0..)              */
    int32_t training;            /* BatchNorm mode, FCN_BN_* (below)                        */
    float   eps, momentum;       /* BatchNorm eps (1e-5) and momentum (0.1)                 */
    int32_t nlc;                 /* 0: feat/dfeat are (B, C3+nvec, L) as the reference returns them;
                                    1: position-major (B, L, C3), no one-hot rows (input of fcn_convnet_*) */
    int32_t precision;           /* FCN_PREC_* (0 = split 16-bit MFMA, fp32-class)                              */
    int32_t grouped;             /* 1: fcn_pn_group_compact prepared ws for this call (entry list, tile list, input moments,
                                    BN1 scale/shift + running statistics, zeroed BN sums): fcn_pn_forward skips its own
                                    BN1 finalisation                                                              */
} fcn_pn_desc;

/* Parameters of the three conv+BN pairs (reference state_dict order: conv{1,2,3}.0.weight,
 * conv{1,2,3}.1.{weight,bias,running_mean,running_var,num_batches_tracked}). */
typedef struct fcn_pn_params {
    const float *W[3];           /* (C1,3) (C2,C1) (C3,C2) row-major                        */
    const float *gamma[3], *beta[3];
    float *running_mean[3], *running_var[3];
    int64_t *num_batches_tracked[3];
} fcn_pn_params;

/* Scratch + saved-for-backward buffers of one scale.  cap = L*K rows per frustum.
 * All must stay alive from fcn_pn_forward until fcn_pn_backward has been enqueued. */
typedef struct fcn_pn_ws {
    int32_t *woff;               /* (B, L+1)   window row offsets, woff[b][L] = live rows    */
    float   *ent;                /* (B, cap, 4) (ux,uy,uz,w)                                 */
    int32_t *ewin;               /* (B, cap)    window of each row                           */
    int32_t *tiles;              /* 4 + B*ceil(cap/128): [0] = live 128-row tiles, [4+i] = b*tps + t */
    float   *y2;                 /* (B, cap, C2) conv2 output (pre-BN)                       */
    float   *y3;                 /* (B, cap, C3) conv3 output (pre-BN)                       */
    int32_t *amax;               /* (B, L, C3)  row of the pooled max, -1 = no gradient      */
    double  *stat;               /* 16 + fcn_stat_replicas() * (2*C2 + 2*C3) doubles: input moments, then the
                                    replicated sum / sumsq blocks of conv2 and conv3                        */
    float   *bn;                 /* 4*(C1+C2+C3) floats: per layer scale, shift, mean, rstd  */
    /* backward -- and, for gmax, the hand-over from a key-pooled TRAINING or FROZEN forward to its backward */
    float   *gmax;               /* (B, L, C3)  dfeat routed to the max rows (written by fcn_pn_backward*).  When the forward
                                    pooled through keys (training = FCN_BN_TRAIN or FCN_BN_FROZEN, nlc = 1, pkey and ewin set) fcn_pn_forward ALSO writes
                                    it: the winners' pre-BN values, position-major, which the first backward kernel reads and
                                    then overwrites with the routed gradient.  Between such a forward and its backward the
                                    buffer is therefore LIVE: do not clear it, do not share it between scales or workspace
                                    sets in flight, and pass the same pointer to both calls.  A training / frozen key-pool
                                    forward with amax set and gmax NULL returns FCN_E_BADARG                                         */
    float   *dy3;                /* (B, cap, C3), or NULL: dy3 is not materialised -- conv3's weight-gradient GEMM rebuilds
                                    it from y3, ewin, amax, gmax and the BN3-backward sums while staging (bit-identical dW3;
                                    measured 0.7 % slower over the step, saves B*cap*C3 floats) */
    float   *dz2;                /* (B, cap, C2)                                             */
    double  *bstat;              /* fcn_stat_replicas() * (2*C3 + 2*C2 + 4*C1) doubles       */
    float   *coef;               /* 5*(C3+C2) floats                                         */
    float   *partial;            /* wgrad partials: nsplit * max(C3*C2, C2*C1) floats (fcn_pn_backward3: nsplit * (C3*C2 + C2*C1)) */
    int32_t  nsplit;             /* capacity of `partial` in splits: >= B*ceil(cap/128) (one per row tile) */
    double  *gmom;               /* (B,12) doubles, fcn_pn_group_compact only (may be NULL otherwise): per-frustum input moments +
                                    an arrival counter; zero it, and tiles[0..3], ONCE at allocation (the call leaves
                                    its counters at zero) */
    float   *wenc;               /* 2*(C2*C1 + C3*C2) floats, 16-byte aligned: the conv2 / conv3 weights split-encoded in MFMA
                                    operand order (forward + data-gradient images), rewritten by every forward
                                    (fcn_pn_pack_weights[_all]) and read by the forward and backward GEMMs                    */
    int32_t *flags;              /* 1 int32 of sticky FCN_FLAG_* bits, or NULL: zero it once, read it whenever convenient    */
    uint64_t *pkey;              /* (B, L, C3) max-pool keys, 16-byte aligned, or NULL: zero it ONCE at allocation (fcn_pn_forward
                                    leaves it zero).  With it (and nlc = 1) the max-pool is taken in conv3's epilogue instead of
                                    by a pass that re-reads y3 (and in eval mode y3 is not written at all)                     */
    int32_t  partial_both;       /* 1 or 2: `partial` holds nsplit * (C3*C2 + C2*C1) floats -- both weight gradients' split partials at
                                    once -- so their two fixed-order reduces (and the layer-1 finalisation) run as ONE launch at the
                                    tail of the chain instead of between its GEMMs; with 1 the one-stream backward (fcn_pn_backward,
                                    fcn_pn_backward2 with stream2 == NULL) also runs conv2's data gradient and both weight-gradient
                                    GEMMs as roles of one launch.  0: `partial` holds nsplit * max(C3*C2, C2*C1) floats, GEMM and
                                    reduce alternate.  Anything else: FCN_E_BADARG -- zero-initialise the struct.  Bit-identical
                                    gradients in all three. */
} fcn_pn_ws;

/* Sticky numeric flags (fcn_pn_ws.flags, fcn_cn_ws.flags): the kernels only ever OR bits in.
 *   FCN_FLAG_NONFINITE  a forward GEMM produced a non-finite output.  In FCN_PREC_SPLIT the forward operands are split into
 *                       fp16 parts, which overflow at |x| >= 65504 (the products turn into inf - inf = NaN and the next ReLU
 *                       would silently turn that into 0): results of this step are not to be trusted -- rerun in FCN_PREC_F32
 *                       or FCN_PREC_BF16, whose operands keep the fp32 exponent range. */
#define FCN_FLAG_NONFINITE 1

/* rows of one row tile (128): the caller sizes ws.tiles / ws.partial with it */
int fcn_pn_wgrad_rows(void);
/* copies of every BatchNorm sum slot (8): same-address fp64 atomics are served one at a time, so workgroups spread over
 * replicas and the consumers sum them in a fixed order; the caller sizes ws.stat / ws.bstat with it */
int fcn_stat_replicas(void);

/* idx/cnt -> entry list + live-tile list + weighted input moments (ws.woff, ws.ent, ws.ewin, ws.tiles, ws.stat[0..9]) */
int fcn_pn_compact(const fcn_pn_desc *d, const float *pc /*(B,3,N)*/, const float *ref /*(B,3,L)*/,
                   const int64_t *idx, const int32_t *cnt, const fcn_pn_ws *ws, void *stream);

/* Grouping + compaction of up to 8 scales of one batch in ONE launch, without the int64 idx: for scale s, window centres
 * ref[s] (B,3,L_s) and half height dis_z[s] produce cnt[s] (B,L_s) and ws[s]->{woff, ent, ewin, tiles, stat[0..9], bn (layer
 * 1)} exactly as fcn_query_depth_point_f32 + fcn_pn_compact + the BN1 finalisation of fcn_pn_forward would (moments up to
 * fp64 summation order, here fixed), zeroes the BN sum slots of ws[s]->stat and, in training mode, updates conv1's running
 * statistics.  All scales share pc (B,3,N), B, N, training, eps, momentum; N <= 65535.  Follow with fcn_pn_forward on
 * descriptors whose `grouped` field is 1. */
int fcn_pn_group_compact(int nscale, const fcn_pn_desc *const *d, const fcn_pn_params *const *p, const float *pc,
                         const float *const *ref, const float *dis_z, const fcn_pn_ws *const *ws, int32_t *const *cnt,
                         void *stream);

/* The same front in two PHASES, so that a loader can prepare the NEXT batch while the current step still runs (the reference's
 * DataLoader workers prefetch batches the same way, datasets/provider_sample.py:291-327 behind train/train_net_det.py:114):
 *   phase 1  everything that depends on the batch alone -- hit lists, entry rows, window offsets, tile lists, input moments,
 *            zeroed BN sums -- into workspaces no launch in flight uses (two launches; p[s] must be valid but its weights are not read);
 *   phase 2  everything that depends on the WEIGHTS of the step that consumes the batch -- the split-encoded conv2 / conv3 images and
 *            the BN1 fold (scale / shift, running statistics) from the moments phase 1 left in ws[s]->stat -- one light launch,
 *            to be issued after the optimiser step, in front of fcn_pn_forward (descriptors with grouped = 1);
 *   phase 3  both at once = fcn_pn_group_compact.
 * Phases 1 + 2 leave every workspace bit-identical to phase 3 (tests/test_gpu_group_compact.py). */
int fcn_pn_group_compact2(int nscale, const fcn_pn_desc *const *d, const fcn_pn_params *const *p, const float *pc,
                          const float *const *ref, const float *dis_z, const fcn_pn_ws *const *ws, int32_t *const *cnt,
                          int phase, void *stream);

/* Split-encodes the conv2 / conv3 weights of one scale into ws->wenc (one small launch).  fcn_pn_forward does it itself on
 * descriptors with grouped == 0; fcn_pn_group_compact does it for all its scales (fcn_pn_pack_weights_all, one launch). */
int fcn_pn_pack_weights(const fcn_pn_desc *d, const fcn_pn_params *p, const fcn_pn_ws *ws, void *stream);
int fcn_pn_pack_weights_all(int nscale, const fcn_pn_desc *const *d, const fcn_pn_params *const *p,
                            const fcn_pn_ws *const *ws, void *stream);

/* Whole forward of one scale after fcn_pn_compact: feat (B, C3+nvec, L), one_hot (B,nvec) or NULL.  In training and frozen mode its
 * last kernel also zeroes ws.bstat (when non-NULL) for the fcn_pn_backward that follows -- and, when the max-pool is taken
 * from keys (nlc = 1, ws.pkey and ws.ewin set), writes the winners' pre-BN values into ws.gmax, which the following
 * fcn_pn_backward* reads before overwriting it (see fcn_pn_ws.gmax; FCN_E_BADARG when ws.amax is set and ws.gmax is NULL). */
int fcn_pn_forward(const fcn_pn_desc *d, const fcn_pn_params *p, const int32_t *cnt,
                   const float *one_hot, const fcn_pn_ws *ws, float *feat, void *stream);

/* Backward: dfeat (B, C3+nvec, L) -> dW[3], dgamma[3], dbeta[3] (overwritten, not accumulated).  After a key-pooled training / frozen
 * forward (fcn_pn_forward above) it expects ws.gmax exactly as that forward left it.  dW[1] and dW[2] must be
 * 16-byte aligned (FCN_E_BADARG otherwise): the fixed-order sum of the split partials writes 16-byte vectors.  Size limits
 * (FCN_E_LIMIT): B * cap * max(C2, C3) < 2^31 elements (32-bit offsets) and B * cap < 2^24 entry rows (24-bit row multiplies). */
int fcn_pn_backward(const fcn_pn_desc *d, const fcn_pn_params *p, const float *dfeat,
                    const fcn_pn_ws *ws, float *dW[3], float *dgamma[3], float *dbeta[3], void *stream);

/* Same as fcn_pn_backward with the two weight-gradient GEMMs (+ their reduces) enqueued on a second stream beside the
 * data-gradient chain; events = 3 caller-owned hipEvent_t.  stream joins on the side stream before returning work. */
int fcn_pn_backward2(const fcn_pn_desc *d, const fcn_pn_params *p, const float *dfeat,
                     const fcn_pn_ws *ws, float *dW[3], float *dgamma[3], float *dbeta[3],
                     void *stream, void *stream2, void *const *events);

/* Backward of the UN-POOLED module output -- PointNetModule.forward's (B, C3, L, nsample) return, models/det_base.py:62-103, whose
 * autograd the reference gets from torch.  dz3 (B, cap, C3) fp32: the gradient w.r.t. relu(bn3(y3)) of every ENTRY row (the K
 * slots of a window summed back onto its rows -- the first hit collects its K - ne + 1 duplicates --, the (cnt > 0) mask and the
 * ReLU mask applied); ws->bstat: replica 0 = sum dz3 [C3], sum dz3 * xhat3 [C3], everything else zero (the caller prepares both:
 * frustum_convnet_amd/pointnet_fused.py does it with device-side indexing).  One stream; needs ws->dy3; not in FCN_PREC_BF16. */
int fcn_pn_backward_dense(const fcn_pn_desc *d, const fcn_pn_params *p, const float *dz3,
                          const fcn_pn_ws *ws, float *dW[3], float *dgamma[3], float *dbeta[3], void *stream);

/* Three-way split: after the first data-gradient GEMM the chain continues on `stream` (dgrad of conv2, layer-1 finalisation),
 * conv3's weight gradient runs on stream2 and conv2's on stream3.  ws.partial must hold BOTH weight gradients' partials at once:
 * nsplit * (C3*C2 + C2*C1) floats.  events = 4 caller-owned hipEvent_t. */
int fcn_pn_backward3(const fcn_pn_desc *d, const fcn_pn_params *p, const float *dfeat,
                     const fcn_pn_ws *ws, float *dW[3], float *dgamma[3], float *dbeta[3],
                     void *stream, void *stream2, void *stream3, void *const *events);

/* ---------------------------------------------------------------------------------------------
 * Single-launch inference forward of one scale (csrc/pn_infer.h): with running statistics the three BatchNorms are affine maps
 * known before the launch; they fold into the weights and one workgroup takes a 64-row tile of entries to pooled features
 * without touching HBM in between.  Results differ from fcn_pn_forward in FCN_BN_RUNNING mode by fp32 rounding only (the scale
 * is rounded into the weight instead of applied to the activation).
 *   fcn_pn_infer_ws  caller-owned buffers of the folded parameters, all 16-byte aligned, rewritten by every fcn_pn_infer_fold.
 *   fcn_pn_infer_fold  ONE small launch for nscale <= 8 scales: scale / shift of every BatchNorm from the running statistics
 *                    (read, never written; num_batches_tracked is not touched), the folded weights into iws[s], and the zero
 *                    fill of feat[s] (fcn_pn_infer publishes into it with atomic maxima: the fill must precede every tile and
 *                    nothing else may write feat[s] in between).  All scales share eps.  p[s]->W[1], W[2] 16-byte aligned.
 *   fcn_pn_infer     one launch: entries (ws->woff, ent, ewin, tiles as fcn_pn_compact / fcn_pn_group_compact[2] left them -- phase
 *                    1 of the phased front is enough, the BN1 fold and weight images of phase 2 are not read) + cnt (B, L) ->
 *                    feat, laid out by d->nlc exactly as fcn_pn_forward's (one_hot (B, nvec) rows appended when nlc = 0).
 *                    Empty windows (cnt == 0) keep the fill value +0.0.  Bit-identical from run to run.  A non-finite GEMM
 *                    output, in every precision, sets FCN_FLAG_NONFINITE in ws->flags (when non-NULL).
 * Contract: d->training must be FCN_BN_RUNNING (FCN_E_BADARG otherwise); ws->y2, y3, pkey, stat, amax, gmax, bn, wenc may be
 * NULL; widths as fcn_pn_forward (multiples of 64, C1 <= 512) except C2 <= 256 (FCN_E_LIMIT above: the h2 tile lives in LDS);
 * L <= 8192, K <= 1024, B * L * K < 2^31.  Precisions: FCN_PREC_SPLIT, FCN_PREC_BF16, FCN_PREC_BF16_OPS (the two bf16 modes are
 * identical here: nothing intermediate is stored).  FCN_PREC_F32 returns FCN_E_BADARG -- take fcn_pn_forward for it (the Python
 * layer does).
 * ------------------------------------------------------------------------------------------- */
typedef struct fcn_pn_infer_ws {
    float *w1f;                  /* 4*C1 floats: rows (s1*W1[c][0..2], t1[c])                                      */
    float *wenc;                 /* C2*C1 + C3*C2 floats: diag(s2) W2, diag(s3) W3 (bf16 modes: W2, W3) in the forward
                                    MFMA operand order                                                                 */
    float *shift;                /* 2*(C2 + C3) floats: t2, t3, then the epilogue scales of conv2 / conv3 (ones in
                                    FCN_PREC_SPLIT, s2, s3 in the bf16 modes, whose images hold the unscaled weights)  */
} fcn_pn_infer_ws;
int fcn_pn_infer_fold(int nscale, const fcn_pn_desc *const *d, const fcn_pn_params *const *p,
                      const fcn_pn_infer_ws *const *iws, float *const *feat, void *stream);
int fcn_pn_infer(const fcn_pn_desc *d, const int32_t *cnt, const float *one_hot, const fcn_pn_ws *ws,
                 const fcn_pn_infer_ws *iws, float *feat, void *stream);

/* Launches ONLY the conv GEMM of `layer` (2 or 3) on the state a previous fcn_pn_compact/fcn_pn_forward left in
 * ws: the unit the roofline figure in bench.py is measured on.  with_stats != 0 keeps the BN-statistics epilogue. */
int fcn_pn_conv_fwd(const fcn_pn_desc *d, const fcn_pn_params *p, const fcn_pn_ws *ws, int layer,
                    int with_stats, void *stream);

/* ---------------------------------------------------------------------------------------------
 * ConvFeatNet + heads (models/det_base.py:163-224,250-251,365-368): 10 Conv1d + 3 ConvTranspose1d (each with
 * BatchNorm1d + ReLU) and the two k=1 heads, as implicit GEMMs over position-major (B*L, C) activations.
 * Layer order of every per-layer array (14 entries; entry 13 = heads, no BN):
 *   0 block1_conv1  1 block2_conv1  2 block2_conv2  3 block2_merge  4 block3_conv1  5 block3_conv2  6 block3_merge
 *   7 block4_conv1  8 block4_conv2  9 block4_merge  10 block2_deconv  11 block3_deconv  12 block4_deconv  13 heads
 * W[l]: the torch weight ((Cout,Cin,k) Conv1d / (Cin,Cout,k) ConvTranspose1d); W[13] = cat(cls_out.weight,
 * reg_out.weight) (2+reg_out, 768, 1), bias = cat of the two biases.
 * ------------------------------------------------------------------------------------------- */
#define FCN_CN_MAXLEV 5          /* pyramid levels: 4 (models/det_base.py) or 5 (models/det_base_sunrgbd.py)     */
#define FCN_CN_MAXLAYER 18       /* 4 * levels - 2 layers: 3*levels-2 convolutions, levels-1 deconvolutions, the heads */

typedef struct fcn_cn_desc {
    int32_t B;
    int32_t L[FCN_CN_MAXLEV];    /* positions of the pooled feature maps (L[1] is the output length); L[j+1] = conv(L[j], k3 s2 p1) */
    int32_t nvec;                /* one-hot width                                                               */
    int32_t reg_out;             /* regression head width (39 for KITTI, 67 for SUN-RGBD); 2 + reg_out <= 128   */
    int32_t training;            /* BatchNorm mode, FCN_BN_* (see fcn_pn_desc)                                  */
    float   eps, momentum;
    int32_t prepacked;           /* 1: fcn_convnet_pack already ran for these weights / one-hot (joined by the caller) */
    int32_t precision;           /* FCN_PREC_*                                                                  */
    int32_t nlev;                /* pyramid levels, 4 or 5 (0 = 4)                                              */
    int32_t c1;                  /* width of block1_conv1: 128 (det_base.py:168) or 64 (det_base_sunrgbd.py:178); 0 = 128 */
} fcn_cn_desc;

/* Layer order of the parameter arrays for n = nlev levels (torch module names of ConvFeatNet):
 *   0                      block1_conv1
 *   1 + 3*(j-2) + {0,1,2}  block{j}_conv1, block{j}_conv2, block{j}_merge      for j = 2..n
 *   3n-2 + (j-2)           block{j}_deconv                                      for j = 2..n
 *   4n-3                   heads: rows 0..1 cls_out, rows 2.. reg_out, over cat of the n-1 deconvolution outputs
 * (n = 4: 0 b1c1, 1-3 block2, 4-6 block3, 7-9 block4, 10-12 deconvs, 13 heads; n = 5: ... 10-12 block5, 13-16 deconvs, 17 heads) */
typedef struct fcn_cn_params {
    const float *W[FCN_CN_MAXLAYER];
    const float *gamma[FCN_CN_MAXLAYER], *beta[FCN_CN_MAXLAYER];
    float *running_mean[FCN_CN_MAXLAYER], *running_var[FCN_CN_MAXLAYER];
    int64_t *num_batches_tracked[FCN_CN_MAXLAYER];
    const float *bias;           /* (2 + reg_out) heads bias */
} fcn_cn_params;

/* Workspace; element counts come from fcn_convnet_sizes (out6: y/dz floats, packed-weight floats, bn floats,
 * stat/bstat doubles, coef floats, wgrad-partial floats).  Size limits (FCN_E_LIMIT from every fcn_convnet_* entry): B * L1 < 2^23
 * rows and every layer's B * L * C (and Cout * Ktot) < 2^30 elements -- the kernels address with 32-bit BYTE offsets. */
typedef struct fcn_cn_ws {
    float  *y, *dz, *wp, *bn;
    double *stat, *bstat;
    float  *coef, *partial;      /* coef: unused since BN backward is finalised by its consumers (kept in the layout) */
    float  *oh64;                /* B * 64 floats: the one-hot vector zero-padded to 64 channels */
    int32_t *flags;              /* 1 int32 of sticky FCN_FLAG_* bits, or NULL (see fcn_pn_ws.flags) */
} fcn_cn_ws;

int fcn_convnet_sizes(const fcn_cn_desc *d, int64_t *out6);
/* Weight re-packing (3.3 M floats, torch layouts -> (N, Ktot)) + one-hot padding of fcn_convnet_forward as a separate
 * launch, so a caller can overlap it with the PointNet scales on another stream (then set d->prepacked = 1).  The launch
 * also zeroes ws.stat and ws.bstat (training): fcn_convnet_forward / _backward enqueue no memset of their own. */
int fcn_convnet_pack(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws, const float *one_hot, void *stream);
/* feats[s], s < nlev: (B, L[s], C_s) with C = 128,128,256,512(,512) (fcn_pn_forward with nlc = 1); logits: (B*L[1], ld) rows
 * with ld = fcn_convnet_logits_ld(d) (64 when 2 + reg_out <= 64, else 128), columns 0..1 = cls_out, 2..2+reg_out = reg_out,
 * rest zero. */
int fcn_convnet_logits_ld(const fcn_cn_desc *d);
int fcn_convnet_forward(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                        const float *const feats[FCN_CN_MAXLEV], const float *one_hot, float *logits, void *stream);
/* Same with nlev optional hipEvent_t: `stream` waits for feat_events[s] right before the first layer that reads feats[s], so
 * the FCN runs beside the PointNet scales that are still in flight (the widest map is needed by the last merge only). */
int fcn_convnet_forward2(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                         const float *const feats[FCN_CN_MAXLEV], const float *one_hot, float *logits, void *stream,
                         void *const *feat_events);
int fcn_convnet_backward(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                         const float *const feats[FCN_CN_MAXLEV], const float *one_hot, const float *dlogits,
                         float *const dfeats[FCN_CN_MAXLEV], float *const dW[FCN_CN_MAXLAYER],
                         float *const dgamma[FCN_CN_MAXLAYER], float *const dbeta[FCN_CN_MAXLAYER], float *dbias,
                         void *stream, void *stream2, void *const *events);
/* One launch per chain layer (the off-chain deconvolution steps ride along): its data-gradient tiles, its weight-gradient
 * row splits and the reduce of the previous layer's splits are workgroup roles of the same kernel.  stream2 / events: NULL,
 * or a second stream + nlev caller-owned events -- after the launch that completes dfeats[nlev-1] the chain continues on
 * stream2 (events[0] = fork, events[k] = dfeats[nlev-1-k] final for k = 1..nlev-2, events[nlev-1] = all outputs final), so
 * work queued on `stream` after the call waits for the widest map's gradient only. */

/* ---------------------------------------------------------------------------------------------
 * Fused train-loss tail of PointNetDet.forward (models/det_base.py:373-476; focal loss models/common.py:217-232,
 * huber + box corners models/model_util.py:9-19,48-72, encode/decode models/box_transform.py:5-65).
 *   cls_raw (B,2,L2), reg_raw (B,3+2*NB+4*NS,L2): raw head outputs;  cls_label (B,L2) int64 in {-1,0,1};
 *   center_ref2 (B,3,L2); box3d_center (B,3); box3d_heading (B,1); box3d_size (B,3); size_class (B,1) int64;
 *   mean_size (NS,3).  NB must be 12 and NS 3 (KITTI) or 10 (SUN-RGBD), else FCN_E_LIMIT.
 *   out16: total, cls, center, head_cls, head_res, size_cls, size_res, corners, cls_acc, head_acc, size_acc, nfg
 *   dcls / dreg: d(total)/d(cls_raw), d(total)/d(reg_raw), same layouts (NULL to skip).
 * ------------------------------------------------------------------------------------------- */
int fcn_det_loss_tail(const float *cls_raw, const float *reg_raw, const int64_t *cls_label,
                      const float *center_ref2, const float *box3d_center, const float *box3d_heading,
                      const float *box3d_size, const int64_t *size_class, const float *mean_size,
                      int B, int L2, int num_heading_bin, int num_size_cluster,
                      float w_box, float w_corner, float w_headreg, float w_sizereg,
                      float *out16, float *dcls, float *dreg, void *stream);
/* Same on the row-major logits of fcn_convnet_forward: logits (B*L2, ld), dlogits same shape (fully written); ld = 64 when
 * 2 + 3 + 2*NB + 4*NS <= 64 (KITTI), else 128 (SUN-RGBD). */
int fcn_det_loss_tail_rows(const float *logits, const int64_t *cls_label, const float *center_ref2,
                           const float *box3d_center, const float *box3d_heading, const float *box3d_size,
                           const int64_t *size_class, const float *mean_size, int B, int L2,
                           int num_heading_bin, int num_size_cluster,
                           float w_box, float w_corner, float w_headreg, float w_sizereg,
                           float *out16, float *dlogits, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser step of the training loop (train/train_net_det.py:321-339 optim.Adam(lr, weight_decay); :131-133
 * optimizer.step()).  One streaming kernel over flat fp32 buffers of n elements (16-byte aligned), torch.optim.Adam
 * arithmetic (L2 weight decay, bias correction from the step counter).  Everything the host may change between steps
 * lives in device memory so the launch can sit inside a captured hipGraph:
 *   hyper6: lr, beta1, beta2, eps, weight_decay, grad_scale (grad is multiplied by grad_scale first: 1/world after a
 *           summing all-reduce);  step_slots: fcn_adam_step_slots(n) int64 counters, all equal (0 at start), every
 *           one advanced by the launch -- one per workgroup, so no workgroup waits on another. */
int64_t fcn_adam_step_slots(int64_t n);
int fcn_adam_step_f32(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, int64_t n,
                      const float *hyper6, int64_t *step_slots, void *stream);

/* The 'sgd' branch of the same loop (train/train_net_det.py:325-327 optim.SGD(lr, momentum, weight_decay)): torch.optim.SGD
 * arithmetic (L2 weight decay, dampening 0, no Nesterov) over the same flat buffers; momentum_buf starts at zero.
 *   hyper4 (device): lr, momentum, weight_decay, grad_scale. */
int fcn_sgd_step_f32(float *param, const float *grad, float *momentum_buf, int64_t n, const float *hyper4, void *stream);

/* Same with a persistent scratch buffer (fcn_det_loss_tail_scratch_floats(B, L2) floats, zeroed ONCE by the caller, then
 * owned by one stream at a time): no memset node in front of the launch, the workgroup partials are summed in a fixed
 * order (the 16 scalars are reproducible bit for bit), and `total` (1 float, may be NULL) receives a copy of out16[0].
 * Alignment (all three loss-tail entry points): cls_label -- and, in the row-major forms, logits and dlogits -- must be 16-byte
 * aligned (the kernel reads two labels / four logits per load and stores four gradient values at once); FCN_E_BADARG otherwise. */
int fcn_det_loss_tail_scratch_floats(int B, int L2);
int fcn_det_loss_tail_rows2(const float *logits, const int64_t *cls_label, const float *center_ref2,
                            const float *box3d_center, const float *box3d_heading, const float *box3d_size,
                            const int64_t *size_class, const float *mean_size, int B, int L2,
                            int num_heading_bin, int num_size_cluster,
                            float w_box, float w_corner, float w_headreg, float w_sizereg,
                            float *out16, float *dlogits, float *scratch, float *total, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rotated-box overlap after the heads.  The reference leaves the device for all of
 * it: numpy loops + boost::geometry polygon clipping on the host.
 * ------------------------------------------------------------------------------------------- */
/* rbbox_iou_3d_pair (ops/pybind11/box_ops.h:173-260, pybind "rbbox_iou_3d_pair"; call site models/det_base.py:495):
 * corners1/corners2 (n,8,3) in the corner order of get_box3d_corners_helper -> out2 (n,2) = [BEV IoU, 3-D IoU]. */
int fcn_box3d_iou_pair_f32(const float *corners1, const float *corners2, int n, float *out2, void *stream);
/* IoU training metrics of models/det_base.py:480-503 (which leaves the device for rbbox_iou_3d_pair on the host every step):
 * on the foreground rows (cls_label == 1) of the row-major logits (B*L2, ld), the box decoded with the arg-max heading bin /
 * size cluster against the label box.  out4 = mean BEV IoU, mean 3-D IoU, fraction with 3-D IoU >= iou_thresh
 * (cfg.IOU_THRESH), foreground count.  scratch8: 8 floats, zeroed ONCE by the caller (the launch leaves them zero). */
int fcn_det_iou_metrics(const float *logits, int ld, const int64_t *cls_label, const float *center_ref2,
                        const float *box3d_center, const float *box3d_heading, const float *box3d_size,
                        const float *mean_size, int B, int L2, int num_heading_bin, int num_size_cluster,
                        float iou_thresh, float *scratch8, float *out4, void *stream);
/* The per-frustum decode loop of train/test_net_det.py:254-293 on the row-major logits (B*L2, ld) of
 * fcn_convnet_forward (cols 0..1 cls, 2.. reg): method 1 ('nms'): every position with p_bg < p_fg, or the arg-max of p_fg
 * when a frustum has none; method 0 ('top'): the arg-max only.  Arg-max heading bin / size cluster decode, centre =
 * offset + center_ref2 (B,3,L2), from_prediction_to_label_format (datasets/provider_sample.py:375-387) with rot_angle (B),
 * ref_center (B,3) or NULL (zeros), rgb_prob (B) or NULL (ones).
 *   dets (B*L2, 8) = tx, ty, tz, l, w, h, ry, score (every row written); valid (B*L2) = selected and h,w,l >= 0.01. */
int fcn_decode_detections(const float *logits, int ld, const float *center_ref2, const float *mean_size,
                          const float *rot_angle, const float *ref_center, const float *rgb_prob, int B, int L2,
                          int num_heading_bin, int num_size_cluster, int method, float *dets, int32_t *valid,
                          void *stream);
/* The same with the decode rule as an argument.  FCN_DECODE_KITTI: the entry above, bit for bit.  FCN_DECODE_SUNRGBD: the loop of
 * train/test_net_det_sunrgbd.py:208-252 -- method 1 selects every position with p_fg > 0.5 (the arg-max of p_fg when a frustum has
 * none), the centre stays the box centre (datasets/provider_sample_sunrgbd.py:374-385: no h/2 shift of ty), and
 * score = rgb_prob + max_j softmax(size scores)_j; the class probability is not part of the score.  Heading / size decode, the
 * rotation by -rot_angle, ref_center, ry = heading + rot_angle and the h,w,l >= 0.01 filter are the same. */
#define FCN_DECODE_KITTI 0
#define FCN_DECODE_SUNRGBD 1
int fcn_decode_detections_rule(const float *logits, int ld, const float *center_ref2, const float *mean_size,
                               const float *rot_angle, const float *ref_center, const float *rgb_prob, int B, int L2,
                               int num_heading_bin, int num_size_cluster, int method, int rule, float *dets, int32_t *valid,
                               void *stream);
/* rotate_nms_3d_cc (ops/pybind11/rbbox_iou.py:294-311) -> rotate_non_max_suppression_3d_cpu (ops/pybind11/nms_cpu.h:148-240)
 * for num_groups independent detection sets at once (one per (frame, class), train/test_net_det.py:126-152): dets rows are
 * organised in units of rows_per_unit consecutive rows (one frustum each), unit_group (num_units) in [0, num_groups) assigns
 * units to groups, valid (rows) or NULL marks the candidate rows.  Greedy in descending score, suppress when the rotated
 * 3-D IoU >= thresh.  keep (num_groups, top_k): row indices in keep order; keep_cnt (num_groups): count, or -1 when a group
 * holds more than 4096 candidates (FCN_E_LIMIT condition reported per group, the other groups are still processed). */
int fcn_rotate_nms_3d(const float *dets, const int32_t *valid, const int32_t *unit_group, int num_units, int rows_per_unit,
                      int num_groups, float thresh, int top_k, int32_t *keep, int32_t *keep_cnt, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SUN-RGBD evaluation behind the NMS (csrc/det_eval.h).  The reference turns every kept row into corners and scores them in
 * Python on the host (train/test_net_det_sunrgbd.py:94-99, train/sunrgbd_eval/eval_det.py:89-169).
 * ------------------------------------------------------------------------------------------- */
/* compute_box_3d (datasets/data_utils.py:44-70) of n rows of dets (num_dets,8) = tx, ty, tz, l, w, h, ry, score with (tx,ty,tz)
 * the box CENTRE: rows (n) int32 picks them (NULL: rows 0 .. n-1, n <= num_dets).  corners (n,8,3) float32, corner k at
 * x = +-l/2 (+ + - - + + - -), y = +-h/2 (+ + + + - - - -), z = +-w/2 (+ - - + + - - +), rotated by roty(ry), moved to the centre.
 * A row index outside [0, num_dets) (an unused keep slot) is never dereferenced: its 24 numbers are NaN. */
int fcn_box3d_corners(const float *dets, int num_dets, const int32_t *rows, int n, float *corners, void *stream);
/* The matching loop of eval_det_cls (eval_det.py:134-159) for G (image, class) groups at once, CSR: the detections of group g are
 * rows [det_off[g], det_off[g+1]) of det_corners (nd,8,3) / scores (nd), its label boxes rows [gt_off[g], gt_off[g+1]) of
 * gt_corners (ng,8,3); both offset arrays (G+1) int32 ON THE DEVICE, ascending from 0 to nd / ng (the caller checks them on the
 * host; the kernel clamps what it reads to the buffers).  Corners in the order of compute_box_3d, as rbbox_iou_3d_pair reads
 * them (BEV polygon 6,7,4,5; y extents from corners 0 and 4).
 *   ovmax (nd): the largest 3-D IoU with a label box of the group (-inf when it has none); jmax (nd) int32: that label's index
 *   INSIDE its group, the first maximum under strict > (-1 when the group has none); tp (nd) int32: 1 when ovmax > thresh and no
 *   detection of the group with the same jmax and ovmax > thresh comes earlier in (score descending, input index ascending) --
 *   the reference's greedy walk, in which a detection whose best label is taken is a false positive even when a second label
 *   would qualify.  Equal scores: the lower input index first (np.argsort in the reference is unstable there). */
int fcn_det_match(const int32_t *det_off, const int32_t *gt_off, int G, const float *det_corners, const float *scores, int nd,
                  const float *gt_corners, int ng, float thresh, int32_t *tp, float *ovmax, int32_t *jmax, void *stream);
/* Precision / recall and AP per class (eval_det.py:161-169 + voc_ap :41-72, use_07_metric=False) of nd detections with flags tp
 * (nd) int32, scores (nd), det_class (nd) int32 in [0, C) and npos (C) int32 label boxes per class (every npos > 0: the caller's
 * duty).  rank (nd) int32: the place of a detection inside its class by (score descending, input index ascending); rec / prec (nd)
 * fp64: class c's curve in rank order at [base_c, base_c + n_c), base_c = number of detections of classes < c; ap (C) fp64, 0
 * for a class without a detection.  Integer cumulative counts; the curve, the envelope and the sum in fp64. */
int fcn_det_ap(const int32_t *tp, const float *scores, const int32_t *det_class, int nd, const int32_t *npos, int C,
               int32_t *rank, double *rec, double *prec, double *ap, void *stream);

/* ---------------------------------------------------------------------------------------------
 * KITTI evaluation behind the NMS (csrc/kitti_eval.h).  The reference writes label-format text files
 * (train/test_net_det.py:88-123) and shells out to train/kitti_eval/evaluate_object_3d_offline.cpp ("the evaluator" below), which
 * clips every (detection, label) pair with boost polygons once per class x difficulty x metric x (1 + thresholds).  Here every
 * pair is clipped once, in fp32, and nothing crosses to the host before the table.  Not restated: the %.4f / %f text round trip
 * of the result files, the plots, the mail.
 *   A LIST is k = (metric * 3 + class) * 3 + difficulty, 27 of them: metric 0 image, 1 ground, 2 3-D; class 0 car, 1 pedestrian,
 *   2 cyclist; difficulty 0 easy, 1 moderate, 2 hard.  A list has 41 threshold SLOTS.
 *   det_table (nd,13) float32 = alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry, score; det_class (nd) int32 in {0,1,2} (anything else:
 *   a type that is not evaluated); gt_table (ng,14) float32 = truncation, occlusion, alpha, x1,y1,x2,y2, h,w,l, tx,ty,tz, ry;
 *   gt_type (ng) int32: 0 Car, 1 Pedestrian, 2 Cyclist, 3 Van, 4 Person_sitting, 5 DontCare, 6 anything else.
 *   The detections / labels of frame f are rows [det_off[f], det_off[f+1]) / [gt_off[f], gt_off[f+1]); its pairs start at
 *   pair_off[f] = sum over the frames before it of (detections x labels); all three (F+1) int32 ON THE DEVICE, checked by the
 *   caller on the host; the kernels clamp what they read to nd / ng / npairs (a frame whose pairs would not fit is empty).
 *   ov (npairs,3) float32: the overlaps of pair (d, g) of frame f for the three metrics, at
 *   pair_off[f] + (d - det_off[f]) * labels_of_f + (g - gt_off[f]).
 *   class_mask: bit c set = class c is evaluated.
 * Every entry: caller-owned buffers and workspace, stream-ordered, no allocation, no synchronisation; FCN_E_BADARG writes nothing.
 * ------------------------------------------------------------------------------------------- */
/* The label-format row of n kept rows of dets (num_dets,8) = tx, ty, tz, l, w, h, ry, score (train/test_net_det.py:88-105,284-293):
 * rows (n) int32 picks them (NULL: rows 0 .. n-1), row_box (n) int32 the row of boxes2d (num_boxes,4) each came from.
 * table (n,13) as det_table above, alpha = compute_alpha (datasets/provider_sample.py:389-394; evaluated in fp64, sign(0) = 0);
 * ok (n) int32 = 0 where h, w or l < 0.01 (the reference drops such a row).  An index outside dets / boxes2d: NaN row, ok = 0. */
int fcn_kitti_label_rows(const float *dets, int num_dets, const int32_t *rows, int n, const float *boxes2d, int num_boxes,
                         const int32_t *row_box, float *table, int32_t *ok, void *stream);
/* imageBoxOverlap (evaluator :229-263), groundBoxOverlap (:296-316) and box3DOverlap (:319-346; y extent t2 - h .. t2) of every
 * pair of every frame, once: criterion -1 (union) against an ordinary label, criterion 0 (over the detection's own area / volume)
 * against a DontCare label, the only one the protocol asks of such a pair (:582).
 * flags (10) int32 (zeroed here): [metric * 3 + class] = 1 when the class has a detection with x1 >= 0 / tx != -1000 /
 * ty != -1000 (:162-170: a class is only evaluated if it is detected), [9] = 1 when some alpha is -10 (:158: no AOS then). */
int fcn_kitti_overlaps(const int32_t *det_off, const int32_t *gt_off, const int32_t *pair_off, int F, const float *det_table,
                       const int32_t *det_class, int nd, const float *gt_table, const int32_t *gt_type, int ng, float *ov,
                       int npairs, int32_t *flags, void *stream);
/* cleanData (:383-456) + computeStatistics(compute_fp = false) (:458-555) for every (frame, list): the labels are walked in input
 * order; each takes the unassigned candidate (class of the list, or below the minimum height: :449-454 look at the height first)
 * with overlap > MIN_OVERLAP and the highest score, the first index among equal scores.
 * assigned (27, nd, 2) int32 workspace (no initialisation needed); tp_score (27, ng) float32 + tp_count (27): the true positives'
 * scores of each list in no particular order; n_gt (27) the labels counted.  tp_count and n_gt are zeroed here. */
int fcn_kitti_pass_a(const int32_t *det_off, const int32_t *gt_off, const int32_t *pair_off, int F, const float *det_table,
                     const int32_t *det_class, int nd, const float *gt_table, const int32_t *gt_type, int ng, float *ov, int npairs,
                     int class_mask, int32_t *assigned, float *tp_score, int32_t *tp_count, int32_t *n_gt, void *stream);
/* getThresholds (:348-381) of the 27 lists: sorted (27, ng) float32 workspace receives each list in descending order, the recall
 * walk runs in fp64 as written.  thresholds (27,41) fp64 (0 behind the count), num_thresholds (27) int32. */
int fcn_kitti_thresholds(const float *tp_score, const int32_t *tp_count, const int32_t *n_gt, int ng, float *sorted,
                         double *thresholds, int32_t *num_thresholds, void *stream);
/* cleanData + computeStatistics(compute_fp = true) (:458-616) for every (frame, list, slot < num_thresholds) in one launch.
 * counts (3,27,41) int32 (zeroed here): tp, fp, fn; fp already without the detections a DontCare area holds (:558-591).
 * sim (F,9,41) fp64: per frame, (class, difficulty) and slot the sum of (1 + cos(alpha_gt - alpha_det)) / 2 over the image metric's
 * true positives in label order; slots < num_thresholds of evaluated classes are written, the rest is never read. */
int fcn_kitti_pass_b(const int32_t *det_off, const int32_t *gt_off, const int32_t *pair_off, int F, const float *det_table,
                     const int32_t *det_class, int nd, const float *gt_table, const int32_t *gt_type, int ng, float *ov, int npairs,
                     int class_mask, const double *thresholds, const int32_t *num_thresholds, int32_t *assigned, int32_t *counts,
                     double *sim, void *stream);
/* The curves and the AP (:680-699, :716-720): precision (27,41) = tp / (tp + fp), aos (9,41) = sum over the frames, in frame order,
 * of sim / (tp + fp); both filtered by the suffix maximum of std::max_element over all 41 entries (0 / 0 = NaN is kept as IEEE
 * has it); ap (27) and aos_ap (9) = (entries 0, 4, .., 40 summed) / 11 * 100 in fp64 -- the reference sums in float for printing
 * only, 11 * 2^-24 * 100 < 7e-5 away.  NaN rows for a class that flags / class_mask leave out; aos NaN when flags[9]. */
int fcn_kitti_curves(const int32_t *counts, const int32_t *num_thresholds, const double *sim, int F, const int32_t *flags,
                     int class_mask, double *precision, double *aos, double *ap, double *aos_ap, void *stream);

/* Measurement aid: stores the device's constant-rate wall clock (100 MHz ticks) into *slot, in stream order. */
int fcn_stamp(uint64_t *slot, void *stream);

/* Which hipGraph capture `stream` is part of, asked of the HIP runtime this library launches on: *id = 0 when the stream is not
 * capturing, the runtime's capture id + 1 otherwise.  Non-zero return: the query failed (hipError_t) or the capture was
 * invalidated (FCN_E_BADARG) -- treat the id as unknown.  No reference counterpart (the reference captures no graphs). */
int fcn_stream_capture_id(void *stream, uint64_t *id);

/* 16 hex characters: sha256 over the kernel sources, headers and compile flags this library was built from
 * (frustum_convnet_amd/build.py source_hash()).  The library travels prebuilt; __graft_entry__.smoke() and bench.py compare
 * it with the tree they run from, so a stale binary cannot pass for the committed sources. */
const char *fcn_build_hash(void);


/* ---------------------------------------------------------------------------------------------
 * On-device construction of one training batch from raw frustum records: replaces the
 * per-sample numpy work of datasets/provider_sample.py::ProviderDataset.__getitem__ (:137-262; generate_ref :291-327,
 * generate_labels :270-289, centre-view helpers :329-372) and torch's default_collate (:396-397).
 *   raw_pts (sum n_b, pt_stride) float32 records in rect camera coordinates, pt_off (B+1) int64 row offsets,
 *   raw_seg (sum n_b) int64 or NULL, choice (B,N) int32 resample indices (the reference's np.random.choice),
 *   frustum_angle (B), box2d (B,4), P (B,3,4), box3d_corners (B,8,3), heading (B), size (B,3) (l,w,h), coin (B)
 *   (flip when > 0.5), normal (B) (depth-shift draw): all fp64 like the pickled records.
 * Outputs (caller-owned): point_cloud (B,3,N), center_ref[s] (B,3,L[s]), cls_label (B,L[1]) int64 in {-1,0,1} (NULL to
 * skip), box3d_center (B,3), box3d_heading (B,1), box3d_size (B,3), rot_angle (B,1), seg_label (B,N) int64 or NULL. */
typedef struct fcn_inp_desc {
    int32_t B, N, pt_stride;     /* frustums, points per frustum after resampling, floats per raw record (>= 3) */
    int32_t L[4];                /* centres per stride: len(arange(0, max_depth, stride[s])) */
    double  stride[4], max_depth;
    int32_t random_flip, random_shift;
} fcn_inp_desc;
int fcn_prepare_inputs(const fcn_inp_desc *d, const float *raw_pts, const int64_t *pt_off, const int64_t *raw_seg,
                       const int32_t *choice, const double *frustum_angle, const double *box2d, const double *P,
                       const double *box3d_corners, const double *heading, const double *size,
                       const double *coin, const double *normal, float *point_cloud, float *const center_ref[4],
                       int64_t *cls_label, float *box3d_center, float *box3d_heading, float *box3d_size,
                       float *rot_angle, int64_t *seg_label, void *stream);

/* The same launch for inference records (datasets/provider_sample.py:184-195, from_rgb_detection): no label box in, no label
 * outputs, no augmentation (d->random_flip / random_shift must be 0).  Writes point_cloud, center_ref[4] and rot_angle. */
int fcn_prepare_inputs_infer(const fcn_inp_desc *d, const float *raw_pts, const int64_t *pt_off, const int32_t *choice,
                             const double *frustum_angle, const double *box2d, const double *P, float *point_cloud,
                             float *const center_ref[4], float *rot_angle, void *stream);

/* SUN-RGBD variant (cfgs/det_sample_sunrgbd.yaml; datasets/provider_sample_sunrgbd.py::ProviderDataset.__getitem__ :116-263,
 * generate_ref :283-326, project_image_to_upright_camera :28-59): five strides; the window centres go through the camera
 * matrix K (B,3,3) and the tilt rotation Rtilt (B,3,3) -- camera (x,y,z) -> (x,z,-y) -> Rtilt . -> (X,-Z,Y) -- instead of
 * the KITTI projection; random_shift also draws a height shift, hshift (B) = the np.random.random() value in [0,1), applied
 * as hshift*0.4-0.2 to the points' y and the box centre.  Everything else as fcn_prepare_inputs. */
typedef struct fcn_inp5_desc {
    int32_t B, N, pt_stride;
    int32_t L[5];
    double  stride[5], max_depth;
    int32_t random_flip, random_shift;
} fcn_inp5_desc;
int fcn_prepare_inputs_sunrgbd(const fcn_inp5_desc *d, const float *raw_pts, const int64_t *pt_off, const int64_t *raw_seg,
                               const int32_t *choice, const double *frustum_angle, const double *box2d, const double *K,
                               const double *Rtilt, const double *box3d_corners, const double *heading, const double *size,
                               const double *coin, const double *normal, const double *hshift, float *point_cloud,
                               float *const center_ref[5], int64_t *cls_label, float *box3d_center, float *box3d_heading,
                               float *box3d_size, float *rot_angle, int64_t *seg_label, void *stream);
/* Inference records of the SUN-RGBD loader (provider_sample_sunrgbd.py:165-186, from_rgb_detection): no label box in, no labels
 * out, no flip and no shift -- point_cloud, center_ref[5] and rot_angle alone.  The same kernel without a label box, as
 * fcn_prepare_inputs_infer is to fcn_prepare_inputs.  d->random_flip / random_shift must be 0. */
int fcn_prepare_inputs_sunrgbd_infer(const fcn_inp5_desc *d, const float *raw_pts, const int64_t *pt_off, const int32_t *choice,
                                     const double *frustum_angle, const double *box2d, const double *K, const double *Rtilt,
                                     float *point_cloud, float *const center_ref[5], float *rot_angle, void *stream);

/* Refinement-stage variant (cfgs/refine_car.yaml; datasets/provider_sample_refine.py::ProviderDataset.__getitem__ :176-315,
 * generate_ref :336-386, generate_labels :317-334, collate_fn :388-419): the sample is normalised to the first-stage
 * prediction (pred_corners (B,8,3), pred_angle (B), pred_size (B,3) = l,w,h, fp64 like the pickled records): points and label
 * box are translated to the predicted centre and rotated by its heading; the window centres span the predicted box's own
 * depth extent -- a different count per sample; every center_ref[s] (B,3,Lpad[s]) and cls_label (B,Lpad[1]) is padded by
 * repeating the last real entry, as the reference's collate_fn does (Lpad = the batch maxima, computed by the caller as
 * max_b len(np.arange(-w_b/2, w_b/2, stride[s]))); lens (B,4) receives the per-sample counts.  box3d_corners == NULL:
 * inference records (no labels; cls_label / box3d_* must be NULL).  Outputs rot_angle (B,1) = pred_angle and
 * ref_center (B,3) = predicted centre are what from_prediction_to_label_format needs to undo the normalisation.
 * PRECONDITION (the caller's: the widths live on the device, this call does not read them on the host): every pred_size width
 * (pred_size[3 b + 1]) is finite and > 0.  A sample whose width is <= 0 or NaN has no window on any stride: its lens are 0, its
 * center_ref rows are not meaningful and its cls_label row is NOT written.  frustum_convnet_amd.inputs.RefineInputBuilder
 * refuses such a batch with ValueError before the launch. */
typedef struct fcn_inp_refine_desc {
    int32_t B, N, pt_stride;
    int32_t Lpad[4];
    double  stride[4];
    int32_t random_flip, random_shift;
} fcn_inp_refine_desc;
int fcn_prepare_inputs_refine(const fcn_inp_refine_desc *d, const float *raw_pts, const int64_t *pt_off,
                              const int32_t *choice, const double *pred_corners, const double *pred_angle,
                              const double *pred_size, const double *box3d_corners, const double *heading,
                              const double *size, const double *coin, const double *normal, float *point_cloud,
                              float *const center_ref[4], int64_t *cls_label, float *box3d_center, float *box3d_heading,
                              float *box3d_size, float *rot_angle, float *ref_center, int32_t *lens, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The random draws fcn_prepare_inputs* reads -- choice (B,N) int32, coin (B), normal (B) and, for SUN-RGBD, hshift (B) fp64 -- made
 * on the device (csrc/draws.h) instead of by np.random on the host (datasets/provider_sample.py:165-168, :225, :238;
 * provider_sample_sunrgbd.py:144, :211, :224, :228).  The stream is a counter-based one, not numpy's; the contract, bit for bit
 * (INTEGRATION.md "Random draws on the device"; tests/draws_ref.py restates it in numpy):
 *   Philox4x32-10, key (seed lo, seed hi), counter (i, b, step lo, ((step >> 32) << 2) | tag); b the row, step = state[0] (< 2^62).
 *   n >= N (tag 0): key k_j = word j & 3 of block j >> 2; choice[b, :] = the j of the N smallest (k_j << 32) | j, ascending.
 *   0 < n < N (tag 1): choice[b, i] = (w * n) >> 32, w = word i & 3 of block i >> 2.
 *   tag 2, blocks 0 and 1 (w0..w7), u(x, y) = ((x >> 5) * 2^26 + (y >> 6)): coin = u(w0, w1) * 2^-53; u1 = (u(w2, w3) + 1) * 2^-53,
 *   u2 = u(w4, w5) * 2^-53, normal = sqrt(-2 ln u1) * cos(2 pi u2); hshift = u(w6, w7) * 2^-53.  random_flip == 0: coin = 0.0;
 *   random_shift == 0: normal = 0.0 and hshift = 0.5 (what inputs.draw*() give).
 * counts (B) int64: the rows n of each sample.  sub (packed int32) + sub_off (B+1) int64, both or neither: where
 * sub_off[b + 1] > sub_off[b], row b's n is that length and the value written is sub[sub_off[b] + c] instead of c.
 * A row with n <= 0 or n >= 2^31 gets choice = 0 throughout and sets bit 0 of *status (int32, device; never cleared here).
 * state (1) int64, device: read by every row, state[0] + 1 left behind in stream order (a second one-thread launch), so a replayed
 * capture draws anew and writing state[0] back reproduces a draw.  hshift may be NULL.  Capturable: no allocation, no host read.
 * B <= 0, N <= 0, a NULL required pointer or only one of sub / sub_off: FCN_E_BADARG; N > 2048: FCN_E_LIMIT; nothing is written. */
typedef struct fcn_draw_desc {
    int32_t B, N;                /* samples, indices per sample */
    int32_t random_flip, random_shift;
} fcn_draw_desc;
int fcn_draw_batch(const fcn_draw_desc *d, const int64_t *counts, const int32_t *sub, const int64_t *sub_off, uint64_t seed,
                   int64_t *state, int32_t *choice, double *coin, double *normal, double *hshift, int32_t *status, void *stream);
/* The largest N of fcn_draw_batch and the row count up to which a row is sorted whole in LDS (above it: radix select first). */
int fcn_draw_limits(int *max_n, int *sort_cap);

/* ---------------------------------------------------------------------------------------------
 * Epoch-exact label sampling on the device (csrc/epoch_pick.h): the D labels of a training step as a rank window of the epoch's
 * permutation, which is what the reference's DataLoader(shuffle=True, drop_last=True) walks (train/train_net_det.py:262-269).
 * The contract, bit for bit (INTEGRATION.md "Epoch-exact label sampling"; tests/draws_ref.choice_row(seed, e, 0, G, G) is perm_e):
 *   perm_e = the j of the G composites (k_j << 32) | j in ascending order, k_j = word j & 3 of Philox4x32-10 block j >> 2 at
 *   counter (block, 0, e lo, ((e >> 32) << 2) | 0), key (seed lo, seed hi): fcn_draw_batch's tag-0 order of row 0 at step e.
 *   pick[i] = perm_e[(t * world + rank) * D + i], i < D, with (e, t) = (state[0], state[1]) and G = count[0].
 *   T = G / (D * world) turns per epoch (integer division; the tail of G - T * D * world labels is dropped for that epoch).
 *   advance != 0: the state left behind is (e, t + 1) if t + 1 < T, else (e + 1, 0) -- stored in stream order behind every read
 *   of it, inside the one launch (one workgroup, behind a barrier), so a replayed capture moves on and writing the state back
 *   reproduces a pick.  Ranks with the same seed hold the same state and take disjoint windows.
 * count (1) int64, state (2) int64, pick (D) int32, status (1) int32: device.  G <= 0, G >= 2^31, D * world > G, e < 0, t < 0 or
 * t >= T: pick is all zeros, bit 0 of *status is set (never cleared here) and the state stays as it was; nothing is dereferenced
 * out of range.  Capturable: no allocation, no host read.  A NULL pointer, D < 1, world < 1 or rank outside [0, world):
 * FCN_E_BADARG; D > 2048: FCN_E_LIMIT; nothing is written. */
int fcn_epoch_pick(const int64_t *count, int D, int rank, int world, uint64_t seed, int64_t *state, int advance, int32_t *pick,
                   int32_t *status, void *stream);
/* The largest D of fcn_epoch_pick and the G up to which the permutation is sorted whole in LDS (above it: rank-window select). */
int fcn_epoch_pick_limits(int *max_d, int *sort_cap);

/* ---------------------------------------------------------------------------------------------
 * The link between the two stages of the cascade: first-stage detections -> the raw points of the refinement stage.  Replaces
 * the host loop of kitti/prepare_data_refine.py::extract_frustum_data_rgb_detection (:649-773): enlarge every predicted box by
 * `ratio` (1.2 there), keep the frame's points inside it (scipy.spatial.Delaunay(...).find_simplex), pickle them for
 * datasets/provider_sample_refine.py.
 *   frame_pts (sum m_f, pt_stride) float32 rect camera coordinates (columns from 3 on are carried along untouched),
 *   frame_off (F+1) int64 row offsets, dets (R,8) float32 rows as fcn_decode_detections writes them (ty = box bottom),
 *   cand_row (D) int32 indices into dets, cand_frame (D) int32 in [0, F).
 * fcn_refine_select_count writes, per candidate and in fp64 like the pickled records fcn_prepare_inputs_refine takes:
 *   pred_corners (D,8,3) of the ENLARGED box in the order of compute_box_3d_obj_array (:56-79: centre (tx, ty - h/2, tz),
 *   roty(ry)), pred_angle (D) = ry, pred_size (D,3) = l,w,h * ratio, and cnt (D) int32 = the number of frame points inside.
 * fcn_refine_select_fill takes out_off (D+1) int64 -- the caller's cumulative sum of cnt -- and writes out_pts
 * (out_off[D], pt_stride): for candidate d the selected rows of its frame at out_off[d].., in ascending frame order, as bit-exact
 * copies of all pt_stride floats (rows past out_off[d+1] are dropped, never stored).
 * Inside: |x'| <= l/2, |dy| <= h/2, |z'| <= w/2 in the enlarged box's frame ((x', z') = p - centre rotated back by ry), evaluated in
 * fp64 from the fp32 inputs, the same predicate in both calls; a point with a non-finite coordinate is never inside.  (The
 * reference's Delaunay test has a tolerance at the faces; this box is closed and exact.)
 * D == 0 or F == 0: nothing to select, returns 0 (cnt is zeroed when F == 0).  A candidate whose row or frame is out of range is
 * never dereferenced: its cnt is 0, nothing else of it is written, the other candidates are processed and the call returns
 * FCN_E_BADARG.  To report that, both calls read the two candidate lists back first (a stream synchronisation: not capturable
 * into a hipGraph). */
int fcn_refine_select_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                            const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, double *pred_corners,
                            double *pred_angle, double *pred_size, int32_t *cnt, void *stream);
int fcn_refine_select_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                           const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, const int64_t *out_off,
                           float *out_pts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The front of the pipeline: LiDAR frames in VELODYNE coordinates + per-frame calibration + 2-D detection boxes -> the raw
 * frustum points of the first stage in rect camera coordinates.  Replaces the host loop of
 * kitti/prepare_data.py::extract_frustum_data_rgb_detection (:462-568; kitti_util.Calibration.project_velo_to_rect /
 * project_rect_to_image / project_image_to_rect, draw_util.get_lidar_in_image_fov).
 *   frame_pts (sum m_f, pt_stride) float32 velodyne x, y, z, then columns that travel untouched (3 = intensity),
 *   frame_off (F+1) int64 row offsets, P (F,3,4), V2C (F,3,4), R0 (F,3,3), img_wh (F,2) = width, height: fp64,
 *   boxes (D,4) fp64 xmin ymin xmax ymax, box_frame (D) int32 in [0, F).
 * The grid is (S, D): workgroup (s, d) scans rows [s * seg, min((s + 1) * seg, m)) of box d's frame, seg =
 * fcn_frustum_select_seg() (a compile-time constant, a multiple of 256); S >= ceil(max m_f / seg), D <= 65535.
 * fcn_frustum_select_count writes seg_cnt (D,S) int32 (0 for segments beyond the frame) and, per box, box2d (D,4) -- the box
 * actually used: with clip_boxes != 0 x is clipped to [0, W-1] and y to [0, H-1] first (:523-524) -- and frustum_angle (D) =
 * -atan2(20, ((cu - P[0,2]) * 20) / P[0,0] + P[0,3] / (-P[0,0])), cu = (xmin + xmax) / 2 of that box (:537-543).
 * fcn_frustum_select_fill takes seg_off (D*S+1) int64 -- the caller's ONE cumulative sum over the flattened counts; entry d*S is
 * box d's offset -- and writes out_pts (seg_off[D*S], pt_stride): the selected rows in ascending frame order as (float) rect x,
 * y, z followed by bit-exact copies of columns 3..pt_stride-1.  A row whose position falls outside its workgroup's slice
 * [seg_off[i], seg_off[i+1]) is dropped, never stored.
 * Selected (one predicate for both calls, fp64 from the fp32 row, every sum left to right): ref = V2C . (x,y,z,1), rect = R0 . ref,
 * img = P . (rect,1), u = img_0 / img_2, v = img_1 / img_2; xmin <= u < xmax, ymin <= v < ymax, 0 <= u < W, 0 <= v < H and
 * (double)x > clip_distance (the velodyne x; get_lidar_in_image_fov's default is 2.0).  A row with a non-finite x, y or z is never
 * selected; img_2 has no guard (the reference has none).
 * D == 0: returns 0, touches nothing.  F == 0: returns 0 (seg_cnt is zeroed).  Both calls read box_frame and frame_off back first (a
 * stream synchronisation: NOT capturable into a hipGraph; the caller reads the counts between the two anyway): a box whose frame is
 * out of range is never dereferenced -- its counts are 0, nothing else of it is written, the other boxes are processed and the call
 * returns FCN_E_BADARG; a frame longer than S * seg rows is FCN_E_BADARG with no launch. */
int fcn_frustum_select_seg(void);
int fcn_frustum_select_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                             const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                             const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, double *box2d,
                             double *frustum_angle, int32_t *seg_cnt, void *stream);
int fcn_frustum_select_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                            const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                            const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const int64_t *seg_off,
                            float *out_pts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The same front for TRAINING: one ground-truth 3-D box beside each 2-D box.  Replaces the host loop of
 * kitti/prepare_data.py::extract_frustum_data (:260-391): the per-point foreground label (extract_pc_in_box3d :31-41, a Delaunay
 * hull of the corners there, the analytic test below here) and the box corners (kitti_util.compute_box_3d :324-359).  Every
 * argument of the select pair keeps its meaning; the grid, the segments, the selection predicate and the selected rows are theirs.
 *   gt_box3d (D,7) fp64 = tx, ty, tz, l, w, h, ry in rect camera coordinates as a KITTI label file has them: t is the centre of
 *   the box's BOTTOM face, y points down, ry turns about y.
 * fcn_frustum_label_count writes what fcn_frustum_select_count writes plus seg_pos (D,S) int32 -- the selected rows of the segment
 * that lie inside the 3-D box -- and corners (D,8,3) fp64 = roty(ry) . (x_k, y_k, z_k) + t with x_k = l/2 l/2 -l/2 -l/2 (twice),
 * y_k = 0 (four times) then -h, z_k = w/2 -w/2 -w/2 w/2 (twice): compute_box_3d's order.
 * fcn_frustum_label_fill writes what fcn_frustum_select_fill writes plus out_seg (seg_off[D*S]) int64: 1 for a row inside the box,
 * else 0, at the row's position in out_pts.  seg_off bounds both stores: a row outside its workgroup's slice is dropped from both,
 * so a box whose slices are all empty writes nothing (the way to leave a rejected box out of the packed buffers).
 * Inside (one function for both calls, fp64, every sum left to right) is decided on the row's rect coordinates AFTER their rounding
 * to float32, the values out_pts holds: c = cos(ry), s = sin(ry), dx = x - tx, dy = y - ty, dz = z - tz, ax = c * dx - s * dz,
 * az = s * dx + c * dz; inside iff |ax| <= l/2, |az| <= w/2 and -h <= dy <= 0.  A point exactly on a face is inside.
 * box2d, frustum_angle, corners, out_pts and out_seg are what fcn_prepare_inputs takes as box2d, frustum_angle, corners, raw and seg
 * (heading = ry, size = l, w, h).
 * D == 0: returns 0, touches nothing.  F == 0: returns 0 (the count zeroes seg_cnt and seg_pos).  NULL pointers, pt_stride < 3,
 * S < 1, D > 65535 and a frame longer than S * seg rows are FCN_E_BADARG with no launch; a box whose frame is out of range is never
 * dereferenced -- its counts are 0, nothing else of it is written, the other boxes are processed and the call returns
 * FCN_E_BADARG.  Both calls synchronise the stream, as the select pair does. */
int fcn_frustum_label_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                            const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                            const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const double *gt_box3d,
                            double *box2d, double *frustum_angle, int32_t *seg_cnt, int32_t *seg_pos, double *corners,
                            void *stream);
int fcn_frustum_label_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                           const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                           const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const double *gt_box3d,
                           const int64_t *seg_off, float *out_pts, int64_t *out_seg, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The first stage's training input with no host read between its launches (csrc/frustum_plan.h; INTEGRATION.md "Capturable
 * first-stage training input" states the contract bit for bit, tests/frustum_plan_ref.py restates it in numpy): perturb, count,
 * plan, fill -- none of them reads anything back, allocates or synchronises, so the sequence can be captured into a hipGraph.
 * Status bits (*status: one int32 on the device, OR-ed, never cleared here): bit 1 (2) fewer than B surviving boxes; bit 2 (4) rows
 * dropped because the total exceeds `capacity`; bit 4 (16) a box fcn_box2d_perturb could not perturb.  (Bit 0 is fcn_draw_batch's.)
 *
 * fcn_box2d_perturb: kitti/prepare_data.py::random_shift_box2d (:55-77) for D boxes.  boxes (D,4) fp64 xmin ymin xmax ymax,
 * box_frame (D) int32, img_wh (F,2) fp64 width, height; out (D,4) fp64.  Philox4x32-10 as fcn_draw_batch keys it, counter
 * (block, d, step lo, ((step >> 32) << 2) | 3), step = state[0]: attempt t takes blocks 2t and 2t + 1 = words w0..w7, its four
 * uniforms u(w0,w1), u(w2,w3), u(w4,w5), u(w6,w7), each * 2^-53, serve cx, cy, h, w in that order.  With r = shift_ratio,
 * w = xmax - xmin, h = ymax - ymin, cx = (xmin + xmax) / 2, cy = (ymin + ymax) / 2, in fp64, one rounding per operation:
 *   cx2 = cx + (w * r) * (u * 2 - 1), cy2 likewise with h; h2 = h * ((1 + (u * 2) * r) - r), w2 likewise with w;
 *   x = fmin(fmax(cx2 -+ w2 / 2, 0), W - 1), y = fmin(fmax(cy2 -+ h2 / 2, 0), H - 1).
 * The first attempt with xmin' < xmax' and ymin' < ymax' wins.  After fcn_box2d_perturb_limits' `attempts` (32) failed attempts,
 * or when box_frame[d] is outside [0, F), out[d] = boxes[d] and bit 4 of *status is set: never silent, never unwritten.
 * advance != 0: a one-thread launch behind the kernel leaves state[0] + 1.  NULL pointers, D < 0, F < 0 or shift_ratio outside
 * [0, 1): FCN_E_BADARG, nothing written. */
int fcn_box2d_perturb(const double *boxes, const int32_t *box_frame, const double *img_wh, int D, int F, double shift_ratio,
                      uint64_t seed, const int64_t *state, int advance, double *out, int32_t *status, void *stream);
int fcn_box2d_perturb_limits(int *attempts);
/* fcn_frustum_label_count / _fill without the read-back of box_frame and frame_off: the same kernels, arguments, outputs and
 * argument refusals.  A box whose frame is out of range is skipped as there (its counts are 0) but NOT reported, and "no frame is
 * longer than S * fcn_frustum_select_seg() rows" is the caller's duty: rows beyond S segments would silently not be searched. */
int fcn_frustum_train_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                            const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                            const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const double *gt_box3d,
                            double *box2d, double *frustum_angle, int32_t *seg_cnt, int32_t *seg_pos, double *corners,
                            void *stream);
int fcn_frustum_train_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                           const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                           const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const double *gt_box3d,
                           const int64_t *seg_off, float *out_pts, int64_t *out_seg, void *stream);
/* fcn_frustum_train_plan: what the host does between count and fill, as one workgroup.  seg_cnt, seg_pos (D,S) int32 from the
 * count; gt_box2d (D,4) fp64 the unperturbed label boxes.  Box d survives iff not (gt_box2d[d,3] - gt_box2d[d,1] < min_box_height)
 * and sum_s seg_pos[d,s] > 0.  The first B survivors in box order take slots 0..n-1: slot_box (B) int32 their box (0 for an empty
 * slot), *n_kept = n.  seg_off (D*S+1) int64 = min(capacity, the exclusive prefix sum over the flattened segments of seg_cnt where
 * the box holds a slot, else 0), the last entry the clamped total: what the fill takes, so a box without a slot writes nothing and
 * rows beyond `capacity` are dropped (bit 2).  off (B+1) int64: off[i] = seg_off[slot_box[i] * S] for i < n, the clamped total
 * from n on (an empty slot has no rows).  n < B sets bit 1.  Every output is written on every call.
 * NULL pointers, D < 0, S < 1, B < 1, capacity < 0: FCN_E_BADARG; D or B > 2048 or D * S > 65536 (fcn_frustum_train_plan_limits):
 * FCN_E_LIMIT; nothing written. */
int fcn_frustum_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, const double *gt_box2d, double min_box_height, int D,
                           int S, int B, int64_t capacity, int32_t *slot_box, int64_t *seg_off, int64_t *off, int32_t *n_kept,
                           int32_t *status, void *stream);
int fcn_frustum_train_plan_limits(int *max_d, int *max_segs);

/* ---------------------------------------------------------------------------------------------
 * The SUN-RGBD front: upright-depth frames + per-frame K and Rtilt + 2-D boxes (+ one label 3-D box beside each) -> the raw
 * records fcn_prepare_inputs_sunrgbd(_infer) takes.  Replaces the host loops of sunrgbd/prepare_data.py::extract_frustum_data
 * (:132-267) and extract_frustum_data_from_rgb_detection (:270-381).  The grid, the segments (fcn_frustum_select_seg() rows), the
 * two-call protocol (count, the caller's cumulative sum over the flattened (D*S) counts, fill), seg_off's bounding of every store
 * and the refusals are those of fcn_frustum_select_count / _fill and fcn_frustum_label_count / _fill; only the geometry differs.
 *   frame_pts (sum m_f, pt_stride >= 3) float32 UPRIGHT DEPTH x, y, z then r, g, b, ...; K (F,9), Rtilt (F,9) fp64 row-major;
 *   boxes (D,4) xmin ymin xmax ymax, used as given (neither reference path clips); box_frame (D).
 * Selected (one predicate, fp64 from the fp32 row, sums left to right): d = Rtilt^T . (x,y,z), c = (d0, -d2, d1), i = K . c,
 * u = i0 / i2, v = i1 / i2; xmin <= u < xmax and ymin <= v < ymax.  There is no image-bounds test, no clip distance and no guard
 * on i2 (the reference has none: a row behind the camera that projects into the box is selected there too).  A row with a
 * non-finite x, y or z is never selected.  A selected row is stored in upright CAMERA coordinates, (x, -z, y) of the input row --
 * an exact swap and negation -- followed by bit-exact copies of columns 3..pt_stride-1.
 * frustum_angle (D) = -atan2(ud1, ud0) with X = ((cu - K02) * 20) / K00, Y = ((cv - K12) * 20) / K11, ud = Rtilt . (X, 20, -Y)
 * for the box centre (cu, cv): project_image_to_upright_camera of (cu, cv, 20).
 * Labelled pair: gt_box3d (D,7) fp64 = cx, cy, cz, l, w, h, heading in upright depth, l w h the HALF extents of the label file
 * (SUNObject3d.l / .w / .h), heading = SUNObject3d.heading_angle.  seg_pos (D,S) counts the selected rows inside the box, out_seg
 * is 1 for such a row; inside (closed, on the INPUT row): c = cos(-heading), s = sin(-heading), dx = x - cx, dy = y - cy,
 * dz = z - cz, ax = c * dx + s * dy, ay = -s * dx + c * dy; |ax| <= l, |ay| <= w and |dz| <= h.  corners (D,8,3) =
 * rotz(-heading) . (x_k, y_k, z_k) + centroid with x_k = -l l l -l (twice), y_k = w w -w -w (twice), z_k = h (four times) then -h
 * (sunrgbd_utils.compute_box_3d's order), flipped to upright camera (X, -Z, Y): what fcn_prepare_inputs_sunrgbd takes as
 * box3d_corners (heading = heading, size = 2l, 2w, 2h).
 * D == 0: returns 0, touches nothing.  F == 0: returns 0 (the counts zero seg_cnt / seg_pos).  NULL pointers, pt_stride < 3,
 * S < 1, D > 65535 and a frame longer than S * seg rows are FCN_E_BADARG with no launch; a box whose frame is out of range is
 * never dereferenced -- its counts are 0, nothing else of it is written, the other boxes are processed and the call returns
 * FCN_E_BADARG.  Every call synchronises the stream (box_frame and frame_off are read back first). */
int fcn_frustum_sunrgbd_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                              const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                              double *frustum_angle, int32_t *seg_cnt, void *stream);
int fcn_frustum_sunrgbd_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                             const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                             const int64_t *seg_off, float *out_pts, void *stream);
int fcn_frustum_sunrgbd_label_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                    const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                    const double *gt_box3d, double *frustum_angle, int32_t *seg_cnt, int32_t *seg_pos,
                                    double *corners, void *stream);
int fcn_frustum_sunrgbd_label_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                   const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                   const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg, void *stream);
/* The positives a unit keeps under a subsample of its rows (prepare_data.py:219-226 rejects on the count AFTER its 2048-row
 * subsample): pos[u] = the number of j in [sub_off[u], sub_off[u+1]) with seg[off[u] + sub[j]] != 0; a unit whose range is empty
 * has no subsample and counts all its cnt[u] rows.  seg int64 (out_seg), off (U) int64 first rows, cnt (U) int32, sub int32,
 * sub_off (U+1) int64, pos (U) int32.  One workgroup per unit.  An index outside [0, cnt[u]) is skipped, never dereferenced.
 * U == 0: returns 0, touches nothing. */
int fcn_frustum_subset_pos(const int64_t *seg, const int64_t *off, const int32_t *cnt, const int32_t *sub, const int64_t *sub_off,
                           int U, int32_t *pos, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The SUN-RGBD training input with no host read between its launches (csrc/frustum_sunrgbd_plan.h; INTEGRATION.md "Capturable
 * SUN-RGBD training input" states the contract bit for bit, tests/sunrgbd_plan_ref.py restates it in numpy): perturb, count, plan,
 * fill, subsample, fcn_frustum_subset_pos, slots, sliced draw -- none of them reads anything back, allocates or synchronises, so the
 * sequence can be captured into a hipGraph.  Status bits (*status: one int32 on the device, OR-ed, never cleared here): bit 1 (2)
 * fewer than B surviving boxes; bit 2 (4) rows dropped because the total exceeds `capacity`.  Bit 0 is the draws'; bit 4 is never set.
 *
 * fcn_box2d_perturb_sunrgbd: sunrgbd/sunrgbd_utils.py::random_shift_box2d (:208-221) for D boxes, no clip, no retry.  boxes, out
 * (D,4) fp64 xmin ymin xmax ymax.  The stream is fcn_box2d_perturb's: Philox4x32-10, counter (block, d, step lo,
 * ((step >> 32) << 2) | 3), step = state[0], blocks 0 and 1 = words w0..w7; the four uniforms u(w0,w1), u(w2,w3), u(w4,w5), u(w6,w7),
 * each * 2^-53, serve cx, cy, h, w in that order.  With r = shift_ratio, w = xmax - xmin, h = ymax - ymin, cx = (xmin + xmax) / 2,
 * cy = (ymin + ymax) / 2, in fp64, one rounding per operation:
 *   cx2 = cx + (w * r) * (u * 2 - 1), cy2 likewise with h; h2 = h * ((1 + (u * 2) * r) - r), w2 likewise with w;
 *   out = cx2 - w2 / 2, cy2 - h2 / 2, cx2 + w2 / 2, cy2 + h2 / 2.
 * D == 0: the pass-through (nothing written).  advance != 0: a one-thread launch behind the kernel leaves state[0] + 1.
 * NULL pointers, D < 0 or shift_ratio outside [0, 1): FCN_E_BADARG, nothing written. */
int fcn_box2d_perturb_sunrgbd(const double *boxes, int D, double shift_ratio, uint64_t seed, const int64_t *state, int advance,
                              double *out, void *stream);
/* fcn_frustum_sunrgbd_label_count / _fill without the read-back of box_frame and frame_off: the same kernels, arguments, outputs and
 * argument refusals.  A box whose frame is out of range is skipped as there (its counts are 0) but NOT reported, and "no frame is
 * longer than S * fcn_frustum_select_seg() rows" is the caller's duty: rows beyond S segments would silently not be searched. */
int fcn_frustum_sunrgbd_train_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                    const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                    const double *gt_box3d, double *frustum_angle, int32_t *seg_cnt, int32_t *seg_pos,
                                    double *corners, void *stream);
int fcn_frustum_sunrgbd_train_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                   const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                   const double *gt_box3d, const int64_t *seg_off, float *out_pts, int64_t *out_seg, void *stream);
/* fcn_frustum_sunrgbd_train_plan: what the host does between count and fill, as one workgroup.  seg_cnt, seg_pos (D,S) int32 from
 * the count.  Box d is PRE-KEPT iff sum_s seg_pos[d,s] >= min_positives.  seg_off (D*S+1) int64 = min(capacity, the exclusive prefix
 * sum over the flattened segments of seg_cnt where the box is pre-kept, else 0), the last entry the clamped total: what the fill
 * takes, so a dropped box writes nothing and rows beyond `capacity` are dropped (bit 2).  row0 (D) int64 = seg_off[d * S].
 * cnt_stored (D) int32 = seg_off[(d + 1) * S] - seg_off[d * S]: the rows of box d that fit under the clamp, 0 for a dropped box.
 * sub_off (D+1) int64 = the exclusive prefix sum of (cnt_stored[d] > cap ? cap : 0): box d's slice of the subsample table, empty
 * for a box of at most `cap` stored rows.  Every output is written on every call; the limits are fcn_frustum_train_plan_limits'.
 * NULL pointers, D < 0, S < 1, cap < 1, capacity < 0: FCN_E_BADARG; D > 2048 or D * S > 65536: FCN_E_LIMIT; nothing written. */
int fcn_frustum_sunrgbd_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, int min_positives, int cap, int D, int S,
                                   int64_t capacity, int64_t *seg_off, int64_t *row0, int32_t *cnt_stored, int64_t *sub_off,
                                   int32_t *status, void *stream);
/* fcn_frustum_subsample_draw: the reference's rng.choice(n, cap, replace=False) of every frustum over `cap` rows
 * (sunrgbd/prepare_data.py:219-224), on the draws' stream.  For every box d with sub_off[d + 1] > sub_off[d]:
 * sub[sub_off[d] + i], i < cap, = row d of fcn_draw_batch's choice at N = cap, n = cnt_stored[d] (tag 0: the indices of the `cap`
 * smallest composites, ascending by composite) -- the same kernel, so `cap` distinct indices in [0, cnt_stored[d]).  Nothing else of
 * sub is written.  A box with such a slice and cnt_stored[d] <= 0 gets zeros and bit 0 of *status (the plan never produces one).
 * D == 0: the pass-through.  advance != 0: state[0] + 1 is left behind.  NULL pointers, D < 0, cap < 1: FCN_E_BADARG; cap > the
 * largest N of fcn_draw_limits: FCN_E_LIMIT; nothing written. */
int fcn_frustum_subsample_draw(const int32_t *cnt_stored, const int64_t *sub_off, int D, int cap, uint64_t seed, int64_t *state,
                               int advance, int32_t *sub, int32_t *status, void *stream);
/* fcn_frustum_sunrgbd_train_slots: behind fcn_frustum_subset_pos (U = D, off = row0, cnt = cnt_stored -> pos (D) int32).  Box d
 * survives iff it is pre-kept (seg_pos, as in the plan) and pos[d] >= min_positives.  The first B survivors in box order take slots
 * 0..n-1; for slot i < n with box d: slot_box[i] = d, off[i] = row0[d], counts[i] = cnt_stored[d], sub_start[i] = sub_off[d] and
 * sub_len[i] = sub_off[d + 1] - sub_off[d] (both 0 for a box without a subsample).  For an empty slot i >= n: slot_box 0, off =
 * capacity (the spare row of the point buffer), counts 0, sub_start 0, sub_len 0.  *n_kept = n; n < B sets bit 1.  slot_box (B) int32,
 * off, counts, sub_start (B) int64, sub_len (B) int32.  Every output is written on every call.
 * NULL pointers, D < 0, S < 1, B < 1, capacity < 0: FCN_E_BADARG; D or B > 2048 or D * S > 65536: FCN_E_LIMIT; nothing written. */
int fcn_frustum_sunrgbd_train_slots(const int32_t *seg_pos, const int32_t *pos, const int64_t *row0, const int32_t *cnt_stored,
                                    const int64_t *sub_off, int min_positives, int D, int S, int B, int64_t capacity,
                                    int32_t *slot_box, int32_t *n_kept, int64_t *off, int64_t *counts, int64_t *sub_start,
                                    int32_t *sub_len, int32_t *status, void *stream);
/* fcn_draw_batch with the subsample slices given per row: where sub_len[b] > 0, row b's n is sub_len[b] and the value written is
 * sub[sub_start[b] + c] instead of c (sub_start, sub_len: B entries each, the slices need not be packed or ordered).  The same
 * words, tags, scalars and status bit; given slices that happen to be packed it equals fcn_draw_batch bit for bit.  sub, sub_start
 * and sub_len are required; otherwise the refusals of fcn_draw_batch. */
int fcn_draw_batch_sliced(const fcn_draw_desc *d, const int64_t *counts, const int32_t *sub, const int64_t *sub_start,
                          const int32_t *sub_len, uint64_t seed, int64_t *state, int32_t *choice, double *coin, double *normal,
                          double *hshift, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The cascade link for TRAINING the refinement stage: first-stage detections + the frames' label boxes -> the labelled raw
 * records fcn_prepare_inputs_refine takes.  Replaces the host loop of kitti/prepare_data_refine.py::extract_frustum_det_data
 * (:406-592) and, with the label boxes themselves as detections, of extract_frustum_data (:239-403).
 *   frame_pts, frame_off, F, pt_stride, dets (R,8), cand_row (D), cand_frame (D), ratio: as fcn_refine_select_count takes them;
 *   gt_box3d (G,7) fp64 = tx, ty, tz, l, w, h, ry as a KITTI label file has them (t the centre of the BOTTOM face).
 * fcn_refine_match: gt_off (F+1) int64 -- the label boxes of frame f are rows [gt_off[f], gt_off[f+1]) of gt_box3d.  Per candidate
 *   the 3-D IoU of its centre form (tx, ty - h/2, tz, l, w, h, ry) against every label box of its frame (the float32 clip core of
 *   the NMS, on the label box taken relative to the candidate's centre in fp64), best_iou (D) float32 = the largest (0 for a frame
 *   without label boxes) and gt_idx (D) int32 = its row of gt_box3d, the LOWEST row among equal maxima, or -1 when the frame has no
 *   label box or !(best_iou >= thresh) (:493-499; a NaN matches nothing).  rbbox_iou_3d's standup-box prefilter only zeroes pairs
 *   whose IoU is 0 anyway and is not restated.
 * fcn_refine_label_count / _fill: units u = d * A + a, candidate d, copy a of A (1 <= A <= 64, D * A <= 65535); cand_gt (D) int32 =
 *   the label row of each candidate, negative: its units are empty (counts 0, nothing else written).  The enlarged box of unit u
 *   is candidate d's box times ratio, then jitter steps 0..a of random_shift_rotate_box3d (:203-236) with r = shift_ratio, each on
 *   the result of the one before (the reference's copies chain, :513-519), from jitter (D,A,7) fp64 uniform draws in [0,1) in the
 *   reference's order l, h, w, cx, cy, cz, angle: l1 = l + l*r*(u*2-1) (h1, w1 likewise), cx1 = cx + l*r*(u*2-1), cy1 = cy +
 *   h*r*(u*2-1), cz1 = cz + w*r*(u*2-1), angle1 = ((ry + pi) + r*(u*2-1)*pi) mod 2 pi (floored) - pi.  jitter == NULL: no jitter,
 *   A must be 1, and the boxes, counts and rows are fcn_refine_select_count / _fill's bit for bit.
 *   The grid is (S, D * A) over the segments of fcn_frustum_select_seg() rows; S >= ceil(max m_f / seg).
 *   count writes seg_cnt (D*A,S) int32 = the rows of the segment inside the unit's enlarged box, seg_pos (D*A,S) int32 = those of
 *   them inside the label box (NOT enlarged; centre (tx, ty - h/2, tz)), and per unit pred_corners (D*A,8,3), pred_angle, pred_size
 *   (D*A,3) of the jittered enlarged box, gt_corners (D*A,8,3), gt_heading, gt_size (D*A,3) of the label box -- both corner sets in
 *   the order of compute_box_3d_obj_array: what fcn_prepare_inputs_refine takes as pred_corners, pred_angle, pred_size,
 *   box3d_corners, heading, size.
 *   fill takes seg_off (D*A*S+1) int64 -- the caller's ONE cumulative sum over the flattened counts, with the counts of a rejected
 *   unit (no positive: :547) set to 0 first -- and writes out_pts as fcn_refine_select_fill does: bit-exact copies of all pt_stride
 *   floats, ascending frame order, a row outside its workgroup's slice [seg_off[i], seg_off[i+1]) dropped, never stored.
 * Inside, for both boxes: fcn_refine_select_count's closed box in fp64 from the fp32 row; a non-finite row is never inside.  The
 * per-point label is not written: the refinement loader never reads it.
 * D == 0: returns 0, touches nothing.  F == 0: returns 0 (match: gt_idx = -1, best_iou = 0; count: both counts zeroed).  NULL
 * pointers, pt_stride < 3, S < 1, A out of range, NULL jitter with A != 1, D * A > 65535 and a frame longer than S * seg rows are
 * FCN_E_BADARG with no launch.  A candidate whose row or frame is out of range, or whose cand_gt >= G, is never dereferenced: its
 * counts are 0 (match: gt_idx = -1), nothing else of it is written, the others are processed and the call returns FCN_E_BADARG.
 * All three calls read their index lists back first (a stream synchronisation: NOT capturable into a hipGraph; the capturable
 * forms are fcn_refine_train_match / _count / _fill below). */
int fcn_refine_match(const float *dets, int R, const int32_t *cand_row, const int32_t *cand_frame, int D, const double *gt_box3d,
                     int G, const int64_t *gt_off, int F, double thresh, int32_t *gt_idx, float *best_iou, void *stream);
int fcn_refine_label_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                           const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, const int32_t *cand_gt,
                           const double *gt_box3d, int G, int A, const double *jitter, double shift_ratio, int S,
                           int32_t *seg_cnt, int32_t *seg_pos, double *pred_corners, double *pred_angle, double *pred_size,
                           double *gt_corners, double *gt_heading, double *gt_size, void *stream);
int fcn_refine_label_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                          const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, const int32_t *cand_gt,
                          const double *gt_box3d, int G, int A, const double *jitter, double shift_ratio, int S,
                          const int64_t *seg_off, float *out_pts, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The refinement stage's training input with no host read between its launches (csrc/refine_plan.h; INTEGRATION.md "Capturable
 * refine-stage training input" states the contract bit for bit, tests/refine_plan_ref.py restates it in numpy): match, jitter
 * draw, count, plan, fill -- none of them reads anything back, allocates or synchronises, so the sequence can be captured into a
 * hipGraph.  Status bits (*status: one int32 on the device, OR-ed, never cleared here): bit 1 (2) fewer than B surviving units;
 * bit 2 (4) rows dropped because the total exceeds `capacity`; bit 5 (32) a unit with positives whose predicted width needs more
 * windows than lpad on some stride; bit 6 (64) a unit with positives whose predicted width is not a positive finite number.
 * (Bit 0 is fcn_draw_batch's.)
 *
 * fcn_refine_train_match / _count / _fill: fcn_refine_match, fcn_refine_label_count / _fill without the read-back of cand_row,
 * cand_frame, cand_gt and frame_off: the same kernels, arguments, outputs and argument refusals.  A candidate whose row or frame is
 * out of range, or whose cand_gt >= G, is skipped as there (its counts are 0; match: gt_idx = -1, best_iou = 0; nothing of it is
 * dereferenced) but NOT reported: the calls return 0.  "No frame is longer than S * fcn_frustum_select_seg() rows" is the caller's
 * duty: rows beyond S segments would silently not be searched. */
int fcn_refine_train_match(const float *dets, int R, const int32_t *cand_row, const int32_t *cand_frame, int D,
                           const double *gt_box3d, int G, const int64_t *gt_off, int F, double thresh, int32_t *gt_idx,
                           float *best_iou, void *stream);
int fcn_refine_train_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                           const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, const int32_t *cand_gt,
                           const double *gt_box3d, int G, int A, const double *jitter, double shift_ratio, int S,
                           int32_t *seg_cnt, int32_t *seg_pos, double *pred_corners, double *pred_angle, double *pred_size,
                           double *gt_corners, double *gt_heading, double *gt_size, void *stream);
int fcn_refine_train_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                          const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, const int32_t *cand_gt,
                          const double *gt_box3d, int G, int A, const double *jitter, double shift_ratio, int S,
                          const int64_t *seg_off, float *out_pts, void *stream);
/* fcn_box3d_jitter_draw: the (D,A,7) fp64 uniforms in [0,1) that fcn_refine_label_count / fcn_refine_train_count take as `jitter`,
 * for every unit u = d * A + a, one lane per unit.  Philox4x32-10 as fcn_draw_batch keys it, counter (block, u, step lo,
 * ((step >> 32) << 2) | 3), step = state[0]: blocks 0..3 give words w0..w15, uniform j = u53(w[2j], w[2j+1]) * 2^-53 for
 * j = 0..6 in the reference's order l, h, w, cx, cy, cz, angle (u53(hi, lo) = (hi >> 5) * 2^26 + (lo >> 6)); words 14 and 15 are
 * unused.  advance != 0: a one-thread launch behind the kernel leaves state[0] + 1.  D == 0 writes nothing (apart from the advance).
 * NULL pointers, D < 0, A < 1 or A > 64: FCN_E_BADARG; D * A > 65535: FCN_E_LIMIT; nothing written. */
int fcn_box3d_jitter_draw(int D, int A, uint64_t seed, const int64_t *state, int advance, double *jitter, void *stream);
/* fcn_refine_train_plan: what the host does between count and fill, as one workgroup.  seg_cnt, seg_pos (U,S) int32 and pred_size
 * (U,3) fp64 from the count; stride[4] fp64 and lpad[4] int32 (host arrays): the builder's strides and the FIXED padded window
 * counts of the batch.  A unit with sum_s seg_pos == 0 takes no slot and no room (the reject rule, :547; it covers the units of
 * unmatched candidates, whose rows of pred_size the count never wrote: pred_size[u] is read only when unit u has a positive).  For
 * a unit with a positive, w = pred_size[3u + 1]: !(w > 0 and finite) -> no slot, bit 6; else ceil((w / 2 - (-w / 2)) / stride[s]) >
 * lpad[s] on any stride (fcn_prepare_inputs_refine's own expression, compared in fp64) -> no slot, bit 5.  The first B surviving
 * units in unit order take slots 0..n-1: slot_unit (B) int32 their unit, U for an empty slot (the spare row of the caller's
 * per-unit tables), *n_kept = n.  seg_off (U*S+1) int64 = min(capacity, the exclusive prefix sum over the flattened segments of
 * seg_cnt where the unit holds a slot, else 0), the last entry the clamped total: what the fill takes.  off (B+1) int64: off[i] =
 * seg_off[slot_unit[i] * S] for i < n, `capacity` for n <= i < B (the spare row of a point buffer of capacity + 1 rows, which the
 * fill never stores), off[B] the clamped total.  counts (B) int64: the STORED rows of each slot, seg_off[(u+1)*S] - seg_off[u*S],
 * 0 for an empty slot.  n < B sets bit 1, a total above capacity bit 2.  Every output is written on every call.
 * NULL pointers, U < 0, S < 1, B < 1, capacity < 0, an lpad[s] < 1 or !(stride[s] > 0): FCN_E_BADARG; U or B > 2048 or U * S > 65536
 * (fcn_refine_train_plan_limits): FCN_E_LIMIT; nothing written. */
int fcn_refine_train_plan(const int32_t *seg_cnt, const int32_t *seg_pos, const double *pred_size, const double *stride,
                          const int32_t *lpad, int U, int S, int B, int64_t capacity, int32_t *slot_unit, int32_t *n_kept,
                          int64_t *seg_off, int64_t *off, int64_t *counts, int32_t *status, void *stream);
int fcn_refine_train_plan_limits(int *max_u, int *max_segs);

/* ---------------------------------------------------------------------------------------------
 * Two-stage inference with no host read between its launches (csrc/cascade_plan.h; INTEGRATION.md "Capturable two-stage inference"
 * states the contract bit for bit, tests/cascade_plan_ref.py restates it in numpy): candidates, count, plan, fill -- none of them
 * reads anything back, allocates or synchronises, so the sequence can be captured into a hipGraph.  Status bits (*status: one int32
 * on the device, OR-ed, never cleared here): bit 2 (4), bit 5 (32), bit 6 (64) as fcn_refine_train_plan sets them; bit 7 (128) more
 * first-stage kept rows than D; bit 8 (256) more surviving candidates than B; bit 9 (512) a first-stage group with cnt < 0 (the NMS
 * overflowed) or cnt > top_k.  (Bit 0 is fcn_draw_batch's; bit 1 is never set: fewer survivors than B is the normal case here.)
 *
 * fcn_cascade_candidates: keep (G, top_k) / cnt (G) int32 as fcn_rotate_nms_3d writes them -> the first D kept rows in the order
 * "groups ascending, keep order inside a group".  For kept row r of frustum u = r / L2: cand_row = r, cand_frame = unit_frame[u],
 * cand_class = unit_class[u], cand_group = unit_group[u] (unit_* (B1) int32), cand_score = dets[r * 8 + 7] (dets (R, 8) fp32);
 * *n_cand = the rows written, at most D.  Rows n_cand..D-1 get the filler: row -1, frame -1, class 0, group G, score 0 (a candidate
 * the count skips, of the spare group).  A group with cnt < 0 or cnt > top_k contributes nothing and sets bit 9; a keep entry
 * outside [0, R), or with r / L2 outside [0, B1), is skipped; none of them is dereferenced.  More kept rows than D: the rest are
 * dropped, bit 7.  One workgroup, an order-preserving prefix sum, no atomics on the data.  Every output is written on every call.
 * NULL pointers or G, top_k, L2, B1, R or D < 1: FCN_E_BADARG; G > 65536 or D > 2048: FCN_E_LIMIT; nothing written. */
int fcn_cascade_candidates(const int32_t *keep, const int32_t *cnt, int G, int top_k, int L2, const int32_t *unit_frame,
                           const int32_t *unit_class, const int32_t *unit_group, int B1, const float *dets, int R, int D,
                           int32_t *cand_row, int32_t *cand_frame, int32_t *cand_class, int32_t *cand_group, float *cand_score,
                           int32_t *n_cand, int32_t *status, void *stream);
/* fcn_refine_detect_count / _fill: the selection of fcn_refine_select_count / _fill -- the same closed fp64 box, the same
 * pred_corners / pred_angle / pred_size, the same stored rows bit for bit -- on a grid of (S, D) workgroups, workgroup (s, d)
 * scanning rows [s * seg, (s + 1) * seg) of candidate d's frame (seg = fcn_frustum_select_seg()), and without the read-back of
 * cand_row / cand_frame.  count writes seg_cnt (D, S) int32; fill takes seg_off (D*S+1) int64, the exclusive prefix sum over the
 * flattened counts (fcn_refine_detect_plan's), which bounds every store.  A candidate whose row is outside [0, R) or whose frame is
 * outside [0, F) is skipped silently: its counts are 0, nothing of it is dereferenced or written, the calls return 0.  "No frame is
 * longer than S * seg rows" is the caller's duty: rows beyond S segments would silently not be searched.
 * pt_stride < 3, D, F or R < 0, D > 65535, S < 1 or a NULL pointer: FCN_E_BADARG, nothing written.  D == 0: nothing to do; F == 0:
 * the counts are zeroed. */
int fcn_refine_detect_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                            const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, int S, int32_t *seg_cnt,
                            double *pred_corners, double *pred_angle, double *pred_size, void *stream);
int fcn_refine_detect_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const float *dets, int R,
                           const int32_t *cand_row, const int32_t *cand_frame, int D, double ratio, int S, const int64_t *seg_off,
                           float *out_pts, void *stream);
/* fcn_refine_detect_plan: fcn_refine_train_plan (its kernel) with seg_cnt as seg_pos -- the reference's lidar_point_threshold = 1: a
 * candidate without a selected row takes no slot -- and U = D.  Same width rules, slots, seg_off, off and STORED counts, same
 * refusals and limits.  Two status differences: fewer survivors than B sets nothing, more survivors than B (the rest are dropped)
 * sets bit 8. */
int fcn_refine_detect_plan(const int32_t *seg_cnt, const double *pred_size, const double *stride, const int32_t *lpad, int D, int S,
                           int B, int64_t capacity, int32_t *slot_unit, int32_t *n_kept, int64_t *seg_off, int64_t *off,
                           int64_t *counts, int32_t *status, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The inference front with no host read between its launches (csrc/frustum_detect_plan.h; INTEGRATION.md "Capturable inference
 * front" states the contract bit for bit, tests/frustum_detect_plan_ref.py restates it in numpy): count, plan, fill over a resident
 * table of at most D 2-D detections -- none of them reads anything back, allocates or synchronises, so the sequence can be captured
 * into a hipGraph.  Status bits of the plan (*status: one int32 on the device, OR-ed, never cleared here): bit 2 (4) rows dropped
 * because the total exceeds the capacity; bit 8 (256) more surviving boxes than B1; bit 10 (1024) *n_boxes outside [0, D] (taken as
 * 0 / D) or a box below *n_boxes whose frame is outside [0, F) (ignored, never dereferenced).  (Bit 0 is fcn_draw_batch's; fewer
 * survivors than B1 is the normal case here and sets nothing.)
 *
 * fcn_frustum_detect_count / _fill: the selection of fcn_frustum_select_count / _fill -- the same fp64 predicate, the same box2d and
 * frustum_angle, the same stored rows bit for bit, clip_boxes per launch -- without the read-back of box_frame and frame_off, and
 * behind n_boxes (1) int32 on the device: box d is skipped silently when d >= *n_boxes or its frame is outside [0, F) -- its counts
 * are 0, its rows of box2d / frustum_angle are NOT written, nothing of it is dereferenced or stored, the calls return 0.  "No frame
 * is longer than S * fcn_frustum_select_seg() rows" is the caller's duty: rows beyond S segments would silently not be searched.
 * Refusals as fcn_frustum_select_count / _fill, plus n_boxes == NULL: FCN_E_BADARG. */
int fcn_frustum_detect_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                             const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                             const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const int32_t *n_boxes,
                             double *box2d, double *frustum_angle, int32_t *seg_cnt, void *stream);
int fcn_frustum_detect_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *P,
                            const double *V2C, const double *R0, const double *img_wh, const double *boxes,
                            const int32_t *box_frame, int D, int S, int clip_boxes, double clip_distance, const int32_t *n_boxes,
                            const int64_t *seg_off, float *out_pts, void *stream);
/* fcn_frustum_detect_plan: what the host does between count and fill and in InputBuilder.build_device, as one workgroup.  seg_cnt
 * (D,S) int32 and box2d (D,4) fp64 from fcn_frustum_detect_count, box_frame (D), n_boxes (1).  With count_d = the sum of box d's
 * positive segment counts, box d survives iff d < min(*n_boxes, D), its frame lies in [0, F), none of ymax - ymin <
 * img_height_threshold, xmax - xmin < 1, (double)count_d < lidar_point_threshold holds (fp64 comparisons: a NaN difference does not
 * skip, as in numpy) and count_d > 0.  The first B1 survivors in box order take the slots: slot_box (B1) int32, D for an empty slot;
 * *n_kept.  seg_off (D*S+1) int64: the exclusive prefix sum of the slot-holding boxes' counts, every entry clamped to capacity (boxes
 * without a slot get empty slices: the fill stores nothing for them).  off (B1+1) int64: a filled slot's first row, capacity (the
 * spare row behind the buffer) for an empty one, off[B1] = the rows stored.  counts (B1) int64: the STORED rows per slot.  Box rows
 * at or beyond *n_boxes and rows of boxes with a frame out of range are never read.  Every output is written on every call.
 * NULL pointers, D < 0, S < 1, B1 < 1, capacity < 0, F < 0 or a NaN threshold: FCN_E_BADARG; D or B1 > 2048 or D * S > 65536
 * (fcn_frustum_detect_plan_limits): FCN_E_LIMIT; nothing written. */
int fcn_frustum_detect_plan(const int32_t *seg_cnt, const double *box2d, const int32_t *box_frame, const int32_t *n_boxes,
                            double img_height_threshold, double lidar_point_threshold, int D, int S, int B1, int64_t capacity, int F,
                            int32_t *slot_box, int32_t *n_kept, int64_t *seg_off, int64_t *off, int64_t *counts, int32_t *status,
                            void *stream);
int fcn_frustum_detect_plan_limits(int *max_d, int *max_segs);
/* fcn_frustum_fov_plan: the plan of the whole-image selection (one box (0, 0, W, H) per frame, box_frame = 0..F-1, clip_boxes = 0,
 * *n_boxes = F through fcn_frustum_detect_count / _fill): seg_cnt (F,S) -> seg_off (F*S+1) int64, the exclusive prefix sum of the
 * positive counts, and fov_off (F+1) int64, every S-th entry of it (the frames' offsets).  No reject rule, no slots, no status.
 * Entries are clamped to capacity; with capacity = the rows of the frame buffer nothing is ever cut, a subset of a frame being no
 * longer than the frame.  NULL pointers, F < 0, S < 1 or capacity < 0: FCN_E_BADARG; F * S > 65536: FCN_E_LIMIT. */
int fcn_frustum_fov_plan(const int32_t *seg_cnt, int F, int S, int64_t capacity, int64_t *seg_off, int64_t *fov_off, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SUN-RGBD inference with no host read between its launches (csrc/frustum_sunrgbd_detect_plan.h, csrc/det_eval.h; INTEGRATION.md
 * "Capturable SUN-RGBD inference" states the contract bit for bit, tests/sunrgbd_detect_plan_ref.py restates it in numpy): count,
 * plan, fill over a resident table of at most D 2-D detections, and the tail behind the NMS -- none of them reads anything back,
 * allocates or synchronises, so the sequence can be captured into a hipGraph.  Status bits (*status: one int32 on the device,
 * OR-ed, never cleared here): bit 2 (4) rows dropped because the total exceeds the capacity; bit 8 (256) more surviving boxes than
 * B; bit 10 (1024) *n_boxes outside [0, D] (taken as 0 / D) or a box below *n_boxes whose frame is outside [0, F) or whose class is
 * outside [0, C) (ignored, never dereferenced); bit 11 (2048) fcn_det_rows met a group whose cnt is -1.  (Bit 0 is the draws';
 * fewer survivors than B is the normal case here and sets nothing.)
 *
 * fcn_frustum_sunrgbd_detect_count / _fill: the selection of fcn_frustum_sunrgbd_count / _fill -- the same fp64 predicate, the same
 * frustum_angle, the same stored rows bit for bit -- without the read-back of box_frame and frame_off, and behind n_boxes (1) int32
 * on the device: box d is skipped silently when d >= *n_boxes or its frame is outside [0, F) -- its counts are 0, its entry of
 * frustum_angle is NOT written, nothing of it is dereferenced or stored, the calls return 0.  "No frame is longer than
 * S * fcn_frustum_select_seg() rows" is the caller's duty: rows beyond S segments would silently not be searched.
 * Refusals as fcn_frustum_sunrgbd_count / _fill, plus n_boxes == NULL: FCN_E_BADARG. */
int fcn_frustum_sunrgbd_detect_count(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                     const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                     const int32_t *n_boxes, double *frustum_angle, int32_t *seg_cnt, void *stream);
int fcn_frustum_sunrgbd_detect_fill(const float *frame_pts, const int64_t *frame_off, int F, int pt_stride, const double *K,
                                    const double *Rtilt, const double *boxes, const int32_t *box_frame, int D, int S,
                                    const int32_t *n_boxes, const int64_t *seg_off, float *out_pts, void *stream);
/* fcn_frustum_sunrgbd_detect_plan: what the host does between count and fill and in SunrgbdInputBuilder.build_device, as ONE
 * launch of one workgroup.  seg_cnt (D,S) int32 from fcn_frustum_sunrgbd_detect_count, box_frame (D), box_class (D), n_boxes (1).
 * With count_d = the sum of box d's positive segment counts, box d survives iff d < min(*n_boxes, D), its frame lies in [0, F), its
 * class in [0, C) and min(count_d, cap) >= max(1, point_threshold) -- build_device's rule on subsampled_counts.  The first B
 * survivors in box order take the slots: slot_box (B) int32, D for an empty slot; *n_kept.  seg_off (D*S+1) int64: the exclusive
 * prefix sum of the slot-holding boxes' counts, every entry clamped to capacity (boxes without a slot get empty slices: the fill
 * stores nothing for them).  off (B+1) int64: a filled slot's first row, capacity (the spare row behind the buffer) for an empty
 * one, off[B] = the rows stored.  counts (B) int64 and cnt32 (B) int32: the STORED rows per slot.  slot_group (B) int32:
 * frame * C + class of the slot's box, F * C (the spare group) for an empty slot.  The subsample table is laid out PER SLOT,
 * packed: sub_off (B+1) int64 is the exclusive prefix sum over the slots of (counts[i] > cap ? cap : 0) -- at most B * cap entries
 * -- so that (cnt32, sub_off, B) is what fcn_frustum_subsample_draw takes as (cnt_stored, sub_off, D); sub_start (B) int64 /
 * sub_len (B) int32 = sub_off[i] / cap where the slot stored more than cap rows, else 0 / 0: what fcn_draw_batch_sliced takes.
 * The subsample is decided on the STORED rows.  Table rows at or beyond *n_boxes are never read.  Every output is written on every
 * call.  NULL pointers, D < 0, S < 1, B < 1, capacity < 0, cap < 1, F < 0, C < 1 or F * C > 2^31 - 1: FCN_E_BADARG; D or B > 2048
 * or D * S > 65536 (fcn_frustum_detect_plan_limits): FCN_E_LIMIT; nothing written. */
int fcn_frustum_sunrgbd_detect_plan(const int32_t *seg_cnt, const int32_t *box_frame, const int32_t *box_class,
                                    const int32_t *n_boxes, int point_threshold, int cap, int D, int S, int B, int64_t capacity, int F,
                                    int C, int32_t *slot_box, int32_t *n_kept, int64_t *seg_off, int64_t *off, int64_t *counts,
                                    int32_t *cnt32, int64_t *sub_off, int64_t *sub_start, int32_t *sub_len, int32_t *slot_group,
                                    int32_t *status, void *stream);
/* fcn_det_rows: the tail behind fcn_rotate_nms_3d, one launch of one workgroup.  keep (G, top_k) int32, cnt (G) int32, dets
 * (num_dets, 8) fp32.  With c_g = clamp(cnt[g], 0, top_k): det_off (G+1) int32 the exclusive prefix sum of c_g; rows (G*top_k) int32
 * keep[g, 0..c_g) group after group, -1 behind det_off[G]; scores (G*top_k) fp32 = dets[row, 7], NaN where the row is -1 or outside
 * [0, num_dets) -- such a row is never dereferenced; *n_rows = det_off[G].  A group with cnt == -1 (more than 4096 candidates) sets
 * bit 11 (2048) of *status and contributes no row.  Order-preserving scans, no atomics on the data.  fcn_box3d_corners(dets,
 * num_dets, rows, G * top_k, ...) follows as it is.  NULL pointers (dets with num_dets > 0), G < 1, top_k < 1 or num_dets < 0:
 * FCN_E_BADARG; G > 65536, top_k > 4096 or G * top_k > 2^31 - 1: FCN_E_LIMIT; nothing written. */
int fcn_det_rows(const int32_t *keep, const int32_t *cnt, int G, int top_k, const float *dets, int num_dets, int32_t *det_off,
                 int32_t *rows, float *scores, int32_t *n_rows, int32_t *status, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* FCN_HIP_H */
