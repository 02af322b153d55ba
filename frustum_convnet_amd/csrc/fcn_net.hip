// ConvFeatNet + heads (models/det_base.py:163-224,250-251,365-368) as hand-written HIP: every Conv1d /
// ConvTranspose1d (+ BatchNorm1d + ReLU) is one implicit-GEMM launch over position-major (NLC) activations, forward and
// backward, on the 16-bit matrix cores with split fp32 operands (gemm_tile.h: fp16x3 forward, bf16x3 backward, fp32
// accumulate; exact fp32 MFMA and single-term bf16 are the other two operand modes).
//
// The reference runs this part through cuDNN/ATen on (B,C,L) tensors: 13 convs + 13 BN + ReLUs + cats, each its
// own kernel(s); on MI355X the MIOpen path spends most of its time in layout transposes and tiny elementwise
// kernels (profiles/r01_b: 1.9 ms of a 4 ms step).  Here:
//   * activations are rows of C floats (row = (frustum, position)), so a k=3 / stride-2 conv is a GEMM whose A rows
//     are gathered from up to three shifted source rows, a k=1 "merge" conv is a GEMM over concatenated sources
//     (torch.cat never materialises), and ConvTranspose1d with kernel == stride is a plain GEMM with N = k*Cout
//     whose output buffer IS the upsampled NLC tensor;
//   * the producer's BatchNorm + ReLU is applied while the A tile is staged (the conv consumes pre-BN outputs),
//     BN batch statistics are accumulated in the GEMM epilogue;
//   * the one-hot class vector (3 extra input channels broadcast over L) is a virtual 64-channel segment;
//   * backward: dgrad kernels gather dy rows through the inverse position map and write dz of the producer (ReLU
//     mask + BN-backward sums in the epilogue), wgrad kernels reduce over rows in splits + a deterministic reduce
//     that scatters straight into the torch weight layout.
#define FCN_TUNING_FCN
#include "gemm_tile.h"

#define CG_T 256
// replicas of the FCN's BatchNorm sum slots (fcn_common.h: same-address fp64 atomics are served one at a time).  Every
// consumer workgroup of this latency-bound chain sums them in its prologue, so fewer than the PointNet kernels' 8.
#ifndef FCN_CG_REP
#define FCN_CG_REP 4
#endif
__device__ __forceinline__ double cg_rep_sum(const double *p, int stride)
{
    double v = p[0];
#pragma unroll
    for (int r = 1; r < FCN_CG_REP; ++r) v += p[(int64_t)r * stride];
    return v;
}
// forward tile of the K-group kernels: (32*FCN_FT_MW) x (32*FCN_FT_WNC) outputs, FCN_FT_G K-groups (tuning builds override)
#ifndef FCN_FT_MW
#define FCN_FT_MW 1
#endif
#ifndef FCN_FT_G
#define FCN_FT_G 4
#endif
#ifndef FCN_FT_WNC
#define FCN_FT_WNC 1
#endif
#ifndef FCN_FT_NTW
#define FCN_FT_NTW 1           // 32-column blocks per wave (a layer whose width is no multiple of the tile falls back to 1)
#endif
#define FCN_FT_THREADS (FCN_FT_G * 64 * FCN_FT_MW * FCN_FT_WNC)
// FCN_FWD_DIRECT (round 6): the one-wave K-groups of the 32 x 32 forward tile take their MFMA operands STRAIGHT FROM GLOBAL MEMORY in
// fragment shape -- a lane (row l & 31, half l >> 5) loads the 8 reduction-adjacent values of ITS row that the 32x32x16 instruction
// wants from it (two 16-byte loads), applies the producer's BatchNorm + ReLU + split in registers and issues the MFMAs; the weight
// image is pre-encoded in fragment order, so its fragments are plain 16-byte loads as well.  No wave shares an operand with another
// (every K-group reduces its own chunks), so the LDS images of the staged form were a pure transposer: 8 ds_write + 8 ds_read_b128
// + two LDS round trips per 6 MFMAs on the critical path of a wave that has ~2 siblings per SIMD to hide them behind.
#ifndef FCN_FWD_DIRECT
#define FCN_FWD_DIRECT 0
#endif
// FCN_FWD_EARLY_BN: the batch sums of the layer's FIRST input segment (its main producer) are requested at kernel entry -- two
// channels per thread, all replicas -- and consumed by cg_fill_bn, so that their round trip runs beside the row divisions, the
// chunk table and the first operand loads instead of behind them (the ablation of EXPERIMENTS 6.2: the consumer-side BatchNorm
// finalisation is 2.7 us of every forward launch).  One channel per thread: a second slot (C = 512) or a second segment costs 36 more
// live VGPRs in front of the K loop -- 158 + scratch, two waves per SIMD, 512 slots for 560 tiles.  Same sums in the same replica
// order: bit-identical outputs.  Measured (session u, four alternating pairs on one box): 1.1057 against 1.1123 ms per step (-0.6 %),
// cgk_fwd_kernel 18.0 against 18.3 us, the probe's prologue phase -0.3 ... -0.6 us on every layer with a BatchNorm in front.
#ifndef FCN_FWD_EARLY_BN
#define FCN_FWD_EARLY_BN 1
#endif
#ifndef FCN_FWD_DEPTH
#define FCN_FWD_DEPTH 2        // chunks in flight per K-group of the direct form (2 or 3 register sets)
#endif
#define LDN 68                 // row-major LDS leading dim of a 64-wide tile (float4 aligned)
#define OH_PAD 64              // channels of the virtual one-hot segment
#define CG_SPLIT_ROWS 512      // rows per wgrad split
#define CN_NLAYER 18           // capacity: 4 * levels - 2 layers (4 levels: 13 conv/deconv+BN + heads = 14; 5 levels: 18)
#define CG_NSEG 4              // input segments of a layer (the 5-level heads read four deconvolution outputs)

struct CgSeg {
    const float *x;            // type 0: (B*Lsrc, C) rows; type 1: one-hot zero-padded to (B, OH_PAD)
    float *bn;                 // scale[C], shift[C], mean[C], rstd[C] of the producer's BN, or nullptr (already activated)
    int C;                     // channels seen by the GEMM (type 1: OH_PAD)
    int Lsrc;                  // rows per frustum in the source buffer (type 1: 1 row per frustum, every position reads it)
    int type, nvec;
    int st16;                  // x is one of the y arenas: stored as bf16 in the bf16 throughput mode (gemm_tile.h: St)
    // The producer's BN is FINALISED BY ITS CONSUMERS: every forward workgroup derives scale/shift from the batch sums
    // in its prologue (a few hundred fp64 operations) instead of waiting for a separate one-workgroup launch between
    // every two layers of a latency-bound chain.  Workgroup (0,0) of the consumer flagged `writer` also publishes
    // bn[] (the backward reads it) and updates the running statistics.
    const double *stat;        // training: sum[C], sumsq[C] over M positions (final); eval: nullptr -> running stats
    const float *gamma, *beta;
    float *rmean, *rvar;
    int64_t *nbt;
    double M;
    int writer;
};

struct CgLayer {
    CgSeg seg[CG_NSEG];
    int nseg;
    int KT, stride, pad;
    int Lin, Lout, B;          // valid input positions, output positions per frustum
    int Cout, Ktot, Cs;        // GEMM N, GEMM K = KT * sum(C), BN channels (col % Cs)
    const float *Wp;           // packed (Cout, Ktot)
    const u32x4 *Wenc;         // its forward image, split-encoded in MFMA operand order: [Ktot/32][plane][4][Cout] (cg_pack_kernel)
    const u32x4 *Wgrd;         // its data-gradient image (reduction over the OUTPUT index n): [Cout/8][plane][Ktot] u32x4, element
                               // (n8, plane, kk) = the packed hi / lo parts of Wp[8*n8 .. 8*n8+7][kk] in the backward operand mode
    const float *bias;         // (nbias) or nullptr
    int nbias;
    float *y;                  // (B*Lout, Cout) pre-BN output
    int y16;                   // y is stored as bf16 (bf16 throughput mode, every layer but the heads' fp32 logits)
    double *stat;              // sum[Cs], sumsq[Cs] (replica 0) or nullptr
    float eps, momentum;
    int rep_stride;            // doubles between the replica blocks of every stat pointer of this layer (the whole arena)
    int32_t *flags;            // sticky numeric flags (fcn_cn_ws.flags) or nullptr
};

#define SEL3(i, a0, a1, a2) ((i) == 0 ? (a0) : ((i) == 1 ? (a1) : (a2)))
#define SEL4(i, a0, a1, a2, a3) ((i) == 0 ? (a0) : ((i) == 1 ? (a1) : ((i) == 2 ? (a2) : (a3))))


// n / d and n % d for 0 <= n < 2^23 through a float reciprocal and one correction step (~10 instructions): hipcc's general
// 32-bit division is ~40 and every workgroup of a 25-launch latency-bound chain paid a dozen of them before its first load.
__device__ __forceinline__ void cg_divmod(int n, int d, float inv, int &q, int &r)
{
    q = (int)((float)n * inv);
    r = n - q * d;
    if (r < 0) { q -= 1; r += d; }
    else if (r >= d) { q += 1; r -= d; }
}
// (v_rcp_f32, 1 ulp: cg_divmod's correction step absorbs it -- the IEEE division was ~10 instructions in every prologue)
__device__ __forceinline__ float cg_inv(int d) { return __builtin_amdgcn_rcpf((float)d); }

// XCD-aware tile order (cdna guide T1).  Workgroup ids are dealt to the 8 XCDs round-robin and every XCD has its own 4 MB
// L2; with the natural order the tiles that share operand rows land on eight different L2s and each of them pulls the
// whole weight matrix AND the whole activation matrix through the fabric (32 x 32 tiles re-read their operands ~20x:
// block4_conv2 moved 215 MB through L2 for 10 MB of distinct data).  Here workgroup `id` of a role takes tile
// (id % 8) * ceil(n / 8) + id / 8, so XCD k works through the CONTIGUOUS range of tiles k*per .. (k+1)*per-1 in order:
// a range of row tiles x all column tiles -> its L2 sees 1/8 of the rows and the weights once.  Roles inside one launch
// start at multiples of 8 workgroups (cg_pad8) so that id % 8 is the XCD for each of them.  Speed only: nothing depends on
// the placement.
__device__ __forceinline__ int cg_xcd_tile(int id, int n)
{
    const int per = (n + 7) >> 3;
    const int t = (id & 7) * per + (id >> 3);
    return (t < n && (id >> 3) < per) ? t : -1;
}
static inline int cg_pad8(int n) { return ((n + 7) / 8) * 8; }

// Pins a wave-uniform value in an SGPR.  Without it LLVM rewrites "select between fields of the by-value kernel
// struct" into "load from a dynamically selected field address", which needs the struct in memory: the whole kernarg
// struct gets memcpy'd to scratch and every later field access becomes a scratch load.
template <class T>
__device__ __forceinline__ T opaque_s(T v)
{
    asm volatile("" : "+s"(v));
    return v;
}
// Several values read THROUGH A POINTER pinned at once: every asm volatile is a scheduling barrier, so a row of opaque_s() calls on
// pointer loads becomes load, wait, load, wait, ... -- one scalar-cache round trip per field.  Plain loads into locals first (the
// compiler issues them back to back), then ONE asm that takes them all.
#define CG_PIN_1(a) "+s"(a)
#define CG_PIN_2(a, ...) "+s"(a), CG_PIN_1(__VA_ARGS__)
#define CG_PIN_3(a, ...) "+s"(a), CG_PIN_2(__VA_ARGS__)
#define CG_PIN_4(a, ...) "+s"(a), CG_PIN_3(__VA_ARGS__)
#define CG_PIN_5(a, ...) "+s"(a), CG_PIN_4(__VA_ARGS__)
#define CG_PIN_6(a, ...) "+s"(a), CG_PIN_5(__VA_ARGS__)
#define CG_PIN_7(a, ...) "+s"(a), CG_PIN_6(__VA_ARGS__)
#define CG_PIN_8(a, ...) "+s"(a), CG_PIN_7(__VA_ARGS__)
#define CG_PIN_9(a, ...) "+s"(a), CG_PIN_8(__VA_ARGS__)
#define CG_PIN_10(a, ...) "+s"(a), CG_PIN_9(__VA_ARGS__)
#define CG_PIN_11(a, ...) "+s"(a), CG_PIN_10(__VA_ARGS__)
#define CG_PIN_12(a, ...) "+s"(a), CG_PIN_11(__VA_ARGS__)
#define CG_PIN_13(a, ...) "+s"(a), CG_PIN_12(__VA_ARGS__)
#define CG_PIN_14(a, ...) "+s"(a), CG_PIN_13(__VA_ARGS__)
#define CG_PIN_15(a, ...) "+s"(a), CG_PIN_14(__VA_ARGS__)
#define CG_PIN_16(a, ...) "+s"(a), CG_PIN_15(__VA_ARGS__)
#define CG_PIN_17(a, ...) "+s"(a), CG_PIN_16(__VA_ARGS__)
#define CG_PIN_18(a, ...) "+s"(a), CG_PIN_17(__VA_ARGS__)
#define CG_PIN(N, ...) asm volatile("" : CG_PIN_##N(__VA_ARGS__))

// (segment, tap, channel) of packed column kk from fields the caller holds in SGPRs.  Only STATIC selects: a dynamically indexed
// by-value kernel struct is copied to scratch and every access becomes a scratch / vector load in the middle of the prefetch.
struct CgGeo {
    int nseg, KT, stride, pad, Lin;
};
__device__ __forceinline__ void cg_locate_s(const CgGeo &G, int C0, int C1, int C2, int C3, int kk, int &sg, int &tap, int &k0,
                                            int &segoff)
{
    sg = 0; segoff = 0;
#pragma unroll
    for (int s = 0; s < CG_NSEG; ++s) {
        if (s < G.nseg) {
            const int span = G.KT * SEL4(s, C0, C1, C2, C3);
            if (sg == s && kk >= span) { kk -= span; segoff += span; sg = s + 1; }
        }
    }
    const int C = SEL4(sg, C0, C1, C2, C3);
    cg_divmod(kk, C, cg_inv(C), tap, k0);               // kk < CG_KMAX
}

// RAW, UNCONDITIONAL load of A[r][kc..kc+3] of the virtual im2col matrix: the position is clamped to a valid row and
// `ok` says whether the value counts.  No branch and no arithmetic on the loaded value here -- the producer's BN +
// ReLU and the ok-mask are applied when the registers go to LDS one iteration later -- so the load stays in flight
// across the MFMA phase (a "load or zero" select makes hipcc wait for the load right away).
// A one-hot segment is a (B, OH_PAD) buffer: one row per frustum (Lsrc = 1), every position reads it (linmul = 0).
template <int MM>
__device__ __forceinline__ v4f cg_load_raw(const CgGeo &L, const float *x, int C, int Lsrc, int linmul, int tap,
                                           int kc, int b, int l, bool rvalid, bool &ok, int s16 = 0)
{
    const int lin = (int)fcn_mad24((unsigned)l, (unsigned)L.stride, (unsigned)(tap - L.pad));     // (l >= 0; wraps like the int form)
    ok = rvalid && lin >= 0 && lin < L.Lin;
    // linmul is wave-uniform: the upper clamp is a scalar, and pinned as one (hipcc otherwise turns it back into a per-lane select)
    const int lc = min(max(lin, 0), fcn_opaque_sgpr((L.Lin - 1) * linmul));
    if constexpr (St<MM>::half) {
        // a layer output (bf16 arena); pooled features / one-hot stay fp32
        if (s16) return lds4e<MM>(x, (unsigned)((b * Lsrc + lc) * C + kc));
    }
    // 32-bit BYTE offset off the wave-uniform base (cn_make_plan checks B * L * C < 2^30 for every arena) -- the SGPR-base +
    // VGPR-offset form of global_load -- from two full-rate 24-bit multiply-adds (rows < 2^23, C < 2^22): the 64-bit
    // multiply-adds and the 64-bit shift-add hipcc emits for the element-index form were 6 quarter-rate-class instructions per load
    const unsigned eb = fcn_mad24(fcn_mad24((unsigned)b, (unsigned)Lsrc, (unsigned)lc), (unsigned)(4 * C), (unsigned)(4 * kc));
    return *(gv4fp)((const char *)x + eb);
}

// 1 / sqrt(x) in fp64 from the fp32 rsqrt + three Newton steps (full double accuracy, x > 0 and within float range -- a
// variance + eps): a dozen fp64 operations instead of the software sqrt + division sequences (~100) every workgroup of every
// layer ran in its prologue
__device__ __forceinline__ double cg_rsqrt64(double x)
{
    double y = (double)rsqrtf((float)x);
#pragma unroll
    for (int i = 0; i < 3; ++i) y = y * (1.5 - 0.5 * x * y * y);
    return y;
}

#define CG_KMAX 1792           // largest Ktot staged as per-column BN scale/shift (block4_conv2: 3*512 = 1536)

// per-column (kk) scale/shift of the virtual A matrix: BN of the producer, or (1,0) for inputs that are already
// activations (pooled features, one-hot: both >= 0, so the ReLU applied uniformly is the identity on them)
// The layer descriptor read THROUGH THE KERNARG POINTER from a given program point on: fields read through the by-value kernel
// parameter are all fetched in the kernel's entry block (the compiler hoists kernel-argument loads there), in as many serialized
// batches as the SGPR budget forces -- each batch a scalar-cache round trip plus v_writelane spills -- in front of the first global
// load of every workgroup, although the BatchNorm fold and the epilogue need theirs much later.  The asm makes the pointer opaque:
// loads through it cannot move above it, so they are issued behind the operand loads already in flight.
typedef __attribute__((address_space(4))) const CgLayer *cg_klayer_p;
__device__ __forceinline__ cg_klayer_p cg_kernarg_layer(int koff)
{
    typedef __attribute__((address_space(4))) const char *kchar_p;
    cg_klayer_p p = (cg_klayer_p)((kchar_p)__builtin_amdgcn_kernarg_segment_ptr() + koff);
    asm volatile("" : "+s"(p) : : "memory");
    return p;
}

// first-slot sums of segment 0 requested at kernel entry (FCN_FWD_EARLY_BN): channel tid, every replica
struct CgBnEarly {
    double s1[1][FCN_CG_REP], s2[1][FCN_CG_REP];
    float g[1], b[1];
    bool on;                   // (wave-uniform) the values above are segment 0's batch sums / gamma / beta
};
template <class LP>            // LP: const CgLayer * (by-value parameter) or cg_klayer_p
__device__ __forceinline__ void cg_fill_bn(LP Lp, float *sS, float *tS, int tid, int nthr, bool pub, const CgBnEarly *early = nullptr)
{
    const auto &L = *Lp;
    int off = 0;
#pragma unroll
    for (int s = 0; s < CG_NSEG; ++s) {
        if (s < L.nseg) {
            const auto &S = L.seg[s];
            const int C = S.C, span = L.KT * C;
            if (S.gamma) {
                const bool batch = S.stat != nullptr;
                const bool wr = pub && S.writer;
                const double invM = 1.0 / S.M;
                const bool pre = s == 0 && early && early->on && batch;
                for (int k = tid; k < C; k += nthr) {
                    double mean, var;
                    float gk, bk;
                    const int slot = (k - tid) / nthr;                 // (0, 1, ...: which of this thread's channels)
                    if (pre && slot < 1) {
                        double a1 = early->s1[0][0], a2 = early->s2[0][0];
#pragma unroll
                        for (int r = 1; r < FCN_CG_REP; ++r) { a1 += early->s1[0][r]; a2 += early->s2[0][r]; }
                        mean = a1 * invM;
                        var = a2 * invM - mean * mean;
                        if (var < 0.0) var = 0.0;
                        gk = early->g[0]; bk = early->b[0];
                    } else {
                        if (batch) {
                            mean = cg_rep_sum(S.stat + k, L.rep_stride) * invM;
                            var = cg_rep_sum(S.stat + C + k, L.rep_stride) * invM - mean * mean;
                            if (var < 0.0) var = 0.0;
                        } else {
                            mean = S.rmean[k];
                            var = S.rvar[k];
                        }
                        gk = S.gamma[k]; bk = S.beta[k];
                    }
                    const double rstd = cg_rsqrt64(var + (double)L.eps);
                    const double sc = (double)gk * rstd;
                    const float fs = (float)sc, ft = (float)((double)bk - mean * sc);
                    for (int t = 0; t < L.KT; ++t) { sS[off + t * C + k] = fs; tS[off + t * C + k] = ft; }
                    if (wr) {
                        S.bn[k] = fs; S.bn[C + k] = ft; S.bn[2 * C + k] = (float)mean; S.bn[3 * C + k] = (float)rstd;
                        if (batch) {
                            S.rmean[k] = (float)((1.0 - L.momentum) * S.rmean[k] + L.momentum * mean);
                            S.rvar[k] = (float)((1.0 - L.momentum) * S.rvar[k] + L.momentum * var * (S.M / (S.M - 1.0)));
                            if (k == 0) S.nbt[0] += 1;
                        }
                    }
                }
            } else {
                for (int i = tid; i < span; i += nthr) { sS[off + i] = 1.f; tS[off + i] = 0.f; }
            }
            off += span;
        }
    }
}

// the bits of ONE ELEMENT of a packed operand vector as a float.  Through a by-value parameter on purpose: __builtin_bit_cast applied
// to a vector-element expression (v[q]) reads the bytes at the START of the vector -- element 0 for every q (clang of ROCm 7.2, host
// and device alike; found by the host emulation of the fp32 operand mode)
__device__ __forceinline__ float cg_u2f(uint32_t u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ float cg_act(float s, float x, float t, bool ok) { return ok ? fmaxf(fmaf(s, x, t), 0.f) : 0.f; }
// the same with the row's mask as fcn_keep(ok): one v_fma_f32 + one v_med3_f32 per element
__device__ __forceinline__ float cg_actk(float s, float x, float t, float keep) { return fcn_relu_keep(fmaf(s, x, t), keep); }

// ------------------------------------------------------------------------------------------------
// K-group kernels: one workgroup of G groups of MW x WNC waves owns one (32*MW) x (32*WNC) output tile; group g reduces
// the K chunks g, g+G, ... through its own LDS buffers, the group accumulators are summed through LDS and ONE pass runs
// the whole epilogue (bias, store, BN statistics).  These GEMMs are small (B*L rows): split-K INSIDE the workgroup
// gives 4-16 resident waves per tile to hide the gather / staging latency, and nothing but the result goes back to HBM.
// In use: <1,4,1> (32 x 32 tile, 4 waves) -- 560 workgroups per layer; <1,4> (32 x 64) and <2,4> (64 x 64) measured
// 5 % slower over the forward (280 tiles for 256 CUs at every level of the pyramid).
template <int MM, int MW, int G, int WNC = 2, int NTW = 1, int EB = FCN_FWD_EARLY_BN>      // WNC waves across N per K-group, NTW 32-column blocks per wave; EB: early batch sums (training launches)
__device__ __forceinline__ void cgk_fwd_body(const CgLayer &L, const int bx, const int by, const int koff)      // tile (32*MW) x (32*WNC*NTW); koff: offset of L in the kernarg segment
{
    constexpr int TG = 64 * MW * WNC, TMB = 32 * MW, TNC = 32 * WNC * NTW, NTHR = G * TG;
    constexpr int LDRA = KbTile<TMB>::LDR, LDRB = KbTile<TNC>::LDR, GU4 = KbTile<TMB>::U4 + KbTile<TNC>::U4;
    constexpr int NA = TMB * 8 / TG;          // 4-vectors of A per thread per chunk
    constexpr int NB = TNC * 8 / TG;          // u32x4 of the encoded weight per thread per chunk
    static_assert(G * GU4 * 4 >= G * TMB * TNC, "the cross-group sum fits the operand images");
    static_assert(2 * TNC <= NTHR && (TMB * 8) % TG == 0 && (TNC * 8) % TG == 0, "epilogue / staging lane mapping");
    constexpr bool DIRECT = FCN_FWD_DIRECT && TG == 64 && NTW == 1;       // (operands straight into fragments: FCN_FWD_DIRECT above)
    __shared__ u32x4 lds4[DIRECT ? G * TMB * TNC / 4 : G * GU4];   // per K-group: kb-major images of its A and W chunk (gemm_tile.h); DIRECT: only the cross-group sum
    __shared__ __attribute__((aligned(16))) float sS[CG_KMAX], tS[CG_KMAX];
    __shared__ int cSeg[CG_KMAX / KC], cTap[CG_KMAX / KC], cK0[CG_KMAX / KC];   // chunk -> (segment, tap, channel)
    __shared__ __attribute__((aligned(16))) int cDesc[DIRECT ? 8 * (CG_KMAX / KC) : 4];      // DIRECT: chunk descriptors
    float *lds = (float *)lds4;
    if (FCN_XF & 128) return;                           // (timing builds: the bare launch -- dispatch + kernel boundary)
    const int tid = threadIdx.x, g = tid / TG, gt = tid % TG;
    const int lane = tid & 63, gw = gt >> 6, l31 = lane & 31, lh = lane >> 5;
    const int wm = gw / WNC, wn = gw % WNC;
    u32x4 *Ab = lds4 + g * GU4, *Bb = Ab + KbTile<TMB>::U4;
    PROBE_DECL;
    PROBE_STAMP();                                      // 0: entry
    // EVERY kernel-argument field the code in front of the first loads reads, fetched as ONE batch of scalar loads and pinned:
    // left to the compiler they are re-fetched from the kernarg segment at each use, one s_load + s_waitcnt round trip after the
    // other (15 of them between here and the first global load, ~1 us of the 2.5 us every workgroup of every layer spent there)
    const int LB = opaque_s(L.B), LLout = opaque_s(L.Lout), LKtot = opaque_s(L.Ktot), LCout = opaque_s(L.Cout);
    CgGeo geo;
    geo.nseg = opaque_s(L.nseg); geo.KT = opaque_s(L.KT); geo.stride = opaque_s(L.stride); geo.pad = opaque_s(L.pad);
    geo.Lin = opaque_s(L.Lin);
    const u32x4 *LWenc = opaque_s(L.Wenc);
    CgBnEarly early;
    early.on = false;
    if constexpr (EB != 0) {
        const double *st0 = opaque_s(L.seg[0].stat);
        const float *gm0 = opaque_s(L.seg[0].gamma), *bt0 = opaque_s(L.seg[0].beta);
        const int rs0 = opaque_s(L.rep_stride), Ce = opaque_s(L.seg[0].C);
        early.on = st0 != nullptr && gm0 != nullptr;
        if (early.on) {
#pragma unroll
            for (int i = 0; i < 1; ++i) {
                const int k = min(tid + i * NTHR, Ce - 1);              // (clamped: unconditional loads)
#pragma unroll
                for (int r = 0; r < FCN_CG_REP; ++r) {
                    early.s1[i][r] = st0[(int64_t)r * rs0 + k];
                    early.s2[i][r] = st0[(int64_t)r * rs0 + Ce + k];
                }
                early.g[i] = gm0[k];
                early.b[i] = bt0[k];
            }
        }
    }
    const int R = LB * LLout;
    const int row0 = bx * TMB, n0 = by * TNC;
    const int kq = gt & 7, rb = gt >> 3;      // rb: 0..31 (MW=2) or 0..15 (MW=1)
    constexpr int RSTEP = TG / 8;
    const int nchunk = LKtot / KC, nit = (nchunk + G - 1) / G;
    // segment fields as scalars (static indices)
    const float *x0 = opaque_s(L.seg[0].x), *x1 = opaque_s(L.seg[1].x), *x2 = opaque_s(L.seg[2].x), *x3 = opaque_s(L.seg[3].x);
    const int C0 = opaque_s(L.seg[0].C), C1 = opaque_s(L.seg[1].C), C2 = opaque_s(L.seg[2].C), C3 = opaque_s(L.seg[3].C);
    const int T0 = opaque_s(L.seg[0].type), T1 = opaque_s(L.seg[1].type), T2 = opaque_s(L.seg[2].type), T3 = opaque_s(L.seg[3].type);
    const int Q0 = opaque_s(L.seg[0].Lsrc), Q1 = opaque_s(L.seg[1].Lsrc), Q2 = opaque_s(L.seg[2].Lsrc), Q3 = opaque_s(L.seg[3].Lsrc);
    const int H0 = opaque_s(L.seg[0].st16), H1 = opaque_s(L.seg[1].st16), H2 = opaque_s(L.seg[2].st16), H3 = opaque_s(L.seg[3].st16);
#if defined(FCN_PROBE) && FCN_PROBE == 2      // (finer stamps of the issue phase: the kernel arguments have arrived ...)
    if (H0 + H1 + H2 + H3 + C0 + Q0 + T0 == -12345) return;
    PROBE_STAMP();
#endif
    f32x16 acc[1][NTW];
    acc_zero<1, NTW>(acc);
    if constexpr (DIRECT) {
        // ---- operands in fragment shape: this lane's row of the tile, its 8-deep half of every 16-deep MFMA step
        const int gr = row0 + l31;
        const bool rv1 = gr < R;
        int bb1 = 0, ll1 = 0;
        cg_divmod(rv1 ? gr : 0, LLout, cg_inv(LLout), bb1, ll1);             // (R < 2^23: cn_make_plan)
        const int lin0 = rv1 ? (int)fcn_mad24((unsigned)ll1, (unsigned)geo.stride, (unsigned)(-geo.pad)) : -(1 << 30);
        const unsigned laneoff = 32u * (unsigned)lh;                          // bytes: this lane's 8-deep half of a 16-deep step
        constexpr bool X3 = !mm_x1<MM>;
        constexpr int NW = X3 || MM == MM_F32 ? 4 : 2;                       // weight fragments per chunk: (step, plane)
        // fragment (s, plane) of the weight image of a chunk: u32x4 ((plane * 4 + 2 s + lh) * Cout + n0 + l31)
        unsigned wofd[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) wofd[q] = (unsigned)((((q & 1) * 4 + 2 * (q >> 1) + lh) * LCout + l31)) * 16u;
        const char *wsrc = (const char *)(LWenc + n0);
        constexpr int DEPTH = FCN_FWD_DEPTH;
        static_assert(DEPTH == 2 || DEPTH == 3, "two or three chunks in flight");
        v4f da0[4], da1[4], da2[4];           // [2 * step + piece]: k = 16 step + 8 lh + 4 piece .. + 3 of the chunk
        u32x4 dw0[4], dw1[4], dw2[4];         // [2 * step + plane]
        bool dk0 = false, dk1 = false, dk2 = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            da0[i] = zero4(); da1[i] = zero4(); da2[i] = zero4();
            dw0[i] = u32x4{0u, 0u, 0u, 0u}; dw1[i] = u32x4{0u, 0u, 0u, 0u}; dw2[i] = u32x4{0u, 0u, 0u, 0u};
        }
        // a chunk's scalars: source base, 4 * channels, rows per frustum, tap, 4 * first channel, position clamp, bf16 flag -- from the
        // descriptor table the prologue builds in LDS (two 16-byte broadcast reads + readfirstlane) instead of five 4-way scalar
        // select chains per chunk
#define CGD_FWD_LOAD_CORE(cc, X, C4, LS, TAP, K04, LHI, H16, RA, RW, OK)                                              \
    {                                                                                                                 \
        const int c_ = (cc);                                                                                          \
        if constexpr (St<MM>::half) {                                                                                 \
            _Pragma("unroll") for (int i = 0; i < 4; ++i)                                                             \
                RA[i] = cg_load_raw<MM>(geo, (X), (C4) >> 2, (LS), (LHI) ? 1 : (geo.Lin == 1 ? 1 : 0), (TAP),         \
                                        ((K04) >> 2) + 16 * (i >> 1) + 8 * lh + 4 * (i & 1), bb1, ll1, rv1, OK, (H16)); \
        } else {                                                                                                      \
            /* ONE address per chunk: the row of tap TAP (lin0 = position of tap 0, hoisted; an invalid row sits at */  \
            /* -2^30, outside every range), clamped; the four 16-byte pieces of the lane's two 8-deep halves are */     \
            /* constant byte offsets (0, 16, 64, 80) off it */                                                        \
            const int lin = lin0 + (TAP);                                                                             \
            OK = (unsigned)lin < (unsigned)geo.Lin;                                                                   \
            const int lc = min(max(lin, 0), fcn_opaque_sgpr(LHI));                                                    \
            const unsigned eb = fcn_mad24(fcn_mad24((unsigned)bb1, (unsigned)(LS), (unsigned)lc), (unsigned)(C4),     \
                                          laneoff + (unsigned)(K04));                                                 \
            const char *xb_ = (const char *)(X) + eb;                                                                 \
            RA[0] = *(gv4fp)(xb_); RA[1] = *(gv4fp)(xb_ + 16); RA[2] = *(gv4fp)(xb_ + 64); RA[3] = *(gv4fp)(xb_ + 80); \
        }                                                                                                             \
        const char *wc_ = wsrc + (size_t)(unsigned)(c_ * 8 * LCout) * 16u;                                            \
        _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                                 \
            if (NW == 4 || !(q & 1)) RW[q] = *(gu4p)(wc_ + wofd[q]);                                                  \
    }
#define CGD_FWD_LOAD_AT(cc, SG, TAP, K0, RA, RW, OK)                                                                  \
    {                                                                                                                 \
        const int sgi = (SG);                                                                                         \
        const float *x = SEL4(sgi, x0, x1, x2, x3);                                                                   \
        const int C = SEL4(sgi, C0, C1, C2, C3), ty = SEL4(sgi, T0, T1, T2, T3), Ls = SEL4(sgi, Q0, Q1, Q2, Q3);      \
        const int h16 = SEL4(sgi, H0, H1, H2, H3);                                                                    \
        CGD_FWD_LOAD_CORE(cc, x, 4 * C, Ls, (TAP), 4 * (K0), (geo.Lin - 1) * (ty ? 0 : 1), h16, RA, RW, OK);          \
    }
#define CGD_FWD_LOAD(cc, RA, RW, OK)                                                                                  \
    {                                                                                                                 \
        const int c__ = __builtin_amdgcn_readfirstlane(cc);                                                           \
        const v4i q0_ = *(const v4i *)(cDesc + 8 * c__), q1_ = *(const v4i *)(cDesc + 8 * c__ + 4);                   \
        const unsigned xlo_ = (unsigned)__builtin_amdgcn_readfirstlane(q0_.x), xhi_ = (unsigned)__builtin_amdgcn_readfirstlane(q0_.y); \
        const float *x_ = (const float *)(((unsigned long long)xhi_ << 32) | (unsigned long long)xlo_);               \
        CGD_FWD_LOAD_CORE(c__, x_, __builtin_amdgcn_readfirstlane(q0_.z), __builtin_amdgcn_readfirstlane(q0_.w),      \
                          __builtin_amdgcn_readfirstlane(q1_.x), __builtin_amdgcn_readfirstlane(q1_.y),               \
                          __builtin_amdgcn_readfirstlane(q1_.z), __builtin_amdgcn_readfirstlane(q1_.w), RA, RW, OK);  \
    }
        // the transform of the staged form, on the 8 values of a step: BatchNorm scale / shift of column k (LDS tables, the 32
        // lanes of a half read the same 16 bytes: a broadcast), ReLU + row mask as one v_med3, split-encode, MFMAs
#define CGD_FWD_ITER(it_, RA, RW, OK)                                                                                 \
    {                                                                                                                 \
        const int c = __builtin_amdgcn_readfirstlane((it_) * G + g);                                                  \
        if (c < nchunk) {                                                                                             \
            const float kp = fcn_keep(OK);                                                                            \
            _Pragma("unroll") for (int st_ = 0; st_ < 2; ++st_) {                                                     \
                const float *sp_ = sS + c * KC + 16 * st_ + 8 * lh, *tp_ = tS + c * KC + 16 * st_ + 8 * lh;           \
                const v4f s0 = *(const v4f *)sp_, s1 = *(const v4f *)(sp_ + 4), t0 = *(const v4f *)tp_,               \
                          t1 = *(const v4f *)(tp_ + 4);                                                               \
                const v4f a0 = RA[2 * st_], a1 = RA[2 * st_ + 1];                                                     \
                const float xv[8] = {cg_actk(s0.x, a0.x, t0.x, kp), cg_actk(s0.y, a0.y, t0.y, kp),                    \
                                     cg_actk(s0.z, a0.z, t0.z, kp), cg_actk(s0.w, a0.w, t0.w, kp),                    \
                                     cg_actk(s1.x, a1.x, t1.x, kp), cg_actk(s1.y, a1.y, t1.y, kp),                    \
                                     cg_actk(s1.z, a1.z, t1.z, kp), cg_actk(s1.w, a1.w, t1.w, kp)};                   \
                u32x4 ah, al;                                                                                         \
                enc8<MM_ENC_A>(xv, ah, al);                                                                           \
                const u32x4 bh = RW[2 * st_], bl = RW[2 * st_ + 1];                                                   \
                if constexpr (MM == MM_F32) {                                                                         \
                    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                     \
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cg_u2f(ah[q]), cg_u2f(bh[q]), acc[0][0], 0, 0, 0); \
                    _Pragma("unroll") for (int q = 0; q < 4; ++q)                                                     \
                        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(cg_u2f(al[q]), cg_u2f(bl[q]), acc[0][0], 0, 0, 0); \
                } else if constexpr (X3) {                                                                            \
                    acc[0][0] = mfma16<MM>(ah, bl, acc[0][0]);                                                        \
                    acc[0][0] = mfma16<MM>(al, bh, acc[0][0]);                                                        \
                    acc[0][0] = mfma16<MM>(ah, bh, acc[0][0]);                                                        \
                } else {                                                                                              \
                    acc[0][0] = mfma16<MM>(ah, bh, acc[0][0]);                                                        \
                }                                                                                                     \
            }                                                                                                         \
        }                                                                                                             \
        if (c + DEPTH * G < nchunk) CGD_FWD_LOAD(c + DEPTH * G, RA, RW, OK);                                          \
    }
        {
            int sg_, tap_, k0_, so_;
            const int ca = min(g, nchunk - 1), cb = min(g + G, nchunk - 1);
            cg_locate_s(geo, C0, C1, C2, C3, ca * KC, sg_, tap_, k0_, so_);
            CGD_FWD_LOAD_AT(__builtin_amdgcn_readfirstlane(ca), __builtin_amdgcn_readfirstlane(sg_), __builtin_amdgcn_readfirstlane(tap_),
                            __builtin_amdgcn_readfirstlane(k0_), da0, dw0, dk0);
            cg_locate_s(geo, C0, C1, C2, C3, cb * KC, sg_, tap_, k0_, so_);
            CGD_FWD_LOAD_AT(__builtin_amdgcn_readfirstlane(cb), __builtin_amdgcn_readfirstlane(sg_), __builtin_amdgcn_readfirstlane(tap_),
                            __builtin_amdgcn_readfirstlane(k0_), da1, dw1, dk1);
            if constexpr (DEPTH == 3) {
                const int cc = min(g + 2 * G, nchunk - 1);
                cg_locate_s(geo, C0, C1, C2, C3, cc * KC, sg_, tap_, k0_, so_);
                CGD_FWD_LOAD_AT(__builtin_amdgcn_readfirstlane(cc), __builtin_amdgcn_readfirstlane(sg_), __builtin_amdgcn_readfirstlane(tap_),
                                __builtin_amdgcn_readfirstlane(k0_), da2, dw2, dk2);
            }
        }
        PROBE_STAMP();                                      // 1: first loads issued
        if (tid < nchunk) {                                 // the chunk descriptors: 8 dwords each
            int sg, tap, k0, so;
            cg_locate_s(geo, C0, C1, C2, C3, tid * KC, sg, tap, k0, so);
            const float *x = SEL4(sg, x0, x1, x2, x3);
            const int C = SEL4(sg, C0, C1, C2, C3), ty = SEL4(sg, T0, T1, T2, T3), Ls = SEL4(sg, Q0, Q1, Q2, Q3);
            const unsigned long long xa = (unsigned long long)x;
            const v4i d0 = {(int)(unsigned)xa, (int)(unsigned)(xa >> 32), 4 * C, Ls};
            const v4i d1 = {tap, 4 * k0, (geo.Lin - 1) * (ty ? 0 : 1), SEL4(sg, H0, H1, H2, H3)};
            *(v4i *)(cDesc + 8 * tid) = d0;
            *(v4i *)(cDesc + 8 * tid + 4) = d1;
        }
        const cg_klayer_p Lk = cg_kernarg_layer(koff);
        cg_fill_bn(Lk, sS, tS, tid, NTHR, bx == 0 && by == 0, &early);
        __syncthreads();                            // sS / tS and the chunk table ready
        PROBE_STAMP();                                      // 2: prologue done
        for (int it = 0; it < nit; it += DEPTH) {
            CGD_FWD_ITER(it, da0, dw0, dk0);
            if (it + 1 < nit) CGD_FWD_ITER(it + 1, da1, dw1, dk1);
            if constexpr (DEPTH == 3) {
                if (it + 2 < nit) CGD_FWD_ITER(it + 2, da2, dw2, dk2);
            }
        }
        PROBE_STAMP();                                      // 3: K loop done (wave 0)
#undef CGD_FWD_ITER
#undef CGD_FWD_LOAD
#undef CGD_FWD_LOAD_AT
#undef CGD_FWD_LOAD_CORE
    } else {
    int bb[NA], ll[NA];
    bool rv[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int gr = row0 + rb + RSTEP * i;
        rv[i] = gr < R;
        int q_ = 0, r_ = 0;
        cg_divmod(rv[i] ? gr : 0, LLout, cg_inv(LLout), q_, r_);           // (R < 2^23: cn_make_plan)
        bb[i] = q_;
        ll[i] = r_;
    }
#if defined(FCN_PROBE) && FCN_PROBE == 2      // (... the row -> (frustum, position) divisions are done)
    if (bb[0] + ll[0] == -12345) return;
    PROBE_STAMP();
#endif
    // TWO register sets: the chunk staged in iteration `it` was requested two iterations earlier, so a load has two
    // MFMA phases (not one) to come back from L2 / MALL / HBM before the LDS store needs it
    v4f ra0[NA], ra1[NA];
    u32x4 rw0[NB], rw1[NB];
    bool ok0[NA], ok1[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) { ra0[i] = zero4(); ra1[i] = zero4(); ok0[i] = false; ok1[i] = false; }
#pragma unroll
    for (int i = 0; i < NB; ++i) { rw0[i] = u32x4{0u, 0u, 0u, 0u}; rw1[i] = u32x4{0u, 0u, 0u, 0u}; }
    // weight image item f = gt + TG * i of a chunk: column f % TNC, (plane, k-block) row f / TNC -- 16-byte pieces, lane-linear
    // in global memory and in LDS (pre-encoded by cg_pack_kernel: no VALU on this operand)
    // (byte offsets: 32-bit, the chunk's part of the address added to the SGPR base -- no vector address arithmetic per load)
    unsigned woff[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int f = gt + TG * i;
        woff[i] = (unsigned)((f / TNC) * LCout + (f % TNC)) * 16u;
    }
    const char *wsrc = (const char *)(LWenc + n0);
    // (macros, not lambdas: the by-reference closure of a lambda called from several places is not always scalarised
    // by hipcc and drags every captured variable into scratch)
    // the chunk (hence the segment) is uniform within a K-group, i.e. within every wave: scalar selects
#define CGK_FWD_LOAD(cc, RA, RW, OK)                                                                                  \
    {                                                                                                                 \
        const int c__ = __builtin_amdgcn_readfirstlane(cc);                                                           \
        CGK_FWD_LOAD_AT(c__, __builtin_amdgcn_readfirstlane(cSeg[c__]), __builtin_amdgcn_readfirstlane(cTap[c__]),    \
                        __builtin_amdgcn_readfirstlane(cK0[c__]), RA, RW, OK);                                        \
    }
#define CGK_FWD_LOAD_AT(cc, SG, TAP, K0, RA, RW, OK)                                                                  \
    {                                                                                                                 \
        const int c_ = (cc);                                                                                          \
        const int sgi = (SG), tap = (TAP), k0 = (K0);                                                                 \
        const float *x = SEL4(sgi, x0, x1, x2, x3);                                                                   \
        const int C = SEL4(sgi, C0, C1, C2, C3), ty = SEL4(sgi, T0, T1, T2, T3), Ls = SEL4(sgi, Q0, Q1, Q2, Q3);      \
        const int h16 = SEL4(sgi, H0, H1, H2, H3);                                                                    \
        if (!((FCN_XF & 1) && c_ >= 2 * G))                                                                           \
        _Pragma("unroll") for (int i = 0; i < NA; ++i)                                                                \
            RA[i] = cg_load_raw<MM>(geo, x, C, Ls, ty ? 0 : 1, tap, k0 + 4 * kq, bb[i], ll[i], rv[i], OK[i], h16);    \
        if (!((FCN_XF & 2) && c_ >= 2 * G))                                                                           \
        {                                                                                                             \
            const char *wc_ = wsrc + (size_t)(unsigned)(c_ * 8 * LCout) * 16u;                                        \
            _Pragma("unroll") for (int i = 0; i < NB; ++i) RW[i] = *(gu4p)(wc_ + woff[i]);                            \
        }                                                                                                             \
    }
#define CGK_FWD_STAGE(c_, RA, RW, OK)                                                                                 \
    {                                                                                                                 \
        const v4f sp = *(const v4f *)(sS + (c_) * KC + 4 * kq), tp = *(const v4f *)(tS + (c_) * KC + 4 * kq);         \
        _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                              \
            const float kp = fcn_keep(OK[i]);                                                                         \
            kb_store4<MM_ENC_A, LDRA>(Ab, rb + RSTEP * i, kq, cg_actk(sp.x, RA[i].x, tp.x, kp),                        \
                                      cg_actk(sp.y, RA[i].y, tp.y, kp), cg_actk(sp.z, RA[i].z, tp.z, kp),             \
                                      cg_actk(sp.w, RA[i].w, tp.w, kp));                                              \
        }                                                                                                             \
        _Pragma("unroll") for (int i = 0; i < NB; ++i) {                                                              \
            const int f = gt + TG * i;                                                                                \
            Bb[(f / TNC) * LDRB + (f % TNC)] = RW[i];                                                                 \
        }                                                                                                             \
    }
#define CGK_FWD_ITER(it_, RA, RW, OK)                                                                                 \
    {                                                                                                                 \
        const int c = (it_) * G + g;                                                                                  \
        const bool act = c < nchunk;                                                                                  \
        if (act && !((FCN_XF & 4) && c >= G)) CGK_FWD_STAGE(c, RA, RW, OK);                                   \
        if constexpr (TG != 64) __syncthreads(); else __builtin_amdgcn_wave_barrier();                                \
        if (c + 2 * G < nchunk) CGK_FWD_LOAD(c + 2 * G, RA, RW, OK);                                         \
        if (act && !(FCN_XF & 8)) mma_chunk_kb<MM, 1, NTW, LDRA, LDRB>(Ab, Bb, wm * 32, wn * 32 * NTW, acc);      \
        if constexpr (TG != 64) __syncthreads(); else __builtin_amdgcn_wave_barrier();                                \
    }
    // A K-group of ONE wave (TG == 64: the 32 x 32 tile in use) owns its LDS buffers alone and the LDS serves a wave's
    // operations in order, so its write -> read -> write sequence needs no barrier: the four waves of the workgroup run
    // through their chunks independently and cover each other's load latency instead of marching in lockstep (two
    // workgroup barriers per K step before).  One barrier remains in front of the cross-group reduction below.
    // (__builtin_amdgcn_wave_barrier emits no instruction: it keeps the COMPILER from moving one lane's LDS reads of
    // other lanes' values above its own stores, or its next stores above those reads.)
    // The first two chunks of this K-group are requested BEFORE the prologue: they depend on neither the BatchNorm
    // statistics nor the LDS tables (their (segment, tap, channel) comes straight from cg_locate), so their trip to L2 / HBM
    // overlaps the fp64 finalisation below instead of following it -- one memory latency per layer off a 25-launch chain
    {
        int sg_, tap_, k0_, so_;
        const int ca = min(g, nchunk - 1), cb = min(g + G, nchunk - 1);
        cg_locate_s(geo, C0, C1, C2, C3, ca * KC, sg_, tap_, k0_, so_);
        CGK_FWD_LOAD_AT(__builtin_amdgcn_readfirstlane(ca), __builtin_amdgcn_readfirstlane(sg_), __builtin_amdgcn_readfirstlane(tap_),
                        __builtin_amdgcn_readfirstlane(k0_), ra0, rw0, ok0);
        cg_locate_s(geo, C0, C1, C2, C3, cb * KC, sg_, tap_, k0_, so_);
        CGK_FWD_LOAD_AT(__builtin_amdgcn_readfirstlane(cb), __builtin_amdgcn_readfirstlane(sg_), __builtin_amdgcn_readfirstlane(tap_),
                        __builtin_amdgcn_readfirstlane(k0_), ra1, rw1, ok1);
    }
    PROBE_STAMP();                                      // 1: first loads issued
    if (tid < nchunk) {
        int sg, tap, k0, so;
        cg_locate_s(geo, C0, C1, C2, C3, tid * KC, sg, tap, k0, so);
        cSeg[tid] = sg; cTap[tid] = tap; cK0[tid] = k0;
    }
    // (from here on the descriptor is read through the kernarg pointer: see cg_kernarg_layer)
    const cg_klayer_p Lk = cg_kernarg_layer(koff);
    if (FCN_XF & 32) { for (int i = tid; i < LKtot; i += NTHR) { sS[i] = 1.f; tS[i] = 0.f; } }
    else cg_fill_bn(Lk, sS, tS, tid, NTHR, bx == 0 && by == 0, &early);
    __syncthreads();                            // sS / tS and the chunk table ready
    if (FCN_XF & 256) { if (sS[0] == 123.456f) Lk->y[0] = 0.f; return; }      // (timing builds: launch + prologue only)
    PROBE_STAMP();                                      // 2: prologue done
    for (int it = 0; it < nit; it += 2) {
        CGK_FWD_ITER(it, ra0, rw0, ok0);
        if (it + 1 < nit) CGK_FWD_ITER(it + 1, ra1, rw1, ok1);
    }
    PROBE_STAMP();                                      // 3: K loop done (wave 0)
    if (FCN_XF & 16) { if (acc[0][0][0] == 123.456f) Lk->y[0] = 0.f; return; }
    }       // (staged form)
    const cg_klayer_p Le = cg_kernarg_layer(koff);      // the epilogue's fields: fetched now, not in the entry block
    // ---- sum the G group accumulators through LDS, then one epilogue pass over the tile
    if constexpr (TG == 64) __syncthreads();            // every group is done with its operand buffers (reused below)
    float *red = lds;                                   // [G][TMB][TNC]
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            red[(g * TMB + wm * 32 + acc_row(reg, lh)) * TNC + (wn * NTW + j) * 32 + l31] = acc[0][j][reg];
    __syncthreads();
    PROBE_STAMP();                                      // 4: all groups done, partials in LDS
    constexpr int NQ = TNC / 4;                         // column quads of the tile
    const int ecq = tid % NQ;
    const int col = n0 + 4 * ecq;
    v4f cs1 = zero4(), cs2 = zero4();                   // per-thread column sums (over its rows)
    for (int er = tid / NQ; er < TMB; er += NTHR / NQ) {
        v4f v = zero4();
#pragma unroll
        for (int q = 0; q < G; ++q) v += *(const v4f *)(red + (q * TMB + er) * TNC + 4 * ecq);
        if (Le->bias) {
            v.x += col + 0 < Le->nbias ? Le->bias[col + 0] : 0.f; v.y += col + 1 < Le->nbias ? Le->bias[col + 1] : 0.f;
            v.z += col + 2 < Le->nbias ? Le->bias[col + 2] : 0.f; v.w += col + 3 < Le->nbias ? Le->bias[col + 3] : 0.f;
        }
        const int row = row0 + er;
        if (row < R) {
            if (St<MM>::half && Le->y16) {
                sts4e<MM>(Le->y, (int64_t)row * Le->Cout + col, v);
                v = st_round4<MM>(v);                      // the sums are over the values as stored
            } else {
                sts4(Le->y + (int64_t)row * Le->Cout + col, v);
            }
            cs1 += v;
            cs2 += v * v;
            // fp16 operand parts overflow at |x| >= 65504 (inf - inf = NaN in the products, which the next layer's ReLU would
            // turn into a silent zero): a non-finite output raises the sticky flag of the workspace
            if constexpr (MM == MM_F16X3) {
                if (!(fabsf(v.x) + fabsf(v.y) + fabsf(v.z) + fabsf(v.w) < 3.0e38f) && Le->flags) atomicOr(Le->flags, FCN_FLAG_NONFINITE);
            }
        }
    }
    PROBE_STAMP();                                      // 5: outputs stored
    if (!Le->stat) { PROBE_FLUSH(((unsigned long long)Le->Ktot << 32) | ((unsigned long long)Le->Cout << 16) | (unsigned long long)(Le->Lout & 0xffff)); return; }
    // rows of one wave: lanes NQ apart share a column quad -> xor-shuffle down to NQ lanes, then across waves via LDS
    float pv[8] = {cs1.x, cs1.y, cs1.z, cs1.w, cs2.x, cs2.y, cs2.z, cs2.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int o = NQ; o < 64; o <<= 1) pv[q] += __shfl_xor(pv[q], o, 64);
    }
    __syncthreads();
    float *st = lds;                                    // [NTHR/64 waves][TNC cols][2]
    if (lane < NQ) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st[((tid >> 6) * TNC + 4 * ecq + j) * 2] = pv[j];
            st[((tid >> 6) * TNC + 4 * ecq + j) * 2 + 1] = pv[4 + j];
        }
    }
    __syncthreads();
    if (tid < 2 * TNC) {
        const int c = tid % TNC, w = tid / TNC;
        double a = 0.0;
#pragma unroll
        for (int r = 0; r < NTHR / 64; ++r) a += (double)st[(r * TNC + c) * 2 + w];
        if (!(FCN_XF & 64) || a == 123.456) atomic_add_f64(&Le->stat[(int64_t)(blockIdx.x % FCN_CG_REP) * Le->rep_stride + w * Le->Cs + (n0 + c) % Le->Cs], a);
    }
    PROBE_STAMP();                                      // 6: statistics added
    PROBE_FLUSH(((unsigned long long)Le->Ktot << 32) | ((unsigned long long)Le->Cout << 16) | (unsigned long long)(Le->Lout & 0xffff));
}

template <int MM, int MW, int G, int WNC = 2, int NTW = 1, int EB = FCN_FWD_EARLY_BN>
__global__ __launch_bounds__(G * 64 * MW * WNC) void cgk_fwd_kernel(CgLayer L)
{
    const int nby = L.Cout / (32 * WNC * NTW), nbx = (L.B * L.Lout + 32 * MW - 1) / (32 * MW);
    const int t = cg_xcd_tile(blockIdx.x, nbx * nby);          // column tiles fastest: a row tile's operand rows stay in one L2
    if (t < 0) return;
    int bx, by;
    cg_divmod(t, nby, cg_inv(nby), bx, by);                    // (t < 2^23: a grid is at most a few thousand workgroups)
    cgk_fwd_body<MM, MW, G, WNC, NTW, EB>(L, bx, by, 0);
}

// Two INDEPENDENT layers in one launch (a deconvolution next to the stride-2 conv that reads the same merge output):
// workgroups [0, na) take layer A's tiles, the rest layer B's -- one launch skeleton less on the chain, and the two small
// grids fill the CUs together.
struct CgLayerPair {
    CgLayer A, B;
    int na;                    // workgroups of A (a multiple of 8); the rest belong to B
};

template <int MM, int MW, int G, int WNC, int NTW = 1, int EB = FCN_FWD_EARLY_BN>
__global__ __launch_bounds__(G * 64 * MW * WNC) void cgk_fwd_pair_kernel(CgLayerPair p)
{
    const int bid = blockIdx.x;
    const bool isA = bid < p.na;
    const CgLayer &L = isA ? p.A : p.B;
    const int nby = L.Cout / (32 * WNC * NTW), nbx = (L.B * L.Lout + 32 * MW - 1) / (32 * MW);
    const int t = cg_xcd_tile(isA ? bid : bid - p.na, nbx * nby);
    if (t < 0) return;
    int bx, by;
    cg_divmod(t, nby, cg_inv(nby), bx, by);
    if (isA) cgk_fwd_body<MM, MW, G, WNC, NTW, EB>(p.A, bx, by, (int)offsetof(CgLayerPair, A));
    else cgk_fwd_body<MM, MW, G, WNC, NTW, EB>(p.B, bx, by, (int)offsetof(CgLayerPair, B));
}

// BN-backward coefficients of one channel from the batch sums (sum dz, sum dz*xhat): gamma*rstd, mean, rstd, dbeta/M,
// dgamma/M.  Like the forward's scale/shift they are derived by every consumer workgroup in its prologue; the
// designated workgroup also exports dgamma / dbeta.
struct CgBnBwd {
    const double *bstat;       // sum dz [Cs], sum dz*xhat [Cs] (final, replica 0); nullptr: the layer has no BN (heads)
    int rep_stride;            // doubles between replica blocks (the whole bstat arena)
    int frozen;                // FCN_BN_FROZEN: the forward normalised with the running statistics -- no batch-mean terms
    const float *gamma, *bn;   // bn: (scale, shift, mean, rstd) published by the forward
    double M;
    float *dgamma, *dbeta;     // non-null on the launch that exports them
};

template <class QT>            // QT: CgBnBwd by value or through the kernarg pointer (address_space(4))
__device__ __forceinline__ void cg_bnbwd_coef(const QT &q, int Cs, int c, float (&cf)[5], bool pub)
{
    const double db = cg_rep_sum(q.bstat + c, q.rep_stride), dg = cg_rep_sum(q.bstat + Cs + c, q.rep_stride);
    const float rstd = q.bn[3 * Cs + c];
    cf[0] = q.gamma[c] * rstd;
    cf[1] = q.bn[2 * Cs + c];
    // (one division; the two per-channel quotients become products.  Frozen statistics: 0, so c2 = c3 = 0 and dy = c0 * dz)
    const double invM = q.frozen ? 0.0 : 1.0 / q.M;
    const double c0 = (double)cf[0];                    // the folded form of fcn_common.h: dy = fma(c0, dz, -fma(c2, y - c1, c3))
    cf[2] = (float)(c0 * (double)rstd * (dg * invM));
    cf[3] = (float)(c0 * (db * invM));
    cf[4] = 0.f;
    if (pub && q.dgamma) { q.dgamma[c] = (float)dg; q.dbeta[c] = (float)db; }
}

// the same from sums / table entries that are already in registers (FCN_BWD_EARLY_BN: requested at kernel entry)
template <class QT>
__device__ __forceinline__ void cg_bnbwd_coef_pre(const QT &q, int Cs, int c, const double (&sb)[FCN_CG_REP], const double (&sg)[FCN_CG_REP],
                                                  float rstd, float mean, float gam, float (&cf)[5], bool pub)
{
    double db = sb[0], dg = sg[0];
#pragma unroll
    for (int r = 1; r < FCN_CG_REP; ++r) { db += sb[r]; dg += sg[r]; }
    cf[0] = gam * rstd;
    cf[1] = mean;
    const double invM = q.frozen ? 0.0 : 1.0 / q.M;
    const double c0 = (double)cf[0];
    cf[2] = (float)(c0 * (double)rstd * (dg * invM));
    cf[3] = (float)(c0 * (db * invM));
    cf[4] = 0.f;
    if (pub && q.dgamma) { q.dgamma[c] = (float)dg; q.dbeta[c] = (float)db; }
}
// FCN_BWD_EARLY_BN: the data-gradient role requests the BatchNorm-backward sums of channel `tid` (all replicas) and its mean / rstd /
// gamma at entry, beside the kernel-argument batch, as FCN_FWD_EARLY_BN does in the forward
#ifndef FCN_BWD_EARLY_BN
#define FCN_BWD_EARLY_BN 0
#endif

#define CG_CMAX 512            // largest BN width (Cs) whose backward coefficients are staged in LDS

// dy of a BN layer from raw (dz, y) and the LDS-staged coefficients: kk*(dz - dbeta/M - xhat*dgamma/M)
__device__ __forceinline__ float cg_dy(const float *coefS, int Cs, int ch, float dz, float y)
{
    return fcn_bn_dy1(coefS[ch], coefS[Cs + ch], coefS[2 * Cs + ch], coefS[3 * Cs + ch], dz, y);
}

// Weight packing descriptor of one layer: conv (Cout, Cin, KT) or deconv (Cin, Cout, k) <-> packed (N, Ktot).
struct CgPack {
    int N, Ktot, KT, nseg;
    int C[CG_NSEG], choff[CG_NSEG], type[CG_NSEG];      // GEMM channels, channel offset in the torch weight, segment type
    int nvec, cin_tot, deconv_k, cout_t;
};

template <class PT>
__device__ __forceinline__ int64_t cg_torch_index(const PT &p, int n, int kk)
{
    if (p.deconv_k > 0) {               // row n = j*Cout + co, kk = ci  ->  W[ci][co][j]
        const int j = n / p.cout_t, co = n % p.cout_t;
        return ((int64_t)kk * p.cout_t + co) * p.deconv_k + j;
    }
    int sg = 0;
#pragma unroll
    for (int s = 0; s < CG_NSEG; ++s)
        if (s < p.nseg && sg == s && kk >= p.KT * p.C[s]) { kk -= p.KT * p.C[s]; sg = s + 1; }
    const int tap = kk / p.C[sg], k = kk % p.C[sg];
    if (p.type[sg] == 1 && k >= p.nvec) return -1;       // padding column of the virtual one-hot segment
    return ((int64_t)n * p.cin_tot + p.choff[sg] + k) * p.KT + tap;
}

struct CgPackAll {
    CgPack p[CN_NLAYER];
    const float *src[CN_NLAYER];
    float *dst[CN_NLAYER];
    int64_t pre[CN_NLAYER + 1];
    int nrow_real[CN_NLAYER];           // rows of the packed matrix that exist in the torch weight (heads: 41 of 64)
    const float *oh;                    // one-hot (B, nvec) -> oh64 (B, OH_PAD), zero padded
    float *oh64;
    int B, nvec;
    // the BN sum buffers of the coming forward (stat) and backward (bstat) are zeroed here too: no memset nodes on the
    // latency-bound chains (the packing runs ahead of both, on its own stream)
    double *z0, *z1;
    int nz;
    // forward operand images (gemm_tile.h "kb-major"): layer l's packed matrix split-encoded in MFMA operand order,
    // [Ktot/32][plane][4][N] u32x4 at enc + pre[l] floats -- the forward K loops stage their weights with plain 16-byte copies
    float *enc;
    int mmf;                            // operand mode of the forward GEMMs (MM_*)
    // data-gradient operand images (CgLayer.Wgrd) at grd + pre[l] floats, encoded in the backward operand mode mmb; written by a
    // second range of threads of the same launch (one thread = the 8 n-adjacent values of one packed column)
    float *grd;
    int mmb;
};

// One thread = 8 reduction-adjacent elements (kk0 .. kk0 + 7, kk0 % 8 == 0) of one packed row n: they lie in ONE (segment, tap)
// run of the torch weight (segment widths are multiples of 8), so ONE index computation + a constant source stride serves all
// eight; the thread writes them to the packed fp32 matrix (the backward's operand) AND as one item of the forward image.
// (Round 2 computed the torch index per ELEMENT with 64-bit divisions: 47 us on the side stream beside the CU-bound PointNet
// forward.)
__device__ __forceinline__ void cg_pack_src8(const CgPack &p, const float *__restrict__ src, int nrow_real, int n, int kk0,
                                              float (&x)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    if (n >= nrow_real) return;
    if (p.deconv_k > 0) {               // row n = j*Cout + co, kk = ci  ->  W[ci][co][j]: source stride Cout * k per kk
        const int jj = n / p.cout_t, co = n % p.cout_t;
        const int64_t o0 = ((int64_t)kk0 * p.cout_t + co) * p.deconv_k + jj, st = (int64_t)p.cout_t * p.deconv_k;
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = src[o0 + j * st];
        return;
    }
    int sg = 0, kk = kk0;
#pragma unroll
    for (int s = 0; s < CG_NSEG; ++s)
        if (s < p.nseg && sg == s && kk >= p.KT * p.C[s]) { kk -= p.KT * p.C[s]; sg = s + 1; }
    const int C = SEL4(sg, p.C[0], p.C[1], p.C[2], p.C[3]), choff = SEL4(sg, p.choff[0], p.choff[1], p.choff[2], p.choff[3]);
    const int ty = SEL4(sg, p.type[0], p.type[1], p.type[2], p.type[3]);
    const int tap = kk / C, k0 = kk % C;
    const int64_t o0 = ((int64_t)n * p.cin_tot + choff + k0) * p.KT + tap;      // + KT per channel
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (ty != 1 || k0 + j < p.nvec) x[j] = src[o0 + (int64_t)j * p.KT];        // (padding columns of the virtual one-hot segment)
}

// The 8 OUTPUT-adjacent values Wp[n0 .. n0+7][kk] (n0 % 8 == 0): one (segment, tap, channel) decomposition of kk serves all eight
// rows, the torch weight is walked with the row stride (conv: cin_tot * KT per n; deconv: rows n = j*Cout + co -> stride k per co)
__device__ __forceinline__ void cg_pack_src8n(const CgPack &p, const float *__restrict__ src, int nrow_real, int n0, int kk,
                                               float (&x)[8])
{
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = 0.f;
    if (p.deconv_k > 0) {               // row n = jj*Cout + co, kk = ci  ->  W[ci][co][jj]
        const int jj = n0 / p.cout_t, co = n0 % p.cout_t;          // (Cout = 256: the 8 rows share jj)
        const int64_t o0 = ((int64_t)kk * p.cout_t + co) * p.deconv_k + jj;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (n0 + j < nrow_real) x[j] = src[o0 + (int64_t)j * p.deconv_k];
        return;
    }
    int sg = 0, k2 = kk;
#pragma unroll
    for (int s = 0; s < CG_NSEG; ++s)
        if (s < p.nseg && sg == s && k2 >= p.KT * p.C[s]) { k2 -= p.KT * p.C[s]; sg = s + 1; }
    const int C = SEL4(sg, p.C[0], p.C[1], p.C[2], p.C[3]), choff = SEL4(sg, p.choff[0], p.choff[1], p.choff[2], p.choff[3]);
    const int ty = SEL4(sg, p.type[0], p.type[1], p.type[2], p.type[3]);
    const int tap = k2 / C, k0 = k2 % C;
    if (ty == 1 && k0 >= p.nvec) return;                            // padding column of the virtual one-hot segment
    const int64_t o0 = ((int64_t)n0 * p.cin_tot + choff + k0) * p.KT + tap, st = (int64_t)p.cin_tot * p.KT;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (n0 + j < nrow_real) x[j] = src[o0 + j * st];
}

template <int MM>
__device__ __forceinline__ void cg_pack_store8n(const CgPack &p, int n0, int kk, const float (&x)[8], u32x4 *__restrict__ img)
{
    u32x4 hi, lo;
    enc8<MM>(x, hi, lo);
    const int n8 = n0 >> 3;
    img[((int64_t)n8 * 2 + 0) * p.Ktot + kk] = hi;
    img[((int64_t)n8 * 2 + 1) * p.Ktot + kk] = lo;
}

template <int MM>
__device__ __forceinline__ void cg_pack_store8(const CgPack &p, int n, int kk0, const float (&x)[8], float *__restrict__ dst,
                                                u32x4 *__restrict__ img)
{
    const v4f a = {x[0], x[1], x[2], x[3]}, b = {x[4], x[5], x[6], x[7]};
    sts4(dst + (int64_t)n * p.Ktot + kk0, a);
    sts4(dst + (int64_t)n * p.Ktot + kk0 + 4, b);
    if (img) {
        const int c = kk0 >> 5, kb = (kk0 >> 3) & 3;
        u32x4 hi, lo;
        enc8<MM>(x, hi, lo);
        img[((int64_t)c * 8 + kb) * p.N + n] = hi;
        img[((int64_t)c * 8 + 4 + kb) * p.N + n] = lo;
    }
}

__global__ void cg_pack_kernel(CgPackAll t)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t ngrp = t.pre[CN_NLAYER] / 8;
    if (t.grd && i >= ngrp && i < 2 * ngrp) {           // the data-gradient images: group m of layer l = (n8, kk), kk fastest
        i -= ngrp;
        int l = 0;
#pragma unroll
        for (int q = 1; q < CN_NLAYER; ++q)
            if (8 * i >= t.pre[q]) l = q;
        const int m = (int)(i - t.pre[l] / 8);
        const int Kt = t.p[l].Ktot;
        const int n8 = m / Kt, kk = m - n8 * Kt;
        float x[8];
        cg_pack_src8n(t.p[l], t.src[l], t.nrow_real[l], 8 * n8, kk, x);
        u32x4 *img = (u32x4 *)(t.grd + t.pre[l]);
        if (t.mmb == MM_F32) cg_pack_store8n<MM_F32>(t.p[l], 8 * n8, kk, x, img);
        else if (t.mmb == MM_BF16X3) cg_pack_store8n<MM_BF16X3>(t.p[l], 8 * n8, kk, x, img);
        else if (t.mmb == MM_F16X3) cg_pack_store8n<MM_F16X3>(t.p[l], 8 * n8, kk, x, img);
        else cg_pack_store8n<MM_BF16X1>(t.p[l], 8 * n8, kk, x, img);
        return;
    }
    if (t.grd && i >= 2 * ngrp) i -= ngrp;
    if (i >= ngrp) {
        int64_t j = i - ngrp;
        if (j < (int64_t)t.B * OH_PAD) {
            const int b = (int)(j / OH_PAD), v = (int)(j % OH_PAD);
            t.oh64[j] = (v < t.nvec) ? t.oh[(int64_t)b * t.nvec + v] : 0.f;
            return;
        }
        j -= (int64_t)t.B * OH_PAD;
        if (j < t.nz) {
            if (t.z0) t.z0[j] = 0.0;
            if (t.z1) t.z1[j] = 0.0;
        }
        return;
    }
    int l = 0;
#pragma unroll
    for (int q = 1; q < CN_NLAYER; ++q)
        if (8 * i >= t.pre[q]) l = q;
    const int m = (int)(i - t.pre[l] / 8);                  // group index inside the layer (N * Ktot / 8 < 2^31)
    const int gpr = t.p[l].Ktot >> 3;                       // groups per packed row
    const int n = m / gpr, kk0 = (m - n * gpr) << 3;
    float x[8];
    cg_pack_src8(t.p[l], t.src[l], t.nrow_real[l], n, kk0, x);
    u32x4 *img = t.enc ? (u32x4 *)(t.enc + t.pre[l]) : nullptr;
    if (t.mmf == MM_F32) cg_pack_store8<MM_F32>(t.p[l], n, kk0, x, t.dst[l], img);
    else if (t.mmf == MM_F16X3) cg_pack_store8<MM_F16X3>(t.p[l], n, kk0, x, t.dst[l], img);
    else if (t.mmf == MM_BF16X3) cg_pack_store8<MM_BF16X3>(t.p[l], n, kk0, x, t.dst[l], img);
    else cg_pack_store8<MM_BF16X1>(t.p[l], n, kk0, x, t.dst[l], img);
}

// ------------------------------------------------------------------------------------------------
// Backward: ONE launch per chain layer.  The data-gradient chain is a latency-bound sequence of small GEMMs (B*L rows) and
// the weight gradients only hang off it; run as separate launches -- even on a second captured stream -- ROCm's graph
// executor serialises them.  So each step's launch carries three kinds of workgroups, picked by block index:
//   [0, w_blk0)       data-gradient tiles of every differentiated input segment of layer l   (the critical chain)
//   [w_blk0, r_blk0)  weight-gradient tiles of layer l, rows split over workgroups -> partials
//   [r_blk0, end)     the fixed-order sum of the PREVIOUS step's partials into the torch weight layout
// The weight-gradient and reduce workgroups fill the CUs the few data-gradient tiles leave idle.
struct CgDgSeg {               // one differentiated input segment of the layer
    int sg, segoff;            // which segment; its column offset in Wp
    const float *ysrc, *bnsrc; // producer's pre-BN output and published BN (scale,shift,mean,rstd); null: plain input
    float *out;                // producer's dz (Rsrc x C) or the input gradient
    int accumulate;            // add to what `out` already holds (a second consumer)
    int out16;                 // `out` is a dz arena: bf16 in the bf16 throughput mode (a feature map's gradient stays fp32)
    double *bstat_src;         // non-null on the LAST consumer: sum dz, sum dz*xhat of the producer
    int tx, ncb;               // row tiles (32 rows each) and 64-channel column blocks; tile t -> (t / ncb, t % ncb)
    int blk0;                  // first workgroup of this segment (a multiple of 8)
    int wave_tiles;            // SHORT reductions (at most CGB_ROWS_MAXCH chunks: the heads, K = 64): a workgroup takes 8 tiles, one per
                               // wave, each wave reducing all chunks of its tile -- no cross-wave sum, an eighth of the workgroups
};

struct CgReduce {
    const float *partial;      // (nsplit, N, Ktot)
    int nsplit;
    CgPack pk;
    int nrow_real;
    float *dW;
    int gr;                    // split groups per workgroup (1, 2, 4, 8)
    // gr == 0: the slot carries the heads' bias gradient instead (first launch, nothing to reduce yet):
    // dW[n] = sum_r partial[r * nsplit + n] for n < nrow_real, one workgroup per column, nsplit = row stride, pk.N = rows
};

struct CgBwdStep {
    CgLayer lay;               // the layer being differentiated
    const float *dz;           // its incoming dz (R x Cout)
    int dz16;                  // dz (and lay.y) are bf16 arenas (bf16 throughput mode; the heads' dlogits are fp32)
    CgBnBwd cb;                // its BN backward (bstat null: no BN)
    int ndg;
    CgDgSeg dg[CG_NSEG];       // read on the device through the kernarg segment only (cg_bwd_step_body), never indexed
                               // dynamically through the by-value copy
    float *partial;            // wgrad partials of this layer
    int rows, w_ns, w_ny;      // rows per split (multiple of KC), splits, 64-row tiles of Wp
    int w_blk0, r_blk0;
    CgReduce red;
};

// K-groups of a data-gradient tile = waves of a backward workgroup (ONE wave each): a template parameter G of the backward kernels, 4
// or 8, chosen per model by the host (cn_bwd_groups).  4 (256 threads, 38 KB of LDS: four workgroups per CU) against the 8 of rounds
// 3-4 (512 threads, 64 KB: two per CU) is the same 16 waves per CU in twice as many, half as long-lived workgroups: car step
// 1.216-1.226 -> 1.177-1.181 ms (-3.4 %), people -1.5 %; but where a launch does not fill the machine anyway (refine: 640 rows, SUN-RGBD:
// 2 560) the longer K loops of four groups only stretch the chain -- refine 0.713 -> 0.750 ms with 4.  2: car +10 %.
#define CGB_KH_ 16
#define CGB_LDW_ 36
#define CG_CMAX_ 512
#define CG_KBWD_ 2048
template <int G>
struct CgB {
    static constexpr int T = 64 * G;                                   // threads
    static constexpr int LDS = G * (CGB_KH_ * CGB_LDW_ + CGB_KH_ * LDN);     // G waves x (A [KH][LDA or LDW] + B [KH][LDN])
    static constexpr int SMEM = LDS + 5 * CG_CMAX_ + 3 * (CG_KBWD_ / CGB_KH_);      // + BN-backward coefficients + chunk tables
};
#define CGB_KH 16              // reduction chunk of a K-group (one 32x32x16 step)

#ifndef CGB_ROWS_MAXCH
#define CGB_ROWS_MAXCH 4       // data-gradient tiles with at most this many chunks run one per WAVE (CgDgSeg.wave_tiles)
#endif
#define CGB_LDA 34             // A leading dimension: 4 * LDA = 8 (mod 32) spreads a half-wave's ds_write_b32 over all banks
#define CGB_LDW 36             // leading dimension of the weight-gradient role's dy operand (float4 stores: rows 16-B aligned)
#define CGB_ASZ (CGB_KH * CGB_LDW)
#define CGB_WSZ (CGB_ASZ + CGB_KH * LDN)     // one wave's operand buffers (both roles)
#define CG_KBWD 2048           // largest reduction length of a data-gradient GEMM (block5_deconv: 8 * 256 output columns)
static_assert(CGB_KH == CGB_KH_ && CGB_LDW == CGB_LDW_ && CG_CMAX == CG_CMAX_ && CG_KBWD == CG_KBWD_ &&
              CgB<4>::LDS == 4 * CGB_WSZ, "CgB mirrors the backward's LDS layout constants");

// ------------------------------------------------------------------------------------------------
// 16-deep kb-major chunk images of the backward data-gradient role (gemm_tile.h "kb-major", two k-blocks instead of four):
// [plane][2 k-blocks][LDR] u32x4 -- a fragment is ONE ds_read_b128 per operand part (the k-major dword layout needed four
// ds_read_b32), and the weight operand arrives PRE-ENCODED (CgLayer.Wgrd, cg_pack_kernel) as plain 16-byte copies.
// LDR: the staging of the dy operand is a ds_write_b64 per lane -- 16-lane groups of 4 rows x (2 k-blocks x 2 halves), 32 banks for
// stores (MI355X_MICROARCH.md, LDS table): the two k-blocks of a group must sit 16 banks apart, 4 * LDR = 16 (mod 32).  With the
// T + 2 of the 32-deep images (4 k-blocks, 8 banks apart) the k-blocks of a 32-row tile were 8 apart and every group wrote
// 2-way: SQ_LDS_BANK_CONFLICT 10.5 / 11.7 % of the backward kernels' LDS cycles (profiles/r04_final_pmc_sq_summary.txt).
template <int T>
struct Kb16 {
    static constexpr int LDR = T + (T % 8 == 0 ? 4 : KB_PAD);
    static constexpr int U4 = 4 * LDR;         // u32x4 per chunk (2 planes x 2 k-blocks)
};
template <int MM, int LDR>
__device__ __forceinline__ void kb16_store4(u32x4 *img, int r, int kq, float x0, float x1, float x2, float x3)
{
    const int kb = kq >> 1, half = kq & 1;      // kq = 0..3: values 4*kq .. 4*kq+3 of the chunk
    if constexpr (MM == MM_F32) {
        const v4f v = {x0, x1, x2, x3};
        *(v4f *)(img + (half * 2 + kb) * LDR + r) = v;
    } else {
        float h0, l0, h1, l1;
        enc2<MM>(x0, x1, h0, l0);
        enc2<MM>(x2, x3, h1, l1);
        const v2f_kb h = {h0, h1}, l = {l0, l1};
        *(v2f_kb *)((float *)(img + kb * LDR + r) + 2 * half) = h;
        if constexpr (!mm_x1<MM>) *(v2f_kb *)((float *)(img + (2 + kb) * LDR + r) + 2 * half) = l;
    }
}
template <int MM, int NT, int LDRA, int LDRB>
__device__ __forceinline__ void mma_chunk_kb16(const u32x4 *A, const u32x4 *B, f32x16 (&acc)[1][NT])
{
    const int lane = threadIdx.x & 63;
    const int l31 = lane & 31, lh = lane >> 5;
    if constexpr (MM == MM_F32) {
        const float *Af = (const float *)A, *Bf = (const float *)B;
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            const int k = kk + lh, kb = k >> 3, j = k & 7;
            const float a = Af[(((j >> 2) * 2 + kb) * LDRA + l31) * 4 + (j & 3)];
            float b[NT];
#pragma unroll
            for (int jn = 0; jn < NT; ++jn) b[jn] = Bf[(((j >> 2) * 2 + kb) * LDRB + jn * 32 + l31) * 4 + (j & 3)];
#pragma unroll
            for (int jn = 0; jn < NT; ++jn) acc[0][jn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[jn], acc[0][jn], 0, 0, 0);
        }
    } else {
        constexpr bool X3 = !mm_x1<MM>;
        const u32x4 ah = A[lh * LDRA + l31];
        u32x4 al, bh[NT], bl[NT];
        if constexpr (X3) al = A[(2 + lh) * LDRA + l31];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            bh[j] = B[lh * LDRB + j * 32 + l31];
            if constexpr (X3) bl[j] = B[(2 + lh) * LDRB + j * 32 + l31];
        }
        if constexpr (X3) {
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[0][j] = mfma16<MM>(ah, bl[j], acc[0][j]);
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[0][j] = mfma16<MM>(al, bh[j], acc[0][j]);
        }
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[0][j] = mfma16<MM>(ah, bh[j], acc[0][j]);
    }
}

// G[rs][k] = sum_tap sum_n dy[r_out(rs,tap)][n] * Wp[n][segoff + tap*C + k]; 32 source rows x 64 source channels by 8
// K-groups, then the producer-side epilogue: ReLU mask from its pre-BN output, accumulate (second consumer),
// BN-backward sums.
// A K-group is ONE wave: it owns its LDS operand buffers alone and the LDS serves a wave's operations in order, so the
// write -> read -> write sequence of its K loop needs no barrier (cgk_fwd_body does the same).  The groups take 16-deep
// chunks g, g + 8, ...: a wave stages the same number of operand values per step as a wave of the former two-wave groups
// did with 32-deep chunks (32 x 16 of dy + 16 x 64 of W), and computes the whole 32 x 64 tile of its chunk.
// ROWS (CgDgSeg.wave_tiles): bx = the workgroup's first tile, by = the segment's tile count; wave g owns tile bx + g alone.
template <int MM, bool ROWS, int G, class LT, class CT>    // LT / CT: CgLayer / CgBnBwd, by value or through the kernarg pointer
__device__ __forceinline__ void cg_dgrad_body(const LT &L, const CT &cb, const float *dzc, const float *yc,
                                              int sgi, int segoff, const float *ysrc, const float *bnsrc, float *outp,
                                              int accumulate, double *bstat_src, int bx, int by, bool pub, float *smem,
                                              int dz16, int out16, int ncb = 1)
{
    // (bf16 throughput mode: dz16 -- this layer's dz / y are bf16 arenas (not the heads' fp32 dlogits); out16 -- `outp` is a
    // layer's dz arena (not a pooled feature map's fp32 gradient); the producer's y behind `ysrc` always is one)
    constexpr int KH = CGB_KH, TMB = 32, NTHR = G * 64;
    constexpr int LDRA = Kb16<TMB>::LDR, LDRB = Kb16<64>::LDR;
    constexpr bool X3 = !mm_x1<MM>;
    constexpr int NA = TMB * (KH / 4) / 64;             // 4-vectors of dy per lane per chunk (2)
    constexpr int NB = (X3 || MM == MM_F32) ? 4 : 2;    // u32x4 of the encoded weight per lane per chunk: (plane, k-block) rows x 64 columns
    constexpr int ASZ = CGB_ASZ, NCH = CG_KBWD / KH;
    static_assert(NTHR == CgB<G>::T && NA == 2 && KH == 16 && Kb16<TMB>::U4 * 4 <= ASZ && Kb16<64>::U4 * 4 <= CGB_WSZ - ASZ,
                  "dgrad lane mapping / operand images fit the wave's LDS region");
    float *lds = smem;
    float *coefS = smem + CgB<G>::LDS;
    int *cTap = (int *)(coefS + 5 * CG_CMAX), *cNb = cTap + NCH, *cCh = cNb + NCH;
    BPROBE_DECL;
    BPROBE_STAMP();                             // 0: entry
    // sgi is workgroup-uniform (a scalar loaded from the role descriptor)
    // everything the code in front of the first loads reads, as ONE batch of scalar loads (L is read through the kernarg pointer:
    // the wave-uniform segment index is address arithmetic)
    int SC = L.seg[sgi].C, SLsrc = L.seg[sgi].Lsrc;
    int LB = L.B, LLin = L.Lin, LLout = L.Lout, LCout = L.Cout, LKT = L.KT, LCs = L.Cs, Lpad = L.pad, Lstride = L.stride, LKtot = L.Ktot;
    const u32x4 *LWgrd = L.Wgrd;
    const double *cbstat = cb.bstat;
    CG_PIN(13, SC, SLsrc, LB, LLin, LLout, LCout, LKT, LCs, Lpad, Lstride, LKtot, LWgrd, cbstat);
    const int tid = threadIdx.x, g = tid >> 6;
    const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    double esb[FCN_CG_REP], esg[FCN_CG_REP];
    float erstd = 0.f, emean = 0.f, egam = 0.f;
    if constexpr (FCN_BWD_EARLY_BN != 0) {
        if (cbstat != nullptr) {
            const int ce = min(tid, LCs - 1);                               // (clamped: unconditional loads)
            const int rs_ = cb.rep_stride;
            const float *bnp = cb.bn, *gmp = cb.gamma;
#pragma unroll
            for (int r = 0; r < FCN_CG_REP; ++r) {
                esb[r] = cbstat[(int64_t)r * rs_ + ce];
                esg[r] = cbstat[(int64_t)r * rs_ + LCs + ce];
            }
            erstd = bnp[3 * LCs + ce]; emean = bnp[2 * LCs + ce]; egam = gmp[ce];
        }
    }
    u32x4 *Ai = (u32x4 *)(lds + g * CGB_WSZ), *Bi = (u32x4 *)(lds + g * CGB_WSZ + ASZ);
    const int C = SC, Rs = LB * SLsrc, Cs = LCs;
    bool wave_live = true;
    if constexpr (ROWS) {                               // this wave's own tile (the prologue's barrier is reached by every wave)
        const int t = bx + g;
        wave_live = t < by;
        int tbx, tby;
        cg_divmod(wave_live ? t : 0, ncb, cg_inv(ncb), tbx, tby);
        bx = __builtin_amdgcn_readfirstlane(tbx); by = __builtin_amdgcn_readfirstlane(tby);
    }
    const int row0 = bx * TMB, c0 = by * 64;
    const int kq = lane & 3, rb = lane >> 2;            // dy: 4 column quads x 16 rows per pass
    constexpr int RSTEP = 16;
    const bool hasbn = cbstat != nullptr;
    int bL[NA], li[NA];                                 // bL: first output row of the source row's frustum
    bool rv[NA], ok[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int gr = row0 + rb + RSTEP * i;
        rv[i] = gr < Rs;
        int q_ = 0, r_ = 0;
        cg_divmod(rv[i] ? gr : 0, SLsrc, cg_inv(SLsrc), q_, r_);           // (Rs < 2^23: cn_make_plan)
        bL[i] = q_ * LLout;
        li[i] = r_;
        rv[i] = rv[i] && li[i] < LLin;
        ok[i] = false;
    }
    f32x16 acc[1][2];
    acc_zero<1, 2>(acc);
    v4f rz[NA], ry[NA];
    u32x4 rw[NB];
    const int ncn = LCout / KH, nchunk = LKT * ncn, nit = ROWS ? nchunk : (nchunk + G - 1) / G;
    // No integer division inside the reduction loop (each one is ~40 VALU instructions and the loop body is otherwise
    // ~100): the (tap, column base, BN channel base) of every chunk comes from a small LDS table.
    if (tid < nchunk) {
        int tp, cn, q_, ch;
        cg_divmod(tid, ncn, cg_inv(ncn), tp, cn);         // (float-reciprocal divisions: three general ones were ~120 instructions)
        const int nb = cn * KH;
        cg_divmod(nb, Cs, cg_inv(Cs), q_, ch);
        cTap[tid] = tp; cNb[tid] = nb; cCh[tid] = ch;
    }
    // the weight operand: this tile's 64 columns of the layer's data-gradient image (CgLayer.Wgrd), one column per lane
    const u32x4 *wg = LWgrd + segoff + c0 + lane;
#define CGK_DGRAD_LOAD(cc)                                                                                            \
    {                                                                                                                 \
        const int c__ = (cc);                                                                                         \
        CGK_DGRAD_LOAD_AT(__builtin_amdgcn_readfirstlane(cTap[c__]), __builtin_amdgcn_readfirstlane(cNb[c__]));       \
    }
#define CGK_DGRAD_LOAD_AT(TAP, NBASE)                                                                                 \
    {                                                                                                                 \
        const int tap = (TAP), nb = (NBASE);                                                                          \
        if (!((FCN_XG & 1) && xg_later))                                                                              \
        _Pragma("unroll") for (int i = 0; i < NA; ++i) {                                                              \
            /* the output position source row li meets through tap t: (li + pad - t) / stride when it divides; */   \
            /* stride is 1 or 2 (cn_make_plan rejects anything else): shift / mask instead of a division */          \
            const int t_ = li[i] + Lpad - tap;                                                                       \
            const int lq = (Lstride == 2) ? (t_ >> 1) : t_;                                                          \
            ok[i] = rv[i] && t_ >= 0 && ((Lstride == 2) ? ((t_ & 1) == 0) : true) && lq < LLout;                    \
            const int lo = min(max(lq, 0), LLout - 1);                                                               \
            /* 32-bit byte offset off the scalar base, one full-rate 24-bit multiply-add (see cg_load_raw) */         \
            const unsigned ob = fcn_mad24((unsigned)(bL[i] + lo), (unsigned)(4 * LCout), (unsigned)(4 * (nb + 4 * kq))); \
            if (St<MM>::half && dz16) {                                                                               \
                rz[i] = lds4e<MM>(dzc, ob >> 2);                                                                      \
                ry[i] = lds4e<MM>(hasbn ? yc : dzc, ob >> 2);                                                         \
            } else {                                                                                                  \
                rz[i] = *(gv4fp)((const char *)dzc + ob);  /* unconditional (clamped row), masked at store time */    \
                ry[i] = *(gv4fp)((const char *)(hasbn ? yc : dzc) + ob);                                              \
            }                                                                                                         \
        }                                                                                                             \
        if (!((FCN_XG & 2) && xg_later))                                                                              \
        _Pragma("unroll") for (int i = 0; i < NB; ++i)          /* row i = (plane i >> 1, k-block i & 1): 16-byte copies */ \
            rw[i] = ldgu4(wg + (unsigned)((((nb >> 3) + (i & 1)) * 2 + (i >> 1)) * LKtot + tap * C));                \
    }
    bool xg_later = false;
    // first chunk requested BEFORE the coefficient prologue (it depends on neither the BN-backward sums nor the LDS tables):
    // its memory latency overlaps the prologue's
    {
        const int c1 = ROWS ? 0 : min(g, nchunk - 1);
        int tp1, cn1;
        cg_divmod(c1, ncn, cg_inv(ncn), tp1, cn1);
        CGK_DGRAD_LOAD_AT(__builtin_amdgcn_readfirstlane(tp1), __builtin_amdgcn_readfirstlane(cn1 * KH));
    }
    BPROBE_STAMP();                             // 1: first loads issued
    if (hasbn) {
        for (int c = tid; c < Cs; c += NTHR) {
            float cf[5];
            if (FCN_BWD_EARLY_BN != 0 && c == tid) cg_bnbwd_coef_pre(cb, Cs, c, esb, esg, erstd, emean, egam, cf, pub);
            else cg_bnbwd_coef(cb, Cs, c, cf, pub);
#pragma unroll
            for (int q = 0; q < 5; ++q) coefS[q * Cs + c] = cf[q];
        }
    }
    __syncthreads();                            // chunk table and coefS ready
    BPROBE_STAMP();                             // 2: prologue done
    if (ROWS && !wave_live) return;             // (no barrier behind this point in the one-tile-per-wave form)
    for (int it = 0; it < nit; ++it) {
        const int c = ROWS ? it : it * G + g;
        if (c >= nchunk) break;                 // wave-uniform: no barrier inside the loop
        xg_later = true;
        if (!((FCN_XG & 4) && it > 0))
        {
            const int chb = __builtin_amdgcn_readfirstlane(cCh[c]) + 4 * kq;     // BN channel of this thread's first column
            // the five coefficients of the thread's four channels as 16-byte LDS reads, ONE branch on hasbn per chunk (per element
            // they were 40 ds_read_b32 and 8 branches in front of 6 MFMAs); the operation order is cg_dy's
            v4f f0 = zero4(), f1 = zero4(), f2 = zero4(), f3 = zero4();
            if (hasbn) {
                const float *cp = coefS + chb;          // (16-byte aligned: coefS, Cs and chb are multiples of 4 floats)
                f0 = *(const v4f *)cp; f1 = *(const v4f *)(cp + Cs); f2 = *(const v4f *)(cp + 2 * Cs);
                f3 = *(const v4f *)(cp + 3 * Cs);
            }
#pragma unroll
            for (int i = 0; i < NA; ++i) {
                const int r = rb + RSTEP * i;
                v4f d = rz[i];
                if (hasbn) {
                    const v4f y = ry[i];
                    d.x = fcn_bn_dy1(f0.x, f1.x, f2.x, f3.x, d.x, y.x); d.y = fcn_bn_dy1(f0.y, f1.y, f2.y, f3.y, d.y, y.y);
                    d.z = fcn_bn_dy1(f0.z, f1.z, f2.z, f3.z, d.z, y.z); d.w = fcn_bn_dy1(f0.w, f1.w, f2.w, f3.w, d.w, y.w);
                }
                d = ok[i] ? d : zero4();
                kb16_store4<MM_ENC_A, LDRA>(Ai, r, kq, d.x, d.y, d.z, d.w);
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) Bi[((i >> 1) * 2 + (i & 1)) * LDRB + lane] = rw[i];
        }
        __builtin_amdgcn_wave_barrier();        // (compiler only) the stores above before the operand reads of every lane
        if (c + (ROWS ? 1 : G) < nchunk) CGK_DGRAD_LOAD(c + (ROWS ? 1 : G));
        if (!(FCN_XG & 8)) mma_chunk_kb16<MM, 2, LDRA, LDRB>(Ai, Bi, acc);
        __builtin_amdgcn_wave_barrier();        // ... and those reads before the next chunk's stores
    }
    BPROBE_STAMP();                             // 3: K loop done (wave 0)
    if (FCN_XG & 16) { if (acc[0][0][0] == 123.456f) outp[0] = 0.f; return; }
    if constexpr (ROWS) {
        // the wave's tile straight from the accumulators (MFMA layout: lane = column l31 (+ 32 j), registers = 16 rows): ReLU mask of
        // the producer, store, BatchNorm-backward sums of the producer -- per column over the lane's rows, the two half-waves joined by
        // one shuffle, then fp64 atomics (the same count per tile as the workgroup form)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int col = c0 + j * 32 + l31;
            float ps = 0.f, pt = 0.f, pm = 0.f, pr = 0.f;
            if (bnsrc) { ps = bnsrc[col]; pt = bnsrc[C + col]; pm = bnsrc[2 * C + col]; pr = bnsrc[3 * C + col]; }
            float yv[16];
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {        // (all loads first: see the PointNet data-gradient epilogue)
                const int row = min(row0 + acc_row(reg, lh), Rs - 1);
                yv[reg] = bnsrc ? lds1e<MM>(ysrc, (int64_t)row * C + col) : 0.f;
            }
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = row0 + acc_row(reg, lh);
                if (row < Rs) {
                    float gs = acc[0][j][reg];
                    float xh = 0.f;
                    if (bnsrc) { gs = fmaf(ps, yv[reg], pt) > 0.f ? gs : 0.f; xh = (yv[reg] - pm) * pr; }
                    const int64_t o = (int64_t)row * C + col;
                    if (St<MM>::half && out16) {
                        if (accumulate) gs += lds1e<MM>(outp, o);
                        sts1e<MM>(outp, o, gs);
                        gs = st_round<MM>(gs);             // the sums are over the values as stored
                    } else {
                        if (accumulate) gs += outp[o];
                        outp[o] = gs;
                    }
                    s1 += gs;
                    s2 = fmaf(gs, xh, s2);
                }
            }
            if (bstat_src) {
                s1 += __shfl_xor(s1, 32, 64);
                s2 += __shfl_xor(s2, 32, 64);
                if (lh == 0) {
                    double *br = bstat_src + (int64_t)(blockIdx.x % FCN_CG_REP) * cb.rep_stride;
                    atomic_add_f64(&br[col], (double)s1);
                    atomic_add_f64(&br[C + col], (double)s2);
                }
            }
        }
        return;
    }
    // sum of the G group accumulators through LDS in two rounds (G x 32 x 64 floats do not fit at G = 8): the upper half park theirs,
    // the lower half add them to their own and park the sums for the epilogue pass
    constexpr int GE = G / 2;
    float *red = lds;                                   // [GE][TMB][64]
    __syncthreads();                            // every group is done with its operand buffers
    if (g >= GE) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                red[((g - GE) * TMB + acc_row(reg, lh)) * 64 + j * 32 + l31] = acc[0][j][reg];
    }
    __syncthreads();
    if (g < GE) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                float *rp = red + (g * TMB + acc_row(reg, lh)) * 64 + j * 32 + l31;
                *rp = acc[0][j][reg] + *rp;
            }
    }
    __syncthreads();
    BPROBE_STAMP();                             // 4: groups summed
    const int ecq = tid & 15;
    const int col = c0 + 4 * ecq;
    v4f ps = zero4(), pt = zero4(), pm = zero4(), pr = zero4();
    if (bnsrc) {
        ps = ldg4(bnsrc + col); pt = ldg4(bnsrc + C + col);
        pm = ldg4(bnsrc + 2 * C + col); pr = ldg4(bnsrc + 3 * C + col);
    }
    v4f cs1 = zero4(), cs2 = zero4();
    for (int er = tid >> 4; er < TMB; er += NTHR / 16) {
        const int row = row0 + er;
        if (row >= Rs) continue;
        v4f gsum = zero4();
#pragma unroll
        for (int q = 0; q < GE; ++q) gsum += *(const v4f *)(red + (q * TMB + er) * 64 + 4 * ecq);
        const int64_t o = (int64_t)row * C + col;
        v4f xh = zero4();
        if (bnsrc) {
            const v4f yv = lds4e<MM>(ysrc, o);
            gsum.x = fmaf(ps.x, yv.x, pt.x) > 0.f ? gsum.x : 0.f; gsum.y = fmaf(ps.y, yv.y, pt.y) > 0.f ? gsum.y : 0.f;
            gsum.z = fmaf(ps.z, yv.z, pt.z) > 0.f ? gsum.z : 0.f; gsum.w = fmaf(ps.w, yv.w, pt.w) > 0.f ? gsum.w : 0.f;
            xh = (yv - pm) * pr;
        }
        if (St<MM>::half && out16) {
            if (accumulate) gsum += lds4e<MM>(outp, o);
            sts4e<MM>(outp, o, gsum);
            gsum = st_round4<MM>(gsum);                    // the sums are over the values as stored
        } else {
            if (accumulate) gsum += ldg4(outp + o);
            sts4(outp + o, gsum);
        }
        cs1 += gsum;
        cs2 += gsum * xh;
    }
    BPROBE_STAMP();                             // 5: outputs stored
    if (!bstat_src) { BPROBE_FLUSH((1ull << 60) | ((unsigned long long)LKtot << 32) | ((unsigned long long)LCout << 16) | (unsigned long long)(C & 0xffff)); return; }
    float pv[8] = {cs1.x, cs1.y, cs1.z, cs1.w, cs2.x, cs2.y, cs2.z, cs2.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        pv[q] += __shfl_xor(pv[q], 16, 64);
        pv[q] += __shfl_xor(pv[q], 32, 64);
    }
    __syncthreads();
    float *st = lds;                                    // [NTHR/64 waves][64 cols][2]
    if (lane < 16) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            st[((tid >> 6) * 64 + 4 * ecq + j) * 2] = pv[j];
            st[((tid >> 6) * 64 + 4 * ecq + j) * 2 + 1] = pv[4 + j];
        }
    }
    __syncthreads();
    if (tid < 128) {
        const int c = tid & 63, w = tid >> 6;
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < NTHR / 64; ++r) v += (double)st[(r * 64 + c) * 2 + w];
        atomic_add_f64(&bstat_src[(int64_t)(blockIdx.x % FCN_CG_REP) * cb.rep_stride + w * C + c0 + c], v);
    }
    BPROBE_STAMP();                             // 6: statistics added
    BPROBE_FLUSH((1ull << 60) | ((unsigned long long)LKtot << 32) | ((unsigned long long)LCout << 16) | (unsigned long long)(C & 0xffff));
}

// dWp[n][kk] = sum_r dy[r][n] * A[r][kk]; tile 64 (n) x 64 (kk); the workgroup owns rows [rbeg, rend) of one split.
// Its waves are G / 2 row-chunk STREAMS (16-row chunks s, s + NS, ...) x two halves of the n side: a wave stages the
// 16 x 32 slice of dy and the 16 x 64 slice of A of its chunk into LDS buffers of its own and computes 32 (n) x 64 (kk) --
// nothing is shared between waves, so the loop has no barrier (the A slice is staged by both waves of a stream: its
// transform is one fma + max per value).  The stream accumulators are summed through LDS at the end.
template <int MM, int G, class AT>              // AT: CgBwdStep, by value or through the kernarg pointer
__device__ __forceinline__ void cg_wgrad_body(const AT &a, int wid, float *smem)
{
    constexpr int KH = CGB_KH, NS = G / 2, LDW = CGB_LDW;
    const auto &L = a.lay;
    BPROBE_DECL;
    BPROBE_STAMP();                             // 0: entry
    const int tid = threadIdx.x, w = tid >> 6, st = w >> 1, wm = w & 1;
    const int lane = tid & 63, l31 = lane & 31, lh = lane >> 5;
    float *As = smem + w * CGB_WSZ, *Bs = As + CGB_ASZ;
    // the kernel-argument fields of the prologue as ONE batch of scalar loads (see cgk_fwd_body)
    int w_ny = a.w_ny, w_ns = a.w_ns, a_rows = a.rows, adz16 = a.dz16;
    int LB = L.B, LLout = L.Lout, LKtot = L.Ktot, LCs = L.Cs, LCout = L.Cout;
    CgGeo geo;
    geo.nseg = L.nseg; geo.KT = L.KT; geo.stride = L.stride; geo.pad = L.pad; geo.Lin = L.Lin;
    int sC0 = L.seg[0].C, sC1 = L.seg[1].C, sC2 = L.seg[2].C, sC3 = L.seg[3].C;
    CG_PIN(18, w_ny, w_ns, a_rows, adz16, LB, LLout, LKtot, LCs, LCout, geo.nseg, geo.KT, geo.stride, geo.pad, geo.Lin, sC0, sC1, sC2, sC3);
    // XCD order: the row split is the slow index, so the workgroups that reduce the same rows (all output tiles) share an L2
    const int nyz = w_ny * (LKtot / 64);
    const int wt = cg_xcd_tile(wid, w_ns * nyz);
    if (wt < 0) return;
    int bx, byz, by, bz;
    cg_divmod(wt, nyz, cg_inv(nyz), bx, byz);                   // (wt < 2^23; float-reciprocal divisions)
    cg_divmod(byz, w_ny, cg_inv(w_ny), bz, by);
    const int R = LB * LLout, Cs = LCs;
    const int rbeg = bx * a_rows, rend = min(R, rbeg + a_rows);
    const int n0 = by * 64 + wm * 32, kk0 = bz * 64;
    int sg, tap, k0, so;
    cg_locate_s(geo, sC0, sC1, sC2, sC3, kk0, sg, tap, k0, so);         // kk0 is workgroup-uniform
    sg = __builtin_amdgcn_readfirstlane(sg);
    // the segment's descriptor: `a` lives in the kernarg segment (cg_bwd_step_body reads it through the kernarg pointer), so a
    // wave-uniform index is plain address arithmetic and the six fields come in ONE batch of scalar loads (selected field by field
    // from four pinned copies they were 24 loads strung along a chain of branches)
    const auto &S = L.seg[sg];
    const float *Sx = S.x, *Sbn = (const float *)S.bn, *adz = a.dz, *Ly = (const float *)L.y;
    const double *cbstat = a.cb.bstat;
    int SC = S.C, Sty = S.type, SLs = S.Lsrc, S16 = S.st16;
    CG_PIN(9, Sx, Sbn, adz, Ly, cbstat, SC, Sty, SLs, S16);
    // dy slice: 8 column quads x 8 row pairs (rows 2*pa, 2*pa + 1: a k pair); A slice: 16 column quads x 4 row pairs, twice
    const int cqa = lane & 7, pa = lane >> 3;
    const int cqb = lane & 15, pb = lane >> 4;
    // constants of the tile's 64 + 64 columns in LDS (registers are short: 4 waves per SIMD): BN-backward coefficients of dy
    // [5][64], BN scale / shift of the A operand [2][64]
    const bool hasbn = cbstat != nullptr;
    float *cfS = smem + CgB<G>::LDS, *abS = cfS + 5 * 64;
    const float *cfp = cfS + wm * 32 + 4 * cqa, *abp = abS + 4 * cqb;
    f32x16 acc[1][2];
    acc_zero<1, 2>(acc);
    v4f rz[2], ry[2], rx[4];
    bool ok[4];
    const int xC = SC, xLs = SLs, xlm = Sty ? 0 : 1;
    const int nch = (rend - rbeg + KH - 1) / KH, nit = (nch + NS - 1) / NS;
    // (frustum, position) of the FIRST row of this thread's two A row pairs, advanced by NS*KH per chunk instead of divided
    // out of the row index; the second row of a pair is the next position (or position 0 of the next frustum)
    int wb[2], wl[2];
    const float invL = cg_inv(L.Lout);
#pragma unroll
    for (int p2 = 0; p2 < 2; ++p2) cg_divmod(rbeg + st * KH + 2 * (pb + 4 * p2), LLout, invL, wb[p2], wl[p2]);      // (R < 2^23: cn_make_plan)
    int bend, lend;
    cg_divmod(rend - 1, LLout, invL, bend, lend);
#define CG_WGRAD_LOAD(rr)                                                                                             \
    {                                                                                                                 \
        const int r0_ = (rr);                                                                                         \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                               \
            const int row = min(r0_ + 2 * pa + i, rend - 1);    /* clamped: unconditional loads, masked at store */   \
            const unsigned ob = fcn_mad24((unsigned)row, (unsigned)(4 * LCout), (unsigned)(4 * (n0 + 4 * cqa)));     \
            if (St<MM>::half && adz16) {                                                                              \
                rz[i] = lds4e<MM>(adz, ob >> 2);                                                                      \
                ry[i] = lds4e<MM>(hasbn ? Ly : adz, ob >> 2);                                                         \
            } else {                 /* byte offset off the scalar base: see cg_load_raw */                           \
                rz[i] = *(gv4fp)((const char *)adz + ob);                                                             \
                ry[i] = *(gv4fp)((const char *)(hasbn ? Ly : adz) + ob);                                              \
            }                                                                                                         \
        }                                                                                                             \
        _Pragma("unroll") for (int p2 = 0; p2 < 2; ++p2) {                                                            \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                           \
                const bool in = r0_ + 2 * (pb + 4 * p2) + i < rend;                                                   \
                const bool wrap = i == 1 && wl[p2] + 1 >= LLout;                                                     \
                const int b_ = wrap ? wb[p2] + 1 : wb[p2], l_ = wrap ? 0 : wl[p2] + i;                                \
                rx[2 * p2 + i] = cg_load_raw<MM>(geo, Sx, xC, xLs, xlm, tap, k0 + 4 * cqb, in ? b_ : bend,            \
                                                 in ? l_ : lend, true, ok[2 * p2 + i], S16);                          \
            }                                                                                                         \
            wl[p2] += NS * KH;                                                                                        \
            while (wl[p2] >= LLout) { wl[p2] -= LLout; wb[p2] += 1; }                                               \
        }                                                                                                             \
    }
    // the first chunk is requested BEFORE the coefficient tables below are filled: they wait for the BatchNorm sums (a memory
    // round trip of waves 0 and 1, which the workgroup's barrier then waits for) and the operand loads depend on neither
    if (st < nch) CG_WGRAD_LOAD(rbeg + st * KH);
    BPROBE_STAMP();                             // 1: first loads issued
    if (tid < 64) {
        float c5[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (hasbn) cg_bnbwd_coef(a.cb, Cs, (by * 64 + tid) % Cs, c5, false);
#pragma unroll
        for (int q = 0; q < 5; ++q) cfS[q * 64 + tid] = c5[q];
    } else if (tid < 128) {
        const int j = tid - 64;
        abS[j] = Sbn ? Sbn[k0 + j] : 1.f;
        abS[64 + j] = Sbn ? Sbn[SC + k0 + j] : 0.f;
    }
    __syncthreads();                            // cfS / abS ready
    BPROBE_STAMP();                             // 2: prologue done
    for (int it = 0; it < nit; ++it) {
        const int c = NS * it + st;
        if (c >= nch) break;                    // wave-uniform: no barrier inside the loop
        const int r0 = rbeg + c * KH;
        if (!((FCN_XG & 512) && it > 0))
        {
            v4f dv2[2];
            {
                const v4f f0 = *(const v4f *)cfp, f1 = *(const v4f *)(cfp + 64), f2 = *(const v4f *)(cfp + 128),
                          f3 = *(const v4f *)(cfp + 192);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    v4f d = rz[i];
                    if (hasbn) {                // elementwise, the same operations as cg_dy
                        const v4f y = ry[i];
                        d.x = fcn_bn_dy1(f0.x, f1.x, f2.x, f3.x, d.x, y.x); d.y = fcn_bn_dy1(f0.y, f1.y, f2.y, f3.y, d.y, y.y);
                        d.z = fcn_bn_dy1(f0.z, f1.z, f2.z, f3.z, d.z, y.z); d.w = fcn_bn_dy1(f0.w, f1.w, f2.w, f3.w, d.w, y.w);
                    }
                    const bool live = (r0 + 2 * pa + i) < rend;
                    dv2[i] = live ? d : zero4();
                }
            }
            const v4f as = *(const v4f *)abp, at = *(const v4f *)(abp + 64);
            v4f hi, lo;
            enc2x4<MM_ENC_A>(dv2[0], dv2[1], hi, lo);
            sts4(As + mma_row_hi<KH>(pa) * LDW + 4 * cqa, hi);          // rows (2 pa, 2 pa + 1) = pair pa: gemm_tile.h "pair-plane" order
            sts4(As + mma_row_lo<KH>(pa) * LDW + 4 * cqa, lo);
#pragma unroll
            for (int p2 = 0; p2 < 2; ++p2) {
                if (FCN_XG & 2048) {            // (timing build: the activation operand as plain 16-byte copies -- a pre-encoded image's cost)
                    // (masked to small finite 16-bit halves: raw fp32 bits read as bf16 pairs would turn the weights into NaN)
                    v4i m0 = __builtin_bit_cast(v4i, rx[2 * p2]) & 0x3f7f3f7f, m1 = __builtin_bit_cast(v4i, rx[2 * p2 + 1]) & 0x3f7f3f7f;
                    sts4(Bs + mma_row_hi<KH>(pb + 4 * p2) * LDN + 4 * cqb, __builtin_bit_cast(v4f, m0));
                    sts4(Bs + mma_row_lo<KH>(pb + 4 * p2) * LDN + 4 * cqb, __builtin_bit_cast(v4f, m1));
                    continue;
                }
                v4f av2[2];
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const int q = 2 * p2 + i;
                    const float live = fcn_keep(ok[q] && (r0 + 2 * (pb + 4 * p2) + i) < rend);
                    v4f av = {cg_actk(as.x, rx[q].x, at.x, live), cg_actk(as.y, rx[q].y, at.y, live),
                              cg_actk(as.z, rx[q].z, at.z, live), cg_actk(as.w, rx[q].w, at.w, live)};
                    av2[i] = av;
                }
                enc2x4<MM_ENC_A>(av2[0], av2[1], hi, lo);
                sts4(Bs + mma_row_hi<KH>(pb + 4 * p2) * LDN + 4 * cqb, hi);
                sts4(Bs + mma_row_lo<KH>(pb + 4 * p2) * LDN + 4 * cqb, lo);
            }
        }
        __builtin_amdgcn_wave_barrier();        // (compiler only) the stores above before the operand reads of every lane
        if (c + NS < nch && !(FCN_XG & 256)) CG_WGRAD_LOAD(r0 + NS * KH);
        if (!(FCN_XG & 1024)) mma_chunk<MM, 1, 2, LDW, LDN, KH>(As, Bs, 0, 0, acc);
        __builtin_amdgcn_wave_barrier();        // ... and those reads before the next chunk's stores
    }
    BPROBE_STAMP();                             // 3: K loop done (wave 0)
    // streams 2, 3 park their accumulators, streams 0, 1 add them to their own; stream 1 parks the sum, stream 0 adds it and
    // writes the split's partial
    float *red = smem + (((st & 1) * 2 + wm) * 32) * 64;    // [2 slots][2 halves][32][64]
    __syncthreads();                            // every wave is done with its operand buffers
#if defined(FCN_PROBE) && FCN_PROBE == 4
    BPROBE_STAMP();                             // (4: every wave has left its K loop)
#endif
    if (NS == 4 ? st >= 2 : st == 1) {          // (two streams, G = 4: stream 1 parks, stream 0 adds and writes)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) red[acc_row(reg, lh) * 64 + j * 32 + l31] = acc[0][j][reg];
    }
    __syncthreads();
    if (NS == 4 && st < 2) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                float *rp = red + acc_row(reg, lh) * 64 + j * 32 + l31;
                acc[0][j][reg] += *rp;
                if (st == 1) *rp = acc[0][j][reg];
            }
    }
    __syncthreads();
#if defined(FCN_PROBE) && FCN_PROBE == 4
    BPROBE_STAMP();                             // (5: the stream sums are in LDS)
#endif
    if (st == 0) {
        const float *r1 = smem + ((2 + wm) * 32) * 64;      // stream 1's slot
        float *out = a.partial + (int64_t)bx * LCout * LKtot;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rr = acc_row(reg, lh), cc = j * 32 + l31;
                out[(int64_t)(n0 + rr) * LKtot + kk0 + cc] = NS == 1 ? acc[0][j][reg] : acc[0][j][reg] + r1[rr * 64 + cc];
            }
    }
    BPROBE_STAMP();                             // 4: partial written (wave 0: behind the last barrier)
    BPROBE_FLUSH((2ull << 60) | ((unsigned long long)LKtot << 32) | ((unsigned long long)LCout << 16) | (unsigned long long)(LLout & 0xffff));
}

// dW (torch layout) = sum of the split partials (fixed order); padding columns/rows are dropped.  The workgroup covers
// CGB_T / gr consecutive packed elements with gr split groups (gr = 1, 2, 4 or 8, chosen on the host from the split
// count): big layers have few splits and many elements (one thread per element), small layers the opposite (a few
// independent loads per thread, then a group sum through LDS).
template <int G, class QT>
__device__ __forceinline__ void cg_reduce_body(const QT &q, int rid, float *smem)
{
    constexpr int CGB_T = CgB<G>::T;
    const auto &p = q.pk;
    if (q.gr == 0) {                    // column sum of dlogits (R = p.N rows, row stride q.nsplit): dbias of the heads
        float t = 0.f;
        for (int r = threadIdx.x; r < p.N; r += CGB_T) t += q.partial[(int64_t)r * q.nsplit + rid];
        smem[threadIdx.x] = t;
        __syncthreads();
        for (int o = CGB_T / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) smem[threadIdx.x] += smem[threadIdx.x + o];
            __syncthreads();
        }
        if (threadIdx.x == 0 && rid < q.nrow_real) q.dW[rid] = smem[0];
        return;
    }
    const int gr = q.gr, per = CGB_T / gr;
    const int x = threadIdx.x % per, y = threadIdx.x / per;
    const int64_t e = (int64_t)rid * per + x;                   // N * Ktot is a multiple of 64 * 8
    const int64_t nelem = (int64_t)p.N * p.Ktot;
    float s0 = 0.f, s1 = 0.f;
    int sp = y;
    for (; sp + gr < q.nsplit; sp += 2 * gr) {
        s0 += q.partial[(int64_t)sp * nelem + e];
        s1 += q.partial[(int64_t)(sp + gr) * nelem + e];
    }
    if (sp < q.nsplit) s0 += q.partial[(int64_t)sp * nelem + e];
    float t = s0 + s1;
    if (gr > 1) {
        smem[y * per + x] = t;
        __syncthreads();
        if (y != 0) return;
        t = 0.f;
        for (int g = 0; g < gr; ++g) t += smem[g * per + x];
    }
    const int n = (int)(e / p.Ktot), kk = (int)(e % p.Ktot);
    if (n >= q.nrow_real) return;
    const int64_t o = cg_torch_index(p, n, kk);
    if (o < 0) return;
    q.dW[o] = t;
}

template <int MM, int G>
__device__ __forceinline__ void cg_bwd_step_body(const CgBwdStep &a, const int bid, float *smem, const int koff)
{
    // The role of this workgroup from ONE batch of scalar loads of the by-value parameter; everything else is read through the kernarg
    // POINTER inside the role that needs it (cg_kernarg_layer explains: fields read through the by-value parameter are all fetched in
    // the entry block -- here the union of what three roles read, a dozen serialized s_load / s_waitcnt / v_writelane batches in front
    // of every one of the 800-2 800 workgroups of a launch).
    const int r_blk0 = opaque_s(a.r_blk0), w_blk0 = opaque_s(a.w_blk0), ndg = opaque_s(a.ndg);
    const int b1 = opaque_s(a.dg[1].blk0), b2 = opaque_s(a.dg[2].blk0), b3 = opaque_s(a.dg[3].blk0);
    typedef __attribute__((address_space(4))) const char *kchar_p;
    typedef __attribute__((address_space(4))) const CgBwdStep *kstep_p;
    kstep_p ak = (kstep_p)((kchar_p)__builtin_amdgcn_kernarg_segment_ptr() + koff);
    asm volatile("" : "+s"(ak) : : "memory");
#ifndef CGB_NO_REDUCE
    if (bid >= r_blk0) { cg_reduce_body<G>(ak->red, bid - r_blk0, smem); return; }
#endif
#ifndef CGB_NO_WGRAD
    if (bid >= w_blk0) { cg_wgrad_body<MM, G>(*ak, bid - w_blk0, smem); return; }
#endif
#ifdef CGB_NO_DGRAD
    return;
#endif
    const int role = __builtin_amdgcn_readfirstlane((ndg > 3 && bid >= b3) ? 3 : ((ndg > 2 && bid >= b2) ? 2 : ((ndg > 1 && bid >= b1) ? 1 : 0)));
    // The role's segment descriptor is one of four: a scalar load at a wave-uniform offset from the kernarg pointer fetches exactly
    // one (selecting it field by field from the by-value struct costs 4 x 14 pinned SGPRs, and indexing the struct dynamically makes
    // LLVM copy the whole kernarg struct to scratch).
    const auto *g = &ak->dg[role];
    int ncb = g->ncb, gtx = g->tx, gblk0 = g->blk0, gwt = g->wave_tiles;
    CG_PIN(4, ncb, gtx, gblk0, gwt);
    if (gwt) {                          // short reduction: eight tiles per workgroup, one per wave
        const int ntile = gtx * ncb;
        const int t = cg_xcd_tile(bid - gblk0, (ntile + G - 1) / G);
        if (t < 0) return;
        cg_dgrad_body<MM, true, G>(ak->lay, ak->cb, ak->dz, ak->lay.y, g->sg, g->segoff, g->ysrc, g->bnsrc, g->out, g->accumulate,
                                g->bstat_src, t * G, ntile, bid == 0, smem, ak->dz16, g->out16, ncb);
        return;
    }
    const int t = cg_xcd_tile(bid - gblk0, gtx * ncb);
    if (t < 0) return;
    int tbx, tby;
    cg_divmod(t, ncb, cg_inv(ncb), tbx, tby);                  // (t < 2^23)
    cg_dgrad_body<MM, false, G>(ak->lay, ak->cb, ak->dz, ak->lay.y, g->sg, g->segoff, g->ysrc, g->bnsrc, g->out, g->accumulate,
                             g->bstat_src, tbx, tby, bid == 0, smem, ak->dz16, g->out16);
}

template <int MM, int G>
__global__ __launch_bounds__(64 * G, 4) void cg_bwd_step_kernel(CgBwdStep a)
{
    __shared__ __attribute__((aligned(16))) float smem[CgB<G>::SMEM];
    cg_bwd_step_body<MM, G>(a, blockIdx.x, smem, 0);
}

// A chain step and an OFF-CHAIN step (the backward of a deconvolution, which only hangs off the heads) in one launch:
// workgroups [0, na) belong to A, the rest to B.  The two must not write the same gradient buffer.
struct CgBwdPair {
    CgBwdStep A, B;
    int na;
};

template <int MM, int G>
__global__ __launch_bounds__(64 * G, 4) void cg_bwd_pair_kernel(CgBwdPair p)
{
    __shared__ __attribute__((aligned(16))) float smem[CgB<G>::SMEM];
    const int bid = blockIdx.x;
    if (bid < p.na) cg_bwd_step_body<MM, G>(p.A, bid, smem, (int)offsetof(CgBwdPair, A));
    else cg_bwd_step_body<MM, G>(p.B, bid - p.na, smem, (int)offsetof(CgBwdPair, B));
}

// ================================================================================================
// Host side: the topology of ConvFeatNet(128, nvec) + heads for n = 4 (models/det_base.py:163-224) or n = 5 pyramid levels
// (models/det_base_sunrgbd.py:174-251).  Layer ids (include/fcn_hip.h):
//   0 block1_conv1;  1 + 3*(j-2) + {0,1,2}: block{j}_conv1 / _conv2 / _merge (j = 2..n);  3n-2 + (j-2): block{j}_deconv;
//   4n-3: heads.
// n = 4:  0 b1c1  1 b2c1  2 b2c2  3 b2m  4 b3c1  5 b3c2  6 b3m  7 b4c1  8 b4c2  9 b4m  10 b2d  11 b3d  12 b4d  13 heads
// ================================================================================================
// Operand mode of the FCN kernels for a precision of the descriptor.  FCN_PREC_BF16 ("bf16 operands AND bf16 storage of the big
// intermediates") keeps its bf16 STORAGE for the PointNet's per-entry tensors only: the FCN's activations are 1-9 k rows per layer
// and live in L2, so halving their bytes buys no memory time while every element pays a conversion on the way in and out --
// per launch (rocprofv3, round 6, profiles/r06_m_bf16_storage_by_kernel.txt) cgk_fwd 16.2 -> 19.8 us, cg_bwd_step 17.3 -> 25.8 us,
// cg_bwd_pair 28.5 -> 39.4 us with bf16 arenas, 164 us per step against the 70 us the PointNet kernels GAIN from theirs.  Here the
// mode therefore means bf16 operands over fp32 arenas (MM_BF16X1), exactly FCN_PREC_BF16_OPS; the y16 / st16 / out16 flags of the
// descriptors are inert without a half-width St<MM>.
#define CN_MM_OF(prec, fwd) ((prec) == FCN_PREC_BF16 ? MM_BF16X1 : FCN_MM_OF(prec, fwd))

struct CnPlan {
    int nlev, nl, heads;        // levels, layers in use (4*nlev - 2), id of the heads
    int KT[CN_NLAYER], stride[CN_NLAYER], pad[CN_NLAYER], Lin[CN_NLAYER], Lout[CN_NLAYER];
    int N[CN_NLAYER], Cs[CN_NLAYER], Ktot[CN_NLAYER], dk[CN_NLAYER];
    int nseg[CN_NLAYER], src[CN_NLAYER][CG_NSEG], C[CN_NLAYER][CG_NSEG], choff[CN_NLAYER][CG_NSEG];   // src: layer id, -1..-5 feats, -9 one-hot
    int cin_tot[CN_NLAYER], nrow_real[CN_NLAYER];
    int conv1[FCN_CN_MAXLEV + 1], conv2[FCN_CN_MAXLEV + 1], merge[FCN_CN_MAXLEV + 1], deconv[FCN_CN_MAXLEV + 1];   // ids by level (1-based)
};

static int conv_len(int L, int k, int s, int p) { return (L + 2 * p - k) / s + 1; }

// waves per backward workgroup (template parameter G of cg_bwd_*_kernel; CgB explains): four where the launches fill the machine
// (car: 8 960 rows at the first level, people: 22 400), eight where they do not (refine: 640, SUN-RGBD: 2 560)
#ifndef FCN_BWD_G4_ROWS
#define FCN_BWD_G4_ROWS 4096
#endif
static int cn_bwd_groups(const fcn_cn_desc *d) { return (int64_t)d->B * d->L[0] >= FCN_BWD_G4_ROWS ? 4 : 8; }

// rows per wgrad split (multiple of 32): ~768 workgroups, >= 256 rows each
static int pick_wrows(int R, int out_tiles)
{
#ifndef FCN_WG_TARGET
#define FCN_WG_TARGET 512      // (768 / 384 / 1024 re-swept in round 3: 1.387 / 1.384 / 1.393 ms per step against 1.380)
#endif
#ifndef FCN_WG_MINROWS
#define FCN_WG_MINROWS 256
#endif
    const int target = FCN_WG_TARGET, minrows = FCN_WG_MINROWS;      // swept on MI355X: fewer, fatter splits beat more partial traffic
    int ns = target / (out_tiles > 0 ? out_tiles : 1);
    if (ns > (R + minrows - 1) / minrows) ns = (R + minrows - 1) / minrows;
    if (ns < 1) ns = 1;
    int rows = (R + ns - 1) / ns;
    rows = (rows + 31) / 32 * 32;
    return rows;
}

static int cn_heads_width(const fcn_cn_desc *d) { return 2 + d->reg_out <= 64 ? 64 : 128; }

extern "C" int fcn_convnet_logits_ld(const fcn_cn_desc *d)
{
    if (!d || d->reg_out < 1 || 2 + d->reg_out > 128) return -1;
    return cn_heads_width(d);
}

static int cn_make_plan(const fcn_cn_desc *d, CnPlan &P)
{
    const int n = d->nlev ? d->nlev : 4;
    const int c1 = d->c1 ? d->c1 : 128;
    if (n != 4 && n != 5) return FCN_E_BADARG;
    if (c1 != 64 && c1 != 128) return FCN_E_BADARG;
    if (d->reg_out < 1 || 2 + d->reg_out > 128) return FCN_E_LIMIT;
    const int *Lv = d->L;                                   // Lv[j-1]: positions of level j
    for (int j = 1; j < n; ++j) {
        if (conv_len(Lv[j - 1], 3, 2, 1) != Lv[j]) return FCN_E_BADARG;
        if (j >= 2 && (Lv[j] << (j - 1)) < Lv[1]) return FCN_E_BADARG;      // the deconvolution output is cut to L2 positions
    }
    const int bw[FCN_CN_MAXLEV + 1] = {0, c1, 128, 256, 512, 512};          // block widths by level
    const int fc[FCN_CN_MAXLEV + 1] = {0, 128, 128, 256, 512, 512};         // pooled feature widths by level (PointNet C3)
    P.nlev = n; P.nl = 4 * n - 2; P.heads = 4 * n - 3;
    for (int l = 0; l < CN_NLAYER; ++l) {
        P.KT[l] = 1; P.stride[l] = 1; P.pad[l] = 0; P.Lin[l] = P.Lout[l] = 1; P.N[l] = P.Cs[l] = 64; P.nrow_real[l] = 0;
        P.dk[l] = 0; P.nseg[l] = 1; P.Ktot[l] = 0; P.cin_tot[l] = 0;
        for (int s = 0; s < CG_NSEG; ++s) { P.src[l][s] = 0; P.C[l][s] = 0; P.choff[l][s] = 0; }
    }
    auto conv = [&](int l, int kt, int st, int Li, int Lo, int width) {
        P.KT[l] = kt; P.stride[l] = st; P.pad[l] = kt == 3 ? 1 : 0; P.Lin[l] = Li; P.Lout[l] = Lo;
        P.N[l] = width; P.Cs[l] = width; P.nrow_real[l] = width;
    };
    // block1_conv1 over cat(feat1, one-hot)
    conv(0, 3, 1, Lv[0], Lv[0], c1);
    P.nseg[0] = 2; P.src[0][0] = -1; P.C[0][0] = fc[1]; P.src[0][1] = -9; P.C[0][1] = OH_PAD; P.choff[0][1] = fc[1];
    P.conv1[1] = P.conv2[1] = P.merge[1] = 0; P.deconv[1] = -1;
    for (int j = 2; j <= n; ++j) {
        const int base = 1 + 3 * (j - 2);
        P.conv1[j] = base; P.conv2[j] = base + 1; P.merge[j] = base + 2; P.deconv[j] = 3 * n - 2 + (j - 2);
        conv(base, 3, 2, Lv[j - 2], Lv[j - 1], bw[j]);
        P.src[base][0] = P.merge[j - 1]; P.C[base][0] = bw[j - 1];
        conv(base + 1, 3, 1, Lv[j - 1], Lv[j - 1], bw[j]);
        P.src[base + 1][0] = base; P.C[base + 1][0] = bw[j];
        conv(base + 2, 1, 1, Lv[j - 1], Lv[j - 1], bw[j]);          // merge over cat(x, feat_j, one-hot)
        P.nseg[base + 2] = 3;
        P.src[base + 2][0] = base + 1; P.C[base + 2][0] = bw[j];
        P.src[base + 2][1] = -j; P.C[base + 2][1] = fc[j]; P.choff[base + 2][1] = bw[j];
        P.src[base + 2][2] = -9; P.C[base + 2][2] = OH_PAD; P.choff[base + 2][2] = bw[j] + fc[j];
        // deconvolution (kernel = stride = 2^(j-2)): a GEMM over the input rows with N = k * 256
        const int l = P.deconv[j], k = 1 << (j - 2);
        P.KT[l] = 1; P.stride[l] = 1; P.pad[l] = 0; P.Lin[l] = Lv[j - 1]; P.Lout[l] = Lv[j - 1];
        P.N[l] = k * 256; P.Cs[l] = 256; P.dk[l] = k; P.nrow_real[l] = P.N[l];
        P.src[l][0] = base + 2; P.C[l][0] = bw[j];
    }
    // heads over cat(xx1, xx2[:L2], ...) -> 2 + reg_out columns, padded to 64 / 128
    const int h = P.heads;
    P.KT[h] = 1; P.stride[h] = 1; P.pad[h] = 0; P.Lin[h] = Lv[1]; P.Lout[h] = Lv[1];
    P.N[h] = P.Cs[h] = cn_heads_width(d);
    P.nrow_real[h] = 2 + d->reg_out; P.nseg[h] = n - 1;
    for (int s = 0; s < n - 1; ++s) { P.src[h][s] = P.deconv[2 + s]; P.C[h][s] = 256; P.choff[h][s] = 256 * s; }
    for (int l = 0; l < P.nl; ++l) {
        int cs = 0, ct = 0;
        for (int s = 0; s < P.nseg[l]; ++s) { cs += P.C[l][s]; ct += (P.src[l][s] == -9) ? d->nvec : P.C[l][s]; }
        P.Ktot[l] = P.KT[l] * cs;
        P.cin_tot[l] = ct;
        // LDS tables of the kernels: per-column BN scale/shift, per-chunk descriptors, BN-backward coefficients
        if (P.Ktot[l] > CG_KMAX || P.KT[l] * P.N[l] > CG_KBWD || P.Cs[l] > CG_CMAX || P.KT[l] > 3 || P.stride[l] > 2) return FCN_E_LIMIT;
        // the kernels address every arena with 32-bit BYTE offsets and divide row indices through a float reciprocal
        // (cg_divmod: exact below 2^23): rows of a layer, elements of its input / output / packed weights
        const int64_t rows = (int64_t)d->B * (P.Lout[l] > P.Lin[l] ? P.Lout[l] : P.Lin[l]);
        if (rows >= ((int64_t)1 << 23) || rows * (P.N[l] > cs ? P.N[l] : cs) >= ((int64_t)1 << 30) ||
            (int64_t)P.N[l] * P.Ktot[l] >= ((int64_t)1 << 30)) return FCN_E_LIMIT;
    }
    return 0;
}

// element offsets of each layer inside the shared workspaces
struct CnOffsets {
    int64_t y[CN_NLAYER + 1], wp[CN_NLAYER + 1];
    int bn[CN_NLAYER + 1], st[CN_NLAYER + 1], coef[CN_NLAYER + 1];
};

static void cn_offsets(const fcn_cn_desc *d, const CnPlan &P, CnOffsets &O)
{
    O.y[0] = O.wp[0] = 0; O.bn[0] = O.st[0] = O.coef[0] = 0;
    for (int l = 0; l < P.nl; ++l) {
        O.y[l + 1] = O.y[l] + (int64_t)d->B * P.Lout[l] * P.N[l];
        O.wp[l + 1] = O.wp[l] + (int64_t)P.N[l] * P.Ktot[l];
        O.bn[l + 1] = O.bn[l] + 4 * P.Cs[l];
        O.st[l + 1] = O.st[l] + 2 * P.Cs[l];
        O.coef[l + 1] = O.coef[l] + 5 * P.Cs[l];
    }
}

static int64_t cn_partial_elems(const fcn_cn_desc *d, const CnPlan &P);

extern "C" int fcn_convnet_sizes(const fcn_cn_desc *d, int64_t *out6)
{
    if (!d || !out6) return FCN_E_BADARG;
    CnPlan P;
    FCN_TRY(cn_make_plan(d, P));
    CnOffsets O;
    cn_offsets(d, P, O);
    const int64_t pmax = 4 * cn_partial_elems(d, P);   // (launch parity) x (chain / off-chain step): a step's reduce runs
                                                       // beside the next launch's weight gradients
    out6[0] = O.y[P.nl];      // floats: y (and dz) of all layers
    out6[1] = 3 * O.wp[P.nl]; // floats: packed weights (N, Ktot) of all layers, their split-encoded forward images, their data-gradient images
    out6[2] = O.bn[P.nl];     // floats: bn scale/shift/mean/rstd
    out6[3] = (int64_t)FCN_CG_REP * O.st[P.nl];     // doubles: stat (and bstat), FCN_CG_REP replica blocks each
    out6[4] = O.coef[P.nl];   // floats: coef
    out6[5] = pmax;                // floats: wgrad partials
    return 0;
}

static void cn_fill_layer(const fcn_cn_desc *d, const fcn_cn_params *p, const CnPlan &P, const CnOffsets &O,
                          const fcn_cn_ws *ws, const float *const *feats, const float *one_hot, int l, CgLayer &L)
{
    L.nseg = P.nseg[l]; L.KT = P.KT[l]; L.stride = P.stride[l]; L.pad = P.pad[l];
    L.Lin = P.Lin[l]; L.Lout = P.Lout[l]; L.B = d->B; L.Cout = P.N[l]; L.Ktot = P.Ktot[l]; L.Cs = P.Cs[l];
    L.Wp = ws->wp + O.wp[l]; L.Wenc = (const u32x4 *)(ws->wp + O.wp[P.nl] + O.wp[l]);
    L.Wgrd = (const u32x4 *)(ws->wp + 2 * O.wp[P.nl] + O.wp[l]); L.bias = nullptr; L.nbias = 0; L.y = ws->y + O.y[l]; L.y16 = 1; L.stat = nullptr; L.flags = ws->flags;
    L.eps = d->eps; L.momentum = d->momentum; L.rep_stride = O.st[P.nl];
    for (int s = 0; s < CG_NSEG; ++s) {
        CgSeg &S = L.seg[s];
        S.x = nullptr; S.bn = nullptr; S.C = P.C[l][s]; S.Lsrc = P.Lin[l]; S.type = 0; S.nvec = 0; S.st16 = 0;
        S.stat = nullptr; S.gamma = S.beta = nullptr; S.rmean = S.rvar = nullptr; S.nbt = nullptr; S.M = 1.0; S.writer = 0;
        if (s >= P.nseg[l]) continue;
        const int src = P.src[l][s];
        if (src == -9) { S.type = 1; S.x = ws->oh64; S.nvec = d->nvec; S.Lsrc = 1; }
        else if (src < 0) { S.x = feats[-src - 1]; S.Lsrc = d->L[-src - 1]; }
        else {
            S.x = ws->y + O.y[src]; S.bn = ws->bn + O.bn[src]; S.st16 = 1;
            S.Lsrc = P.Lout[src] * (P.dk[src] > 0 ? P.dk[src] : 1);     // a deconv's buffer is (B, L*k, 256)
            S.stat = uses_batch_stats(d) ? ws->stat + O.st[src] : nullptr;
            S.gamma = p->gamma[src]; S.beta = p->beta[src]; S.rmean = p->running_mean[src]; S.rvar = p->running_var[src];
            S.nbt = p->num_batches_tracked[src];
            S.M = (double)d->B * P.Lout[src] * (P.dk[src] > 0 ? P.dk[src] : 1);
        }
    }
}

static void cn_fill_pack(const fcn_cn_desc *d, const CnPlan &P, int l, CgPack &p)
{
    p.N = P.N[l]; p.Ktot = P.Ktot[l]; p.KT = P.KT[l]; p.nseg = P.nseg[l];
    for (int s = 0; s < CG_NSEG; ++s) { p.C[s] = P.C[l][s]; p.choff[s] = P.choff[l][s]; p.type[s] = (P.src[l][s] == -9) ? 1 : 0; }
    p.nvec = d->nvec; p.cin_tot = P.cin_tot[l]; p.deconv_k = P.dk[l]; p.cout_t = 256;
}

// all weights -> packed (N, Ktot) layout in one launch (heads: rows 0..1 cls_out, 2.. reg_out); one-hot -> (B, 64)
static int cn_pack(const fcn_cn_desc *d, const fcn_cn_params *p, const CnPlan &P, const CnOffsets &O, const fcn_cn_ws *ws,
                   const float *one_hot, hipStream_t st)
{
    CgPackAll t;
    t.pre[0] = 0;
    for (int l = 0; l < P.nl; ++l) {
        cn_fill_pack(d, P, l, t.p[l]);
        t.src[l] = p->W[l]; t.dst[l] = ws->wp + O.wp[l];
        t.pre[l + 1] = t.pre[l] + (int64_t)P.N[l] * P.Ktot[l];
        t.nrow_real[l] = P.nrow_real[l];
    }
    for (int l = P.nl; l < CN_NLAYER; ++l) {            // unused slots: empty ranges
        cn_fill_pack(d, P, 0, t.p[l]);
        t.src[l] = nullptr; t.dst[l] = nullptr; t.pre[l + 1] = t.pre[l]; t.nrow_real[l] = 0;
    }
    t.oh = one_hot; t.oh64 = ws->oh64; t.B = d->B; t.nvec = d->nvec;
    t.z0 = uses_batch_stats(d) ? ws->stat : nullptr; t.z1 = saves_for_backward(d) ? ws->bstat : nullptr; t.nz = FCN_CG_REP * O.st[P.nl];
    t.enc = ws->wp + O.wp[P.nl];            // second third of the weight arena (fcn_convnet_sizes)
    t.mmf = CN_MM_OF(d->precision, true);
    t.grd = saves_for_backward(d) ? ws->wp + 2 * O.wp[P.nl] : nullptr;      // third third: only a backward reads it
    t.mmb = CN_MM_OF(d->precision, false);
    hipLaunchKernelGGL(cg_pack_kernel,
                       dim3((unsigned)(((t.grd ? 2 : 1) * (t.pre[CN_NLAYER] / 8) + (int64_t)d->B * OH_PAD + t.nz + 255) / 256)),
                       dim3(256), 0, st, t);
    FCN_CHECK_LAUNCH();
    return 0;
}

// The packing depends on the weights and the one-hot vector only: a caller may run it early on another stream (beside
// the PointNet scales) and then call fcn_convnet_forward with d->prepacked = 1 once that stream is joined.
extern "C" int fcn_convnet_pack(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws, const float *one_hot,
                                void *stream)
{
    if (!d || !p || !ws || !ws->wp || !ws->oh64 || !bn_mode_valid(d)) return FCN_E_BADARG;
    if (d->nvec > 0 && !one_hot) return FCN_E_BADARG;
    if (d->nvec > OH_PAD) return FCN_E_LIMIT;
    CnPlan P;
    FCN_TRY(cn_make_plan(d, P));
    CnOffsets O;
    cn_offsets(d, P, O);
    return cn_pack(d, p, P, O, ws, one_hot, (hipStream_t)stream);
}

extern "C" int fcn_convnet_forward2(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                                    const float *const feats[FCN_CN_MAXLEV], const float *one_hot, float *logits,
                                    void *stream, void *const *feat_events);

extern "C" int fcn_convnet_forward(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                                   const float *const feats[FCN_CN_MAXLEV], const float *one_hot, float *logits,
                                   void *stream)
{
    return fcn_convnet_forward2(d, p, ws, feats, one_hot, logits, stream, nullptr);
}

// feat_events: nlev hipEvent_t (or NULL entries), recorded by the caller when pooled feature map s is complete on whatever
// stream produced it.  `stream` waits for event s right before the FIRST layer that reads map s (block1_conv1,
// block{j}_merge): the FCN starts as soon as the finest scale is pooled and its first layers run beside the widest
// scale's PointNet (the long pole of the forward), instead of after all scales.
extern "C" int fcn_convnet_forward2(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                                    const float *const feats[FCN_CN_MAXLEV], const float *one_hot, float *logits,
                                    void *stream, void *const *feat_events)
{
    if (!d || !p || !ws || !feats || !logits || !bn_mode_valid(d)) return FCN_E_BADARG;
    if (!ws->y || !ws->wp || !ws->bn || !ws->stat || !ws->partial || !ws->oh64) return FCN_E_BADARG;
    if (d->nvec > 0 && !one_hot) return FCN_E_BADARG;
    if (d->nvec > OH_PAD) return FCN_E_LIMIT;
    hipStream_t st = (hipStream_t)stream;
    CnPlan P;
    FCN_TRY(cn_make_plan(d, P));
    CnOffsets O;
    cn_offsets(d, P, O);
    const int tr = uses_batch_stats(d) ? 1 : 0;          // (frozen statistics: no batch sums, no running-stat update)
    if (d->precision < 0 || d->precision > FCN_PREC_BF16_OPS) return FCN_E_BADARG;
    const int mmf = CN_MM_OF(d->precision, true);
    if (!d->prepacked) FCN_TRY(cn_pack(d, p, P, O, ws, one_hot, st));      // (also zeroes ws->stat / ws->bstat)
    // launches in dependency order; block{j}_conv1 and block{j-1}_deconv (j >= 3) are pairs of independent layers reading
    // the same merge output and share a launch (n = 4: {4, 10} and {7, 11})
    int order[CN_NLAYER], norder = 0;
    bool pair_head[CN_NLAYER];
    for (int l = 0; l < CN_NLAYER; ++l) pair_head[l] = false;
    order[norder++] = 0;
    for (int j = 2; j <= P.nlev; ++j) {
        order[norder++] = P.conv1[j];
        if (j >= 3) { pair_head[P.conv1[j]] = true; order[norder++] = P.deconv[j - 1]; }
        order[norder++] = P.conv2[j];
        order[norder++] = P.merge[j];
    }
    order[norder++] = P.deconv[P.nlev];
    order[norder++] = P.heads;
    bool published[CN_NLAYER];
    for (int l = 0; l < CN_NLAYER; ++l) published[l] = false;
    bool waited[FCN_CN_MAXLEV] = {false, false, false, false, false};
    auto prep = [&](int l, CgLayer &L) -> int {
        cn_fill_layer(d, p, P, O, ws, feats, one_hot, l, L);
        for (int s = 0; s < P.nseg[l]; ++s) {       // the first consumer of a BN layer publishes its statistics
            const int src = P.src[l][s];
            if (src >= 0 && !published[src]) { L.seg[s].writer = 1; published[src] = true; }
            if (src < 0 && src != -9 && feat_events && feat_events[-src - 1] && !waited[-src - 1]) {
                hipError_t e = hipStreamWaitEvent(st, (hipEvent_t)feat_events[-src - 1], 0);
                if (e != hipSuccess) return (int)e;
                waited[-src - 1] = true;
            }
        }
        if (l == P.heads) { L.y = logits; L.y16 = 0; L.bias = p->bias; L.nbias = P.nrow_real[l]; }
        else if (tr) L.stat = ws->stat + O.st[l];
        return 0;
    };
    // (the early batch sums only in TRAINING launches: an eval forward reads running statistics and would only pay for the bigger
    // entry batch -- 57.5 -> 56.6 k frustums/s of inference with them, session x)
#define CN_FWD_LAUNCH(KERNEL, NTW_, GRID, BLOCK, ARG)                                                                 \
    if (tr) { FCN_MM_SWITCH(mmf, hipLaunchKernelGGL((KERNEL<MM, FCN_FT_MW, FCN_FT_G, FCN_FT_WNC, NTW_, FCN_FWD_EARLY_BN>), GRID, BLOCK, 0, st, ARG)); } \
    else { FCN_MM_SWITCH(mmf, hipLaunchKernelGGL((KERNEL<MM, FCN_FT_MW, FCN_FT_G, FCN_FT_WNC, NTW_, 0>), GRID, BLOCK, 0, st, ARG)); }
    // 32 x 32 tiles: 560 workgroups of 4 waves (2-3 resident per CU) instead of 280 of 8 (every level of the pyramid has
    // B*L*N/2048 = 280 tiles of 32 x 64 for 256 CUs); measured 369 -> 352 us over the forward
    for (int q = 0; q < norder; ++q) {
        const int l = order[q];
        const int R = d->B * P.Lout[l];
        const bool pair = pair_head[l] && q + 1 < norder;
        if (pair) {
            const int l2 = order[q + 1];
            CgLayerPair pp;
            FCN_TRY(prep(l, pp.A));
            FCN_TRY(prep(l2, pp.B));
            const int R2 = d->B * P.Lout[l2];
            constexpr int TR = 32 * FCN_FT_MW, TCW = 32 * FCN_FT_WNC * FCN_FT_NTW;
            if (FCN_FT_NTW > 1 && P.N[l] % TCW == 0 && P.N[l2] % TCW == 0) {
                pp.na = cg_pad8(((R + TR - 1) / TR) * (P.N[l] / TCW));
                const int nb = cg_pad8(((R2 + TR - 1) / TR) * (P.N[l2] / TCW));
                CN_FWD_LAUNCH(cgk_fwd_pair_kernel, FCN_FT_NTW, dim3(pp.na + nb), dim3(FCN_FT_THREADS), pp);
            } else {
                constexpr int TC = 32 * FCN_FT_WNC;
                pp.na = cg_pad8(((R + TR - 1) / TR) * (P.N[l] / TC));
                const int nb = cg_pad8(((R2 + TR - 1) / TR) * (P.N[l2] / TC));
                CN_FWD_LAUNCH(cgk_fwd_pair_kernel, 1, dim3(pp.na + nb), dim3(FCN_FT_THREADS), pp);
            }
            FCN_CHECK_LAUNCH();
            ++q;
        } else {
            CgLayer L;
            FCN_TRY(prep(l, L));
            constexpr int TR = 32 * FCN_FT_MW, TCW = 32 * FCN_FT_WNC * FCN_FT_NTW;
            if (FCN_FT_NTW > 1 && P.N[l] % TCW == 0) {
                CN_FWD_LAUNCH(cgk_fwd_kernel, FCN_FT_NTW, dim3(cg_pad8(((R + TR - 1) / TR) * (P.N[l] / TCW))), dim3(FCN_FT_THREADS), L);
            } else {
                constexpr int TC = 32 * FCN_FT_WNC;
                CN_FWD_LAUNCH(cgk_fwd_kernel, 1, dim3(cg_pad8(((R + TR - 1) / TR) * (P.N[l] / TC))), dim3(FCN_FT_THREADS), L);
            }
            FCN_CHECK_LAUNCH();
        }
    }
    return 0;
}

// rows per wgrad split for the fused step kernel and the resulting split count
static void cn_wgrad_split(int R, int out_tiles, int &rows, int &ns)
{
    rows = pick_wrows(R, out_tiles);
    if (rows < 2 * KC) rows = 2 * KC;                   // both halves of a workgroup get a chunk
    ns = (R + rows - 1) / rows;
}

static int64_t cn_partial_elems(const fcn_cn_desc *d, const CnPlan &P)
{
    int64_t pmax = 0;
    for (int l = 0; l < P.nl; ++l) {
        int rows, ns;
        cn_wgrad_split(d->B * P.Lout[l], (P.N[l] / 64) * (P.Ktot[l] / 64), rows, ns);
        const int64_t v = (int64_t)ns * P.N[l] * P.Ktot[l];
        if (v > pmax) pmax = v;
    }
    return pmax;
}

extern "C" int fcn_convnet_backward(const fcn_cn_desc *d, const fcn_cn_params *p, const fcn_cn_ws *ws,
                                    const float *const feats[FCN_CN_MAXLEV], const float *one_hot, const float *dlogits,
                                    float *const dfeats[FCN_CN_MAXLEV], float *const dW[CN_NLAYER],
                                    float *const dgamma[CN_NLAYER], float *const dbeta[CN_NLAYER], float *dbias,
                                    void *stream, void *stream2, void *const *events)
{
    if (!d || !p || !ws || !feats || !dlogits || !dfeats || !dW || !dgamma || !dbeta || !dbias) return FCN_E_BADARG;
    if (!bn_mode_valid(d) || !saves_for_backward(d)) return FCN_E_BADARG;
    if (!ws->y || !ws->dz || !ws->wp || !ws->bn || !ws->bstat || !ws->coef || !ws->partial) return FCN_E_BADARG;
    // stream2 / events (nlev caller-owned hipEvent_t), optional: the gradient of the widest feature map (dfeats[nlev-1]) is
    // final after the third launch (heads, last deconvolution, last merge).  From there the remaining launches continue
    // on stream2 so that `stream` is free again: the caller's widest PointNet backward -- the long pole -- starts beside
    // the rest of the FCN backward instead of after it.  events[0]: fork; events[k]: dfeats[nlev-1-k] final (after
    // block{nlev-k}_merge), k = 1..nlev-2; events[nlev-1]: everything final (dfeats[0], all dW).
    const bool cont = stream2 != nullptr && events != nullptr;
    hipStream_t st = (hipStream_t)stream;
    if (d->precision < 0 || d->precision > FCN_PREC_BF16_OPS) return FCN_E_BADARG;
    const int mmb = CN_MM_OF(d->precision, false);
    CnPlan P;
    FCN_TRY(cn_make_plan(d, P));
    CnOffsets O;
    cn_offsets(d, P, O);
    hipError_t e = hipSuccess;          // ws->bstat was zeroed by the packing launch of this forward (cn_pack)
    const int64_t pquart = cn_partial_elems(d, P);      // ws->partial holds four: (launch parity) x (chain / off-chain step)

    // consumers still to come for each producer layer (to know which dgrad is the last one)
    int pending[CN_NLAYER];
    for (int l = 0; l < CN_NLAYER; ++l) pending[l] = 0;
    for (int l = 0; l < P.nl; ++l)
        for (int s = 0; s < P.nseg[l]; ++s)
            if (P.src[l][s] >= 0) pending[P.src[l][s]] += 1;
    int seen[CN_NLAYER];
    for (int l = 0; l < CN_NLAYER; ++l) seen[l] = 0;

    auto blank_reduce = [&](CgReduce &r) {
        r.partial = nullptr; r.nsplit = 0; r.nrow_real = 0; r.dW = nullptr; r.gr = 1; cn_fill_pack(d, P, 0, r.pk);
    };
    const int BG = cn_bwd_groups(d);           // waves per backward workgroup (4 or 8): one choice for the whole chain
    // data-gradient + weight-gradient roles of layer l (l < 0: none); returns the workgroups in front of the reduce role
    auto make_step = [&](int l, float *pbuf, CgBwdStep &a, CgReduce &own, int &own_blocks) -> int {
        a.ndg = 0; a.w_ns = 0; a.w_ny = 1; a.rows = 2 * KC; a.partial = nullptr; a.dz = nullptr; a.dz16 = 0;
        a.cb.bstat = nullptr; a.cb.rep_stride = O.st[P.nl]; a.cb.frozen = frozen_stats(d) ? 1 : 0; a.cb.gamma = nullptr; a.cb.bn = nullptr; a.cb.M = 1.0; a.cb.dgamma = nullptr; a.cb.dbeta = nullptr;
        CgDgSeg *dgs[CG_NSEG] = {&a.dg[0], &a.dg[1], &a.dg[2], &a.dg[3]};
        for (int s = 0; s < CG_NSEG; ++s) {
            dgs[s]->sg = 0; dgs[s]->segoff = 0; dgs[s]->ysrc = dgs[s]->bnsrc = nullptr; dgs[s]->out = nullptr;
            dgs[s]->accumulate = 0; dgs[s]->out16 = 0; dgs[s]->bstat_src = nullptr; dgs[s]->tx = 1; dgs[s]->ncb = 1; dgs[s]->blk0 = 0;
            dgs[s]->wave_tiles = 0;
        }
        blank_reduce(own);
        own_blocks = 0;
        int nblk = 0;
        if (l < 0) {
            cn_fill_layer(d, p, P, O, ws, feats, one_hot, 0, a.lay);      // unused by a reduce-only step
            a.w_blk0 = 0;
            return 0;
        }
        cn_fill_layer(d, p, P, O, ws, feats, one_hot, l, a.lay);
        const int R = d->B * P.Lout[l];
        a.dz = (l == P.heads) ? dlogits : ws->dz + O.y[l];
        a.dz16 = (l == P.heads) ? 0 : 1;
        if (l == P.heads) {
            a.lay.y = nullptr;
        } else {
            a.cb.bstat = ws->bstat + O.st[l]; a.cb.gamma = p->gamma[l]; a.cb.bn = ws->bn + O.bn[l];
            a.cb.M = (double)R * (P.dk[l] > 0 ? P.dk[l] : 1);
            a.cb.dgamma = dgamma[l]; a.cb.dbeta = dbeta[l];      // exported by workgroup 0 (a data-gradient tile)
        }
        int segoff = 0;
        for (int s = 0; s < P.nseg[l]; ++s) {       // data gradients into every non-constant source
            const int src = P.src[l][s];
            if (src != -9) {
                CgDgSeg &g = *dgs[a.ndg];
                g.sg = s; g.segoff = segoff;
                if (src >= 0) {
                    g.ysrc = ws->y + O.y[src]; g.bnsrc = ws->bn + O.bn[src]; g.out = ws->dz + O.y[src]; g.out16 = 1;
                    g.accumulate = seen[src] > 0 ? 1 : 0;
                    seen[src] += 1;
                    g.bstat_src = (seen[src] == pending[src]) ? ws->bstat + O.st[src] : nullptr;
                } else {
                    g.out = dfeats[-src - 1]; g.out16 = 0;
                }
                const int Rs = d->B * a.lay.seg[s].Lsrc;
                g.tx = (Rs + 31) / 32;
                g.ncb = P.C[l][s] / 64;
                g.blk0 = nblk;
#if (FCN_EXP & 8)       // timing experiment (tools build, wrong gradients): one data-gradient tile per segment only
                g.tx = 1; g.ncb = 1;
#endif
#ifndef FCN_NO_WAVE_TILES
                g.wave_tiles = (P.KT[l] * (P.N[l] / CGB_KH) <= CGB_ROWS_MAXCH) ? 1 : 0;       // (chunks of the reduction: KT * Cout / 16)
#endif
                nblk += cg_pad8(g.wave_tiles ? (g.tx * g.ncb + BG - 1) / BG : g.tx * g.ncb);
                a.ndg += 1;
            }
            segoff += P.KT[l] * P.C[l][s];
        }
        a.w_blk0 = nblk;                            // weight-gradient partials of this layer
        a.partial = pbuf;
        a.w_ny = P.N[l] / 64;
        cn_wgrad_split(R, a.w_ny * (P.Ktot[l] / 64), a.rows, a.w_ns);
#if (FCN_EXP & 4)       // timing experiment (tools build, wrong gradients): the chain without its weight-gradient roles
        a.w_ns = 0;
#endif
        nblk += cg_pad8(a.w_ns * a.w_ny * (P.Ktot[l] / 64));
        own.partial = a.partial; own.nsplit = a.w_ns; cn_fill_pack(d, P, l, own.pk); own.nrow_real = P.nrow_real[l];
        own.dW = dW[l];
        own.gr = a.w_ns >= 32 ? 8 : (a.w_ns >= 16 ? 4 : (a.w_ns >= 8 ? 2 : 1));
        own_blocks = (int)(((int64_t)P.N[l] * P.Ktot[l]) / (64 * BG / own.gr));
        return nblk;
    };

    // Launch plan: the chain heads, last deconvolution, then merge / conv2 / conv1 of every level downwards, block1_conv1
    // and a final reduce-only step (n = 4: 13 12 9 8 7 6 5 4 3 2 1 0 -1), with the off-chain deconvolution steps riding
    // along: block{j-1}_deconv beside block{j}_conv2 (n = 4: 11 beside 8, 10 beside 5) -- each BEFORE the chain step that
    // accumulates into the same gradient buffer (block{j}_conv1 -> dz[block{j-1}_merge]), never in the same launch.
    int chain[CN_NLAYER + 1], rider[CN_NLAYER + 1], nchain = 0;
    for (int k = 0; k <= CN_NLAYER; ++k) rider[k] = -1;
    chain[nchain++] = P.heads;
    chain[nchain++] = P.deconv[P.nlev];
    for (int j = P.nlev; j >= 2; --j) {
        chain[nchain++] = P.merge[j];
        if (j >= 3) rider[nchain] = P.deconv[j - 1];
        chain[nchain++] = P.conv2[j];
        chain[nchain++] = P.conv1[j];
    }
    chain[nchain++] = 0;
    chain[nchain++] = -1;
    CgReduce pendA, pendB;              // reduces that ride in the next launch
    int pendA_blocks = 0, pendB_blocks = 0;
    blank_reduce(pendA); blank_reduce(pendB);
    // the heads' bias gradient rides in the first launch, in the (still empty) reduce slot
    pendA.partial = dlogits; pendA.nsplit = P.N[P.heads]; pendA.pk.N = d->B * P.Lout[P.heads];
    pendA.nrow_real = P.nrow_real[P.heads];
    pendA.dW = dbias; pendA.gr = 0; pendA_blocks = P.N[P.heads];
    for (int k = 0; k < nchain; ++k) {
        CgBwdPair pp;
        CgReduce ownA, ownB;
        int ownA_blocks = 0, ownB_blocks = 0;
        float *bufA = ws->partial + ((k & 1) * 2 + 0) * pquart, *bufB = ws->partial + ((k & 1) * 2 + 1) * pquart;
        int nA = make_step(chain[k], bufA, pp.A, ownA, ownA_blocks);
        pp.A.r_blk0 = nA;
        if (pendA_blocks > 0) { pp.A.red = pendA; nA += pendA_blocks; } else blank_reduce(pp.A.red);
        const bool needB = rider[k] >= 0 || pendB_blocks > 0;
        int nB = 0;
        if (needB) {
            nB = make_step(rider[k], bufB, pp.B, ownB, ownB_blocks);
            pp.B.r_blk0 = nB;
            if (pendB_blocks > 0) { pp.B.red = pendB; nB += pendB_blocks; } else blank_reduce(pp.B.red);
        }
        pp.na = nA;
        if (nA + nB > 0) {
            if (BG == 4) {
                if (nB > 0) { FCN_MM_SWITCH(mmb, hipLaunchKernelGGL((cg_bwd_pair_kernel<MM, 4>), dim3(nA + nB), dim3(256), 0, st, pp)); }
                else { FCN_MM_SWITCH(mmb, hipLaunchKernelGGL((cg_bwd_step_kernel<MM, 4>), dim3(nA), dim3(256), 0, st, pp.A)); }
            } else {
                if (nB > 0) { FCN_MM_SWITCH(mmb, hipLaunchKernelGGL((cg_bwd_pair_kernel<MM, 8>), dim3(nA + nB), dim3(512), 0, st, pp)); }
                else { FCN_MM_SWITCH(mmb, hipLaunchKernelGGL((cg_bwd_step_kernel<MM, 8>), dim3(nA), dim3(512), 0, st, pp.A)); }
            }
            FCN_CHECK_LAUNCH();
        }
        pendA = ownA; pendA_blocks = ownA_blocks;
        pendB = ownB; pendB_blocks = ownB_blocks;
        if (cont) {
            const int l = chain[k];
            int ev = -1;
            if (l == -1) ev = P.nlev - 1;
            else for (int j = 2; j <= P.nlev; ++j) if (l == P.merge[j]) ev = P.nlev - j;
            if (ev >= 0) {
                e = hipEventRecord((hipEvent_t)events[ev], st);
                if (e != hipSuccess) return (int)e;
            }
            if (ev == 0) {              // hand the chain over to the continuation stream
                e = hipStreamWaitEvent((hipStream_t)stream2, (hipEvent_t)events[0], 0);
                if (e != hipSuccess) return (int)e;
                st = (hipStream_t)stream2;
            }
        }
    }
    return 0;
}
