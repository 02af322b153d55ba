// On-device construction of one training batch from raw frustum records: what the reference's data loader does per
// sample on the host in numpy (datasets/provider_sample.py::ProviderDataset.__getitem__ :137-262 with generate_ref
// :291-327, generate_labels :270-289, centre-view helpers :329-372; datasets/data_utils.py rotate_pc_along_y :7-21,
// compute_box_3d :44-70, project_image_to_rect :73-93) and collates into the dict PointNetDet.forward consumes.
// One workgroup per frustum; HBM/latency-bound gather + a few hundred fp64 operations -- no GEMM in sight.
//   points:  resample (indices drawn on the host: the reference's np.random.choice), rotate to the frustum's centre
//            view, optional x-flip and depth shift, written channel-major (B,3,N) with lanes along N
//   centres: arange(0, max_depth, stride) + stride/2 on the ray through the 2-D box centre (calibration P), rotated
//   labels:  +1 inside the half-size box, -1 inside the full box, nearest centre when none is inside the half box
// fp64 where numpy computes in fp64, rounded to fp32 exactly where the reference stores fp32.
// The same kernel serves the SUN-RGBD loader (datasets/provider_sample_sunrgbd.py::ProviderDataset.__getitem__ :116-263 with
// generate_ref :283-326 and project_image_to_upright_camera :28-59): five strides, window centres through the camera
// matrix K and the tilt rotation Rtilt instead of the KITTI projection P, and an extra height shift in the augmentation.
#include "fcn_common.h"
#include "../../include/fcn_hip.h"

#define INP_T 256

struct InpDescG {              // both entry points in one shape
    int B, N, pt_stride, nsc;
    int L[5];
    double stride[5], max_depth;
    int random_flip, random_shift;
};

struct InpArgs {
    InpDescG d;
    const float *raw;
    const int64_t *off, *raw_seg;
    const int32_t *choice;
    const double *fangle, *box2d, *P, *corners, *heading, *size, *coin, *normal;
    const double *K, *Rtilt;   // SUN-RGBD: (B,3,3) camera matrix and tilt rotation (P == nullptr then)
    const double *hshift;      // SUN-RGBD: the uniform [0,1) draw of the height shift (random_shift), else nullptr
    float *pc, *ref[5];
    int64_t *cls;
    float *center, *head, *osize, *rot;
    int64_t *seg;
};

__device__ __forceinline__ bool inp_in_box(double dx, double dy, double dz, double c, double s, double l, double w, double h)
{
    const double lx = c * dx - s * dz, lz = s * dx + c * dz;
    return fabs(lx) <= l / 2.0 && fabs(dy) <= h / 2.0 && fabs(lz) <= w / 2.0;
}

// ---- what the two kernels below share.  The first stage passes the origin 0 and the scales 0.5 / 1.0 where its text used to
// have no operation at all: x - 0.0 and x * 1.0 are x for every IEEE double (either zero keeps its sign, an infinity and a NaN
// stay what they are), so the bits are the ones of the unshared statements.
struct InpBox { double cx, cy, cz, ang, sl, sw, sh; };   // the label box in the sample's frame: centre, heading, size (l, w, h)

// A: InpArgs or InpRefineArgs -- the members the helpers read have the same names in both, and each is read where it is used.
// Label box of sample b: its centre (the mean of corners 0 and 6) relative to the origin o, rotated by rot (c, s = cos, sin);
// heading minus rot; the x-flip; the size as it came.
template <class A> __device__ __forceinline__ void inp_label_box(InpBox &k, const A &a, int b, double ox, double oy, double oz,
                                                                 double rot, double c, double s, bool flip)
{
    const double *cr = a.corners + (int64_t)b * 24;
    const double dx = (cr[0] + cr[18]) / 2.0 - ox, dy = (cr[1] + cr[19]) / 2.0 - oy, dz = (cr[2] + cr[20]) / 2.0 - oz;
    k.cx = dx * c + dz * (-s); k.cy = dy; k.cz = dx * s + dz * c;
    k.ang = a.heading[b] - rot;
    if (flip) { k.cx = -k.cx; k.ang = M_PI - k.ang; }
    k.sl = a.size[3 * b]; k.sw = a.size[3 * b + 1]; k.sh = a.size[3 * b + 2];
}

template <class A> __device__ __forceinline__ void inp_store_box(const InpBox &k, const A &a, int b)
{
    a.center[3 * b] = (float)k.cx; a.center[3 * b + 1] = (float)k.cy; a.center[3 * b + 2] = (float)k.cz;
    a.head[b] = (float)k.ang;
    a.osize[3 * b] = (float)k.sl; a.osize[3 * b + 1] = (float)k.sw; a.osize[3 * b + 2] = (float)k.sh;
}

// Window centre l of sample b's row of L labels, at (x, y, z): +1 inside the box scaled by f1, -1 inside the one scaled by f2, else 0; the thread's nearest centre
// so far (l ascends per thread: the first minimum is kept) and whether it has seen a positive.
template <class A> __device__ __forceinline__ void inp_classify(const A &a, int b, int L, int l, double x, double y, double z,
                                                                const InpBox &k, double ca, double sa, double f1, double f2,
                                                                bool &any1, double &best, int &bidx)
{
    const double dx = x - k.cx, dy = y - k.cy, dz = z - k.cz;
    const bool in1 = inp_in_box(dx, dy, dz, ca, sa, k.sl * f1, k.sw * f1, k.sh * f1);
    const bool in2 = inp_in_box(dx, dy, dz, ca, sa, k.sl * f2, k.sw * f2, k.sh * f2);
    a.cls[(int64_t)b * L + l] = in1 ? 1 : (in2 ? -1 : 0);
    any1 = any1 || in1;
    const double dd = sqrt(dx * dx + dy * dy + dz * dz);
    if (dd < best) { best = dd; bidx = l; }
}

// After the window loop, by every thread of the workgroup: when nobody saw a centre inside the inner box, the nearest centre is
// the positive (np.argmin: the first of equal minima).  *sany is zeroed, behind a barrier, before the loop.
template <class A> __device__ __forceinline__ void inp_nearest_positive(const A &a, int b, int L, double *sdist, int *sidx, int *sany,
                                                                        int tid, bool any1, double best, int bidx)
{
    if (any1) *sany = 1;
    sdist[tid] = best; sidx[tid] = bidx;
    __syncthreads();
    if (*sany) return;
    for (int o = INP_T / 2; o > 0; o >>= 1) {
        if (tid < o) {
            const double d2 = sdist[tid + o];
            const int i2 = sidx[tid + o];
            if (d2 < sdist[tid] || (d2 == sdist[tid] && i2 < sidx[tid])) { sdist[tid] = d2; sidx[tid] = i2; }
        }
        __syncthreads();
    }
    if (tid == 0 && sidx[0] != 0x7fffffff) a.cls[(int64_t)b * L + sidx[0]] = 1;
}

__global__ __launch_bounds__(INP_T) void prepare_inputs_kernel(InpArgs a)
{
    __shared__ double sdist[INP_T];
    __shared__ int sidx[INP_T];
    __shared__ int sany;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.d.N;
    // ---- per-frustum scalars (every thread computes the same values)
    const double rot = M_PI / 2.0 + a.fangle[b];
    const double c = cos(rot), s = sin(rot);
    // corners == nullptr: inference records (fcn_prepare_inputs_infer) -- no label box, so no flip, no shift and no label outputs
    const bool train = a.corners != nullptr;
    InpBox k = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const bool flip = train && a.d.random_flip && a.coin[b] > 0.5;
    if (train) inp_label_box(k, a, b, 0.0, 0.0, 0.0, rot, c, s, flip);
    const bool do_shift = train && a.d.random_shift;
    double shift = 0.0;
    if (do_shift) {
        const double dist = sqrt(k.sl * k.sl + k.sw * k.sw);
        shift = fmin(fmax(a.normal[b] * dist * 0.2, -0.5 * dist), 0.5 * dist);
        shift = fmin(fmax(shift + k.cz, 0.0), a.d.max_depth) - k.cz;
        k.cz += shift;
    }
    // provider_sample_sunrgbd.py:228-230: height_shift = np.random.random() * 0.4 - 0.2 on the points' y and the box centre
    const bool has_h = do_shift && a.hshift != nullptr;
    const double hsh = has_h ? a.hshift[b] * 0.4 - 0.2 : 0.0;
    if (has_h) k.cy += hsh;
    if (tid == 0) {
        if (train) inp_store_box(k, a, b);
        a.rot[b] = (float)rot;
    }
    // ---- points
    const int64_t o0 = a.off[b];
    const int ps = a.d.pt_stride;
    for (int i = tid; i < N; i += INP_T) {
        const int64_t j = o0 + a.choice[(int64_t)b * N + i];
        const float *p = a.raw + j * ps;
        const double x = p[0], z = p[2];
        float xr = (float)(x * c + z * (-s));              // the reference stores the rotated record back as float32
        float zr = (float)(x * s + z * c);
        if (flip) xr = -xr;
        if (do_shift) zr = (float)((double)zr + shift);
        float yr = p[1];
        if (has_h) yr = (float)((double)yr + hsh);         // float32 record += float64 scalar
        float *o = a.pc + (int64_t)b * 3 * N;
        o[i] = xr; o[N + i] = yr; o[2 * N + i] = zr;
        if (a.seg) a.seg[(int64_t)b * N + i] = a.raw_seg[j];
    }
    // ---- frustum centres of the strides, labels on stride 2
    const bool upright = a.P == nullptr;
    double cu, cv, fu, fv, bx = 0.0, by = 0.0;
    double Rt[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (!upright) {
        const double *P = a.P + (int64_t)b * 12;
        cu = P[2]; cv = P[6]; fu = P[0]; fv = P[5];
        bx = P[3] / (-fu); by = P[7] / (-fv);
    } else {
        const double *K = a.K + (int64_t)b * 9;
        cu = K[2]; cv = K[5]; fu = K[0]; fv = K[4];
        for (int i = 0; i < 9; ++i) Rt[i] = a.Rtilt[(int64_t)b * 9 + i];
    }
    const double u0 = (a.box2d[4 * b] + a.box2d[4 * b + 2]) / 2.0, v0 = (a.box2d[4 * b + 1] + a.box2d[4 * b + 3]) / 2.0;
    const double ca = cos(k.ang), sa = sin(k.ang);
    double best = 1e300;
    int bidx = 0x7fffffff;
    bool any1 = false;
    if (tid == 0) sany = 0;
    __syncthreads();
#pragma unroll 1
    for (int sc = 0; sc < a.d.nsc; ++sc) {
        const int L = a.d.L[sc];
        const double st = a.d.stride[sc];
        for (int l = tid; l < L; l += INP_T) {
            const double zd = (double)l * st + st / 2.0;
            double x = ((u0 - cu) * zd) / fu + bx, y = ((v0 - cv) * zd) / fv + by, z = zd;
            if (upright) {
                // project_image_to_upright_camera (provider_sample_sunrgbd.py:44-59): camera (x, y, z) -> depth frame
                // (x, z, -y) -> Rtilt . -> (X, -Z, Y)
                const double d0 = x, d1 = zd, d2 = -y;
                const double u_0 = Rt[0] * d0 + Rt[1] * d1 + Rt[2] * d2;
                const double u_1 = Rt[3] * d0 + Rt[4] * d1 + Rt[5] * d2;
                const double u_2 = Rt[6] * d0 + Rt[7] * d1 + Rt[8] * d2;
                x = u_0; y = -u_2; z = u_1;
            }
            double xr = x * c + z * (-s);
            const double zr = x * s + z * c;
            if (flip) xr = -xr;
            float *o = a.ref[sc] + (int64_t)b * 3 * L;
            o[l] = (float)xr; o[L + l] = (float)y; o[2 * L + l] = (float)zr;
            if (sc == 1 && a.cls)                              // the half-size box is the positive, the full box the ignore region
                inp_classify(a, b, L, l, xr, y, zr, k, ca, sa, 0.5, 1.0, any1, best, bidx);
        }
    }
    if (!a.cls) return;
    inp_nearest_positive(a, b, a.d.L[1], sdist, sidx, &sany, tid, any1, best, bidx);
}

// Every scale of a descriptor has windows, a positive stride (a NaN is refused) and an output.
static bool inp_scales_ok(int nsc, const int32_t *L, const double *stride, float *const *center_ref)
{
    for (int s = 0; s < nsc; ++s)
        if (L[s] <= 0 || !(stride[s] > 0.0) || !center_ref[s]) return false;
    return true;
}

template <class D> static InpDescG inp_view(const D *d, int nsc)      // fcn_inp_desc / fcn_inp5_desc in the kernel's one shape
{
    InpDescG v = {d->B, d->N, d->pt_stride, nsc, {0, 0, 0, 0, 0}, {1.0, 1.0, 1.0, 1.0, 1.0}, d->max_depth, d->random_flip, d->random_shift};
    for (int s = 0; s < nsc; ++s) { v.L[s] = d->L[s]; v.stride[s] = d->stride[s]; }
    return v;
}

// The checks and the launch of the four first-stage entries below.  The calibration is P, or K and Rtilt with P == nullptr.
// labels: the entry takes a label box -- corners, heading, size and the three box outputs are required then, coin / normal where the
// descriptor asks for flip / shift, raw_seg beside seg_label; cls_label and seg_label stay optional.  Without, the entry passes
// nullptr for all of them.
static int inp_first_stage(const InpDescG &v, bool labels, const float *raw_pts, const int64_t *pt_off, const int64_t *raw_seg,
                           const int32_t *choice, const double *frustum_angle, const double *box2d, const double *P, const double *K,
                           const double *Rtilt, const double *box3d_corners, const double *heading, const double *size,
                           const double *coin, const double *normal, const double *hshift, float *point_cloud,
                           float *const *center_ref, int64_t *cls_label, float *box3d_center, float *box3d_heading,
                           float *box3d_size, float *rot_angle, int64_t *seg_label, void *stream)
{
    if (!raw_pts || !pt_off || !choice || !frustum_angle || !box2d || !(P || (K && Rtilt)) || !point_cloud || !center_ref || !rot_angle)
        return FCN_E_BADARG;
    if (labels && (!box3d_corners || !heading || !size || !box3d_center || !box3d_heading || !box3d_size)) return FCN_E_BADARG;
    if (v.B <= 0 || v.N <= 0 || v.pt_stride < 3) return FCN_E_BADARG;
    if ((v.random_flip && !coin) || (v.random_shift && !normal) || (seg_label && !raw_seg)) return FCN_E_BADARG;
    if (!inp_scales_ok(v.nsc, v.L, v.stride, center_ref)) return FCN_E_BADARG;
    InpArgs a;
    a.d = v; a.raw = raw_pts; a.off = pt_off; a.raw_seg = raw_seg; a.choice = choice; a.fangle = frustum_angle; a.box2d = box2d;
    a.P = P; a.K = K; a.Rtilt = Rtilt; a.corners = box3d_corners; a.heading = heading; a.size = size; a.coin = coin;
    a.normal = normal; a.hshift = hshift; a.pc = point_cloud; a.cls = cls_label; a.center = box3d_center; a.head = box3d_heading;
    a.osize = box3d_size; a.rot = rot_angle; a.seg = seg_label;
    for (int s = 0; s < 5; ++s) a.ref[s] = s < v.nsc ? center_ref[s] : nullptr;
    hipLaunchKernelGGL(prepare_inputs_kernel, dim3(v.B), dim3(INP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

extern "C" int fcn_prepare_inputs(const fcn_inp_desc *d, const float *raw_pts, const int64_t *pt_off, const int64_t *raw_seg,
                                  const int32_t *choice, const double *frustum_angle, const double *box2d, const double *P,
                                  const double *box3d_corners, const double *heading, const double *size,
                                  const double *coin, const double *normal, float *point_cloud, float *const center_ref[4],
                                  int64_t *cls_label, float *box3d_center, float *box3d_heading, float *box3d_size,
                                  float *rot_angle, int64_t *seg_label, void *stream)
{
    if (!d) return FCN_E_BADARG;
    return inp_first_stage(inp_view(d, 4), true, raw_pts, pt_off, raw_seg, choice, frustum_angle, box2d, P, nullptr, nullptr,
                           box3d_corners, heading, size, coin, normal, nullptr, point_cloud, center_ref, cls_label, box3d_center,
                           box3d_heading, box3d_size, rot_angle, seg_label, stream);
}

// Inference records of the first stage (datasets/provider_sample.py:184-195, from_rgb_detection): no label box in, no labels out,
// no augmentation -- point_cloud, center_ref[4] and rot_angle alone.  The same kernel with corners == nullptr.
extern "C" int fcn_prepare_inputs_infer(const fcn_inp_desc *d, const float *raw_pts, const int64_t *pt_off, const int32_t *choice,
                                        const double *frustum_angle, const double *box2d, const double *P, float *point_cloud,
                                        float *const center_ref[4], float *rot_angle, void *stream)
{
    if (!d || d->random_flip || d->random_shift) return FCN_E_BADARG;
    return inp_first_stage(inp_view(d, 4), false, raw_pts, pt_off, nullptr, choice, frustum_angle, box2d, P, nullptr, nullptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, point_cloud, center_ref, nullptr, nullptr, nullptr,
                           nullptr, rot_angle, nullptr, stream);
}

// SUN-RGBD loader (cfgs/det_sample_sunrgbd.yaml; datasets/provider_sample_sunrgbd.py:116-326): five strides, centres through
// K and Rtilt, depth + height shift (the kernel applies the latter where it is handed hshift).
extern "C" int fcn_prepare_inputs_sunrgbd(const fcn_inp5_desc *d, const float *raw_pts, const int64_t *pt_off,
                                          const int64_t *raw_seg, const int32_t *choice, const double *frustum_angle,
                                          const double *box2d, const double *K, const double *Rtilt,
                                          const double *box3d_corners, const double *heading, const double *size,
                                          const double *coin, const double *normal, const double *hshift,
                                          float *point_cloud, float *const center_ref[5], int64_t *cls_label,
                                          float *box3d_center, float *box3d_heading, float *box3d_size, float *rot_angle,
                                          int64_t *seg_label, void *stream)
{
    if (!d || (d->random_shift && !hshift)) return FCN_E_BADARG;
    return inp_first_stage(inp_view(d, 5), true, raw_pts, pt_off, raw_seg, choice, frustum_angle, box2d, nullptr, K, Rtilt,
                           box3d_corners, heading, size, coin, normal, d->random_shift ? hshift : nullptr, point_cloud, center_ref,
                           cls_label, box3d_center, box3d_heading, box3d_size, rot_angle, seg_label, stream);
}

// Inference records of the SUN-RGBD loader (provider_sample_sunrgbd.py:165-186, from_rgb_detection): the same kernel with
// corners == nullptr, as fcn_prepare_inputs_infer has it -- point_cloud, center_ref[5] and rot_angle alone.
extern "C" int fcn_prepare_inputs_sunrgbd_infer(const fcn_inp5_desc *d, const float *raw_pts, const int64_t *pt_off,
                                                const int32_t *choice, const double *frustum_angle, const double *box2d,
                                                const double *K, const double *Rtilt, float *point_cloud,
                                                float *const center_ref[5], float *rot_angle, void *stream)
{
    if (!d || d->random_flip || d->random_shift) return FCN_E_BADARG;
    return inp_first_stage(inp_view(d, 5), false, raw_pts, pt_off, nullptr, choice, frustum_angle, box2d, nullptr, K, Rtilt,
                           nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, point_cloud, center_ref, nullptr, nullptr, nullptr,
                           nullptr, rot_angle, nullptr, stream);
}

// ------------------------------------------------------------------------------------------------
// Refinement stage (cfgs/refine_car.yaml; datasets/provider_sample_refine.py::ProviderDataset.__getitem__ :176-315 with
// get_center_view_point / _box3d :137-152, generate_ref :336-386, generate_labels :317-334, and collate_fn :388-419).  The
// sample is normalised to the FIRST-STAGE PREDICTION: points and label box are translated to the predicted box centre and
// rotated by its heading; the window centres span the predicted box's own depth extent -- in that frame the box is
// axis-aligned at the origin, so they are (0, 0, -w/2 + l*s + s/2) for l < ceil(w / s) (np.arange(z1, z2, s)) -- a different
// count per sample, which the reference's collate_fn pads by repeating the last centre / label up to the batch maximum
// (Lpad, handed in by the caller).  Positive / ignore boxes are the label box scaled by 0.3 / 0.6.
struct InpRefineArgs {
    fcn_inp_refine_desc d;
    const float *raw;
    const int64_t *off;
    const int32_t *choice;
    const double *pred_corners, *pred_angle, *pred_size, *corners, *heading, *size, *coin, *normal;
    float *pc, *ref[4];
    int64_t *cls;
    float *center, *head, *osize, *rot, *refc;
    int32_t *lens;
};

__global__ __launch_bounds__(INP_T) void prepare_inputs_refine_kernel(InpRefineArgs a)
{
    __shared__ double sdist[INP_T];
    __shared__ int sidx[INP_T];
    __shared__ int sany;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int N = a.d.N;
    const double *pcn = a.pred_corners + (int64_t)b * 24;
    const double pcx = (pcn[0] + pcn[18]) / 2.0, pcy = (pcn[1] + pcn[19]) / 2.0, pcz = (pcn[2] + pcn[20]) / 2.0;
    const double rot = a.pred_angle[b];
    const double c = cos(rot), s = sin(rot);
    const bool train = a.corners != nullptr;
    const bool flip = train && a.d.random_flip && a.coin[b] > 0.5;
    InpBox k = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double shift = 0.0;
    if (train) {
        inp_label_box(k, a, b, pcx, pcy, pcz, rot, c, s, flip);
        if (a.d.random_shift) {
            const double dist = sqrt(k.sl * k.sl + k.sw * k.sw), s1 = a.d.stride[0];
            shift = fmin(fmax(a.normal[b] * dist * 0.1, -2.0 * s1), 2.0 * s1);
            k.cz += shift;
        }
    }
    if (tid == 0) {
        if (train) inp_store_box(k, a, b);
        a.rot[b] = (float)rot;
        a.refc[3 * b] = (float)pcx; a.refc[3 * b + 1] = (float)pcy; a.refc[3 * b + 2] = (float)pcz;
    }
    // ---- points: (p - centre) rotated by the predicted heading, stored as float32
    const int64_t o0 = a.off[b];
    const int ps = a.d.pt_stride;
    for (int i = tid; i < N; i += INP_T) {
        const int64_t j = o0 + a.choice[(int64_t)b * N + i];
        const float *p = a.raw + j * ps;
        const double x = (double)p[0] - pcx, y = (double)p[1] - pcy, z = (double)p[2] - pcz;
        float xr = (float)(x * c + z * (-s));
        float zr = (float)(x * s + z * c);
        if (flip) xr = -xr;
        if (train && a.d.random_shift) zr = (float)((double)zr + shift);
        float *o = a.pc + (int64_t)b * 3 * N;
        o[i] = xr; o[N + i] = (float)y; o[2 * N + i] = zr;
    }
    // ---- window centres over the predicted box's depth extent, edge-padded to Lpad; labels on stride 2
    const double w = a.pred_size[3 * b + 1];
    const double z1 = -w / 2.0, z2 = w / 2.0;
    const double ca = cos(k.ang), sa = sin(k.ang);
    double best = 1e300;
    int bidx = 0x7fffffff;
    bool any1 = false;
    if (tid == 0) sany = 0;
    __syncthreads();
#pragma unroll 1
    for (int sc = 0; sc < 4; ++sc) {
        const int Lp = a.d.Lpad[sc];
        const double st = a.d.stride[sc];
        int Lb = (int)ceil((z2 - z1) / st);                         // len(np.arange(z1, z2, st))
        Lb = Lb < 0 ? 0 : (Lb > Lp ? Lp : Lb);
        if (tid == 0) a.lens[4 * b + sc] = Lb;
        for (int l = tid; l < Lp; l += INP_T) {
            const int le = l < Lb ? l : Lb - 1;                     // collate_fn: np.pad(..., mode='edge')
            const double z = (z1 + (double)le * st) + st / 2.0;
            const double xr = flip ? -0.0 : 0.0;
            float *o = a.ref[sc] + (int64_t)b * 3 * Lp;
            o[l] = (float)xr; o[Lp + l] = 0.f; o[2 * Lp + l] = (float)z;
            if (sc == 1 && a.cls && l < Lb)                             // the real windows; the label box scaled by 0.3 / 0.6
                inp_classify(a, b, Lp, l, xr, 0.0, z, k, ca, sa, 0.3, 0.6, any1, best, bidx);
        }
    }
    if (!a.cls) return;
    inp_nearest_positive(a, b, a.d.Lpad[1], sdist, sidx, &sany, tid, any1, best, bidx);
    __syncthreads();                                                    // thread 0's positive, before the padding reads it
    __threadfence_block();
    // edge padding of the labels: positions >= L_b repeat the last real one
    {
        const int Lp = a.d.Lpad[1];
        int Lb = (int)ceil((z2 - z1) / a.d.stride[1]);
        Lb = Lb < 0 ? 0 : (Lb > Lp ? Lp : Lb);
        if (Lb > 0) {
            const int64_t last = a.cls[(int64_t)b * Lp + Lb - 1];
            for (int l = Lb + tid; l < Lp; l += INP_T) a.cls[(int64_t)b * Lp + l] = last;
        }
    }
}

extern "C" int fcn_prepare_inputs_refine(const fcn_inp_refine_desc *d, const float *raw_pts, const int64_t *pt_off,
                                         const int32_t *choice, const double *pred_corners, const double *pred_angle,
                                         const double *pred_size, const double *box3d_corners, const double *heading,
                                         const double *size, const double *coin, const double *normal, float *point_cloud,
                                         float *const center_ref[4], int64_t *cls_label, float *box3d_center,
                                         float *box3d_heading, float *box3d_size, float *rot_angle, float *ref_center,
                                         int32_t *lens, void *stream)
{
    if (!d || !raw_pts || !pt_off || !choice || !pred_corners || !pred_angle || !pred_size || !point_cloud || !center_ref ||
        !rot_angle || !ref_center || !lens)
        return FCN_E_BADARG;
    if (d->B <= 0 || d->N <= 0 || d->pt_stride < 3) return FCN_E_BADARG;
    const bool train = box3d_corners != nullptr;
    if (train && (!heading || !size || !box3d_center || !box3d_heading || !box3d_size)) return FCN_E_BADARG;
    if (!train && cls_label) return FCN_E_BADARG;
    if (train && ((d->random_flip && !coin) || (d->random_shift && !normal))) return FCN_E_BADARG;
    if (!inp_scales_ok(4, d->Lpad, d->stride, center_ref)) return FCN_E_BADARG;
    InpRefineArgs a;
    a.d = *d; a.raw = raw_pts; a.off = pt_off; a.choice = choice; a.pred_corners = pred_corners; a.pred_angle = pred_angle;
    a.pred_size = pred_size; a.corners = box3d_corners; a.heading = heading; a.size = size; a.coin = coin; a.normal = normal;
    a.pc = point_cloud;
    for (int s = 0; s < 4; ++s) a.ref[s] = center_ref[s];
    a.cls = cls_label; a.center = box3d_center; a.head = box3d_heading; a.osize = box3d_size; a.rot = rot_angle;
    a.refc = ref_center; a.lens = lens;
    hipLaunchKernelGGL(prepare_inputs_refine_kernel, dim3(d->B), dim3(INP_T), 0, (hipStream_t)stream, a);
    FCN_CHECK_LAUNCH();
    return 0;
}

// ------------------------------------------------------------------------------------------------
// First-stage detections -> the raw points of the refinement stage (fcn_refine_select_count / _fill): csrc/refine_select.h
#include "refine_select.h"

// ------------------------------------------------------------------------------------------------
// LiDAR frames + calibration + 2-D boxes -> the raw points of the first stage (fcn_frustum_select_count / _fill): csrc/frustum_select.h
#include "frustum_select.h"

// ------------------------------------------------------------------------------------------------
// The same with one ground-truth 3-D box beside each 2-D box: the first stage's TRAINING records -- points, per-point foreground
// labels, box corners (fcn_frustum_label_count / _fill): csrc/frustum_label.h
#include "frustum_label.h"

// ------------------------------------------------------------------------------------------------
// The SUN-RGBD front: upright-depth frames + K + Rtilt + 2-D boxes (+ a label 3-D box beside each) -> the raw records of the
// five-scale model (fcn_frustum_sunrgbd_count / _fill, _label_count / _label_fill, fcn_frustum_subset_pos): csrc/frustum_sunrgbd.h
#include "frustum_sunrgbd.h"

// ------------------------------------------------------------------------------------------------
// First-stage detections + the frames' label boxes -> the refinement stage's TRAINING records: match, enlarge, jitter, select, count
// the positives (fcn_refine_match, fcn_refine_label_count / _fill): csrc/refine_label.h
#include "refine_label.h"

// ------------------------------------------------------------------------------------------------
// The random draws the prepare kernels above read -- resample indices, flip coin, depth-shift normal, height shift -- made on the
// device by a counter-based generator (fcn_draw_batch, fcn_draw_limits): csrc/draws.h
#include "draws.h"

// ------------------------------------------------------------------------------------------------
// The training sources' labels per step as a rank window of the epoch's permutation -- every label at most once per epoch, the
// tail dropped, 16 bytes of state -- on the draws' generator (fcn_epoch_pick, fcn_epoch_pick_limits): csrc/epoch_pick.h
#include "epoch_pick.h"

// ------------------------------------------------------------------------------------------------
// The first stage's training input without a host read: box perturbation on the draws' stream, the labelled count / fill without
// their read-back, and the one-workgroup plan between them (fcn_box2d_perturb, fcn_frustum_train_count / _plan / _fill):
// csrc/frustum_plan.h
#include "frustum_plan.h"

// ------------------------------------------------------------------------------------------------
// The SUN-RGBD training input without a host read: box perturbation, the labelled count / fill without their read-back, the
// one-workgroup plan and slots kernels around the frustum subsample drawn on the device, and the draw with per-row subsample
// slices (fcn_box2d_perturb_sunrgbd, fcn_frustum_sunrgbd_train_count / _plan / _fill / _slots, fcn_frustum_subsample_draw,
// fcn_draw_batch_sliced): csrc/frustum_sunrgbd_plan.h
#include "frustum_sunrgbd_plan.h"

// ------------------------------------------------------------------------------------------------
// The refinement stage's training input without a host read: the match and the labelled count / fill without their read-backs, the
// box jitter drawn on the device and the one-workgroup plan between count and fill (fcn_refine_train_match / _count / _fill,
// fcn_box3d_jitter_draw, fcn_refine_train_plan): csrc/refine_plan.h
#include "refine_plan.h"

// ------------------------------------------------------------------------------------------------
// Two-stage inference without a host read: the first stage's keep lists to a candidate table, the selection of refine_select.h on
// the segmented grid without its read-backs, and the training plan's kernel between count and fill (fcn_cascade_candidates,
// fcn_refine_detect_count / _plan / _fill): csrc/cascade_plan.h
#include "cascade_plan.h"

// ------------------------------------------------------------------------------------------------
// The inference front without a host read: frames + a resident table of 2-D detections -> the first-stage batch's raw points at a
// fixed number of slots and the second stage's image-FOV search set -- the selection of frustum_select.h behind a device-resident
// box count, without its read-backs, and the one-workgroup plans between count and fill (fcn_frustum_detect_count / _plan / _fill,
// fcn_frustum_fov_plan): csrc/frustum_detect_plan.h
#include "frustum_detect_plan.h"

// ------------------------------------------------------------------------------------------------
// SUN-RGBD inference without a host read: depth frames + a resident table of 2-D detections -> the five-scale batch's raw points at
// a fixed number of slots -- the selection of frustum_sunrgbd.h behind a device-resident box count, without its read-backs, and the
// one-workgroup plan between count and fill with the per-slot subsample slices (fcn_frustum_sunrgbd_detect_count / _plan / _fill):
// csrc/frustum_sunrgbd_detect_plan.h
#include "frustum_sunrgbd_detect_plan.h"
