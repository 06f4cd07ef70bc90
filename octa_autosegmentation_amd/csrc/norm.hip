// norm.hip -- fused InstanceNorm2d(affine) + LeakyReLU, forward and backward (statistics and affine parameters in fp32). Reference: the norm1/lrelu
// and norm2/lrelu pairs of MONAI's UnetBasicBlock that DynUNet is made of (models/networks.py:6 imports it; restated in
// octa_autosegmentation_amd/models/networks.py). torch runs this as batch-norm + a separate activation pass (and, under autocast, extra casts); at
// 1216x1216 every pass over a 32-channel map moves 95 MB, so the step is HBM-bound. Every kernel here is a streaming pass: forward =
// 2 reads + 1 write of the activation, backward = 2 x (x, dy) reads + 1 write, nothing else. Five kernel families, in the order of the file; the
// formulas they share are written once, in the device helpers below the vector type.
//   1. NCHW, bf16 or fp32 (in_fwd_stats / _apply, in_bwd_stats / _apply): octa_instnorm_lrelu_fwd / _bwd, called by models/fused_ops.py for the
//      channels-first networks and the fp32 inference passes. A (b, c) plane is split over `splits` workgroups so that >= ~2 workgroups per CU are
//      in flight even for the 128-plane top level; the statistics kernel leaves per-split partial sums, the apply kernel folds them (a few doubles)
//      and streams the plane with 16-byte accesses.
//   2. NHWC bf16 (in_nhwc_stats<0 / 1>, in_nhwc_fwd_apply, in_nhwc_bwd_apply): octa_instnorm_lrelu_nhwc_fwd / _bwd, the norm layers of the MFMA
//      convolution path (models/mfma_conv.py).
//   3. Statistics only + lazy application (in_nhwc_finalize, scale_shift_lrelu_nhwc): octa_instnorm_nhwc_stats / octa_scale_shift_lrelu_nhwc, the
//      normalise-on-load route of models/mfma_conv.py: the consuming convolution applies scale / shift while it loads.
//   4. Statistics from the producing convolution's epilogue: the d_stat_partials (in_nhwc_fold_partials) and d_stat_slots (slot_sum, in the apply
//      pass's prologue) sources of octa_instnorm_lrelu_nhwc_fwd.
//   5. Last norm + 1x1 output convolution to one channel, fused (in_nhwc_head_fwd / _head_bwd_stats / _head_bwd_apply):
//      octa_instnorm_lrelu_head1_nhwc_fwd / _bwd, the U-Net's last layer in models/mfma_conv.py.
#include <type_traits>
#include "common.h"
#include <cstdlib>

namespace {

constexpr int NT = 256;

template <class T> struct Vec;
template <> struct Vec<float> {
    static constexpr int N = 4;
    __device__ static void load(const float *p, float (&v)[8]) { float4 t = *reinterpret_cast<const float4 *>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    __device__ static void store(float *p, const float (&v)[8]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    __device__ static float ld1(const float *p) { return *p; }
    __device__ static void st1(float *p, float v) { *p = v; }
};
template <> struct Vec<unsigned short> {  // bf16 bits
    static constexpr int N = 8;
    __device__ static float up(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
    __device__ static unsigned short down(float f) { return octa_f2bf(f); }  // round to nearest even (v_cvt_pk_bf16_f32)
    __device__ static void load(const unsigned short *p, float (&v)[8]) {
        uint4 t = *reinterpret_cast<const uint4 *>(p);
        const unsigned w[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int k = 0; k < 4; k++) { v[2 * k] = __uint_as_float(w[k] << 16); v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u); }
    }
    __device__ static void store(unsigned short *p, const float (&v)[8]) {
        unsigned w[4];
#pragma unroll
        for (int k = 0; k < 4; k++) w[k] = octa_pack_bf16x2(v[2 * k], v[2 * k + 1]);
        *reinterpret_cast<uint4 *>(p) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    __device__ static float ld1(const unsigned short *p) { return up(*p); }
    __device__ static void st1(unsigned short *p, float v) { *p = down(v); }
};

// ---- the formulas, each once (NCHW and NHWC kernels alike) --------------------------------------------------------------------
__device__ __forceinline__ float lrelu(float z, float slope) { return z > 0.f ? z : z * slope; }
// gradient d through the LeakyReLU whose pre-activation is xh * wc + bc
__device__ __forceinline__ float lrelu_gate(float xh, float wc, float bc, float d, float slope) { return (xh * wc + bc) > 0.f ? d : d * slope; }
// input gradient of the normalisation: scale = wc * rstd, mg / mgx = the plane's means of g and of g * xhat
__device__ __forceinline__ float norm_dx(float scale, float g, float mg, float xh, float mgx) { return scale * (g - mg - xh * mgx); }
// (sum x, sum x^2) over hw elements -> mean and 1 / sqrt(var + eps), in double: E[x^2] - mean^2 may come out below zero by rounding
__device__ __forceinline__ void mean_rstd_of(double sa, double sq, long hw, float eps, float &mean, float &rstd) {
    const double mean_d = sa / (double)hw;
    double var = sq / (double)hw - mean_d * mean_d;
    if (var < 0) var = 0;
    mean = (float)mean_d; rstd = (float)(1.0 / sqrt(var + (double)eps));
}

__device__ __forceinline__ void block_reduce2(double &a, double &b, double *sh) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { a += __shfl_xor(a, d, 64); b += __shfl_xor(b, d, 64); }
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) { sh[2 * wv] = a; sh[2 * wv + 1] = b; }
    __syncthreads();
    a = 0; b = 0;
    for (int k = 0; k < NT / 64; k++) { a += sh[2 * k]; b += sh[2 * k + 1]; }
}

// ---- 1. NCHW, bf16 or fp32 -----------------------------------------------------------------------------------------------------
// chunk [e0, e1) of plane p handled by split s
__device__ __forceinline__ void chunk_of(long hw, int splits, int s, int vecn, long &e0, long &e1) {
    long per = ((hw + splits - 1) / splits + vecn - 1) / vecn * vecn;
    e0 = (long)s * per;
    e1 = e0 + per < hw ? e0 + per : hw;
    if (e0 > hw) e0 = hw;
}

template <class T>
__global__ void __launch_bounds__(NT) in_fwd_stats(const T *__restrict__ x, long hw, int splits, double *__restrict__ partial) {
    __shared__ double sh[2 * NT / 64];
    const long plane = blockIdx.y;
    const int s = blockIdx.x;
    long e0, e1;
    chunk_of(hw, splits, s, Vec<T>::N, e0, e1);
    const T *px = x + plane * hw;
    // fp32 activations (the reference's fp32 passes: test.py, validate.py, the frozen generator) accumulate in double: E[x^2] - mean^2 on
    // single-precision sums loses every digit of the variance of a nearly constant channel (round 6: the reference-made GAN fixture, whose
    // channels are, came out 5e-3 off; the torch modules 8e-4). bf16 activations keep the float sums: their rounding is far above this.
    typedef typename std::conditional<std::is_same<T, float>::value, double, float>::type acc_t;
    acc_t sum = 0, sq = 0;
    const bool vec = (hw % Vec<T>::N == 0) && ((reinterpret_cast<size_t>(px) & 15) == 0);
    if (vec) {
        for (long i = e0 + (long)threadIdx.x * Vec<T>::N; i + Vec<T>::N <= e1; i += (long)NT * Vec<T>::N) {
            float v[8];
            Vec<T>::load(px + i, v);
#pragma unroll
            for (int k = 0; k < Vec<T>::N; k++) { sum += (acc_t)v[k]; sq += (acc_t)v[k] * (acc_t)v[k]; }
        }
    } else {
        for (long i = e0 + threadIdx.x; i < e1; i += NT) { const acc_t v = (acc_t)Vec<T>::ld1(px + i); sum += v; sq += v * v; }
    }
    double a = sum, b = sq;
    block_reduce2(a, b, sh);
    if (threadIdx.x == 0) { partial[(plane * splits + s) * 2] = a; partial[(plane * splits + s) * 2 + 1] = b; }
}

template <class T>
__global__ void __launch_bounds__(NT) in_fwd_apply(const T *__restrict__ x, T *__restrict__ y, const float *__restrict__ w,
                                                   const float *__restrict__ bias, long hw, int C, int splits,
                                                   const double *__restrict__ partial, float slope, float eps,
                                                   float *__restrict__ mean_out, float *__restrict__ rstd_out) {
    const long plane = blockIdx.y;
    const int s = blockIdx.x, c = (int)(plane % C);
    double a = 0, b = 0;
    for (int k = 0; k < splits; k++) { a += partial[(plane * splits + k) * 2]; b += partial[(plane * splits + k) * 2 + 1]; }
    float mean, rstd; mean_rstd_of(a, b, hw, eps, mean, rstd);
    if (s == 0 && threadIdx.x == 0) { mean_out[plane] = mean; rstd_out[plane] = rstd; }
    // fp32: (x - mean) * g + b as torch evaluates it -- x * g - mean * g cancels in single precision where |mean| >> std; bf16: one fma
    constexpr bool F32 = std::is_same<T, float>::value;
    const float g = w ? w[c] * rstd : rstd, b0 = bias ? bias[c] : 0.f, sh = b0 - mean * g;
    long e0, e1;
    chunk_of(hw, splits, s, Vec<T>::N, e0, e1);
    const T *px = x + plane * hw;
    T *py = y + plane * hw;
    const bool vec = (hw % Vec<T>::N == 0) && ((reinterpret_cast<size_t>(px) & 15) == 0) && ((reinterpret_cast<size_t>(py) & 15) == 0);
    if (vec) {
        for (long i = e0 + (long)threadIdx.x * Vec<T>::N; i + Vec<T>::N <= e1; i += (long)NT * Vec<T>::N) {
            float v[8];
            Vec<T>::load(px + i, v);
#pragma unroll
            for (int k = 0; k < Vec<T>::N; k++) v[k] = lrelu(F32 ? (v[k] - mean) * g + b0 : v[k] * g + sh, slope);
            Vec<T>::store(py + i, v);
        }
    } else {
        for (long i = e0 + threadIdx.x; i < e1; i += NT) {
            const float xv = Vec<T>::ld1(px + i);
            Vec<T>::st1(py + i, lrelu(F32 ? (xv - mean) * g + b0 : xv * g + sh, slope));
        }
    }
}

template <class T>
__global__ void __launch_bounds__(NT) in_bwd_stats(const T *__restrict__ x, const T *__restrict__ dy, const float *__restrict__ w,
                                                   const float *__restrict__ bias, const float *__restrict__ mean,
                                                   const float *__restrict__ rstd, long hw, int C, int splits, float slope,
                                                   double *__restrict__ partial) {
    __shared__ double sh[2 * NT / 64];
    const long plane = blockIdx.y;
    const int s = blockIdx.x, c = (int)(plane % C);
    const float mu = mean[plane], rs = rstd[plane], wc = w ? w[c] : 1.f, bc = bias ? bias[c] : 0.f;
    long e0, e1;
    chunk_of(hw, splits, s, Vec<T>::N, e0, e1);
    const T *px = x + plane * hw, *pd = dy + plane * hw;
    float sg = 0.f, sgx = 0.f;
    const bool vec = (hw % Vec<T>::N == 0) && ((reinterpret_cast<size_t>(px) & 15) == 0) && ((reinterpret_cast<size_t>(pd) & 15) == 0);
    if (vec) {
        for (long i = e0 + (long)threadIdx.x * Vec<T>::N; i + Vec<T>::N <= e1; i += (long)NT * Vec<T>::N) {
            float v[8], d[8];
            Vec<T>::load(px + i, v);
            Vec<T>::load(pd + i, d);
#pragma unroll
            for (int k = 0; k < Vec<T>::N; k++) {
                float xh = (v[k] - mu) * rs;
                float g = lrelu_gate(xh, wc, bc, d[k], slope);
                sg += g; sgx += g * xh;
            }
        }
    } else {
        for (long i = e0 + threadIdx.x; i < e1; i += NT) {
            float xh = (Vec<T>::ld1(px + i) - mu) * rs, d = Vec<T>::ld1(pd + i);
            float g = lrelu_gate(xh, wc, bc, d, slope);
            sg += g; sgx += g * xh;
        }
    }
    double a = sg, b = sgx;
    block_reduce2(a, b, sh);
    if (threadIdx.x == 0) { partial[(plane * splits + s) * 2] = a; partial[(plane * splits + s) * 2 + 1] = b; }
}

template <class T>
__global__ void __launch_bounds__(NT) in_bwd_apply(const T *__restrict__ x, const T *__restrict__ dy, T *__restrict__ dx,
                                                   const float *__restrict__ w, const float *__restrict__ bias,
                                                   const float *__restrict__ mean, const float *__restrict__ rstd, long hw, int C,
                                                   int splits, float slope, const double *__restrict__ partial,
                                                   float *__restrict__ dw, float *__restrict__ db) {
    const long plane = blockIdx.y;
    const int s = blockIdx.x, c = (int)(plane % C);
    double a = 0, b = 0;
    for (int k = 0; k < splits; k++) { a += partial[(plane * splits + k) * 2]; b += partial[(plane * splits + k) * 2 + 1]; }
    if (s == 0 && threadIdx.x == 0) {
        if (db) atomicAdd(&db[c], (float)a);
        if (dw) atomicAdd(&dw[c], (float)b);
    }
    const float mu = mean[plane], rs = rstd[plane], wc = w ? w[c] : 1.f, bc = bias ? bias[c] : 0.f;
    const float mg = (float)(a / (double)hw), mgx = (float)(b / (double)hw), k0 = wc * rs;
    long e0, e1;
    chunk_of(hw, splits, s, Vec<T>::N, e0, e1);
    const T *px = x + plane * hw, *pd = dy + plane * hw;
    T *po = dx + plane * hw;
    const bool vec = (hw % Vec<T>::N == 0) && ((reinterpret_cast<size_t>(px) & 15) == 0) && ((reinterpret_cast<size_t>(pd) & 15) == 0) &&
                     ((reinterpret_cast<size_t>(po) & 15) == 0);
    if (vec) {
        for (long i = e0 + (long)threadIdx.x * Vec<T>::N; i + Vec<T>::N <= e1; i += (long)NT * Vec<T>::N) {
            float v[8], d[8];
            Vec<T>::load(px + i, v);
            Vec<T>::load(pd + i, d);
#pragma unroll
            for (int k = 0; k < Vec<T>::N; k++) {
                float xh = (v[k] - mu) * rs;
                v[k] = norm_dx(k0, lrelu_gate(xh, wc, bc, d[k], slope), mg, xh, mgx);
            }
            Vec<T>::store(po + i, v);
        }
    } else {
        for (long i = e0 + threadIdx.x; i < e1; i += NT) {
            float xh = (Vec<T>::ld1(px + i) - mu) * rs, d = Vec<T>::ld1(pd + i);
            Vec<T>::st1(po + i, norm_dx(k0, lrelu_gate(xh, wc, bc, d, slope), mg, xh, mgx));
        }
    }
}

int pick_splits(const octa_ctx *ctx, long planes, long hw) {
    long want = 2L * ctx->num_cus;
    int s = (int)((want + planes - 1) / planes);
    if (s < 1) s = 1;
    long max_by_size = hw / (NT * 8) > 0 ? hw / (NT * 8) : 1;   // at least one vector per thread
    if (s > max_by_size) s = (int)max_by_size;
    if (s > 64) s = 64;
    return s;
}

// clears the affine gradients that the backward apply kernels accumulate into with atomics (either may be NULL)
int zero_affine_grads(float *d_dw, float *d_db, int C, hipStream_t stream) {
    if (d_dw && d_db == d_dw + C) {                                   // allocated back to back by the host side: one fill
        OCTA_HIP_CHECK(hipMemsetAsync(d_dw, 0, sizeof(float) * 2 * C, stream));
    } else {
        if (d_dw) OCTA_HIP_CHECK(hipMemsetAsync(d_dw, 0, sizeof(float) * C, stream));
        if (d_db) OCTA_HIP_CHECK(hipMemsetAsync(d_db, 0, sizeof(float) * C, stream));
    }
    return 0;
}

}  // namespace

extern "C" int octa_instnorm_lrelu_fwd(octa_ctx *ctx, const void *d_x, void *d_y, const float *d_w, const float *d_b, float *d_mean,
                                       float *d_rstd, int B, int C, int64_t hw, int dtype, float slope, float eps, void *stream_) {
    if (!ctx || !d_x || !d_y || !d_mean || !d_rstd || B <= 0 || C <= 0 || hw <= 0) { octa::set_error("octa_instnorm_lrelu_fwd: bad arguments"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const long planes = (long)B * C;
    if (planes > 65535L * 16) { octa::set_error("octa_instnorm_lrelu_fwd: too many planes"); return -2; }
    const int splits = pick_splits(ctx, planes, hw);
    double *partial = ctx->work[3].take<double>(2 * planes * splits);
    if (!partial) return -1;
    dim3 grid((unsigned)splits, (unsigned)planes);
    auto launch = [&](auto t) {   // t: an element of the activations' type
        typedef decltype(t) T;
        hipLaunchKernelGGL(in_fwd_stats<T>, grid, dim3(NT), 0, stream, (const T *)d_x, (long)hw, splits, partial);
        hipLaunchKernelGGL(in_fwd_apply<T>, grid, dim3(NT), 0, stream, (const T *)d_x, (T *)d_y, d_w, d_b, (long)hw, C, splits, partial, slope, eps, d_mean, d_rstd);
    };
    if (dtype == 0) launch(float());
    else if (dtype == 1) launch((unsigned short)0);
    else { octa::set_error("octa_instnorm_lrelu_fwd: dtype must be 0 (f32) or 1 (bf16)"); return -2; }
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_instnorm_lrelu_bwd(octa_ctx *ctx, const void *d_x, const void *d_dy, const float *d_w, const float *d_b,
                                       const float *d_mean, const float *d_rstd, void *d_dx, float *d_dw, float *d_db, int B, int C,
                                       int64_t hw, int dtype, float slope, void *stream_) {
    if (!ctx || !d_x || !d_dy || !d_dx || !d_mean || !d_rstd || B <= 0 || C <= 0 || hw <= 0) { octa::set_error("octa_instnorm_lrelu_bwd: bad arguments"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const long planes = (long)B * C;
    const int splits = pick_splits(ctx, planes, hw);
    double *partial = ctx->work[3].take<double>(2 * planes * splits);
    if (!partial) return -1;
    dim3 grid((unsigned)splits, (unsigned)planes);
    if (zero_affine_grads(d_dw, d_db, C, stream)) return -1;
    auto launch = [&](auto t) {   // t: an element of the activations' type
        typedef decltype(t) T;
        hipLaunchKernelGGL(in_bwd_stats<T>, grid, dim3(NT), 0, stream, (const T *)d_x, (const T *)d_dy, d_w, d_b, d_mean, d_rstd, (long)hw, C, splits, slope, partial);
        hipLaunchKernelGGL(in_bwd_apply<T>, grid, dim3(NT), 0, stream, (const T *)d_x, (const T *)d_dy, (T *)d_dx, d_w, d_b, d_mean, d_rstd, (long)hw, C, splits, slope,
                           partial, d_dw, d_db);
    };
    if (dtype == 0) launch(float());
    else if (dtype == 1) launch((unsigned short)0);
    else { octa::set_error("octa_instnorm_lrelu_bwd: dtype must be 0 (f32) or 1 (bf16)"); return -2; }
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- 2. NHWC (channels-last) bf16, for the MFMA convolution path (csrc/conv.hip) ----------------------------------------------
// Activations [B][HW][C] bf16, C a multiple of 8. A thread owns 8 consecutive channels (one 16-byte access) of a
// strided set of pixels; per-channel partial sums meet in LDS, then one double atomicAdd per channel and block
// into sums[b][c][2]. The apply kernels read the finished sums, derive scale / shift per channel into LDS and
// stream the image. Same arithmetic as the NCHW kernels above.
namespace {

constexpr int NHWC_MAXC = 512;

__device__ __forceinline__ void nhwc_geometry(int C, int &cg, int &pl, int &npl) {
    const int groups = C / 8;
    cg = threadIdx.x % groups;
    pl = threadIdx.x / groups;
    npl = NT / groups;
}

// pixels [p0, p1) of an image handled by split s
__device__ __forceinline__ void pixel_range(long hw, int splits, int s, long &p0, long &p1) {
    const long per = (hw + splits - 1) / splits;
    p0 = (long)s * per;
    p1 = p0 + per < hw ? p0 + per : hw;
}

// the per-group constants of the backward kernels, for channel c (one of the thread's eight) of image b: saved statistics, affine parameters (absent: 1, 0)
__device__ __forceinline__ void load_consts(const float *mean, const float *rstd, const float *w, const float *bias, int b, int C, int c, float &mu,
                                            float &rs, float &wc, float &bc) {
    mu = mean[(long)b * C + c]; rs = rstd[(long)b * C + c]; wc = w ? w[c] : 1.f; bc = bias ? bias[c] : 0.f;
}

// sum over the slots of sums[nslot][.][2] at element e (sum, sum of squares): the loads of eight slots are issued together (index clamped,
// branch-free) -- a run-time loop with one load per trip waits for memory once per slot in every workgroup's prologue
__device__ __forceinline__ void slot_sum(const double *__restrict__ sums, long e, int nslot, long slot_stride, double &sa, double &sq) {
    sa = 0; sq = 0;
    for (int k0 = 0; k0 < nslot; k0 += 8) {
        double a[8], q[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int k = k0 + j < nslot ? k0 + j : k0;
            a[j] = sums[k * slot_stride + e * 2]; q[j] = sums[k * slot_stride + e * 2 + 1];
        }
#pragma unroll
        for (int j = 0; j < 8; j++)
            if (k0 + j < nslot) { sa += a[j]; sq += q[j]; }
    }
}

// prologue of the forward apply passes, for channel c of image b: the sums of all slots -> mean / rstd (stored by split 0) -> scale / shift in LDS.
// One slot with stride 0 = plain sums[B][C][2]; more = the slot form [nslot][B][C][2] of the producing convolution's epilogue (csrc/conv.hip,
// octa_conv3x3_nhwc_fwd). The loop over c stays in the kernels: with a loop inside, a helper changes the device code
__device__ __forceinline__ void scale_shift_to_lds(const double *sums, int nslot, long slot_stride, const float *w, const float *bias, long hw, int C,
                                                   int b, int c, int s, float eps, float *mean_out, float *rstd_out, float (&s_g)[NHWC_MAXC],
                                                   float (&s_sh)[NHWC_MAXC]) {
    double sa, sq;
    slot_sum(sums, (long)b * C + c, nslot, slot_stride, sa, sq);
    float mean, rstd; mean_rstd_of(sa, sq, hw, eps, mean, rstd);
    if (s == 0) { mean_out[(long)b * C + c] = mean; rstd_out[(long)b * C + c] = rstd; }
    const float g = w ? w[c] * rstd : rstd;
    s_g[c] = g; s_sh[c] = (bias ? bias[c] : 0.f) - mean * g;
}

// mode 0: (sum x, sum x^2); mode 1: (sum g, sum g*xhat) with g = dy * lrelu'(pre)
template <int MODE>
__global__ void __launch_bounds__(NT)
in_nhwc_stats(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dy, const float *__restrict__ w,
              const float *__restrict__ bias, const float *__restrict__ mean, const float *__restrict__ rstd, long hw, int C,
              int splits, float slope, double *__restrict__ sums, int b0) {
    __shared__ float s_red[2 * NT * 8];
    const int b = blockIdx.y + b0, s = blockIdx.x;
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);
    const bool active = pl < npl && cg < C / 8;   // NT need not be a multiple of C/8
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float a[8], q[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { a[k] = 0.f; q[k] = 0.f; }
    float mu[8], rs[8], wc[8], bc[8];
    if (MODE == 1 && active) {
#pragma unroll
        for (int k = 0; k < 8; k++) load_consts(mean, rstd, w, bias, b, C, cg * 8 + k, mu[k], rs[k], wc[k], bc[k]);
    }
    if (active) {
        const unsigned short *px = x + ((long)b * hw) * C + cg * 8;
        const unsigned short *pd = MODE == 1 ? dy + ((long)b * hw) * C + cg * 8 : nullptr;
        long p = p0 + pl;
        if (MODE == 0) {
            for (; p + 3L * npl < p1; p += 4L * npl) {
                float v[4][8];
#pragma unroll
                for (int u = 0; u < 4; u++) Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]);
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int k = 0; k < 8; k++) { a[k] += v[u][k]; q[k] += v[u][k] * v[u][k]; }
            }
        } else {
            for (; p + (long)npl < p1; p += 2L * npl) {
                float v[2][8], d[2][8];
#pragma unroll
                for (int u = 0; u < 2; u++) { Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]); Vec<unsigned short>::load(pd + (p + (long)u * npl) * C, d[u]); }
#pragma unroll
                for (int u = 0; u < 2; u++)
#pragma unroll
                    for (int k = 0; k < 8; k++) {
                        const float xh = (v[u][k] - mu[k]) * rs[k];
                        const float g = lrelu_gate(xh, wc[k], bc[k], d[u][k], slope);
                        a[k] += g; q[k] += g * xh;
                    }
            }
        }
        for (; p < p1; p += npl) {
            float v[8];
            Vec<unsigned short>::load(px + p * C, v);
            if (MODE == 0) {
#pragma unroll
                for (int k = 0; k < 8; k++) { a[k] += v[k]; q[k] += v[k] * v[k]; }
            } else {
                float d[8];
                Vec<unsigned short>::load(pd + p * C, d);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const float xh = (v[k] - mu[k]) * rs[k];
                    const float g = lrelu_gate(xh, wc[k], bc[k], d[k], slope);
                    a[k] += g; q[k] += g * xh;
                }
            }
        }
    }
    // fold the pixel lanes of every channel group (in_nhwc_head_bwd_stats repeats it: as a shared helper it changed all three kernels' code)
#pragma unroll
    for (int k = 0; k < 8; k++) { s_red[(threadIdx.x * 8 + k) * 2] = a[k]; s_red[(threadIdx.x * 8 + k) * 2 + 1] = q[k]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NT) {
        const int g = c / 8, k = c % 8, groups = C / 8;
        double sa = 0, sq = 0;
        for (int l = 0; l < npl; l++) {
            const int t = l * groups + g;
            sa += s_red[(t * 8 + k) * 2]; sq += s_red[(t * 8 + k) * 2 + 1];
        }
        atomicAdd(&sums[((long)b * C + c) * 2], sa);
        atomicAdd(&sums[((long)b * C + c) * 2 + 1], sq);
    }
}

__global__ void __launch_bounds__(NT)
in_nhwc_fwd_apply(const unsigned short *__restrict__ x, unsigned short *__restrict__ y, const float *__restrict__ w,
                  const float *__restrict__ bias, long hw, int C, int splits, const double *__restrict__ sums, float slope, float eps,
                  float *__restrict__ mean_out, float *__restrict__ rstd_out, int b0, int nslot, long slot_stride) {
    __shared__ float s_g[NHWC_MAXC], s_sh[NHWC_MAXC];
    const int b = blockIdx.y + b0, s = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += NT) scale_shift_to_lds(sums, nslot, slot_stride, w, bias, hw, C, b, c, s, eps, mean_out, rstd_out, s_g, s_sh);
    __syncthreads();
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);
    if (pl >= npl) return;
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float g[8], sh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { g[k] = s_g[cg * 8 + k]; sh[k] = s_sh[cg * 8 + k]; }
    const unsigned short *px = x + ((long)b * hw) * C + cg * 8;
    unsigned short *py = y + ((long)b * hw) * C + cg * 8;
    long p = p0 + pl;
    for (; p + 3L * npl < p1; p += 4L * npl) {   // four independent 16-byte streams per thread keep more bytes in flight
        float v[4][8];
#pragma unroll
        for (int u = 0; u < 4; u++) Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int k = 0; k < 8; k++) v[u][k] = lrelu(v[u][k] * g[k] + sh[k], slope);
            Vec<unsigned short>::store(py + (p + (long)u * npl) * C, v[u]);
        }
    }
    for (; p < p1; p += npl) {
        float v[8];
        Vec<unsigned short>::load(px + p * C, v);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = lrelu(v[k] * g[k] + sh[k], slope);
        Vec<unsigned short>::store(py + p * C, v);
    }
}

__global__ void __launch_bounds__(NT)
in_nhwc_bwd_apply(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dy, unsigned short *__restrict__ dx,
                  const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ mean,
                  const float *__restrict__ rstd, long hw, int C, int splits, float slope, const double *__restrict__ sums,
                  float *__restrict__ dw, float *__restrict__ db, int b0, int Bsum) {
    __shared__ float s_mg[NHWC_MAXC], s_mgx[NHWC_MAXC];
    const int b = blockIdx.y + b0, s = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += NT) {
        const double sa = sums[((long)b * C + c) * 2], sq = sums[((long)b * C + c) * 2 + 1];
        if (s == 0) {
            if (Bsum > 0) {
                // whole batch in this launch: ONE workgroup folds the per-image sums and stores the affine gradients -- no cleared
                // output, no atomics (17 fills per U-Net step), and a fixed summation order
                if (b == 0) {
                    double ta = 0, tq = 0;
                    for (int bb = 0; bb < Bsum; bb++) { ta += sums[((long)bb * C + c) * 2]; tq += sums[((long)bb * C + c) * 2 + 1]; }
                    if (db) db[c] = (float)ta;
                    if (dw) dw[c] = (float)tq;
                }
            } else {
                if (db) atomicAdd(&db[c], (float)sa);
                if (dw) atomicAdd(&dw[c], (float)sq);
            }
        }
        s_mg[c] = (float)(sa / (double)hw); s_mgx[c] = (float)(sq / (double)hw);
    }
    __syncthreads();
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);
    if (pl >= npl) return;
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float mu[8], rs[8], wc[8], bc[8], mg[8], mgx[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int c = cg * 8 + k;
        load_consts(mean, rstd, w, bias, b, C, c, mu[k], rs[k], wc[k], bc[k]);
        mg[k] = s_mg[c]; mgx[k] = s_mgx[c];
    }
    const unsigned short *px = x + ((long)b * hw) * C + cg * 8, *pd = dy + ((long)b * hw) * C + cg * 8;
    unsigned short *po = dx + ((long)b * hw) * C + cg * 8;
    long p = p0 + pl;
    for (; p + (long)npl < p1; p += 2L * npl) {
        float v[2][8], d[2][8];
#pragma unroll
        for (int u = 0; u < 2; u++) { Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]); Vec<unsigned short>::load(pd + (p + (long)u * npl) * C, d[u]); }
#pragma unroll
        for (int u = 0; u < 2; u++) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float xh = (v[u][k] - mu[k]) * rs[k];
                v[u][k] = norm_dx(wc[k] * rs[k], lrelu_gate(xh, wc[k], bc[k], d[u][k], slope), mg[k], xh, mgx[k]);
            }
            Vec<unsigned short>::store(po + (p + (long)u * npl) * C, v[u]);
        }
    }
    for (; p < p1; p += npl) {
        float v[8], d[8];
        Vec<unsigned short>::load(px + p * C, v);
        Vec<unsigned short>::load(pd + p * C, d);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float xh = (v[k] - mu[k]) * rs[k];
            v[k] = norm_dx(wc[k] * rs[k], lrelu_gate(xh, wc[k], bc[k], d[k], slope), mg[k], xh, mgx[k]);
        }
        Vec<unsigned short>::store(po + p * C, v);
    }
}

int nhwc_splits(const octa_ctx *ctx, int B, long hw) {
    long s = (4L * ctx->num_cus + B - 1) / B;
    // at least this many pixels per workgroup: 512, and 128 for planes below 256 x 256 (round 4: a 76 x 76 x 256 plane of the GAN's
    // residual stages ran on 11 x B workgroups, 17 % of the CUs at B = 4; GAN-seg step 56.8 -> 55.4 ms, U-Net step unchanged;
    // profiles/r04_norm_min_pixels.log). For the planes of these networks the bound, not the batch size, decides the split count at
    // B <= 4, so an image's partial sums are formed alike alone and in a batch (tests/test_training_cli_gpu.py compares the two).
    const long min_px = hw < 65536 ? 128 : 512;
    const long by_size = hw / min_px > 0 ? hw / min_px : 1;
    if (s > by_size) s = by_size;
    if (s < 1) s = 1;
    if (s > 1024) s = 1024;
    return (int)s;
}

// Images per launch group of the two-pass norm kernels: as many as fit OCTA_NORM_CACHE_MB together (at least one). Default 0 =
// the whole batch in one launch: image-by-image launches (application pass served from the 256 MB Infinity Cache) were
// measured SLOWER on MI355X (U-Net step 22.0 ms at 192 MB, 23.6 ms at 96 MB vs 21.2 ms) -- short launches, longer tails.
int nhwc_group(int B, size_t bytes_per_image) {
    static const size_t budget = [] { const char *e = getenv("OCTA_NORM_CACHE_MB"); return (size_t)(e ? atol(e) : 0) << 20; }();
    if (budget == 0) return B;
    size_t g = budget / (bytes_per_image ? bytes_per_image : 1);
    if (g < 1) g = 1;
    return g > (size_t)B ? B : (int)g;
}

int nhwc_check(const char *who, int B, int C, int64_t hw) {
    // every channel group needs a thread of the block (C / 8 <= NT). A group count that does not divide NT is supported: the
    // NT % (C / 8) threads past the last whole pixel lane idle (C = 24, 40: tests/test_norm_gpu.py cases 3 and 4)
    static_assert(NHWC_MAXC / 8 <= NT, "a block holds at least one pixel lane of every channel group");
    if (B <= 0 || hw <= 0 || C <= 0 || C % 8 || C > NHWC_MAXC || C / 8 > NT) { octa::set_error("%s: C must be a multiple of 8, <= %d (got B=%d C=%d)", who, NHWC_MAXC, B, C); return -2; }
    if (B > 65535) { octa::set_error("%s: B > 65535", who); return -2; }
    return 0;
}

// what an NHWC entry point does first: null pointers, then the shape, then the device
int nhwc_enter(const char *who, const octa_ctx *ctx, bool ptrs, int B, int C, int64_t hw, int (*check)(const char *, int, int, int64_t) = nhwc_check) {
    if (!ctx || !ptrs) { octa::set_error("%s: null pointer", who); return -2; }
    if (check(who, B, C, hw)) return -2;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    return 0;
}

// (sum x, sum x^2) of the images [b0, b0 + grid.y) added into sums: in_nhwc_stats<0> reads no dy, affine parameters, saved statistics or slope
void launch_x_stats(dim3 grid, hipStream_t stream, const unsigned short *x, long hw, int C, double *sums, int b0) {
    hipLaunchKernelGGL(in_nhwc_stats<0>, grid, dim3(NT), 0, stream, x, (const unsigned short *)nullptr, (const float *)nullptr, (const float *)nullptr,
                       (const float *)nullptr, (const float *)nullptr, hw, C, (int)grid.x, 0.f, sums, b0);
}

// ---- 3. statistics only + lazy application (normalise-on-load path of csrc/conv.hip) -------------------------------------------
__global__ void __launch_bounds__(NT)
in_nhwc_finalize(const double *__restrict__ sums, const float *__restrict__ w, const float *__restrict__ bias, long hw, int C, long total,
                 float eps, float *__restrict__ mean_out, float *__restrict__ rstd_out, float *__restrict__ scale, float *__restrict__ shift) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % C);
    float mean, rstd; mean_rstd_of(sums[2 * i], sums[2 * i + 1], hw, eps, mean, rstd);
    mean_out[i] = mean; rstd_out[i] = rstd;
    const float g = w ? w[c] * rstd : rstd;
    scale[i] = g;
    shift[i] = (bias ? bias[c] : 0.f) - mean * g;
}

__global__ void __launch_bounds__(NT)
scale_shift_lrelu_nhwc(const unsigned short *__restrict__ x, unsigned short *__restrict__ y, const float *__restrict__ scale,
                       const float *__restrict__ shift, long hw, int C, int splits, float slope) {
    const int b = blockIdx.y, s = blockIdx.x;
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);
    if (pl >= npl) return;
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float g[8], sh[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { g[k] = scale[(long)b * C + cg * 8 + k]; sh[k] = shift[(long)b * C + cg * 8 + k]; }
    const unsigned short *px = x + ((long)b * hw) * C + cg * 8;
    unsigned short *py = y + ((long)b * hw) * C + cg * 8;
    for (long p = p0 + pl; p < p1; p += npl) {
        float v[8];
        Vec<unsigned short>::load(px + p * C, v);
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = lrelu(v[k] * g[k] + sh[k], slope);
        Vec<unsigned short>::store(py + p * C, v);
    }
}

}  // namespace

extern "C" int octa_instnorm_nhwc_stats(octa_ctx *ctx, const void *d_x, const float *d_w, const float *d_b, float *d_mean, float *d_rstd,
                                        float *d_scale, float *d_shift, int B, int C, int64_t hw, float eps, void *stream_) {
    if (int rc = nhwc_enter("octa_instnorm_nhwc_stats", ctx, d_x && d_mean && d_rstd && d_scale && d_shift, B, C, hw)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    double *sums = static_cast<double *>(ctx->zeroed(sizeof(double) * 2 * (size_t)B * C, stream));   // pre-zeroed ring slot
    if (!sums) return -1;
    const int splits = nhwc_splits(ctx, B, hw);
    launch_x_stats(dim3((unsigned)splits, (unsigned)B), stream, static_cast<const unsigned short *>(d_x), (long)hw, C, sums, 0);
    const long total = (long)B * C;
    hipLaunchKernelGGL(in_nhwc_finalize, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, stream, sums, d_w, d_b, (long)hw, C, total, eps,
                       d_mean, d_rstd, d_scale, d_shift);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_scale_shift_lrelu_nhwc(octa_ctx *ctx, const void *d_x, void *d_y, const float *d_scale, const float *d_shift, int B, int C,
                                           int64_t hw, float slope, void *stream_) {
    if (int rc = nhwc_enter("octa_scale_shift_lrelu_nhwc", ctx, d_x && d_y && d_scale && d_shift, B, C, hw)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int splits = nhwc_splits(ctx, B, hw);
    hipLaunchKernelGGL(scale_shift_lrelu_nhwc, dim3((unsigned)splits, (unsigned)B), dim3(NT), 0, stream, static_cast<const unsigned short *>(d_x),
                       static_cast<unsigned short *>(d_y), d_scale, d_shift, (long)hw, C, splits, slope);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- 4. forward, optionally with the statistics already accumulated by the producing convolution (csrc/conv.hip) ---------------
namespace {

// partials [B][tiles][C][2] float -> sums [B][C][2] double. Block = 8 tile lanes x 32 channels.
__global__ void __launch_bounds__(NT)
in_nhwc_fold_partials(const float *__restrict__ part, int tiles, int C, double *__restrict__ sums) {
    __shared__ double s_red[NT * 2];
    const int b = blockIdx.y, c = blockIdx.x * 32 + (threadIdx.x & 31), tl = threadIdx.x >> 5;
    double a = 0, q = 0;
    if (c < C)
        for (int t = tl; t < tiles; t += NT / 32) {
            const float2 v = *reinterpret_cast<const float2 *>(part + (((size_t)b * tiles + t) * C + c) * 2);
            a += v.x; q += v.y;
        }
    s_red[threadIdx.x * 2] = a; s_red[threadIdx.x * 2 + 1] = q;
    __syncthreads();
    if (tl == 0 && c < C) {
        for (int k = 1; k < NT / 32; k++) { a += s_red[(k * 32 + threadIdx.x) * 2]; q += s_red[(k * 32 + threadIdx.x) * 2 + 1]; }
        sums[((size_t)b * C + c) * 2] = a; sums[((size_t)b * C + c) * 2 + 1] = q;
    }
}

}  // namespace

// Statistics source: none of the two = a statistics pass of its own over d_x; d_stat_partials = the per-tile float partials [B][tiles][C][2] of
// the convolution that wrote x (folded here, then applied); d_stat_slots = the same sums in slot form, double [nslot][B][C][2], accumulated by that
// convolution's epilogue (octa_conv3x3_nhwc_fwd, _fwd_pad, octa_conv3x3_c1_fwd): one launch, the apply pass adds the slots up while it derives
// scale / shift. Both at once are refused.
extern "C" int octa_instnorm_lrelu_nhwc_fwd(octa_ctx *ctx, const void *d_x, void *d_y, const float *d_w, const float *d_b, float *d_mean,
                                            float *d_rstd, int B, int C, int64_t hw, float slope, float eps, const float *d_stat_partials,
                                            int tiles, const double *d_stat_slots, int nslot, void *stream_) {
    // the one entry point with a check between the null pointers and the shape: spelled out, so that errors are reported in the same order
    if (!ctx || !d_x || !d_y || !d_mean || !d_rstd) { octa::set_error("octa_instnorm_lrelu_nhwc_fwd: null pointer"); return -2; }
    if ((d_stat_partials && (d_stat_slots || tiles <= 0)) || (d_stat_slots && (nslot <= 0 || nslot > 1024))) {
        octa::set_error("octa_instnorm_lrelu_nhwc_fwd: one statistics source at most, with tiles >= 1 or 1..1024 slots");
        return -2;
    }
    if (nhwc_check("octa_instnorm_lrelu_nhwc_fwd", B, C, hw)) return -2;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned short *x = static_cast<const unsigned short *>(d_x);
    unsigned short *y = static_cast<unsigned short *>(d_y);
    if (d_stat_slots) {
        const int splits = nhwc_splits(ctx, B, hw);
        hipLaunchKernelGGL(in_nhwc_fwd_apply, dim3((unsigned)splits, (unsigned)B), dim3(NT), 0, stream, x, y, d_w, d_b, (long)hw, C, splits, d_stat_slots,
                           slope, eps, d_mean, d_rstd, 0, nslot, (long)B * C * 2);
    } else if (d_stat_partials) {
        double *sums = ctx->work[3].take<double>(2 * (size_t)B * C);
        if (!sums) return -1;
        hipLaunchKernelGGL(in_nhwc_fold_partials, dim3((unsigned)((C + 31) / 32), (unsigned)B), dim3(NT), 0, stream, d_stat_partials, tiles, C, sums);
        const int splits = nhwc_splits(ctx, B, hw);
        hipLaunchKernelGGL(in_nhwc_fwd_apply, dim3((unsigned)splits, (unsigned)B), dim3(NT), 0, stream, x, y, d_w, d_b, (long)hw, C, splits, sums, slope,
                           eps, d_mean, d_rstd, 0, 1, 0L);
    } else {
        double *sums = static_cast<double *>(ctx->zeroed(sizeof(double) * 2 * (size_t)B * C, stream));   // pre-zeroed ring slot
        if (!sums) return -1;
        // optional image groups (nhwc_group): statistics and application of one group back to back
        const int group = nhwc_group(B, (size_t)hw * C * 2);
        const int splits = nhwc_splits(ctx, group, hw);
        dim3 grid((unsigned)splits, (unsigned)group);
        for (int b0 = 0; b0 < B; b0 += group) {
            if (b0 + group > B) grid.y = (unsigned)(B - b0);
            launch_x_stats(grid, stream, x, (long)hw, C, sums, b0);
            hipLaunchKernelGGL(in_nhwc_fwd_apply, grid, dim3(NT), 0, stream, x, y, d_w, d_b, (long)hw, C, splits, sums, slope, eps, d_mean, d_rstd, b0, 1, 0L);
        }
    }
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_instnorm_lrelu_nhwc_bwd(octa_ctx *ctx, const void *d_x, const void *d_dy, const float *d_w, const float *d_b,
                                            const float *d_mean, const float *d_rstd, void *d_dx, float *d_dw, float *d_db, int B,
                                            int C, int64_t hw, float slope, void *stream_) {
    if (int rc = nhwc_enter("octa_instnorm_lrelu_nhwc_bwd", ctx, d_x && d_dy && d_dx && d_mean && d_rstd, B, C, hw)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    double *sums = static_cast<double *>(ctx->zeroed(sizeof(double) * 2 * (size_t)B * C, stream));   // pre-zeroed ring slot
    if (!sums) return -1;
    const int group = nhwc_group(B, (size_t)hw * C * 2 * 2);   // two tensors (x, dy) are read twice
    const int bsum = group == B ? B : 0;                         // one launch covers the batch: gradients are stored, not accumulated
    if (!bsum && zero_affine_grads(d_dw, d_db, C, stream)) return -1;
    const int splits = nhwc_splits(ctx, group, hw);
    dim3 grid((unsigned)splits, (unsigned)group);
    const unsigned short *x = static_cast<const unsigned short *>(d_x), *dy = static_cast<const unsigned short *>(d_dy);
    for (int b0 = 0; b0 < B; b0 += group) {
        if (b0 + group > B) grid.y = (unsigned)(B - b0);
        hipLaunchKernelGGL(in_nhwc_stats<1>, grid, dim3(NT), 0, stream, x, dy, d_w, d_b, d_mean, d_rstd, (long)hw, C, splits, slope, sums, b0);
        hipLaunchKernelGGL(in_nhwc_bwd_apply, grid, dim3(NT), 0, stream, x, dy, static_cast<unsigned short *>(d_dx), d_w, d_b, d_mean, d_rstd,
                           (long)hw, C, splits, slope, sums, d_dw, d_db, b0, bsum);
    }
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- 5. last layer of the U-Net fused: InstanceNorm(affine) + LeakyReLU + 1x1 convolution to ONE channel ---------------------
// DynUNet's last UnetBasicBlock norm followed by UnetOutBlock (MONAI, models/networks.py:6; 32 -> 1 at 1216^2). Unfused, the
// normalised tensor y (378 MB at B = 4) is written by the norm, read by the head, its gradient is written by the head's backward
// and read twice by the norm's backward. Here y and dL/dy never exist in HBM: the head's dot product runs on the values the
// apply pass has in registers, and backward rebuilds dL/dy[p][c] = dlogit[p] * head_w[c] from the one-channel logit gradient.
// HBM traffic per step: forward x twice + logits (instead of x twice, y twice); backward x twice + dx once (instead of
// x twice, dy three times, y once, dx once). Same thread layout as the kernels above: the C/8 channel groups of a pixel sit in
// adjacent lanes, so the dot product closes with C/8 - 1 lane exchanges.
namespace {

__global__ void __launch_bounds__(NT)
in_nhwc_head_fwd(const unsigned short *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, long hw, int C, int splits,
                 const double *__restrict__ sums, float slope, float eps, float *__restrict__ mean_out, float *__restrict__ rstd_out,
                 const float *__restrict__ headw, const float *__restrict__ headb, unsigned short *__restrict__ logits, int nslot,
                 long slot_stride) {
    __shared__ float s_g[NHWC_MAXC], s_sh[NHWC_MAXC];
    const int b = blockIdx.y, s = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += NT) scale_shift_to_lds(sums, nslot, slot_stride, w, bias, hw, C, b, c, s, eps, mean_out, rstd_out, s_g, s_sh);
    __syncthreads();
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);                 // host guarantees NT % (C / 8) == 0 and C / 8 a power of two <= 64
    const int groups = C / 8;
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float g[8], sh[8], hv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { g[k] = s_g[cg * 8 + k]; sh[k] = s_sh[cg * 8 + k]; hv[k] = headw[cg * 8 + k]; }
    const float hb = headb ? *headb : 0.f;
    const unsigned short *px = x + ((long)b * hw) * C + cg * 8;
    unsigned short *pl_out = logits + (long)b * hw;
    long p = p0 + pl;
    for (; p + 3L * npl < p1; p += 4L * npl) {
        float v[4][8], dot[4];
#pragma unroll
        for (int u = 0; u < 4; u++) Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            dot[u] = 0.f;
#pragma unroll
            for (int k = 0; k < 8; k++) dot[u] += lrelu(v[u][k] * g[k] + sh[k], slope) * hv[k];
            for (int d = 1; d < groups; d <<= 1) dot[u] += __shfl_xor(dot[u], d, 64);
            if (cg == 0) pl_out[p + (long)u * npl] = octa_f2bf(dot[u] + hb);
        }
    }
    for (; p < p1; p += npl) {
        float v[8], dot = 0.f;
        Vec<unsigned short>::load(px + p * C, v);
#pragma unroll
        for (int k = 0; k < 8; k++) dot += lrelu(v[k] * g[k] + sh[k], slope) * hv[k];
        for (int d = 1; d < groups; d <<= 1) dot += __shfl_xor(dot, d, 64);
        if (cg == 0) pl_out[p] = octa_f2bf(dot + hb);
    }
}

// sums[b][c] = (sum g, sum g * xhat) with g = dlogit * head_w[c] * lrelu'(pre); hsums[c] += sum y * dlogit (head weight gradient),
// hsums[C] += sum dlogit (head bias gradient)
__global__ void __launch_bounds__(NT)
in_nhwc_head_bwd_stats(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dl, const float *__restrict__ w,
                       const float *__restrict__ bias, const float *__restrict__ mean, const float *__restrict__ rstd, long hw, int C, int splits,
                       float slope, const float *__restrict__ headw, double *__restrict__ sums, double *__restrict__ hsums) {
    __shared__ float s_red[2 * NT * 8];
    const int b = blockIdx.y, s = blockIdx.x;
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float a[8], q[8], t[8], sdl = 0.f, mu[8], rs[8], wc[8], bc[8], hv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int c = cg * 8 + k;
        a[k] = 0.f; q[k] = 0.f; t[k] = 0.f;
        load_consts(mean, rstd, w, bias, b, C, c, mu[k], rs[k], wc[k], bc[k]);
        hv[k] = headw[c];
    }
    const unsigned short *px = x + ((long)b * hw) * C + cg * 8;
    const unsigned short *pd = dl + (long)b * hw;
    long p = p0 + pl;
    for (; p + (long)npl < p1; p += 2L * npl) {
        float v[2][8], d[2];
#pragma unroll
        for (int u = 0; u < 2; u++) { Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]); d[u] = Vec<unsigned short>::up(pd[p + (long)u * npl]); }
#pragma unroll
        for (int u = 0; u < 2; u++) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float xh = (v[u][k] - mu[k]) * rs[k];
                const float gk = lrelu_gate(xh, wc[k], bc[k], d[u] * hv[k], slope);
                a[k] += gk; q[k] += gk * xh; t[k] += lrelu(xh * wc[k] + bc[k], slope) * d[u];
            }
            sdl += d[u];
        }
    }
    for (; p < p1; p += npl) {
        float v[8];
        Vec<unsigned short>::load(px + p * C, v);
        const float d = Vec<unsigned short>::up(pd[p]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float xh = (v[k] - mu[k]) * rs[k];
            const float gk = lrelu_gate(xh, wc[k], bc[k], d * hv[k], slope);
            a[k] += gk; q[k] += gk * xh; t[k] += lrelu(xh * wc[k] + bc[k], slope) * d;
        }
        sdl += d;
    }
    const int groups = C / 8;
#pragma unroll
    for (int k = 0; k < 8; k++) { s_red[(threadIdx.x * 8 + k) * 2] = a[k]; s_red[(threadIdx.x * 8 + k) * 2 + 1] = q[k]; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NT) {
        const int g = c / 8, k = c % 8;
        double sa = 0, sq = 0;
        for (int l = 0; l < npl; l++) { const int tt = l * groups + g; sa += s_red[(tt * 8 + k) * 2]; sq += s_red[(tt * 8 + k) * 2 + 1]; }
        atomicAdd(&sums[((long)b * C + c) * 2], sa);
        atomicAdd(&sums[((long)b * C + c) * 2 + 1], sq);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 8; k++) { s_red[(threadIdx.x * 8 + k) * 2] = t[k]; s_red[(threadIdx.x * 8 + k) * 2 + 1] = (k == 0 && cg == 0) ? sdl : 0.f; }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += NT) {
        const int g = c / 8, k = c % 8;
        double st = 0;
        for (int l = 0; l < npl; l++) { const int tt = l * groups + g; st += s_red[(tt * 8 + k) * 2]; }
        atomicAdd(&hsums[c], st);
    }
    if (threadIdx.x == 0) {
        double sd = 0;
        for (int l = 0; l < npl; l++) sd += s_red[((l * groups) * 8) * 2 + 1];
        atomicAdd(&hsums[C], sd);
    }
}

__global__ void __launch_bounds__(NT)
in_nhwc_head_bwd_apply(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dl, unsigned short *__restrict__ dx,
                       const float *__restrict__ w, const float *__restrict__ bias, const float *__restrict__ mean, const float *__restrict__ rstd,
                       long hw, int C, int splits, float slope, const float *__restrict__ headw, const double *__restrict__ sums,
                       const double *__restrict__ hsums, float *__restrict__ dw, float *__restrict__ db, float *__restrict__ dheadw,
                       float *__restrict__ dheadb) {
    __shared__ float s_mg[NHWC_MAXC], s_mgx[NHWC_MAXC];
    const int b = blockIdx.y, s = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += NT) {
        const double sa = sums[((long)b * C + c) * 2], sq = sums[((long)b * C + c) * 2 + 1];
        if (s == 0) {
            if (db) atomicAdd(&db[c], (float)sa);
            if (dw) atomicAdd(&dw[c], (float)sq);
            if (b == 0) dheadw[c] = (float)hsums[c];
        }
        s_mg[c] = (float)(sa / (double)hw); s_mgx[c] = (float)(sq / (double)hw);
    }
    if (s == 0 && b == 0 && threadIdx.x == 0 && dheadb) *dheadb = (float)hsums[C];
    __syncthreads();
    int cg, pl, npl;
    nhwc_geometry(C, cg, pl, npl);
    long p0, p1; pixel_range(hw, splits, s, p0, p1);
    float mu[8], rs[8], wc[8], bc[8], mg[8], mgx[8], hv[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const int c = cg * 8 + k;
        load_consts(mean, rstd, w, bias, b, C, c, mu[k], rs[k], wc[k], bc[k]);
        mg[k] = s_mg[c]; mgx[k] = s_mgx[c]; hv[k] = headw[c];
    }
    const unsigned short *px = x + ((long)b * hw) * C + cg * 8;
    const unsigned short *pd = dl + (long)b * hw;
    unsigned short *po = dx + ((long)b * hw) * C + cg * 8;
    long p = p0 + pl;
    for (; p + 3L * npl < p1; p += 4L * npl) {
        float v[4][8], d[4];
#pragma unroll
        for (int u = 0; u < 4; u++) { Vec<unsigned short>::load(px + (p + (long)u * npl) * C, v[u]); d[u] = Vec<unsigned short>::up(pd[p + (long)u * npl]); }
#pragma unroll
        for (int u = 0; u < 4; u++) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const float xh = (v[u][k] - mu[k]) * rs[k];
                v[u][k] = norm_dx(wc[k] * rs[k], lrelu_gate(xh, wc[k], bc[k], d[u] * hv[k], slope), mg[k], xh, mgx[k]);
            }
            Vec<unsigned short>::store(po + (p + (long)u * npl) * C, v[u]);
        }
    }
    for (; p < p1; p += npl) {
        float v[8];
        Vec<unsigned short>::load(px + p * C, v);
        const float d = Vec<unsigned short>::up(pd[p]);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const float xh = (v[k] - mu[k]) * rs[k];
            v[k] = norm_dx(wc[k] * rs[k], lrelu_gate(xh, wc[k], bc[k], d * hv[k], slope), mg[k], xh, mgx[k]);
        }
        Vec<unsigned short>::store(po + p * C, v);
    }
}

int head_check(const char *who, int B, int C, int64_t hw) {
    if (nhwc_check(who, B, C, hw)) return -2;
    const int groups = C / 8;
    if (C > 256 || (groups & (groups - 1)) || NT % groups) { octa::set_error("%s: C must be 8, 16, 32, 64, 128 or 256 (got %d)", who, C); return -2; }
    return 0;
}

}  // namespace

// d_slots (NULL = a statistics pass of its own): the statistics of d_x in slot form, double [nslot][B][C][2], from the convolution that wrote it
// (octa_conv3x3_nhwc_fwd's d_stat_slots): no statistics pass over the 1216^2 x 32 tensor in front of the head.
extern "C" int octa_instnorm_lrelu_head1_nhwc_fwd(octa_ctx *ctx, const void *d_x, const float *d_w, const float *d_b, const float *d_head_w,
                                                  const float *d_head_b, float *d_mean, float *d_rstd, void *d_logits, int B, int C, int64_t hw,
                                                  float slope, float eps, const double *d_slots, int nslot, void *stream_) {
    if (int rc = nhwc_enter("octa_instnorm_lrelu_head1_nhwc_fwd", ctx, d_x && d_head_w && d_mean && d_rstd && d_logits && !(d_slots && nslot <= 0), B, C, hw,
                            head_check))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    const int splits = nhwc_splits(ctx, B, hw);
    const dim3 grid((unsigned)splits, (unsigned)B);
    const unsigned short *x = static_cast<const unsigned short *>(d_x);
    const double *sums = d_slots;
    if (!d_slots) {
        double *own = static_cast<double *>(ctx->zeroed(sizeof(double) * 2 * (size_t)B * C, stream));
        if (!own) return -1;
        launch_x_stats(grid, stream, x, (long)hw, C, own, 0);
        sums = own;
    }
    hipLaunchKernelGGL(in_nhwc_head_fwd, grid, dim3(NT), 0, stream, x, d_w, d_b, (long)hw, C, splits, sums, slope, eps, d_mean, d_rstd, d_head_w, d_head_b,
                       static_cast<unsigned short *>(d_logits), d_slots ? nslot : 1, d_slots ? (long)B * C * 2 : 0L);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_instnorm_lrelu_head1_nhwc_bwd(octa_ctx *ctx, const void *d_x, const void *d_dlogits, const float *d_w, const float *d_b,
                                                  const float *d_head_w, const float *d_mean, const float *d_rstd, void *d_dx, float *d_dw,
                                                  float *d_db, float *d_dhead_w, float *d_dhead_b, int B, int C, int64_t hw, float slope,
                                                  void *stream_) {
    if (int rc = nhwc_enter("octa_instnorm_lrelu_head1_nhwc_bwd", ctx, d_x && d_dlogits && d_head_w && d_mean && d_rstd && d_dx && d_dhead_w, B, C, hw,
                            head_check))
        return rc;
    hipStream_t stream = (hipStream_t)stream_;
    double *sums = static_cast<double *>(ctx->zeroed(sizeof(double) * (2 * (size_t)B * C + C + 1), stream));
    if (!sums) return -1;
    double *hsums = sums + 2 * (size_t)B * C;
    if (zero_affine_grads(d_dw, d_db, C, stream)) return -1;
    const int splits = nhwc_splits(ctx, B, hw);
    const dim3 grid((unsigned)splits, (unsigned)B);
    const unsigned short *x = static_cast<const unsigned short *>(d_x), *dl = static_cast<const unsigned short *>(d_dlogits);
    hipLaunchKernelGGL(in_nhwc_head_bwd_stats, grid, dim3(NT), 0, stream, x, dl, d_w, d_b, d_mean, d_rstd, (long)hw, C, splits, slope, d_head_w, sums, hsums);
    hipLaunchKernelGGL(in_nhwc_head_bwd_apply, grid, dim3(NT), 0, stream, x, dl, static_cast<unsigned short *>(d_dx), d_w, d_b, d_mean, d_rstd,
                       (long)hw, C, splits, slope, d_head_w, sums, hsums, d_dw, d_db, d_dhead_w, d_dhead_b);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
