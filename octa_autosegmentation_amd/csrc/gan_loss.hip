// gan_loss.hip -- the elementwise tail of the CycleGAN step (reference models/cycle_gan.py:169-228): weighted L1 terms, LSGAN terms,
// background mixing and the image pool. The tensors are small (B x 1 x 304 x 304 and PatchGAN maps) and the torch composition is a
// chain of 70 - 80 short dependent launches; here every group of terms is one launch each way.
//
// Deterministic, no atomics: every sum is a per-thread serial sum over a fixed stride, a fixed shuffle tree per wave, a fixed order over
// the waves of a workgroup and (L1) a fixed order over the workgroups' partials -- all in double. Elements are dtype 0 = float32 or
// 1 = bfloat16 (the octa_dice_bce_* convention). Rows whose base is 16-byte aligned move as 16-byte vectors, eight elements per thread
// and trip, with a scalar tail; other rows (a slice at an odd offset) run the scalar loop throughout.

#include "common.h"

namespace {

typedef unsigned short bf16_t;

template <class T> __device__ __forceinline__ float ld1(const T *p, long i);
template <> __device__ __forceinline__ float ld1<float>(const float *p, long i) { return p[i]; }
template <> __device__ __forceinline__ float ld1<bf16_t>(const bf16_t *p, long i) { return __uint_as_float((unsigned)p[i] << 16); }
template <class T> __device__ __forceinline__ void st1(T *p, long i, float v);
template <> __device__ __forceinline__ void st1<float>(float *p, long i, float v) { p[i] = v; }
template <> __device__ __forceinline__ void st1<bf16_t>(bf16_t *p, long i, float v) { p[i] = octa_f2bf(v); }
// a value as the tensor's dtype holds it
template <class T> __device__ __forceinline__ float rnd(float v);
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }
template <> __device__ __forceinline__ float rnd<bf16_t>(float v) { return __uint_as_float((unsigned)octa_f2bf(v) << 16); }

struct F8 { float v[8]; };
// elements 8c .. 8c + 7 of a row with a 16-byte-aligned base
template <class T> __device__ __forceinline__ F8 ld8(const T *p, long c);
template <> __device__ __forceinline__ F8 ld8<float>(const float *p, long c) {
    const float4 a = reinterpret_cast<const float4 *>(p)[2 * c], b = reinterpret_cast<const float4 *>(p)[2 * c + 1];
    return {{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
template <> __device__ __forceinline__ F8 ld8<bf16_t>(const bf16_t *p, long c) {
    const uint4 a = reinterpret_cast<const uint4 *>(p)[c];
    return {{__uint_as_float(a.x << 16), __uint_as_float(a.x & 0xffff0000u), __uint_as_float(a.y << 16), __uint_as_float(a.y & 0xffff0000u),
             __uint_as_float(a.z << 16), __uint_as_float(a.z & 0xffff0000u), __uint_as_float(a.w << 16), __uint_as_float(a.w & 0xffff0000u)}};
}
template <class T> __device__ __forceinline__ void st8(T *p, long c, const F8 &f);
template <> __device__ __forceinline__ void st8<float>(float *p, long c, const F8 &f) {
    reinterpret_cast<float4 *>(p)[2 * c] = make_float4(f.v[0], f.v[1], f.v[2], f.v[3]);
    reinterpret_cast<float4 *>(p)[2 * c + 1] = make_float4(f.v[4], f.v[5], f.v[6], f.v[7]);
}
template <> __device__ __forceinline__ void st8<bf16_t>(bf16_t *p, long c, const F8 &f) {
    reinterpret_cast<uint4 *>(p)[c] = make_uint4(octa_pack_bf16x2(f.v[0], f.v[1]), octa_pack_bf16x2(f.v[2], f.v[3]),
                                                 octa_pack_bf16x2(f.v[4], f.v[5]), octa_pack_bf16x2(f.v[6], f.v[7]));
}

__host__ __device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// sum over the workgroup (up to 16 waves), the same tree every time; every thread gets the result
__device__ __forceinline__ double block_sum(double a, double *sh) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = a;
    __syncthreads();
    double r = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); w++) r += sh[w];
    __syncthreads();
    return r;
}

// the grid-stride range of this thread: vector chunks [0, nv) of eight, then scalars [8 nv, n)
#define OCTA_FOR_CHUNKS(c, nv) for (long c = (long)blockIdx.x * blockDim.x + threadIdx.x; c < (nv); c += (long)gridDim.x * blockDim.x)
#define OCTA_FOR_TAIL(i, nv, n) for (long i = 8 * (nv) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// ---- weighted L1 terms ------------------------------------------------------------------------------------------------------------
constexpr int L1_MAX = 4;
struct L1Terms {
    const void *pred[L1_MAX];
    const void *target[L1_MAX];
    void *dpred[L1_MAX];
    long n[L1_MAX];
    float coef[L1_MAX];       // float(w_k / n_k)
};

template <class TP, class TT>
__global__ void __launch_bounds__(256)
l1_partial_kernel(L1Terms t, double *__restrict__ partials) {
    __shared__ double sh[16];
    const int k = blockIdx.y;
    const TP *p = static_cast<const TP *>(t.pred[k]);
    const TT *q = static_cast<const TT *>(t.target[k]);
    const long n = t.n[k], nv = aligned16(p) && aligned16(q) ? n / 8 : 0;
    double acc = 0;
    OCTA_FOR_CHUNKS(c, nv) {
        const F8 a = ld8(p, c), b = ld8(q, c);
#pragma unroll
        for (int j = 0; j < 8; j++) acc += fabs((double)a.v[j] - (double)b.v[j]);
    }
    OCTA_FOR_TAIL(i, nv, n) acc += fabs((double)ld1(p, i) - (double)ld1(q, i));
    const double r = block_sum(acc, sh);
    if (threadIdx.x == 0) partials[(long)k * gridDim.x + blockIdx.x] = r;
}

// one wave per term: the partials in a fixed order
__global__ void __launch_bounds__(64)
l1_fold_kernel(const double *__restrict__ partials, int gx, double *__restrict__ sums) {
    const int k = blockIdx.x;
    double a = 0;
    for (int i = threadIdx.x; i < gx; i += 64) a += partials[(long)k * gx + i];
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d, 64);
    if (threadIdx.x == 0) sums[k] = a;
}

struct L1Finish { double w[L1_MAX]; double n[L1_MAX]; };
__global__ void l1_finish_kernel(const double *__restrict__ sums, int K, L1Finish f, float *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double total = 0;
    for (int k = 0; k < K; k++) {
        const double v = f.w[k] * sums[k] / f.n[k];
        out[k] = (float)v;
        total += v;
    }
    out[K] = (float)total;
}

template <class TP, class TT>
__global__ void __launch_bounds__(256)
l1_bwd_kernel(L1Terms t, const float *__restrict__ gout) {
    const int k = blockIdx.y;
    const TP *p = static_cast<const TP *>(t.pred[k]);
    const TT *q = static_cast<const TT *>(t.target[k]);
    TP *d = static_cast<TP *>(t.dpred[k]);
    const long n = t.n[k], nv = aligned16(p) && aligned16(q) && aligned16(d) ? n / 8 : 0;
    const float c = gout[0] * t.coef[k];
    OCTA_FOR_CHUNKS(ch, nv) {
        const F8 a = ld8(p, ch), b = ld8(q, ch);
        F8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) o.v[j] = c * (float)((a.v[j] > b.v[j]) - (a.v[j] < b.v[j]));
        st8(d, ch, o);
    }
    OCTA_FOR_TAIL(i, nv, n) {
        const float a = ld1(p, i), b = ld1(q, i);
        st1(d, i, c * (float)((a > b) - (a < b)));
    }
}

// ---- LSGAN terms ------------------------------------------------------------------------------------------------------------------
constexpr int LS_MAX = 2;
struct LsTerms {
    const void *p[LS_MAX];
    void *dp[LS_MAX];
    long n[LS_MAX];
    float target[LS_MAX];
    double scale[LS_MAX];
    float coef[LS_MAX];       // float(2 scale_k / n_k)
};

// one workgroup: PatchGAN maps are a few thousand elements
template <class T>
__global__ void __launch_bounds__(1024)
lsgan_fwd_kernel(LsTerms t, int nterms, double *__restrict__ sums, float *__restrict__ loss) {
    __shared__ double sh[16];
    double total = 0;
    for (int k = 0; k < nterms; k++) {
        const T *p = static_cast<const T *>(t.p[k]);
        const long n = t.n[k], nv = aligned16(p) ? n / 8 : 0;
        const double tg = (double)t.target[k];
        double acc = 0;
        OCTA_FOR_CHUNKS(c, nv) {
            const F8 a = ld8(p, c);
#pragma unroll
            for (int j = 0; j < 8; j++) { const double d = (double)a.v[j] - tg; acc += d * d; }
        }
        OCTA_FOR_TAIL(i, nv, n) { const double d = (double)ld1(p, i) - tg; acc += d * d; }
        const double r = block_sum(acc, sh);
        const double v = t.scale[k] * r / (double)n;
        if (threadIdx.x == 0) { sums[k] = r; loss[k] = (float)v; }
        total += v;
    }
    if (threadIdx.x == 0) loss[nterms] = (float)total;
}

template <class T>
__global__ void __launch_bounds__(256)
lsgan_bwd_kernel(LsTerms t, const float *__restrict__ gout) {
    const int k = blockIdx.y;
    const T *p = static_cast<const T *>(t.p[k]);
    T *d = static_cast<T *>(t.dp[k]);
    const long n = t.n[k], nv = aligned16(p) && aligned16(d) ? n / 8 : 0;
    const float c = gout[0] * t.coef[k], tg = t.target[k];
    OCTA_FOR_CHUNKS(ch, nv) {
        const F8 a = ld8(p, ch);
        F8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) o.v[j] = c * (a.v[j] - tg);
        st8(d, ch, o);
    }
    OCTA_FOR_TAIL(i, nv, n) st1(d, i, c * (ld1(p, i) - tg));
}

// ---- background mixing: out = max(x, bg * u) ----------------------------------------------------------------------------------------
__device__ __forceinline__ float max_like_torch(float x, float m) { return (x > m || x != x) ? x : m; }    // NaN of either side comes through

template <class TX, class TM, class TO>
__global__ void __launch_bounds__(256)
mix_max_fwd_kernel(const TX *__restrict__ x, const TM *__restrict__ bg, const TM *__restrict__ u, long n, TO *__restrict__ out) {
    const long nv = aligned16(x) && aligned16(bg) && aligned16(u) && aligned16(out) ? n / 8 : 0;
    OCTA_FOR_CHUNKS(c, nv) {
        const F8 a = ld8(x, c), b = ld8(bg, c), r = ld8(u, c);
        F8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) o.v[j] = max_like_torch(a.v[j], rnd<TM>(b.v[j] * r.v[j]));
        st8(out, c, o);
    }
    OCTA_FOR_TAIL(i, nv, n) st1(out, i, max_like_torch(ld1(x, i), rnd<TM>(ld1(bg, i) * ld1(u, i))));
}

__device__ __forceinline__ float mix_max_grad(float x, float m, float d) { return x > m ? d : (x == m ? 0.5f * d : 0.f); }

template <class TX, class TM, class TO>
__global__ void __launch_bounds__(256)
mix_max_bwd_kernel(const TX *__restrict__ x, const TM *__restrict__ bg, const TM *__restrict__ u, long n, const TO *__restrict__ dout, TX *__restrict__ dx) {
    const long nv = aligned16(x) && aligned16(bg) && aligned16(u) && aligned16(dout) && aligned16(dx) ? n / 8 : 0;
    OCTA_FOR_CHUNKS(c, nv) {
        const F8 a = ld8(x, c), b = ld8(bg, c), r = ld8(u, c), g = ld8(dout, c);
        F8 o;
#pragma unroll
        for (int j = 0; j < 8; j++) o.v[j] = mix_max_grad(a.v[j], rnd<TM>(b.v[j] * r.v[j]), g.v[j]);
        st8(dx, c, o);
    }
    OCTA_FOR_TAIL(i, nv, n) st1(dx, i, mix_max_grad(ld1(x, i), rnd<TM>(ld1(bg, i) * ld1(u, i)), ld1(dout, i)));
}

// ---- image pool -------------------------------------------------------------------------------------------------------------------
constexpr int POOL_MAX_BATCH = 32;
struct PoolTables {
    int src[POOL_MAX_BATCH];        // per returned image: k >= 0 = input k, -1 - s = the old content of slot s
    int wslot[POOL_MAX_BATCH];      // per touched slot ...
    int winput[POOL_MAX_BATCH];     // ... the input that ends up in it
};

// One thread owns unit e of EVERY image: it reads what the outputs need from the old slots, then overwrites the slots. No other
// thread touches unit e of any slot, so an old slot is never written before it has been read. `pool` is read and written through the one
// pointer (no __restrict__): the compiler keeps the loads in front of the stores.
template <class U>
__global__ void __launch_bounds__(256)
pool_exchange_kernel(U *pool, const U *in, U *out, long E, int B, int nw, PoolTables t) {
    for (long e = (long)blockIdx.x * 256 + threadIdx.x; e < E; e += (long)gridDim.x * 256) {
        for (int b = 0; b < B; b++) {
            const int s = t.src[b];
            out[(long)b * E + e] = s >= 0 ? in[(long)s * E + e] : pool[(long)(-1 - s) * E + e];
        }
        for (int j = 0; j < nw; j++) pool[(long)t.wslot[j] * E + e] = in[(long)t.winput[j] * E + e];
    }
}

unsigned stream_grid(const octa_ctx *ctx, long n, int rows) {
    long gx = (n + 256 * 8 - 1) / (256 * 8);
    const long cap = (8L * ctx->num_cus + rows - 1) / rows;
    if (gx > cap) gx = cap;
    return (unsigned)(gx < 1 ? 1 : gx);
}

bool dtype_ok(int d) { return d == 0 || d == 1; }

int fill_l1(const char *who, L1Terms &t, int K, const void *const *pred, const void *const *target, const int64_t *n, const double *w, void *const *dpred, long &n_max) {
    if (K < 1 || K > L1_MAX || !pred || !target || !n) { octa::set_error("%s: bad arguments (1 <= K <= %d terms)", who, L1_MAX); return -2; }
    n_max = 0;
    for (int k = 0; k < K; k++) {
        if (!pred[k] || !target[k] || n[k] <= 0 || (dpred && !dpred[k])) { octa::set_error("%s: term %d has a null pointer or no elements", who, k); return -2; }
        t.pred[k] = pred[k]; t.target[k] = target[k]; t.dpred[k] = dpred ? dpred[k] : nullptr; t.n[k] = (long)n[k];
        t.coef[k] = w ? (float)(w[k] / (double)n[k]) : 0.f;
        if (n[k] > n_max) n_max = (long)n[k];
    }
    return 0;
}

int fill_ls(const char *who, LsTerms &t, int T, const void *const *p, const int64_t *n, const float *target, const double *scale, void *const *dp, long &n_max) {
    if (T < 1 || T > LS_MAX || !p || !n || !target || !scale) { octa::set_error("%s: bad arguments (1 <= T <= %d terms)", who, LS_MAX); return -2; }
    n_max = 0;
    for (int k = 0; k < T; k++) {
        if (!p[k] || n[k] <= 0 || (dp && !dp[k])) { octa::set_error("%s: term %d has a null pointer or no elements", who, k); return -2; }
        t.p[k] = p[k]; t.dp[k] = dp ? dp[k] : nullptr; t.n[k] = (long)n[k]; t.target[k] = target[k]; t.scale[k] = scale[k];
        t.coef[k] = (float)(2.0 * scale[k] / (double)n[k]);
        if (n[k] > n_max) n_max = (long)n[k];
    }
    return 0;
}

}  // namespace

#define OCTA_L1_DISPATCH(kernel, grid, ...)                                                                                    \
    do {                                                                                                                       \
        if (pred_dtype == 0 && target_dtype == 0) hipLaunchKernelGGL((kernel<float, float>), grid, dim3(256), 0, stream, __VA_ARGS__);       \
        else if (pred_dtype == 0) hipLaunchKernelGGL((kernel<float, bf16_t>), grid, dim3(256), 0, stream, __VA_ARGS__);       \
        else if (target_dtype == 0) hipLaunchKernelGGL((kernel<bf16_t, float>), grid, dim3(256), 0, stream, __VA_ARGS__);     \
        else hipLaunchKernelGGL((kernel<bf16_t, bf16_t>), grid, dim3(256), 0, stream, __VA_ARGS__);                           \
    } while (0)

extern "C" int octa_l1_pairs_fwd(octa_ctx *ctx, int K, const void *const *h_pred, const void *const *h_target, const int64_t *h_n, int pred_dtype,
                                 int target_dtype, double *d_sums, void *stream_) {
    if (!ctx || !d_sums || !dtype_ok(pred_dtype) || !dtype_ok(target_dtype)) { octa::set_error("octa_l1_pairs_fwd: bad arguments"); return -2; }
    L1Terms t = {};
    long n_max;
    if (int rc = fill_l1("octa_l1_pairs_fwd", t, K, h_pred, h_target, h_n, nullptr, nullptr, n_max)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned gx = stream_grid(ctx, n_max, K);
    double *partials = ctx->work[3].take<double>((size_t)K * gx);
    if (!partials) return -1;
    OCTA_L1_DISPATCH(l1_partial_kernel, dim3(gx, (unsigned)K), t, partials);
    OCTA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(l1_fold_kernel, dim3((unsigned)K), dim3(64), 0, stream, partials, (int)gx, d_sums);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_l1_pairs_finish(octa_ctx *ctx, int K, const double *d_sums, const int64_t *h_n, const double *h_w, float *d_out, void *stream_) {
    if (!ctx || !d_sums || !h_n || !h_w || !d_out || K < 1 || K > L1_MAX) { octa::set_error("octa_l1_pairs_finish: bad arguments"); return -2; }
    L1Finish f = {};
    for (int k = 0; k < K; k++) {
        if (h_n[k] <= 0) { octa::set_error("octa_l1_pairs_finish: term %d has no elements", k); return -2; }
        f.w[k] = h_w[k]; f.n[k] = (double)h_n[k];
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(64), 0, stream, d_sums, K, f, d_out);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_l1_pairs_bwd(octa_ctx *ctx, int K, const void *const *h_pred, const void *const *h_target, const int64_t *h_n, const double *h_w,
                                 int pred_dtype, int target_dtype, const float *d_grad_out, void *const *h_dpred, void *stream_) {
    if (!ctx || !h_w || !d_grad_out || !h_dpred || !dtype_ok(pred_dtype) || !dtype_ok(target_dtype)) { octa::set_error("octa_l1_pairs_bwd: bad arguments"); return -2; }
    L1Terms t = {};
    long n_max;
    if (int rc = fill_l1("octa_l1_pairs_bwd", t, K, h_pred, h_target, h_n, h_w, h_dpred, n_max)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    OCTA_L1_DISPATCH(l1_bwd_kernel, dim3(stream_grid(ctx, n_max, K), (unsigned)K), t, d_grad_out);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_lsgan_fwd(octa_ctx *ctx, int T, const void *const *h_p, const int64_t *h_n, const float *h_target, const double *h_scale, int dtype,
                              double *d_sums, float *d_loss, void *stream_) {
    if (!ctx || !d_sums || !d_loss || !dtype_ok(dtype)) { octa::set_error("octa_lsgan_fwd: bad arguments"); return -2; }
    LsTerms t = {};
    long n_max;
    if (int rc = fill_ls("octa_lsgan_fwd", t, T, h_p, h_n, h_target, h_scale, nullptr, n_max)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    if (dtype == 0) hipLaunchKernelGGL(lsgan_fwd_kernel<float>, dim3(1), dim3(1024), 0, stream, t, T, d_sums, d_loss);
    else hipLaunchKernelGGL(lsgan_fwd_kernel<bf16_t>, dim3(1), dim3(1024), 0, stream, t, T, d_sums, d_loss);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_lsgan_bwd(octa_ctx *ctx, int T, const void *const *h_p, const int64_t *h_n, const float *h_target, const double *h_scale, int dtype,
                              const float *d_grad_out, void *const *h_dp, void *stream_) {
    if (!ctx || !d_grad_out || !h_dp || !dtype_ok(dtype)) { octa::set_error("octa_lsgan_bwd: bad arguments"); return -2; }
    LsTerms t = {};
    long n_max;
    if (int rc = fill_ls("octa_lsgan_bwd", t, T, h_p, h_n, h_target, h_scale, h_dp, n_max)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid(stream_grid(ctx, n_max, T), (unsigned)T);
    if (dtype == 0) hipLaunchKernelGGL(lsgan_bwd_kernel<float>, grid, dim3(256), 0, stream, t, d_grad_out);
    else hipLaunchKernelGGL(lsgan_bwd_kernel<bf16_t>, grid, dim3(256), 0, stream, t, d_grad_out);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// out (and dout) are bfloat16 when x and bg / u both are, float32 otherwise: torch's promotion of maximum(x, bg * u)
extern "C" int octa_mix_max_fwd(octa_ctx *ctx, const void *d_x, int x_dtype, const void *d_bg, const void *d_u, int m_dtype, int64_t n, void *d_out, void *stream_) {
    if (!ctx || !d_x || !d_bg || !d_u || !d_out || n <= 0 || !dtype_ok(x_dtype) || !dtype_ok(m_dtype)) { octa::set_error("octa_mix_max_fwd: bad arguments"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid(stream_grid(ctx, (long)n, 1));
    if (x_dtype == 0 && m_dtype == 0) hipLaunchKernelGGL((mix_max_fwd_kernel<float, float, float>), grid, dim3(256), 0, stream, (const float *)d_x, (const float *)d_bg, (const float *)d_u, (long)n, (float *)d_out);
    else if (x_dtype == 0) hipLaunchKernelGGL((mix_max_fwd_kernel<float, bf16_t, float>), grid, dim3(256), 0, stream, (const float *)d_x, (const bf16_t *)d_bg, (const bf16_t *)d_u, (long)n, (float *)d_out);
    else if (m_dtype == 0) hipLaunchKernelGGL((mix_max_fwd_kernel<bf16_t, float, float>), grid, dim3(256), 0, stream, (const bf16_t *)d_x, (const float *)d_bg, (const float *)d_u, (long)n, (float *)d_out);
    else hipLaunchKernelGGL((mix_max_fwd_kernel<bf16_t, bf16_t, bf16_t>), grid, dim3(256), 0, stream, (const bf16_t *)d_x, (const bf16_t *)d_bg, (const bf16_t *)d_u, (long)n, (bf16_t *)d_out);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_mix_max_bwd(octa_ctx *ctx, const void *d_x, int x_dtype, const void *d_bg, const void *d_u, int m_dtype, int64_t n, const void *d_dout,
                                void *d_dx, void *stream_) {
    if (!ctx || !d_x || !d_bg || !d_u || !d_dout || !d_dx || n <= 0 || !dtype_ok(x_dtype) || !dtype_ok(m_dtype)) { octa::set_error("octa_mix_max_bwd: bad arguments"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const dim3 grid(stream_grid(ctx, (long)n, 1));
    if (x_dtype == 0 && m_dtype == 0) hipLaunchKernelGGL((mix_max_bwd_kernel<float, float, float>), grid, dim3(256), 0, stream, (const float *)d_x, (const float *)d_bg, (const float *)d_u, (long)n, (const float *)d_dout, (float *)d_dx);
    else if (x_dtype == 0) hipLaunchKernelGGL((mix_max_bwd_kernel<float, bf16_t, float>), grid, dim3(256), 0, stream, (const float *)d_x, (const bf16_t *)d_bg, (const bf16_t *)d_u, (long)n, (const float *)d_dout, (float *)d_dx);
    else if (m_dtype == 0) hipLaunchKernelGGL((mix_max_bwd_kernel<bf16_t, float, float>), grid, dim3(256), 0, stream, (const bf16_t *)d_x, (const float *)d_bg, (const float *)d_u, (long)n, (const float *)d_dout, (bf16_t *)d_dx);
    else hipLaunchKernelGGL((mix_max_bwd_kernel<bf16_t, bf16_t, bf16_t>), grid, dim3(256), 0, stream, (const bf16_t *)d_x, (const bf16_t *)d_bg, (const bf16_t *)d_u, (long)n, (const bf16_t *)d_dout, (bf16_t *)d_dx);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_pool_exchange(octa_ctx *ctx, void *d_pool, int pool_size, const void *d_in, int B, void *d_out, int64_t elems, int dtype, const int *h_src,
                                  int nw, const int *h_wslot, const int *h_winput, void *stream_) {
    if (!ctx || !d_pool || !d_in || !d_out || !h_src || pool_size < 1 || B < 1 || B > POOL_MAX_BATCH || elems <= 0 || !dtype_ok(dtype) || nw < 0 || nw > B ||
        nw > pool_size || (nw > 0 && (!h_wslot || !h_winput))) {
        octa::set_error("octa_pool_exchange: bad arguments (1 <= B <= %d, at most one write per input and slot)", POOL_MAX_BATCH);
        return -2;
    }
    PoolTables t = {};
    for (int b = 0; b < B; b++) {
        if (h_src[b] >= B || h_src[b] < -pool_size) { octa::set_error("octa_pool_exchange: source %d of image %d is neither an input nor a slot", h_src[b], b); return -2; }
        t.src[b] = h_src[b];
    }
    for (int j = 0; j < nw; j++) {
        if (h_wslot[j] < 0 || h_wslot[j] >= pool_size || h_winput[j] < 0 || h_winput[j] >= B) { octa::set_error("octa_pool_exchange: write %d is outside the pool or the batch", j); return -2; }
        for (int i = 0; i < j; i++)
            if (h_wslot[i] == h_wslot[j]) { octa::set_error("octa_pool_exchange: slot %d is written twice", h_wslot[j]); return -2; }
        t.wslot[j] = h_wslot[j]; t.winput[j] = h_winput[j];
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const size_t esz = dtype == 0 ? 4 : 2, row = (size_t)elems * esz;
    if (row % 16 == 0 && aligned16(d_pool) && aligned16(d_in) && aligned16(d_out)) {
        const long E = (long)(row / 16);
        hipLaunchKernelGGL(pool_exchange_kernel<uint4>, dim3(stream_grid(ctx, E * 8, 1)), dim3(256), 0, stream, (uint4 *)d_pool, (const uint4 *)d_in, (uint4 *)d_out, E, B, nw, t);
    } else if (dtype == 0) {
        hipLaunchKernelGGL(pool_exchange_kernel<unsigned>, dim3(stream_grid(ctx, (long)elems * 8, 1)), dim3(256), 0, stream, (unsigned *)d_pool, (const unsigned *)d_in, (unsigned *)d_out, (long)elems, B, nw, t);
    } else {
        hipLaunchKernelGGL(pool_exchange_kernel<bf16_t>, dim3(stream_grid(ctx, (long)elems * 8, 1)), dim3(256), 0, stream, (bf16_t *)d_pool, (const bf16_t *)d_in, (bf16_t *)d_out, (long)elems, B, nw, t);
    }
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
