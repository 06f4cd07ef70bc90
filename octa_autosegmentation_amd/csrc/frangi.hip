// frangi.hip -- the Frangi vesselness filter, the classical baseline of `General.model.name: frangi` (reference models/frangi.py:
// skimage.filters.frangi(img * 255, sigmas, alpha=1, beta, black_ridges=False), configs/config_frangi.yml), 2-D.
//
// The filter is discontinuous (a pixel jumps between 0 and ~1 with the order and the sign of two eigenvalues), so the Hessian and
// its eigenvalues are computed to the BIT as scipy.ndimage.gaussian_filter and numpy compute them in float32; only the two exp
// calls of the vesselness may differ from numpy's, by float32 ulps.
//
// Hessian of one scale (skimage hessian_matrix, use_gaussian_derivatives=True, mode 'reflect'): five gaussian_filter calls at
// sigma' = sigma / sqrt(2), each a 1-D pass down the rows (axis 0) followed by one along the rows (axis 1), every pass rounded
// to float32:      g0 = G(1,0) a,  g1 = G(0,1) a,  Hrr = G(1,0) g0,  Hrc = G(0,1) g0,  Hcc = G(0,1) g1.
// One pass over a line x (scipy's correlate1d, the symmetric / antisymmetric branch): with the weights t[j] of offset +j,
//     out[l] = float32( x[l] t[0] + sum over j = R, R-1, ..., 1 of (x[l-j] +- x[l+j]) t[j] ),        + order 0, - order 1,
// in double, one add per term in that order, no fused multiply-add (the pragma below and -ffp-contract=off), indices reflected
// with period 2n. Taps beyond the last non-zero weight are dropped (the host passes the effective radius): a term that is +-0
// changes nothing but the sign of a zero sum.
// The pass is sep_pass.h's sep_pass_kernel<AXIS> (shared with morph.hip); it may write two outputs of the same input with two
// tables -- the axis-0 passes of a and of g0 are needed in both orders -- so a scale is 8 launches.
//
// Eigenvalues (skimage hessian_matrix_eigvals, float32): m = (Hrr + Hcc) / 2, d = sqrt(Hrc^2 + ((Hrr - Hcc) / 2)^2), e0 = m + d,
// e1 = m - d, sorted by magnitude stably (e0 first on a tie). Vesselness (skimage frangi): l2c = max(l2, 1e-10f), rb = |l1| / l2c,
// s = sqrt(l1^2 + l2^2), E = exp(-rb^2 / (2 beta^2)), T = 1 - exp(-s^2 / (2 gamma^2)) in float32, v = E T in double, the output
// the maximum of v over the scales. gamma = max(s) / 2 of the FIRST scale per image (1 when 0): a block maximum, then an integer
// atomic maximum on the bit pattern of the non-negative float -- order-independent, so the result is the same on every run.
// float32 divide and square root go through double ((float)((double)a / b), (float)sqrt((double)x)): correctly rounded whatever
// the compiler's float32 settings (53 >= 2 * 24 + 2), subnormal results included. exp is the double exp rounded to float32.

#include "sep_pass.h"

#include <algorithm>

#pragma clang fp contract(off)

namespace {

using octa::sep::kThreads;
using octa::sep::kMaxRadius;
using octa::sep::Taps;
using octa::sep::pass;
using octa::sep::div_rn;
using octa::sep::sqrt_rn;

constexpr int kMaxDim = 4096;
constexpr int kMaxScales = 8;
constexpr int kMaxTableRadius = 1 << 20;

__device__ __forceinline__ float exp_f32(float a) { return (float)exp((double)a); }

// sorted eigenvalues (|l1| <= |l2|, e0 first on a tie) of [[rr, rc], [rc, cc]] and s = sqrt(l1^2 + l2^2), float32
__device__ __forceinline__ void eigen(float rr, float rc, float cc, float &l1, float &l2, float &s) {
    const float m = (rr + cc) / 2.0f, q = (rr - cc) / 2.0f;
    const float d = sqrt_rn(rc * rc + q * q);
    const float e0 = m + d, e1 = m - d;
    const bool swap = fabsf(e1) < fabsf(e0);
    l1 = swap ? e1 : e0;
    l2 = swap ? e0 : e1;
    s = sqrt_rn(l1 * l1 + l2 * l2);
}

// grid (chunks, b). smax_bits[img] (zeroed before) = bit pattern of max s over the image; l1 / l2 (may be null) the sorted eigenvalues
__global__ void __launch_bounds__(kThreads) frangi_eigen_kernel(const float *__restrict__ rr, const float *__restrict__ rc, const float *__restrict__ cc,
                                                               float *__restrict__ l1o, float *__restrict__ l2o, unsigned *__restrict__ smax_bits, long long hw) {
    __shared__ float red[kThreads];
    const long long base = (long long)blockIdx.y * hw;
    float m = 0.0f;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (long long)gridDim.x * kThreads) {
        float l1, l2, s;
        eigen(rr[base + i], rc[base + i], cc[base + i], l1, l2, s);
        if (l1o) { l1o[base + i] = l1; l2o[base + i] = l2; }
        m = fmaxf(m, s);
    }
    red[threadIdx.x] = m;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + k]);
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicMax(smax_bits + blockIdx.y, __float_as_uint(red[0]));   // s >= +0: the bit patterns order as the values do
}

// gamma[img] = max(s) / 2, or 1 when that is 0 (float32)
__global__ void frangi_gamma_kernel(const unsigned *__restrict__ smax_bits, float *__restrict__ gamma, int b) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= b) return;
    const float g = __uint_as_float(smax_bits[i]) / 2.0f;
    gamma[i] = g == 0.0f ? 1.0f : g;
}

// grid (chunks, b). planes: per scale Hrr, Hrc, Hcc of `total` floats each. out = max over the scales of E T (double), from 0.
// den_t > 0: the fixed 2 gamma^2; otherwise 2 gamma^2 of the image's own gamma, formed in float32.
__global__ void __launch_bounds__(kThreads) frangi_vesselness_kernel(const float *__restrict__ planes, int n_scales, long long total, const unsigned *__restrict__ smax_bits,
                                                                    float den_b, float den_t, double *__restrict__ out, long long hw) {
    float den = den_t;
    if (!(den > 0.0f)) {
        float g = __uint_as_float(smax_bits[blockIdx.y]) / 2.0f;
        if (g == 0.0f) g = 1.0f;
        den = 2.0f * (g * g);
    }
    const long long base = (long long)blockIdx.y * hw;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (long long)gridDim.x * kThreads) {
        double best = 0.0;
        for (int sc = 0; sc < n_scales; ++sc) {
            const float *p = planes + 3 * sc * total + base + i;
            float l1, l2, s;
            eigen(p[0], p[total], p[2 * total], l1, l2, s);
            const float l2c = fmaxf(l2, 1e-10f);
            const float rb = div_rn(fabsf(l1), l2c);
            const float E = exp_f32(div_rn(-(rb * rb), den_b));
            const float T = 1.0f - exp_f32(div_rn(-(s * s), den));
            best = fmax(best, (double)E * (double)T);
        }
        out[base + i] = best;
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

bool bad_dims(int b, int h, int w, const char *who) {
    if (b < 1 || b > 65535 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim) {
        octa::set_error("%s: need 1 <= b <= 65535 and 1 <= h, w <= %d (got b=%d h=%d w=%d)", who, kMaxDim, b, h, w);
        return true;
    }
    return false;
}

// workspace: 3 Hessian planes per scale, 4 scratch planes (two gradients, two axis-0 results), max-s bits per image
struct Ws {
    float *planes, *g0, *g1, *t0, *t1;
    unsigned *smax;
};
size_t ws_layout(int b, int h, int w, int n_scales, char *base, Ws *ws) {
    const size_t plane = (size_t)b * h * w * sizeof(float);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align256(bytes); return p; };
    char *planes = take(3 * (size_t)n_scales * plane), *g0 = take(plane), *g1 = take(plane), *t0 = take(plane), *t1 = take(plane);
    char *smax = take((size_t)b * sizeof(unsigned));
    if (ws) {
        ws->planes = reinterpret_cast<float *>(planes);
        ws->g0 = reinterpret_cast<float *>(g0);
        ws->g1 = reinterpret_cast<float *>(g1);
        ws->t0 = reinterpret_cast<float *>(t0);
        ws->t1 = reinterpret_cast<float *>(t1);
        ws->smax = reinterpret_cast<unsigned *>(smax);
    }
    return off;
}

// the two tables of one scale (host, 2 radius + 1 doubles each: order 0, then order 1) as kernel arguments
struct ScaleTaps {
    Taps o0, o1;
    int re;
};
int make_taps(int radius, const double *weights, ScaleTaps *st, const char *who) {
    if (radius < 0 || radius > kMaxTableRadius || !weights) {
        octa::set_error("%s: need weight tables of radius 0 .. %d (got %d)", who, kMaxTableRadius, radius);
        return -2;
    }
    const double *w0 = weights + radius, *w1 = weights + (2 * (size_t)radius + 1) + radius;   // centres
    int re = 0;
    for (int j = 1; j <= radius; ++j)
        if (w0[j] != 0.0 || w1[j] != 0.0) re = j;
    if (re > kMaxRadius) {
        octa::set_error("%s: %d non-zero taps per side, at most %d are supported", who, re, kMaxRadius);
        return -2;
    }
    st->re = re;
    st->o0.sgn = 1.0;
    st->o1.sgn = -1.0;
    for (int j = 0; j <= kMaxRadius; ++j) {
        st->o0.t[j] = j <= re ? w0[j] : 0.0;
        st->o1.t[j] = j <= re ? w1[j] : 0.0;
    }
    return 0;
}

// Hrr, Hrc, Hcc of one scale (each b h w floats) from d_in * scale (negated when `negate`)
int hessian(const float *d_in, float *hrr, float *hrc, float *hcc, int b, int h, int w, const ScaleTaps &k, float scale, int negate, const Ws &ws, hipStream_t st) {
    const int re = k.re;
    if (pass<0>(d_in, ws.t0, ws.t1, b, h, w, re, k.o1, k.o0, scale, negate, st)) return -1;    // a: order 1 and order 0 down the rows
    if (pass<1>(ws.t0, ws.g0, nullptr, b, h, w, re, k.o0, k.o0, 1.0f, 0, st)) return -1;       // g0 = G(1,0) a
    if (pass<1>(ws.t1, ws.g1, nullptr, b, h, w, re, k.o1, k.o1, 1.0f, 0, st)) return -1;       // g1 = G(0,1) a
    if (pass<0>(ws.g0, ws.t0, ws.t1, b, h, w, re, k.o1, k.o0, 1.0f, 0, st)) return -1;
    if (pass<1>(ws.t0, hrr, nullptr, b, h, w, re, k.o0, k.o0, 1.0f, 0, st)) return -1;         // Hrr = G(1,0) g0
    if (pass<1>(ws.t1, hrc, nullptr, b, h, w, re, k.o1, k.o1, 1.0f, 0, st)) return -1;         // Hrc = G(0,1) g0
    if (pass<0>(ws.g1, ws.t0, nullptr, b, h, w, re, k.o0, k.o0, 1.0f, 0, st)) return -1;
    return pass<1>(ws.t0, hcc, nullptr, b, h, w, re, k.o1, k.o1, 1.0f, 0, st);                 // Hcc = G(0,1) g1
}

inline unsigned chunks(long long hw) { return (unsigned)std::min<long long>(1024, (hw + kThreads - 1) / kThreads); }

int max_s(const float *rr, const float *rc, const float *cc, float *l1, float *l2, unsigned *smax, int b, long long hw, hipStream_t st) {
    OCTA_HIP_CHECK(hipMemsetAsync(smax, 0, (size_t)b * sizeof(unsigned), st));
    hipLaunchKernelGGL(frangi_eigen_kernel, dim3(chunks(hw), b), dim3(kThreads), 0, st, rr, rc, cc, l1, l2, smax, hw);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" size_t octa_frangi_workspace_bytes(int b, int h, int w, int n_scales) {
    if (b < 1 || b > 65535 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim || n_scales < 1 || n_scales > kMaxScales) return 0;
    return ws_layout(b, h, w, n_scales, nullptr, nullptr);
}

extern "C" int octa_frangi_hessian(const float *d_in, float *d_hrr, float *d_hrc, float *d_hcc, int b, int h, int w, int radius, const double *weights,
                                   float in_scale, int black_ridges, void *d_ws, void *stream) {
    const char *who = "octa_frangi_hessian";
    if (bad_dims(b, h, w, who)) return -2;
    if (!d_in || !d_hrr || !d_hrc || !d_hcc || !d_ws) { octa::set_error("%s: null pointer", who); return -2; }
    ScaleTaps k;
    if (int rc = make_taps(radius, weights, &k, who)) return rc;
    Ws ws;
    ws_layout(b, h, w, 1, static_cast<char *>(d_ws), &ws);
    return hessian(d_in, d_hrr, d_hrc, d_hcc, b, h, w, k, in_scale, black_ridges ? 0 : 1, ws, static_cast<hipStream_t>(stream));
}

extern "C" int octa_frangi_eigenvalues(const float *d_in, float *d_l1, float *d_l2, float *d_gamma, int b, int h, int w, int radius, const double *weights,
                                       float in_scale, int black_ridges, void *d_ws, void *stream) {
    const char *who = "octa_frangi_eigenvalues";
    if (bad_dims(b, h, w, who)) return -2;
    if (!d_in || !d_l1 || !d_l2 || !d_gamma || !d_ws) { octa::set_error("%s: null pointer", who); return -2; }
    ScaleTaps k;
    if (int rc = make_taps(radius, weights, &k, who)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    Ws ws;
    ws_layout(b, h, w, 1, static_cast<char *>(d_ws), &ws);
    const long long hw = (long long)h * w, total = hw * b;
    float *p = ws.planes;
    if (hessian(d_in, p, p + total, p + 2 * total, b, h, w, k, in_scale, black_ridges ? 0 : 1, ws, st)) return -1;
    if (max_s(p, p + total, p + 2 * total, d_l1, d_l2, ws.smax, b, hw, st)) return -1;
    hipLaunchKernelGGL(frangi_gamma_kernel, dim3((b + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ws.smax, d_gamma, b);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_frangi_2d(const float *d_in, double *d_out, int b, int h, int w, int n_scales, const int *radii, const double *weights, float in_scale,
                              double beta, double gamma, int black_ridges, void *d_ws, void *stream) {
    const char *who = "octa_frangi_2d";
    if (bad_dims(b, h, w, who)) return -2;
    if (n_scales < 1 || n_scales > kMaxScales) { octa::set_error("%s: need 1 .. %d scales (got %d)", who, kMaxScales, n_scales); return -2; }
    if (!d_in || !d_out || !d_ws || !radii || !weights) { octa::set_error("%s: null pointer", who); return -2; }
    if (!(beta > 0.0) || !(gamma >= 0.0)) { octa::set_error("%s: need beta > 0 and gamma >= 0 (0: max(s) / 2 of the first scale per image)", who); return -2; }
    ScaleTaps k[kMaxScales];
    const double *wt = weights;
    for (int s = 0; s < n_scales; ++s) {
        if (int rc = make_taps(radii[s], wt, &k[s], who)) return rc;
        wt += 2 * (2 * (size_t)radii[s] + 1);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    Ws ws;
    ws_layout(b, h, w, n_scales, static_cast<char *>(d_ws), &ws);
    const long long hw = (long long)h * w, total = hw * b;
    for (int s = 0; s < n_scales; ++s) {
        float *p = ws.planes + 3 * s * total;
        if (hessian(d_in, p, p + total, p + 2 * total, b, h, w, k[s], in_scale, black_ridges ? 0 : 1, ws, st)) return -1;
    }
    const float den_b = (float)(2.0 * (beta * beta)), den_t = gamma > 0.0 ? (float)(2.0 * (gamma * gamma)) : 0.0f;
    if (!(den_t > 0.0f) && max_s(ws.planes, ws.planes + total, ws.planes + 2 * total, nullptr, nullptr, ws.smax, b, hw, st)) return -1;
    hipLaunchKernelGGL(frangi_vesselness_kernel, dim3(chunks(hw), b), dim3(kThreads), 0, st, ws.planes, n_scales, total, ws.smax, den_b, den_t, d_out, hw);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
