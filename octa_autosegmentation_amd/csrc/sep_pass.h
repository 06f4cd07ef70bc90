// sep_pass.h -- one separable 1-D pass of scipy.ndimage's correlate1d (the symmetric / antisymmetric branch, mode 'reflect') on
// float32 images, to the bit; shared by frangi.hip (Gaussian-derivative Hessians) and morph.hip (Sobel, Gaussian).
//
// One pass over a line x, with the weights t[j] of offset +j (= the reversed table at -j):
//     out[l] = float32( x[l] t[0] + sum over j = R, R-1, ..., 1 of (x[l-j] +- x[l+j]) t[j] ),        + symmetric, - antisymmetric,
// in double, one add per term in that order, no fused multiply-add (the pragma below and -ffp-contract=off), indices reflected
// with period 2n, so a line shorter than the radius reflects several times. Taps beyond the last non-zero weight may be dropped
// (the caller passes the effective radius): a term that is +-0 changes nothing but the sign of a zero sum.
// sep_pass_kernel<AXIS> stages a tile with its halo along AXIS in LDS (float32, widened at use) and may write two outputs of the
// same input with two tables.
// float32 divide and square root go through double ((float)((double)a / b), (float)sqrt((double)x)): correctly rounded whatever
// the compiler's float32 settings (53 >= 2 * 24 + 2), subnormal results included.
#pragma once

#include "common.h"

#pragma clang fp contract(off)

namespace octa {
namespace sep {

constexpr int kThreads = 256;
constexpr int kMaxRadius = 96;      // effective (non-zero) taps per side; bounds the LDS tile of the axis-0 pass below 64 KiB

// tile of outputs per workgroup: axis 0 (down the rows) 32 rows x 64 columns, axis 1 (along the rows) 4 rows x 256 columns
template <int AXIS> struct Tile { static constexpr int X = AXIS == 0 ? 64 : 256, Y = AXIS == 0 ? 32 : 4; };

struct Taps {
    double sgn;                 // +1 symmetric (order 0), -1 antisymmetric (order 1)
    double t[kMaxRadius + 1];   // t[j]: scipy's weight at offset +j (= the reversed table at -j); zero beyond the table's own radius
};

__device__ __forceinline__ int reflect(int i, int n) {
    const int m = 2 * n;
    int p = i % m;
    if (p < 0) p += m;
    return p < n ? p : m - 1 - p;
}

__device__ __forceinline__ float div_rn(float a, float b) { return (float)((double)a / (double)b); }
__device__ __forceinline__ float sqrt_rn(float a) { return (float)sqrt((double)a); }

// out0 (and out1 when not null) [b][h][w] = one pass of `in` along AXIS with the tables ta (tb), re taps per side. The input is
// in * scale in float32, negated when `negate`.
template <int AXIS>
__global__ void __launch_bounds__(kThreads) sep_pass_kernel(const float *__restrict__ in, float *__restrict__ out0, float *__restrict__ out1, int h, int w,
                                                           int re, Taps ta, Taps tb, float scale, int negate) {
    extern __shared__ float tile[];
    constexpr int TX = Tile<AXIS>::X, TY = Tile<AXIS>::Y;
    const long long img = (long long)blockIdx.z * h * w;
    const int x0 = blockIdx.x * TX, y0 = blockIdx.y * TY;
    const int sw = AXIS == 0 ? TX : TX + 2 * re, sh = AXIS == 0 ? TY + 2 * re : TY;   // staged columns, rows
    for (int i = threadIdx.x; i < sw * sh; i += kThreads) {
        const int r = i / sw, c = i % sw;
        int gy = y0 + r, gx = x0 + c;
        if (AXIS == 0) gy = reflect(gy - re, h); else gx = reflect(gx - re, w);
        float v = 0.0f;
        if (gy < h && gx < w) {
            v = in[img + (long long)gy * w + gx] * scale;
            if (negate) v = -v;
        }
        tile[i] = v;
    }
    __syncthreads();
    const int c = threadIdx.x % TX, r0 = (threadIdx.x / TX) * (TY * TX / kThreads);
    const int gx = x0 + c;
    if (gx >= w) return;
    const int step = AXIS == 0 ? sw : 1;
    for (int k = 0; k < TY * TX / kThreads; ++k) {
        const int r = r0 + k, gy = y0 + r;
        if (gy >= h) break;
        const float *ctr = tile + (AXIS == 0 ? (r + re) * sw + c : r * sw + c + re);
        const double xc = (double)ctr[0];
        double a = xc * ta.t[0], b = xc * tb.t[0];
        for (int j = re; j >= 1; --j) {
            const double lo = (double)ctr[-j * step], hi = (double)ctr[j * step];
            a += (lo + ta.sgn * hi) * ta.t[j];
            b += (lo + tb.sgn * hi) * tb.t[j];
        }
        const long long o = img + (long long)gy * w + gx;
        out0[o] = (float)a;
        if (out1) out1[o] = (float)b;
    }
}

template <int AXIS>
inline int pass(const float *in, float *out0, float *out1, int b, int h, int w, int re, const Taps &ta, const Taps &tb, float scale, int negate, hipStream_t st) {
    constexpr int TX = Tile<AXIS>::X, TY = Tile<AXIS>::Y;
    const size_t lds = sizeof(float) * (AXIS == 0 ? (size_t)TX * (TY + 2 * re) : (size_t)TY * (TX + 2 * re));   // <= 56 KiB at re = 96
    hipLaunchKernelGGL(sep_pass_kernel<AXIS>, dim3((w + TX - 1) / TX, (h + TY - 1) / TY, b), dim3(kThreads), lds, st, in, out0, out1, h, w, re, ta, tb, scale, negate);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace sep
}  // namespace octa
