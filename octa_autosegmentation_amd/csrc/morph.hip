// morph.hip -- grey-level area opening / closing and the SkrGAN sketch filter, the classical baseline of `General.model.name: skrgan`
// (reference models/skrgan.py: Sobel magnitude, Gaussian, skimage.morphology.area_opening and area_closing, each stage min/max
// normalised), 2-D, float32, to the bit.
//
// Area opening, 4-connectivity: with C_p(h) the component of {f >= h} that contains p,
//     open(f)(p) = max{ h <= f(p) : |C_p(h)| >= lambda }.
// No arithmetic: every output value is one of the input's. The kernel evaluates it per SEED, a pixel with no strictly higher
// 4-neighbour. From a seed the region grows greedily, always by the highest-valued frontier pixel (Prim's order; ties any way),
// until it holds lambda pixels; lvl is the lowest value in it then, k the position in growth order of the first pixel whose
// value is <= lvl. The seed writes lvl to the pixels taken before k and to nothing else; every other pixel keeps its input value
// (the output starts as a copy of the input, the growth reads the input only). Seeds that write the same pixel write the same
// value, so plain stores suffice and every run gives the same bits. Two shortcuts are WRONG and not taken: stopping a growth at
// a pixel above the current level or the seed (two hills below lambda joined by a saddle: the lower hill's growth must climb the
// other hill), and writing lvl to every region pixel above lvl (a small hill's growth spills over its saddle onto a large hill,
// whose pixels are above lvl and must not change).
//
// One wave per 64 consecutive pixels; it grows its seeds one after another. The region (at most 128 pixels) lives in registers,
// pixel i of the growth order in lane i % 64, slot i / 64, together with the values of its four neighbours and a mask of those
// that are still frontier (inside the image, not in the region). The frontier maximum is a per-lane maximum over at most 8
// candidates and a wave reduction; a frontier pixel that borders several region pixels is a candidate of each, and all of them
// are struck when it is taken. Every loop is bounded by lambda; no LDS, no atomics, no waiting between waves.
//
// The filter's arithmetic stages: Sobel and Gaussian are sep_pass.h's passes (scipy's correlate1d to the bit); the magnitude is
// sqrt(sh sh + sv sv) with separately rounded float32 products and sum and a correctly rounded root; a normalisation is
// (x - min) / (max - min) in float32 with a correctly rounded divide, min and max per image from integer atomics on an
// order-preserving key (order-independent: a batch equals its images run alone); 1 - x is float32. An image whose max - min is
// not positive (a constant stage: numpy divides 0 by 0) is all-NaN from there on and its floods are skipped.

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

constexpr int kMaxDim = 4096;           // coordinates are packed as y << 16 | x
constexpr int kMaxLambda = 128;
constexpr int kMaxTableRadius = 1 << 20;
constexpr int kNoPixel = 0x7fffffff;    // an empty region slot: no packed coordinate or neighbour of one has this value
constexpr int kWavesPerBlock = kThreads / 64;

__device__ __forceinline__ int dir_offset(int k) { return k == 0 ? -65536 : k == 1 ? 65536 : k == 2 ? -1 : 1; }   // up, down, left, right

// Grow the region of the seed (packed position q, value qv) of image plane f and write its level to o. All 64 lanes call this
// together with the same arguments.
template <int SLOTS>
__device__ __forceinline__ void grow(const float *__restrict__ f, float *__restrict__ o, int h, int w, int lambda, int q, float qv, int lane) {
    int rp[SLOTS];          // packed position of this lane's region pixels
    float rv[SLOTS];        // their values
    float nv[SLOTS][4];     // the values of their four neighbours
    unsigned nm[SLOTS];     // bit k: neighbour k is a frontier pixel
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) { rp[s] = kNoPixel; rv[s] = 0.0f; nm[s] = 0u; nv[s][0] = nv[s][1] = nv[s][2] = nv[s][3] = 0.0f; }
    float lvl = qv;
    int n = 0;
    for (;;) {
        // q joins the region as pixel n: it stops being anyone's candidate, and its neighbours outside the region become the owner's
        const int qy = q >> 16, qx = q & 0xffff;
        unsigned fresh = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int r = q + dir_offset(k);
            const bool inside = k == 0 ? qy > 0 : k == 1 ? qy < h - 1 : k == 2 ? qx > 0 : qx < w - 1;
            bool mine = false;
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                mine = mine || rp[s] == r;
                if (rp[s] != kNoPixel && rp[s] + dir_offset(k) == q) nm[s] &= ~(1u << k);
            }
            if (inside && __ballot(mine) == 0ull) fresh |= 1u << k;
        }
        if (lane == (n & 63)) {
#pragma unroll
            for (int s = 0; s < SLOTS; ++s) {
                if ((n >> 6) == s) {
                    rp[s] = q;
                    rv[s] = qv;
                    nm[s] = fresh;
                    const long long c = (long long)qy * w + qx;
                    nv[s][0] = (fresh & 1u) ? f[c - w] : 0.0f;
                    nv[s][1] = (fresh & 2u) ? f[c + w] : 0.0f;
                    nv[s][2] = (fresh & 4u) ? f[c - 1] : 0.0f;
                    nv[s][3] = (fresh & 8u) ? f[c + 1] : 0.0f;
                }
            }
        }
        lvl = qv < lvl ? qv : lvl;      // selects, not fminf / fmaxf: the bits of the input pass through
        if (++n == lambda) break;
        // the highest frontier pixel: this lane's best candidate, then the wave's
        bool has = false;
        float best = 0.0f;
        int bpos = 0;
#pragma unroll
        for (int s = 0; s < SLOTS; ++s) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (((nm[s] >> k) & 1u) && (!has || nv[s][k] > best)) {
                    has = true;
                    best = nv[s][k];
                    bpos = rp[s] + dir_offset(k);
                }
            }
        }
        float m = has ? best : -INFINITY;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float other = __shfl_xor(m, d);
            m = other > m ? other : m;
        }
        const unsigned long long who = __ballot(has && best == m);
        if (who == 0ull) return;        // the frontier is empty: the image has fewer than lambda pixels (refused on the host)
        const int src = __builtin_ctzll(who);
        q = __shfl(bpos, src);
        qv = __shfl(best, src);
    }
    // k: the first pixel of the growth order at the final level; the pixels before it are this seed's
    unsigned long long at = __ballot(rp[0] != kNoPixel && rv[0] <= lvl);
    int k = at ? __builtin_ctzll(at) : 64;
    if (SLOTS > 1 && at == 0ull) {
        at = __ballot(rp[SLOTS - 1] != kNoPixel && rv[SLOTS - 1] <= lvl);
        k = at ? 64 + __builtin_ctzll(at) : 128;
    }
#pragma unroll
    for (int s = 0; s < SLOTS; ++s)
        if (lane + 64 * s < k && rp[s] != kNoPixel) o[(long long)(rp[s] >> 16) * w + (rp[s] & 0xffff)] = lvl;
}

// grid (chunks of 4 x 64 pixels, b). out holds a copy of in; in is only read, out only written. skip (may be null): images to leave alone.
template <int SLOTS>
__global__ void __launch_bounds__(kThreads) area_open_kernel(const float *__restrict__ in, float *__restrict__ out, int h, int w, int lambda,
                                                            const unsigned *__restrict__ skip) {
    if (skip && skip[blockIdx.y]) return;
    const int lane = threadIdx.x & 63;
    const long long hw = (long long)h * w;
    const long long first = ((long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)) * 64;
    if (first >= hw) return;            // the whole wave
    const float *f = in + (long long)blockIdx.y * hw;
    float *o = out + (long long)blockIdx.y * hw;
    const long long i = first + lane;
    bool seed = false;
    int pos = 0;
    float v = 0.0f;
    if (i < hw) {
        const int y = (int)(i / w), x = (int)(i % w);
        v = f[i];
        seed = !((y > 0 && f[i - w] > v) || (y < h - 1 && f[i + w] > v) || (x > 0 && f[i - 1] > v) || (x < w - 1 && f[i + 1] > v));
        pos = (y << 16) | x;
    }
    unsigned long long seeds = __ballot(seed);
    while (seeds) {
        const int s = __builtin_ctzll(seeds);
        seeds &= seeds - 1;
        grow<SLOTS>(f, o, h, w, lambda, __shfl(pos, s), __shfl(v, s), lane);
    }
}

// order-preserving key of a float: a < b <=> key(a) < key(b) for all non-NaN a, b (-0 below +0)
__device__ __forceinline__ unsigned order_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float key_value(unsigned k) { return __uint_as_float((k & 0x80000000u) ? k & 0x7fffffffu : ~k); }

// per stage s and image i: mm[(s b + i) 2] the key of the minimum, [.. + 1] of the maximum; flag[s b + i] != 0: the image is all-NaN
// from stage s on
__global__ void skr_init_kernel(unsigned *__restrict__ mm, unsigned *__restrict__ flag, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mm[2 * i] = 0xffffffffu;
    mm[2 * i + 1] = 0u;
    flag[i] = 0u;
}

// grid (chunks, b): minimum and maximum of each image
__global__ void __launch_bounds__(kThreads) skr_minmax_kernel(const float *__restrict__ x, unsigned *__restrict__ mm, long long hw) {
    __shared__ unsigned lo[kThreads], hi[kThreads];
    const long long base = (long long)blockIdx.y * hw;
    unsigned a = 0xffffffffu, b = 0u;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (long long)gridDim.x * kThreads) {
        const unsigned k = order_key(x[base + i]);
        a = min(a, k);
        b = max(b, k);
    }
    lo[threadIdx.x] = a;
    hi[threadIdx.x] = b;
    __syncthreads();
    for (int k = kThreads / 2; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) {
            lo[threadIdx.x] = min(lo[threadIdx.x], lo[threadIdx.x + k]);
            hi[threadIdx.x] = max(hi[threadIdx.x], hi[threadIdx.x + k]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicMin(mm + 2 * blockIdx.y, lo[0]);
        atomicMax(mm + 2 * blockIdx.y + 1, hi[0]);
    }
}

// grid (chunks, b): out = (x - min) / (max - min), numpy's `x -= x.min(); x /= x.max()`: the subtraction is monotone, so the second
// maximum is the rounded max - min. prev (may be null): the image's flag of the stage before; flag: this stage's.
__global__ void __launch_bounds__(kThreads) skr_normalise_kernel(const float *__restrict__ x, float *__restrict__ out, const unsigned *__restrict__ mm,
                                                                const unsigned *__restrict__ prev, unsigned *__restrict__ flag, long long hw) {
    const float mn = key_value(mm[2 * blockIdx.y]), d = key_value(mm[2 * blockIdx.y + 1]) - mn;
    const bool bad = (prev && prev[blockIdx.y]) || !(d > 0.0f);
    if (blockIdx.x == 0 && threadIdx.x == 0) flag[blockIdx.y] = bad ? 1u : 0u;
    const long long base = (long long)blockIdx.y * hw;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (long long)gridDim.x * kThreads)
        out[base + i] = bad ? __uint_as_float(0x7fc00000u) : div_rn(x[base + i] - mn, d);
}

__global__ void __launch_bounds__(kThreads) skr_magnitude_kernel(const float *__restrict__ sh, const float *__restrict__ sv, float *__restrict__ out, long long n) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const float a = sh[i] * sh[i], b = sv[i] * sv[i];
        out[i] = sqrt_rn(a + b);
    }
}

// out0 (and out1 when not null) = 1 - x, float32; out0 may be x itself
__global__ void __launch_bounds__(kThreads) skr_invert_kernel(const float *x, float *out0, float *out1, long long n) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const float v = 1.0f - x[i];
        out0[i] = v;
        if (out1) out1[i] = v;
    }
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned chunks(long long n) { return (unsigned)std::min<long long>(4096, (n + kThreads - 1) / kThreads); }

bool bad_dims(int b, int h, int w, const char *who) {
    if (b < 1 || b > 65535 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim) {
        octa::set_error("%s: need 1 <= b <= 65535 and 1 <= h, w <= %d (got b=%d h=%d w=%d)", who, kMaxDim, b, h, w);
        return true;
    }
    return false;
}

bool bad_lambda(int lambda, int h, int w, const char *who) {
    if (lambda < 1 || lambda > kMaxLambda || (long long)h * w < lambda) {
        octa::set_error("%s: need 1 <= area threshold <= %d and an image of at least that many pixels (got %d for %d x %d)", who, kMaxLambda, lambda, h, w);
        return true;
    }
    return false;
}

// out = opening of in (out != in), both [b][h][w]
int open_planes(const float *in, float *out, int b, int h, int w, int lambda, const unsigned *skip, hipStream_t st) {
    const long long hw = (long long)h * w;
    OCTA_HIP_CHECK(hipMemcpyAsync(out, in, (size_t)b * hw * sizeof(float), hipMemcpyDeviceToDevice, st));
    if (lambda == 1) return 0;          // every component has a pixel
    const dim3 grid((unsigned)((hw + 64 * kWavesPerBlock - 1) / (64 * kWavesPerBlock)), b);
    if (lambda <= 64) hipLaunchKernelGGL(area_open_kernel<1>, grid, dim3(kThreads), 0, st, in, out, h, w, lambda, skip);
    else hipLaunchKernelGGL(area_open_kernel<2>, grid, dim3(kThreads), 0, st, in, out, h, w, lambda, skip);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

int invert(const float *x, float *out0, float *out1, long long n, hipStream_t st) {
    hipLaunchKernelGGL(skr_invert_kernel, dim3(chunks(n)), dim3(kThreads), 0, st, x, out0, out1, n);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// workspace: six planes, then per stage and image two keys and a flag
struct Ws {
    float *p[6];
    unsigned *mm, *flag;
};
size_t ws_layout(int b, int h, int w, char *base, Ws *ws) {
    const size_t plane = (size_t)b * h * w * sizeof(float);
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align256(bytes); return p; };
    char *p[6];
    for (int i = 0; i < 6; ++i) p[i] = take(plane);
    char *mm = take(3 * (size_t)b * 2 * sizeof(unsigned)), *flag = take(3 * (size_t)b * sizeof(unsigned));
    if (ws) {
        for (int i = 0; i < 6; ++i) ws->p[i] = reinterpret_cast<float *>(p[i]);
        ws->mm = reinterpret_cast<unsigned *>(mm);
        ws->flag = reinterpret_cast<unsigned *>(flag);
    }
    return off;
}

// stage s: out = x normalised per image
int normalise(const float *x, float *out, int s, int b, long long hw, const Ws &ws, hipStream_t st) {
    unsigned *mm = ws.mm + 2 * (size_t)s * b, *flag = ws.flag + (size_t)s * b;
    hipLaunchKernelGGL(skr_minmax_kernel, dim3(chunks(hw), b), dim3(kThreads), 0, st, x, mm, hw);
    OCTA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(skr_normalise_kernel, dim3(chunks(hw), b), dim3(kThreads), 0, st, x, out, mm, s ? flag - b : nullptr, flag, hw);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

void fixed_taps(Taps *t, double sgn, double t0, double t1) {
    t->sgn = sgn;
    for (int j = 0; j <= kMaxRadius; ++j) t->t[j] = 0.0;
    t->t[0] = t0;
    t->t[1] = t1;
}

}  // namespace

extern "C" size_t octa_skr_workspace_bytes(int b, int h, int w) {
    if (b < 1 || b > 65535 || h < 1 || w < 1 || h > kMaxDim || w > kMaxDim) return 0;
    return ws_layout(b, h, w, nullptr, nullptr);
}

extern "C" int octa_area_opening(const float *d_in, float *d_out, int b, int h, int w, int area_threshold, int closing, void *d_ws, void *stream) {
    const char *who = "octa_area_opening";
    if (bad_dims(b, h, w, who) || bad_lambda(area_threshold, h, w, who)) return -2;
    if (!d_in || !d_out || (closing && !d_ws)) { octa::set_error("%s: null pointer", who); return -2; }
    if (d_in == d_out) { octa::set_error("%s: the output must not be the input", who); return -2; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!closing) return open_planes(d_in, d_out, b, h, w, area_threshold, nullptr, st);
    Ws ws;
    ws_layout(b, h, w, static_cast<char *>(d_ws), &ws);
    const long long n = (long long)b * h * w;
    if (invert(d_in, ws.p[0], nullptr, n, st)) return -1;
    if (open_planes(ws.p[0], d_out, b, h, w, area_threshold, nullptr, st)) return -1;
    return invert(d_out, d_out, nullptr, n, st);
}

extern "C" int octa_skr_filter(const float *d_in, float *d_magnitude, float *d_filtered, float *d_opened, float *d_out, int b, int h, int w, int radius,
                               const double *weights, int area_open, int area_close, void *d_ws, void *stream) {
    const char *who = "octa_skr_filter";
    if (bad_dims(b, h, w, who) || bad_lambda(area_open, h, w, who) || bad_lambda(area_close, h, w, who)) return -2;
    if (!d_in || !d_out || !d_ws) { octa::set_error("%s: null pointer", who); return -2; }
    if (radius > kMaxTableRadius || (radius >= 0 && !weights)) {
        octa::set_error("%s: need a weight table of radius 0 .. %d, or radius < 0 for no Gaussian (got %d)", who, kMaxTableRadius, radius);
        return -2;
    }
    Taps gauss;
    int re = 0;
    if (radius >= 0) {
        const double *c = weights + radius;     // the centre; the table is symmetric
        for (int j = 1; j <= radius; ++j)
            if (c[j] != 0.0) re = j;
        if (re > kMaxRadius) { octa::set_error("%s: %d non-zero taps per side, at most %d are supported", who, re, kMaxRadius); return -2; }
        gauss.sgn = 1.0;
        for (int j = 0; j <= kMaxRadius; ++j) gauss.t[j] = j <= re ? c[j] : 0.0;
    }
    Taps diff, smooth;
    fixed_taps(&diff, -1.0, 0.0, -1.0);         // correlate [-1, 0, 1]: (x[l-1] - x[l+1]) * -1
    fixed_taps(&smooth, 1.0, 2.0, 1.0);         // correlate [1, 2, 1]
    hipStream_t st = static_cast<hipStream_t>(stream);
    Ws ws;
    ws_layout(b, h, w, static_cast<char *>(d_ws), &ws);
    const long long hw = (long long)h * w, n = hw * b;
    float *t0 = ws.p[0], *t1 = ws.p[1], *sh = ws.p[2], *sv = ws.p[3];
    float *mag = d_magnitude ? d_magnitude : ws.p[4], *filt = d_filtered ? d_filtered : ws.p[5];
    hipLaunchKernelGGL(skr_init_kernel, dim3((3 * b + kThreads - 1) / kThreads), dim3(kThreads), 0, st, ws.mm, ws.flag, 3 * b);
    OCTA_HIP_CHECK(hipGetLastError());
    // sobel(x, 0): the difference down the rows, then the smoothing along them; sobel(x, 1): the difference along the rows first
    if (pass<0>(d_in, t0, nullptr, b, h, w, 1, diff, diff, 1.0f, 0, st)) return -1;
    if (pass<1>(t0, sh, nullptr, b, h, w, 1, smooth, smooth, 1.0f, 0, st)) return -1;
    if (pass<1>(d_in, t1, nullptr, b, h, w, 1, diff, diff, 1.0f, 0, st)) return -1;
    if (pass<0>(t1, sv, nullptr, b, h, w, 1, smooth, smooth, 1.0f, 0, st)) return -1;
    hipLaunchKernelGGL(skr_magnitude_kernel, dim3(chunks(n)), dim3(kThreads), 0, st, sh, sv, t0, n);
    OCTA_HIP_CHECK(hipGetLastError());
    if (normalise(t0, mag, 0, b, hw, ws, st)) return -1;
    if (radius >= 0) {
        if (pass<0>(mag, t1, nullptr, b, h, w, re, gauss, gauss, 1.0f, 0, st)) return -1;
        if (pass<1>(t1, filt, nullptr, b, h, w, re, gauss, gauss, 1.0f, 0, st)) return -1;
    } else {
        OCTA_HIP_CHECK(hipMemcpyAsync(filt, mag, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    // opening, normalised (sh is free now)
    float *opened = d_opened ? d_opened : sh;
    if (open_planes(filt, t0, b, h, w, area_open, ws.flag, st)) return -1;
    if (normalise(t0, opened, 1, b, hw, ws, st)) return -1;
    // closing = 1 - open(1 - x), normalised
    if (invert(opened, t1, nullptr, n, st)) return -1;
    if (open_planes(t1, t0, b, h, w, area_close, ws.flag + b, st)) return -1;
    if (invert(t0, t0, nullptr, n, st)) return -1;
    return normalise(t0, d_out, 2, b, hw, ws, st);
}
