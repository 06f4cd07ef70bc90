// oof.hip -- the Optimally Oriented Flux (OOF) vessel filter, the classical baseline of `General.model.name: oof`
// (reference models/oof.py, configs/config_oof.yml), and the batched complex-double 2-D FFT it runs on.
//
// FFT. One workgroup per line, the whole line in LDS (two ping-pong buffers of N complex doubles: 2 x 64 KiB at N = 4096). The
// line is transformed by a self-sorting Stockham pass per radix of N = 4^a 2^b 3^c 5^d p1 p2 ...: radices 2, 3, 4 and 5 as register
// butterflies (N / R of them per stage), every other prime factor p by a generic stage that computes each of the N outputs as a
// p-term sum (O(N p) work: 1217 x 1217 complex multiply-adds per line of the prime size 1217, ~10x an all-radix-4 line of that
// length). A stage of radix R after Ns = R1 R2 ... (the radices before it) reads x[j + r N / R], r < R, and writes
//     y[(j / Ns) Ns R + j % Ns + q Ns] = sum_r x[j + r N / R] exp(-+2 pi i r (j % Ns + q Ns) / (Ns R)),   q < R,
// so no digit-reversal pass is needed. Twiddles are read from a table w[t] = exp(-2 pi i t / N) that oof_twiddles_kernel fills
// with sincospi(2 t / N) in double -- never by recurrence -- and the generic stage steps through it with exact integer indices.
// A line pass writes its result TRANSPOSED ([B][W][H] from [B][H][W]), so the second pass is again a pass over contiguous lines
// and leaves the natural layout. The inverse multiplies every line by 1 / N (numpy's ifft2 normalisation, 1 / (H W) in all).
//
// OOF (reference oof.py:53-131, settings fixed there: radii 1..5, spacing (1, 1), sigma 1, response_type 1, use_absolute,
// normalization_type 1). For the input f (float32 [B][H][W], multiplied by 255 in float32, then widened), F = FFT2(f) and per
// radius r the real radial filter H_r(rho) (rho = sqrt(x^2 + y^2) + 1e-12 on the fftfreq grid, per-radius constants on the host):
//     o11 = Re IFFT2(x^2 H_r F),  o12 = Re IFFT2(x y H_r F),  o22 = Re IFFT2(y^2 H_r F).
// Real results are paired in one complex inverse transform: A_r = (x^2 + i y^2) H_r F gives o11 + i o22, and
// C = x y (H_r + i H_r') F gives o12 of two radii. That is exact only for Hermitian spectra: x y H_r F is antisymmetric on the
// Nyquist row (H even) and column (W even), where the reference's np.real discards the part that is not Hermitian, so the kernel
// sets x y to 0 there -- except on the shared Nyquist corner, which is its own mirror image. Radii are
// processed in pairs (1, 2), (3, 4), (5): 3 + 3 + 2 inverse transforms instead of 15. Per pixel the eigenvalues of
// [[o11, o12], [o12, o22]] in closed form give the response maxe + mide (oof.py:88-115), which replaces the running output
// where its magnitude is strictly larger (oof.py:129-130). Finally out = (out + M) / max(out + M) per image, M = max(out);
// max(out + M) = M + M exactly (rounding is monotone), so one max reduction per image suffices.
//
// Everything is per line or per pixel (the two reductions are max operations): no atomics, bit-identical from run to run and
// between a batch and its images run one at a time.

#include "common.h"

#include <algorithm>

namespace {

constexpr int kThreads = 256;
constexpr int kMaxN = 4096;
constexpr int kMaxStages = 16;

struct FftPlan {
    int nst;
    int rad[kMaxStages];
};

FftPlan make_plan(int n) {
    FftPlan p{};
    auto push = [&](int r) { p.rad[p.nst++] = r; };
    while (n % 4 == 0) { push(4); n /= 4; }
    for (int f : {2, 3, 5})
        while (n % f == 0) { push(f); n /= f; }
    for (int f = 7; n > 1; f += 2)
        while (n % f == 0) { push(f); n /= f; }
    return p;   // at most 12 factors below 4097 (2^12)
}

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cscale(double2 a, double s) { return make_double2(a.x * s, a.y * s); }
// a * (-i sg): forward (sg = +1) multiplies by -i, inverse (sg = -1) by +i
__device__ __forceinline__ double2 cmul_mi(double2 a, double sg) { return make_double2(sg * a.y, -sg * a.x); }

// w[t] = exp(-2 pi i t / N), t < N
__global__ void __launch_bounds__(kThreads) oof_twiddles_kernel(double2 *__restrict__ tw, int n) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t >= n) return;
    double s, c;
    sincospi(2.0 * (double)t / (double)n, &s, &c);
    tw[t] = make_double2(c, -s);
}

// DFT of R values in registers, sign sg (+1 forward, -1 inverse)
template <int R> __device__ __forceinline__ void dft_small(double2 (&v)[R], double sg);
template <> __device__ __forceinline__ void dft_small<2>(double2 (&v)[2], double) {
    const double2 a = v[0], b = v[1];
    v[0] = cadd(a, b);
    v[1] = csub(a, b);
}
template <> __device__ __forceinline__ void dft_small<3>(double2 (&v)[3], double sg) {
    const double s3 = 0.86602540378443864676;   // sin(2 pi / 3)
    const double2 t = cadd(v[1], v[2]);
    const double2 u = csub(v[0], cscale(t, 0.5));
    const double2 w = cscale(cmul_mi(csub(v[1], v[2]), sg), s3);
    v[0] = cadd(v[0], t);
    v[1] = cadd(u, w);
    v[2] = csub(u, w);
}
template <> __device__ __forceinline__ void dft_small<4>(double2 (&v)[4], double sg) {
    const double2 t0 = cadd(v[0], v[2]), t1 = csub(v[0], v[2]), t2 = cadd(v[1], v[3]), t3 = cmul_mi(csub(v[1], v[3]), sg);
    v[0] = cadd(t0, t2);
    v[2] = csub(t0, t2);
    v[1] = cadd(t1, t3);
    v[3] = csub(t1, t3);
}
template <> __device__ __forceinline__ void dft_small<5>(double2 (&v)[5], double sg) {
    const double c1 = 0.30901699437494742410, c2 = -0.80901699437494742410;   // cos(2 pi / 5), cos(4 pi / 5)
    const double s1 = 0.95105651629515357212, s2 = 0.58778525229247312917;    // sin(2 pi / 5), sin(4 pi / 5)
    const double2 b1 = cadd(v[1], v[4]), b2 = cadd(v[2], v[3]), d1 = csub(v[1], v[4]), d2 = csub(v[2], v[3]);
    const double2 e1 = cadd(v[0], cadd(cscale(b1, c1), cscale(b2, c2)));
    const double2 e2 = cadd(v[0], cadd(cscale(b1, c2), cscale(b2, c1)));
    const double2 f1 = cmul_mi(cadd(cscale(d1, s1), cscale(d2, s2)), sg);
    const double2 f2 = cmul_mi(csub(cscale(d1, s2), cscale(d2, s1)), sg);
    v[0] = cadd(v[0], cadd(b1, b2));
    v[1] = cadd(e1, f1);
    v[4] = csub(e1, f1);
    v[2] = cadd(e2, f2);
    v[3] = csub(e2, f2);
}

__device__ __forceinline__ double2 twiddle(const double2 *__restrict__ tw, int t, bool inverse) {
    const double2 w = tw[t];
    return inverse ? make_double2(w.x, -w.y) : w;
}

template <int R>
__device__ __forceinline__ void stage_small(const double2 *src, double2 *dst, int n, int ns, const double2 *__restrict__ tw, bool inverse) {
    const int m = n / R, L = ns * R, tstep = n / L;
    const double sg = inverse ? -1.0 : 1.0;
    for (int j = threadIdx.x; j < m; j += kThreads) {
        const int k = j % ns;
        double2 v[R];
        v[0] = src[j];
#pragma unroll
        for (int r = 1; r < R; ++r) v[r] = cmul(src[j + r * m], twiddle(tw, r * k * tstep, inverse));   // r k < L: index < n
        dft_small<R>(v, sg);
        const int d = (j / ns) * L + k;
#pragma unroll
        for (int r = 0; r < R; ++r) dst[d + r * ns] = v[r];
    }
}

// any radix R (the prime factors above 5): one p-term sum per output
__device__ __forceinline__ void stage_generic(const double2 *src, double2 *dst, int n, int ns, int R, const double2 *__restrict__ tw, bool inverse) {
    const int m = n / R, L = ns * R, tstep = n / L;
    for (int o = threadIdx.x; o < n; o += kThreads) {
        const int rem = o % L, q = rem / ns, k = rem % ns, j = (o / L) * ns + k;
        const int step = (int)(((long long)(k + q * ns) * tstep) % n);
        double2 acc = src[j];
        int t = step;
        for (int r = 1; r < R; ++r) {
            acc = cadd(acc, cmul(src[j + r * m], twiddle(tw, t, inverse)));
            t += step;
            if (t >= n) t -= n;
        }
        dst[o] = acc;
    }
}

// One line of length n per workgroup; line l = b * nlines + row of the input ([B][nlines][n], complex double or -- F32X255 --
// float32 multiplied by 255 in float32), written transposed to out[b][i][row] ([B][n][nlines]) times `scale`.
template <bool F32X255>
__global__ void __launch_bounds__(kThreads) fft_line_kernel(const void *__restrict__ in, double2 *__restrict__ out, int n, int nlines, FftPlan plan,
                                                           const double2 *__restrict__ tw, int inverse, double scale) {
    extern __shared__ double2 lds[];
    double2 *a = lds, *b = lds + n;
    const long long line = blockIdx.x;
    if constexpr (F32X255) {
        const float *src = static_cast<const float *>(in) + line * n;
        for (int i = threadIdx.x; i < n; i += kThreads) a[i] = make_double2((double)(src[i] * 255.0f), 0.0);
    } else {
        const double2 *src = static_cast<const double2 *>(in) + line * n;
        for (int i = threadIdx.x; i < n; i += kThreads) a[i] = src[i];
    }
    __syncthreads();
    int ns = 1;
    for (int s = 0; s < plan.nst; ++s) {
        const int R = plan.rad[s];
        switch (R) {
            case 2: stage_small<2>(a, b, n, ns, tw, inverse); break;
            case 3: stage_small<3>(a, b, n, ns, tw, inverse); break;
            case 4: stage_small<4>(a, b, n, ns, tw, inverse); break;
            case 5: stage_small<5>(a, b, n, ns, tw, inverse); break;
            default: stage_generic(a, b, n, ns, R, tw, inverse); break;
        }
        __syncthreads();
        double2 *t = a; a = b; b = t;
        ns *= R;
    }
    const long long img = line / nlines, row = line % nlines;
    double2 *dst = out + img * n * (long long)nlines + row;
    for (int i = threadIdx.x; i < n; i += kThreads) dst[(long long)i * nlines] = cscale(a[i], scale);
}

// the per-radius constants of oof.py:65-83, evaluated on the host in the reference's operation order
struct RadiusConst {
    double norm;     // volume / bessel / r^2 * base
    double circle;   // 2 pi r
    double kb;       // pi^2 r
};

RadiusConst radius_const(int r) {
    const double pi = 3.141592653589793, eps = 1e-12, sigma = 1.0;
    RadiusConst c;
    c.circle = 2 * pi * r;
    // besselj(1.5, z) / eps^1.5 at z = circle * eps (~3e-11): the leading term of the series (z / 2)^1.5 / Gamma(2.5); the next
    // one is smaller by (z / 2)^2 / 2.5 ~ 1e-22. The closed form sqrt(2 / (pi z)) (sin z / z - cos z) cancels to nothing here.
    const double z = c.circle * eps;
    const double bessel = std::pow(z / 2, 1.5) / std::tgamma(2.5) / std::pow(eps, 1.5);
    const double base = r / std::sqrt(2 * r * sigma - sigma * sigma);
    const double volume = pi * (double)(r * r);
    c.norm = volume / bessel / (double)(r * r) * base;
    c.kb = (pi * pi) * r;
    return c;
}

__device__ __forceinline__ double freq(int k, int n) { return (double)(k < n - n / 2 ? k : k - n) / (double)n; }

// H_r(rho) (oof.py:75-83, same operation order)
__device__ __forceinline__ double radial_filter(double rho, const RadiusConst &c) {
    const double pi2 = 3.141592653589793 * 3.141592653589793;
    const double num = c.norm * exp((-2.0 * pi2) * (rho * rho));
    const double den = pow(rho, 1.5);
    const double cs = c.circle * rho;
    const double a = sin(cs) / cs - cos(cs);
    const double b = sqrt(1.0 / (c.kb * rho));
    return num / den * a * b;
}

// Spectra of one radius pair (ra, rb) or of the single radius ra (has_b = 0), planes of B*H*W:
//   has_b: P0 = (x^2 + i y^2) H_ra F,  P1 = (x^2 + i y^2) H_rb F,  P2 = x y (H_ra + i H_rb) F
//   else : P0 = (x^2 + i y^2) H_ra F,  P1 = x y H_ra F
__global__ void __launch_bounds__(kThreads) oof_spectrum_kernel(const double2 *__restrict__ F, double2 *__restrict__ P, int H, int W, long long total,
                                                               RadiusConst ca, RadiusConst cb, int has_b) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const long long hw = (long long)H * W;
    const int p = (int)(i % hw), kx = p / W, ky = p % W;
    const double x = freq(kx, H), y = freq(ky, W);
    const double rho = sqrt(x * x + y * y) + 1e-12;
    const bool nyq_row = (H % 2 == 0) && kx == H / 2, nyq_col = (W % 2 == 0) && ky == W / 2;
    const double xx = x * x, yy = y * y, xy = (nyq_row != nyq_col) ? 0.0 : x * y;   // Hermitian-symmetrised x y
    const double2 f = F[i];
    const double ha = radial_filter(rho, ca);
    const double2 ga = make_double2(ha * f.x, ha * f.y);
    P[i] = make_double2(xx * ga.x - yy * ga.y, xx * ga.y + yy * ga.x);
    if (has_b) {
        const double hb = radial_filter(rho, cb);
        const double2 gb = make_double2(hb * f.x, hb * f.y);
        P[total + i] = make_double2(xx * gb.x - yy * gb.y, xx * gb.y + yy * gb.x);
        P[2 * total + i] = make_double2(xy * ga.x - xy * gb.y, xy * ga.y + xy * gb.x);
    } else {
        P[total + i] = make_double2(xy * ga.x, xy * ga.y);
    }
}

// Response of one radius from A = o11 + i o22 and o12 = Re / Im C; replaces out where strictly stronger (first: out = 0 before)
__global__ void __launch_bounds__(kThreads) oof_eig_kernel(const double2 *__restrict__ A, const double2 *__restrict__ C, int c_imag, double *__restrict__ out,
                                                          long long total, int first) {
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const double2 a = A[i];
    const double o11 = a.x, o22 = a.y, o12 = c_imag ? C[i].y : C[i].x;
    const double h = (o11 + o22) * 0.5, q = (o11 - o22) * 0.5;
    const double d = sqrt(q * q + o12 * o12);
    const double l1 = h + d, l2 = h - d;
    const double maxe = fabs(l2) > fabs(l1) ? l2 : l1;
    const double mine = fabs(l2) < fabs(l1) ? l2 : l1;
    const double mide = (l1 + l2) - (maxe + mine);
    const double resp = maxe + mide;
    const double prev = first ? 0.0 : out[i];
    out[i] = fabs(resp) > fabs(prev) ? resp : prev;
}

constexpr int kMaxParts = kThreads;

__device__ __forceinline__ double block_max(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid (parts, B): part[b][p] = max of a strided share of image b
__global__ void __launch_bounds__(kThreads) oof_max_partial_kernel(const double *__restrict__ out, double *__restrict__ part, long long hw) {
    __shared__ double red[kThreads];
    const double *img = out + (long long)blockIdx.y * hw;
    double m = -INFINITY;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (long long)gridDim.x * kThreads) m = fmax(m, img[i]);
    m = block_max(m, red);
    if (threadIdx.x == 0) part[blockIdx.y * gridDim.x + blockIdx.x] = m;
}

// grid (chunks, B): M = max of the image's parts; out = (out + M) / (M + M)
__global__ void __launch_bounds__(kThreads) oof_normalize_kernel(double *__restrict__ out, const double *__restrict__ part, int parts, long long hw) {
    __shared__ double red[kThreads];
    const double M = block_max((int)threadIdx.x < parts ? part[blockIdx.y * parts + threadIdx.x] : -INFINITY, red);
    const double den = M + M;
    double *img = out + (long long)blockIdx.y * hw;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < hw; i += (long long)gridDim.x * kThreads) img[i] = (img[i] + M) / den;
}

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline unsigned blocks(long long total) { return (unsigned)((total + kThreads - 1) / kThreads); }

bool bad_dims(int b, int h, int w, const char *who) {
    if (b < 1 || h < 1 || w < 1 || h > kMaxN || w > kMaxN) {
        octa::set_error("%s: need b >= 1 and 1 <= h, w <= %d (got b=%d h=%d w=%d)", who, kMaxN, b, h, w);
        return true;
    }
    if ((long long)b * h * w > 0x7fffffffLL * kThreads / 4) {
        octa::set_error("%s: batch too large", who);
        return true;
    }
    return false;
}

size_t fft_ws_bytes(long long nimg, int h, int w) { return align256((size_t)nimg * h * w * sizeof(double2)) + align256((size_t)(h + w) * sizeof(double2)); }

// twiddle tables for h (tw_h) and w (tw_w: = tw_h when h == w)
int make_twiddles(double2 *tw_h, double2 *tw_w, int h, int w, hipStream_t st) {
    hipLaunchKernelGGL(oof_twiddles_kernel, dim3(blocks(h)), dim3(kThreads), 0, st, tw_h, h);
    if (w != h) hipLaunchKernelGGL(oof_twiddles_kernel, dim3(blocks(w)), dim3(kThreads), 0, st, tw_w, w);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

template <bool F32X255>
int line_pass(const void *in, double2 *out, int n, int nlines, long long nimg, const double2 *tw, bool inverse, hipStream_t st) {
    const size_t lds = 2 * (size_t)n * sizeof(double2);
    OCTA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&fft_line_kernel<F32X255>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const FftPlan plan = make_plan(n);
    hipLaunchKernelGGL(fft_line_kernel<F32X255>, dim3((unsigned)(nimg * nlines)), dim3(kThreads), lds, st, in, out, n, nlines, plan, tw, inverse ? 1 : 0,
                       inverse ? 1.0 / n : 1.0);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// 2-D transform of nimg images [h][w]: rows (length w) into tmp [nimg][w][h], columns (length h) back into out [nimg][h][w]
template <bool F32X255>
int fft2(const void *in, double2 *out, double2 *tmp, long long nimg, int h, int w, const double2 *tw_h, const double2 *tw_w, bool inverse, hipStream_t st) {
    if (line_pass<F32X255>(in, tmp, w, h, nimg, tw_w, inverse, st)) return -1;
    return line_pass<false>(tmp, out, h, w, nimg, tw_h, inverse, st);
}

// OOF workspace: F, three spectrum planes, the transposed scratch of the FFT (three planes), twiddles, partial maxima
struct OofWs {
    double2 *F, *P, *T, *tw_h, *tw_w;
    double *part;
};
size_t oof_ws_layout(int b, int h, int w, char *base, OofWs *ws) {
    const size_t plane = align256((size_t)b * h * w * sizeof(double2));
    size_t off = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + off : nullptr; off += align256(bytes); return p; };
    char *F = take(plane), *P = take(3 * plane), *T = take(3 * plane), *tw = take((size_t)(h + w) * sizeof(double2));
    char *part = take((size_t)b * kMaxParts * sizeof(double));
    if (ws) {
        ws->F = reinterpret_cast<double2 *>(F);
        ws->P = reinterpret_cast<double2 *>(P);
        ws->T = reinterpret_cast<double2 *>(T);
        ws->tw_h = reinterpret_cast<double2 *>(tw);
        ws->tw_w = h == w ? ws->tw_h : ws->tw_h + h;
        ws->part = reinterpret_cast<double *>(part);
    }
    return off;
}

int oof_run(const float *d_in, double *d_out, int b, int h, int w, void *d_ws, void *stream, bool normalize, const char *who) {
    if (bad_dims(b, h, w, who)) return -2;
    if (!d_in || !d_out || !d_ws) { octa::set_error("%s: null pointer", who); return -2; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    OofWs ws;
    oof_ws_layout(b, h, w, static_cast<char *>(d_ws), &ws);
    const long long total = (long long)b * h * w, hw = (long long)h * w;
    if (make_twiddles(ws.tw_h, ws.tw_w, h, w, st)) return -1;
    if (fft2<true>(d_in, ws.F, ws.T, b, h, w, ws.tw_h, ws.tw_w, false, st)) return -1;
    const int pairs[3][2] = {{1, 2}, {3, 4}, {5, 0}};
    for (int k = 0; k < 3; ++k) {
        const int ra = pairs[k][0], rb = pairs[k][1], nplanes = rb ? 3 : 2;
        const RadiusConst ca = radius_const(ra), cb = rb ? radius_const(rb) : ca;
        hipLaunchKernelGGL(oof_spectrum_kernel, dim3(blocks(total)), dim3(kThreads), 0, st, ws.F, ws.P, h, w, total, ca, cb, rb ? 1 : 0);
        OCTA_HIP_CHECK(hipGetLastError());
        if (fft2<false>(ws.P, ws.P, ws.T, (long long)nplanes * b, h, w, ws.tw_h, ws.tw_w, true, st)) return -1;
        const double2 *C = ws.P + (nplanes - 1) * total;
        hipLaunchKernelGGL(oof_eig_kernel, dim3(blocks(total)), dim3(kThreads), 0, st, ws.P, C, 0, d_out, total, k == 0 ? 1 : 0);
        if (rb) hipLaunchKernelGGL(oof_eig_kernel, dim3(blocks(total)), dim3(kThreads), 0, st, ws.P + total, C, 1, d_out, total, 0);
        OCTA_HIP_CHECK(hipGetLastError());
    }
    if (normalize) {
        const int parts = (int)std::min<long long>(kMaxParts, (hw + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(oof_max_partial_kernel, dim3(parts, b), dim3(kThreads), 0, st, d_out, ws.part, hw);
        const unsigned chunks = (unsigned)std::min<long long>(1024, (hw + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(oof_normalize_kernel, dim3(chunks, b), dim3(kThreads), 0, st, d_out, ws.part, parts, hw);
        OCTA_HIP_CHECK(hipGetLastError());
    }
    return 0;
}

}  // namespace

extern "C" size_t octa_fft2_c2c_f64_workspace_bytes(int b, int h, int w) {
    if (b < 1 || h < 1 || w < 1) return 0;
    return fft_ws_bytes(b, h, w);
}

extern "C" int octa_fft2_c2c_f64(const void *d_in, void *d_out, int b, int h, int w, int inverse, void *d_ws, void *stream) {
    if (bad_dims(b, h, w, "octa_fft2_c2c_f64")) return -2;
    if (!d_in || !d_out || !d_ws) { octa::set_error("octa_fft2_c2c_f64: null pointer"); return -2; }
    hipStream_t st = static_cast<hipStream_t>(stream);
    double2 *tmp = static_cast<double2 *>(d_ws);
    double2 *tw_h = reinterpret_cast<double2 *>(static_cast<char *>(d_ws) + align256((size_t)b * h * w * sizeof(double2)));
    double2 *tw_w = h == w ? tw_h : tw_h + h;
    if (make_twiddles(tw_h, tw_w, h, w, st)) return -1;
    return fft2<false>(d_in, static_cast<double2 *>(d_out), tmp, b, h, w, tw_h, tw_w, inverse != 0, st);
}

extern "C" size_t octa_oof_workspace_bytes(int b, int h, int w) {
    if (b < 1 || h < 1 || w < 1) return 0;
    return oof_ws_layout(b, h, w, nullptr, nullptr);
}

extern "C" int octa_oof_2d(const float *d_in, double *d_out, int b, int h, int w, void *d_ws, void *stream) {
    return oof_run(d_in, d_out, b, h, w, d_ws, stream, true, "octa_oof_2d");
}

extern "C" int octa_oof_2d_response(const float *d_in, double *d_out, int b, int h, int w, void *d_ws, void *stream) {
    return oof_run(d_in, d_out, b, h, w, d_ws, stream, false, "octa_oof_2d_response");
}
