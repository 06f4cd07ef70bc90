// menten.hip -- the augmentation of Menten et al. (MICCAI 2022) on samples resident in HBM: the reference's comparison baseline
// `MentenAugmentationd` (data/data_transforms.py:44-325) = BinomialVesselNoised -> AddVitreousFloater -> AddMotionArtifact.
//
// Every random number is drawn on the host from numpy's global stream, in the reference's order (data/data_transforms.py of this
// package), and passed in; the kernels are the arithmetic, all of it in float64 like the reference's numpy / scipy code:
//   vessel noise : blur_rows_kernel<VesselSrc>  -- 3x3 cross dilation of the Bernoulli field (zero border), the five 0.7 rings and the
//                                                  row pass of scipy's gaussian_filter on an LDS tile with its reflect halo;
//                  blur_cols_kernel<.., VesselCombine> -- the column pass, + image + quantum noise, / (1 + scaling / 1.5), clip;
//   floater      : floater_lines_kernel    -- skimage.draw.line (Bresenham, both end points) per segment, clipped to the image;
//                  floater_coldist_kernel  -- distance to the nearest line pixel along axis 0 (two running scans per column);
//                  floater_rowdist_kernel  -- min-plus along axis 1 as a prefix and a suffix minimum in LDS: L1 distance <= n, which is
//                                             what n iterations of the cross-shaped binary dilation give (no n launches of a stencil);
//                  blur_cols_kernel<MaskSrc> + blur_rows_kernel<.., FloaterMul> -- gaussian_filter(sigma 10) and img * (1 - floater);
//   motion       : motion_gather_kernel    -- the cuts folded into a per-row (source row | whiteout row, column shift) table: a pure
//                                             gather, exact in every dtype.
// scipy's `reflect` boundary (d c b a | a b c d) is index folding with period 2 N, exact for images smaller than the filter radius too.
// The sums run in tap order, scipy pairs the symmetric taps: results agree to a few ulp of float64 (tests: 1e-12 absolute).

#include "common.h"

namespace {

__device__ __forceinline__ int fold_reflect(int i, int n) {
    const int p = 2 * n;
    int m = i % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}

constexpr int TX = 64, TY = 4;       // output tile of blur_rows_kernel: one wave per row, 256 threads

// ---- sources ---------------------------------------------------------------------------------------------------------------

// binary_dilation(bernoulli, cross, zero border) as 1.0 / 0.0, times 0.7 once for every ring m with sqrt((y - H/2)^2 + (x - W/2)^2) < r - 3 m.
// Integral r: the compare is done on 4 d^2 = (2y - H)^2 + (2x - W)^2 against 4 (r - 3m)^2 in integers, which is the float64 compare of the
// reference for every pixel, those exactly on a ring included; otherwise on the correctly rounded double square root, as numpy computes it.
struct VesselSrc {
    const unsigned char *bern;
    int H, W, integral;
    long long thr4[5];
    double thr[5];
    __device__ double operator()(int b, int y, int x) const {
        const unsigned char *p = bern + ((size_t)b * H + y) * W + x;
        int d = p[0];
        if (y > 0) d |= p[-W];
        if (y < H - 1) d |= p[W];
        if (x > 0) d |= p[-1];
        if (x < W - 1) d |= p[1];
        double v = d ? 1.0 : 0.0;
        if (integral) {
            const long long a = 2LL * y - H, c = 2LL * x - W, q = a * a + c * c;
            for (int m = 0; m < 5; m++)
                if (q < thr4[m]) v = v * 0.7;
        } else {
            const double a = (double)y - (double)H / 2.0, c = (double)x - (double)W / 2.0;
            const double s = __dsqrt_rn(a * a + c * c);
            for (int m = 0; m < 5; m++)
                if (s < thr[m]) v = v * 0.7;
        }
        return v;
    }
};

struct F64Src {
    const double *p;
    int H, W;
    __device__ double operator()(int b, int y, int x) const { return p[((size_t)b * H + y) * W + x]; }
};

struct MaskSrc {
    const unsigned char *p;
    int H, W;
    __device__ double operator()(int b, int y, int x) const { return p[((size_t)b * H + y) * W + x] ? 1.0 : 0.0; }
};

// ---- epilogues -------------------------------------------------------------------------------------------------------------

struct StoreF64 {
    double *out;
    int H, W;
    __device__ void operator()(int b, int y, int x, double v) const { out[((size_t)b * H + y) * W + x] = v; }
};

// clip((img + blurred * scaling + quantum) / denom, 0, 1), the image float32 or float64
struct VesselCombine {
    const void *img;
    const double *quantum;
    double *out;
    int H, W, img_f64;
    double scaling, denom;
    __device__ void operator()(int b, int y, int x, double v) const {
        const size_t i = ((size_t)b * H + y) * W + x;
        const double a = img_f64 ? static_cast<const double *>(img)[i] : (double)static_cast<const float *>(img)[i];
        double r = (a + v * scaling + quantum[i]) / denom;
        r = r < 0.0 ? 0.0 : r;               // np.clip = minimum(maximum(x, 0), 1)
        r = r > 1.0 ? 1.0 : r;
        out[i] = r;
    }
};

struct FloaterMul {
    const double *img;
    double *out;
    int H, W;
    __device__ void operator()(int b, int y, int x, double v) const {
        const size_t i = ((size_t)b * H + y) * W + x;
        out[i] = img[i] * (1.0 - v);
    }
};

// ---- the two passes of gaussian_filter -------------------------------------------------------------------------------------

// axis 1: a TY x (TX + 2 radius) tile of the source, halo folded, in LDS; thread (tx, ty) sums its 2 radius + 1 taps from it
template <class Src, class Epi>
__global__ void __launch_bounds__(TX *TY)
blur_rows_kernel(Src src, Epi epi, const double *__restrict__ w, int radius, int H, int W) {
    extern __shared__ __align__(16) double tile[];
    const int b = blockIdx.z, y0 = blockIdx.y * TY, x0 = blockIdx.x * TX;
    const int tw = TX + 2 * radius;
    for (int i = threadIdx.x; i < tw * TY; i += TX * TY) {
        const int ry = i / tw, cx = i - ry * tw, y = y0 + ry;
        tile[i] = y < H ? src(b, y, fold_reflect(x0 - radius + cx, W)) : 0.0;
    }
    __syncthreads();
    const int tx = threadIdx.x % TX, ty = threadIdx.x / TX, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const double *row = tile + ty * tw + tx;
    double acc = 0.0;
    for (int k = 0; k <= 2 * radius; k++) acc += w[k] * row[k];
    epi(b, y, x, acc);
}

// axis 0: neighbouring threads read neighbouring columns of the folded rows (coalesced; the rows stay in L2)
template <class Src, class Epi>
__global__ void __launch_bounds__(256)
blur_cols_kernel(Src src, Epi epi, const double *__restrict__ w, int radius, int H, int W) {
    const int b = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= W) return;
    double acc = 0.0;
    for (int k = 0; k <= 2 * radius; k++) acc += w[k] * src(b, fold_reflect(y - radius + k, H), x);
    epi(b, y, x, acc);
}

// ---- floater mask ----------------------------------------------------------------------------------------------------------

constexpr int DIST_INF = 1 << 28;

// skimage.draw.line(r0, c0, r1, c1) for segment s of sample b, points outside [0, N)^2 dropped; mask is pre-zeroed, every writer stores 1
__global__ void __launch_bounds__(64)
floater_lines_kernel(const int *__restrict__ pts, const int *__restrict__ npts, int P, int N, unsigned char *__restrict__ mask) {
    const int b = blockIdx.y, s = blockIdx.x * 64 + threadIdx.x;
    int np = npts[b];
    np = np > P ? P : np;
    if (s + 1 >= np) return;
    const int *q = pts + ((size_t)b * P + s) * 2;
    const int r0 = q[0], c0 = q[1], r1 = q[2], c1 = q[3];
    unsigned char *m = mask + (size_t)b * N * N;
    int r = r0, c = c0, dr = abs(r1 - r0), dc = abs(c1 - c0);
    int sc = (c1 - c) > 0 ? 1 : -1, sr = (r1 - r) > 0 ? 1 : -1;
    const int steep = dr > dc;
    if (steep) { int t = c; c = r; r = t; t = dc; dc = dr; dr = t; t = sc; sc = sr; sr = t; }
    if (dc > (1 << 24)) return;                                  // not a walk inside or near an image
    int d = 2 * dr - dc;
    for (int i = 0; i < dc; i++) {
        const int rr = steep ? c : r, cc = steep ? r : c;
        if (rr >= 0 && rr < N && cc >= 0 && cc < N) m[(size_t)rr * N + cc] = 1;
        while (d >= 0) { r += sr; d -= 2 * dc; }
        c += sc;
        d += 2 * dr;
    }
    if (r1 >= 0 && r1 < N && c1 >= 0 && c1 < N) m[(size_t)r1 * N + c1] = 1;
}

// g[y][x] = min over y' with mask[y'][x] of |y - y'| (DIST_INF for an empty column): a running count down, then up
__global__ void __launch_bounds__(256)
floater_coldist_kernel(const unsigned char *__restrict__ mask, int N, int *__restrict__ g) {
    const int b = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x >= N) return;
    const unsigned char *m = mask + (size_t)b * N * N + x;
    int *o = g + (size_t)b * N * N + x;
    int run = DIST_INF;
    for (int y = 0; y < N; y++) {
        run = m[(size_t)y * N] ? 0 : (run < DIST_INF ? run + 1 : DIST_INF);
        o[(size_t)y * N] = run;
    }
    run = DIST_INF;
    for (int y = N - 1; y >= 0; y--) {
        run = m[(size_t)y * N] ? 0 : (run < DIST_INF ? run + 1 : DIST_INF);
        const int f = o[(size_t)y * N];
        o[(size_t)y * N] = run < f ? run : f;
    }
}

// One row per block. d[x] = min_j (g[j] + |x - j|) = min(x + prefix-min(g[j] - j), suffix-min(g[j] + j) - x): two scans (Hillis-Steele in
// LDS, three buffers of N ints), then mask = d <= dilations[b].
__global__ void __launch_bounds__(256)
floater_rowdist_kernel(const int *__restrict__ g, const int *__restrict__ dilations, int N, unsigned char *__restrict__ mask) {
    extern __shared__ __align__(16) int sbuf[];
    const int b = blockIdx.y, y = blockIdx.x;
    const int *row = g + ((size_t)b * N + y) * N;
    int *fwd = sbuf + 2 * N;
    int cur = 0;
    for (int dir = 0; dir < 2; dir++) {
        cur = 0;
        for (int j = threadIdx.x; j < N; j += 256) sbuf[j] = dir == 0 ? row[j] - j : row[j] + j;
        __syncthreads();
        for (int off = 1; off < N; off <<= 1) {
            const int *a = sbuf + cur * N;
            int *o = sbuf + (cur ^ 1) * N;
            for (int j = threadIdx.x; j < N; j += 256) {
                const int k = dir == 0 ? j - off : j + off;
                const int v = a[j];
                o[j] = (k >= 0 && k < N && a[k] < v) ? a[k] : v;
            }
            __syncthreads();
            cur ^= 1;
        }
        if (dir == 0) {
            for (int j = threadIdx.x; j < N; j += 256) fwd[j] = sbuf[cur * N + j] + j;
            __syncthreads();
        }
    }
    const int n = dilations[b];
    unsigned char *out = mask + ((size_t)b * N + y) * N;
    for (int j = threadIdx.x; j < N; j += 256) {
        const int bw = sbuf[cur * N + j] - j, f = fwd[j];
        out[j] = (bw < f ? bw : f) <= n ? 1 : 0;
    }
}

// ---- motion ----------------------------------------------------------------------------------------------------------------

// out[b][R][j] = j < shift ? 0 : source[j - shift], source = row `src` of the input (src >= 0) or whiteout row -src - 1; U is the unit of
// the copy (4, 8 or 16 bytes), widths and shifts counted in units. A table entry that points outside its array gives zeros.
template <class U>
__global__ void __launch_bounds__(256)
motion_gather_kernel(const U *__restrict__ in, U *__restrict__ out, const int *__restrict__ table, const U *__restrict__ white, int n_white,
                     int Hh, int Wu, int unit) {
    const int b = blockIdx.z, R = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Wu) return;
    const int *t = table + ((size_t)b * Hh + R) * 2;
    const int src = t[0], sh = t[1] / unit;
    U v = {};
    if (sh >= 0 && j >= sh) {
        if (src >= 0 && src < Hh) v = in[((size_t)b * Hh + src) * Wu + (j - sh)];
        else if (src < 0 && -src - 1 < n_white && white) v = white[(size_t)(-src - 1) * Wu + (j - sh)];
    }
    out[((size_t)b * Hh + R) * Wu + j] = v;
}

bool bad_dims(int B, int H, int W) { return B <= 0 || H <= 0 || W <= 0 || B > 65535 || H > 65535 || W > (1 << 20); }

int floater_mask_launch(const int *d_pts, const int *d_npts, const int *d_dilations, int B, int P, int N, unsigned char *d_mask, int *d_dist,
                        hipStream_t stream) {
    OCTA_HIP_CHECK(hipMemsetAsync(d_mask, 0, (size_t)B * N * N, stream));
    if (P > 1) hipLaunchKernelGGL(floater_lines_kernel, dim3((unsigned)((P - 1 + 63) / 64), (unsigned)B), dim3(64), 0, stream, d_pts, d_npts, P, N, d_mask);
    hipLaunchKernelGGL(floater_coldist_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256), 0, stream, d_mask, N, d_dist);
    hipLaunchKernelGGL(floater_rowdist_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), (size_t)3 * N * sizeof(int), stream, d_dist, d_dilations, N, d_mask);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

constexpr int MAX_RADIUS = 512;      // LDS tile of blur_rows_kernel: TY * (TX + 2 radius) doubles = 34 KB at the cap
constexpr int MAX_FLOATER_N = 4096;  // LDS of floater_rowdist_kernel: 3 N ints = 48 KB at the cap

}  // namespace

extern "C" int octa_menten_vessel_noise(octa_ctx *ctx, const void *d_img, int img_dtype, const unsigned char *d_bernoulli, const double *d_quantum,
                                        const double *d_weights, int radius, double scaling, double r, int B, int H, int W, double *d_tmp,
                                        double *d_out, void *stream_) {
    if (!ctx || !d_img || !d_bernoulli || !d_quantum || !d_weights || !d_tmp || !d_out || bad_dims(B, H, W) || radius < 0 || radius > MAX_RADIUS ||
        (img_dtype != 0 && img_dtype != 1) || d_tmp == d_out) {
        octa::set_error("octa_menten_vessel_noise: bad arguments (img_dtype 0 = float32, 1 = float64; radius <= %d)", MAX_RADIUS); return -2;
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    VesselSrc src{d_bernoulli, H, W, 0, {0, 0, 0, 0, 0}, {0, 0, 0, 0, 0}};
    src.integral = (r == std::floor(r) && std::fabs(r) < 1e8) ? 1 : 0;
    for (int m = 0; m < 5; m++) {
        const double t = r - 3.0 * m;
        src.thr[m] = t;
        src.thr4[m] = (src.integral && t > 0) ? 4LL * (long long)t * (long long)t : 0;
    }
    const size_t lds = (size_t)TY * (TX + 2 * radius) * sizeof(double);
    hipLaunchKernelGGL((blur_rows_kernel<VesselSrc, StoreF64>), dim3((unsigned)((W + TX - 1) / TX), (unsigned)((H + TY - 1) / TY), (unsigned)B), dim3(TX * TY), lds,
                       stream, src, StoreF64{d_tmp, H, W}, d_weights, radius, H, W);
    hipLaunchKernelGGL((blur_cols_kernel<F64Src, VesselCombine>), dim3((unsigned)((W + 255) / 256), (unsigned)H, (unsigned)B), dim3(256), 0, stream,
                       F64Src{d_tmp, H, W}, VesselCombine{d_img, d_quantum, d_out, H, W, img_dtype, scaling, 1.0 + scaling / 1.5}, d_weights, radius, H, W);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_menten_floater_mask(octa_ctx *ctx, const int *d_pts, const int *d_npts, const int *d_dilations, int B, int P, int N,
                                        unsigned char *d_mask, int *d_dist, void *stream_) {
    if (!ctx || !d_pts || !d_npts || !d_dilations || !d_mask || !d_dist || bad_dims(B, N, N) || P < 1 || N > MAX_FLOATER_N) {
        octa::set_error("octa_menten_floater_mask: bad arguments (N <= %d)", MAX_FLOATER_N); return -2;
    }
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    return floater_mask_launch(d_pts, d_npts, d_dilations, B, P, N, d_mask, d_dist, (hipStream_t)stream_);
}

extern "C" int octa_menten_floater(octa_ctx *ctx, const double *d_img, const int *d_pts, const int *d_npts, const int *d_dilations,
                                   const double *d_weights, int radius, int B, int P, int N, unsigned char *d_mask, int *d_dist, double *d_tmp,
                                   double *d_out, void *stream_) {
    if (!ctx || !d_img || !d_pts || !d_npts || !d_dilations || !d_weights || !d_mask || !d_dist || !d_tmp || !d_out || bad_dims(B, N, N) || P < 1 ||
        N > MAX_FLOATER_N || radius < 0 || radius > MAX_RADIUS || d_tmp == d_out || d_tmp == d_img) {
        octa::set_error("octa_menten_floater: bad arguments (N <= %d, radius <= %d)", MAX_FLOATER_N, MAX_RADIUS); return -2;
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    if (int rc = floater_mask_launch(d_pts, d_npts, d_dilations, B, P, N, d_mask, d_dist, stream)) return rc;
    hipLaunchKernelGGL((blur_cols_kernel<MaskSrc, StoreF64>), dim3((unsigned)((N + 255) / 256), (unsigned)N, (unsigned)B), dim3(256), 0, stream,
                       MaskSrc{d_mask, N, N}, StoreF64{d_tmp, N, N}, d_weights, radius, N, N);
    const size_t lds = (size_t)TY * (TX + 2 * radius) * sizeof(double);
    hipLaunchKernelGGL((blur_rows_kernel<F64Src, FloaterMul>), dim3((unsigned)((N + TX - 1) / TX), (unsigned)((N + TY - 1) / TY), (unsigned)B), dim3(TX * TY), lds,
                       stream, F64Src{d_tmp, N, N}, FloaterMul{d_img, d_out, N, N}, d_weights, radius, N, N);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_menten_motion(octa_ctx *ctx, const void *d_in, void *d_out, int elem_size, const int *d_table, const void *d_white, int n_white,
                                  int unit_elems, int B, int H, int W, void *stream_) {
    const size_t ub = (size_t)elem_size * (size_t)(unit_elems > 0 ? unit_elems : 1);
    if (!ctx || !d_in || !d_out || !d_table || d_in == d_out || bad_dims(B, H, W) || (elem_size != 4 && elem_size != 8) || n_white < 0 ||
        (n_white > 0 && !d_white) || (ub != 4 && ub != 8 && ub != 16) || W % unit_elems != 0 || (uintptr_t)d_in % ub || (uintptr_t)d_out % ub ||
        (uintptr_t)d_white % ub) {
        octa::set_error("octa_menten_motion: bad arguments (elem_size 4 or 8; unit of 4, 8 or 16 bytes dividing the row, tensors aligned to it)"); return -2;
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const int Wu = W / unit_elems;
    const dim3 grid((unsigned)((Wu + 255) / 256), (unsigned)H, (unsigned)B);
    if (ub == 4) hipLaunchKernelGGL(motion_gather_kernel<uint32_t>, grid, dim3(256), 0, stream, static_cast<const uint32_t *>(d_in), static_cast<uint32_t *>(d_out), d_table, static_cast<const uint32_t *>(d_white), n_white, H, Wu, unit_elems);
    else if (ub == 8) hipLaunchKernelGGL(motion_gather_kernel<uint64_t>, grid, dim3(256), 0, stream, static_cast<const uint64_t *>(d_in), static_cast<uint64_t *>(d_out), d_table, static_cast<const uint64_t *>(d_white), n_white, H, Wu, unit_elems);
    else hipLaunchKernelGGL(motion_gather_kernel<uint4>, grid, dim3(256), 0, stream, static_cast<const uint4 *>(d_in), static_cast<uint4 *>(d_out), d_table, static_cast<const uint4 *>(d_white), n_white, H, Wu, unit_elems);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
