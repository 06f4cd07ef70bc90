// noise_model.hip -- the reference's handcrafted noise model (models/noise_model.py NoiseModel.forward with adversarial=False, behind
// data/data_transforms.py NoiseModeld) as ONE fused pass over a mini-batch in HBM, and its backward with respect to the control grids for
// adversarial training (utils/losses.py ANTLoss; second half of this file):
//
//   A_v, B_v, A_s, B_s = max(bicubic(control grids), 1e-3)        Gamma = bicubic(clamp(g, 0, 1) 2 lg + (1 - lg))
//   Delta ~ Beta(A_v, B_v), N ~ Beta(A_s, B_s)                    per pixel
//   out = pow(max(I, I_d ld Delta) (ls N + 1 - ls) + 1e-6, Gamma) float32, in the reference's order of operations
//
// The five control grids of a sample (gh x gw each, 9 x 9 by default) are staged in LDS; the bicubic upsampling is torch's
// upsample_bicubic2d (align_corners False, A = -0.75, source = (dst + 0.5) in / out - 0.5 unclamped, the four tap indices clamped to the grid).
//
// The per-pixel Beta draws are made here, not on the host (the reference draws two 304^2 fields from torch.distributions.Beta per sample, 17 ms
// each on a CPU core). Generator: Philox-4x32-10 (philox.h), key = the call's 64-bit seed, counter = (pixel y W + x, sample, field, round):
// a pixel's draws depend on nothing else -- not on the launch geometry, not on the batch size -- and a rerun with the same seed is
// bit-identical. field 0 = Delta, 1 = N. round 0 holds the two uniforms of the small-shape boost, rounds 1 .. MT_ROUNDS one attempt each of
// the two Gamma variates of a Beta sample: words 0, 1 -> two normals (Box-Muller), words 2, 3 -> the two acceptance uniforms.
//
// Sampler, fp32: Beta = G_a / (G_a + G_b) from two Gamma draws, carried as logarithms, Beta = 1 / (1 + exp(log G_b - log G_a)): shapes go down
// to the clamp 1e-3, where U^(1 / a) underflows every float format. Gamma(a >= 1): Marsaglia-Tsang (ACM TOMS 26, 2000): d = a - 1/3,
// c = 1 / sqrt(9 d), v = (1 + c x)^3, accept when v > 0 and log u < x^2 / 2 + d - d v + d log v; log G = log d + log v. Gamma(a < 1):
// log G(a) = log G(a + 1) + log(U) / a. An attempt succeeds with probability > 0.95 for every shape; after MT_ROUNDS = 16 refusals in a row
// (probability < 1e-20 per variate) the variate is d, the v = 1 value, so no loop here can run longer than 16 rounds whatever the input is.
// The result is clamped to [0, 1] with NaN -> 0, so it is finite for every control grid, non-finite ones included.

#include "common.h"
#include "philox.h"

namespace {

constexpr int MT_ROUNDS = 16;
constexpr int NM_THREADS = 256;
constexpr int MAX_GRID_POINTS = 1024;      // 5 grids x 1024 floats = 20 KB of LDS at the cap

// torch's cubic convolution weights for fraction t (aten/native/UpSample.h get_cubic_upsample_coefficients, A = -0.75)
__device__ __forceinline__ void cubic_weights(float t, float w[4]) {
    const float A = -0.75f;
    const float x0 = t + 1.0f, x1 = t, x2 = 1.0f - t, x3 = 2.0f - t;
    w[0] = ((A * x0 - 5.0f * A) * x0 + 8.0f * A) * x0 - 4.0f * A;
    w[1] = ((A + 2.0f) * x1 - (A + 3.0f)) * x1 * x1 + 1.0f;
    w[2] = ((A + 2.0f) * x2 - (A + 3.0f)) * x2 * x2 + 1.0f;
    w[3] = ((A * x3 - 5.0f * A) * x3 + 8.0f * A) * x3 - 4.0f * A;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

struct GammaDraw {
    float d, c, boost;      // Marsaglia-Tsang constants of shape max(a, a + 1); boost = log(U) / a for a < 1, else 0
    float logg;
    bool done;
};

__device__ __forceinline__ GammaDraw gamma_begin(float a, float u_boost) {
    GammaDraw g;
    const bool small = !(a >= 1.0f);
    const float a1 = small ? a + 1.0f : a;
    g.d = a1 - 1.0f / 3.0f;
    g.c = 1.0f / sqrtf(9.0f * g.d);
    g.boost = small ? logf(u_boost) / a : 0.0f;
    g.logg = logf(g.d) + g.boost;          // the value when every attempt is refused (v = 1)
    g.done = false;
    return g;
}

__device__ __forceinline__ void gamma_attempt(GammaDraw &g, float x, float u) {
    if (g.done) return;
    const float t = 1.0f + g.c * x;
    const float v = t * t * t;
    if (v > 0.0f) {
        const float lv = logf(v);
        if (logf(u) < 0.5f * x * x + g.d - g.d * v + g.d * lv) {
            g.logg = logf(g.d) + lv + g.boost;
            g.done = true;
        }
    }
}

// the log-odds t = log G_a - log G_b of one Beta(a, b) variate for (pixel, sample, field) under key (k0, k1): x = 1 / (1 + e^-t),
// 1 - x = 1 / (1 + e^t). The forward takes x alone; the backward (below) needs both and must never form 1 - x by subtraction.
__device__ float beta_logodds(float a, float b, uint32_t pixel, uint32_t sample, uint32_t field, uint32_t k0, uint32_t k1) {
    const octa::Philox4 r0 = octa::philox4x32_10(pixel, sample, field, 0u, k0, k1);
    GammaDraw ga = gamma_begin(a, octa::philox_unit(r0.v[0]));
    GammaDraw gb = gamma_begin(b, octa::philox_unit(r0.v[1]));
    for (uint32_t round = 1; round <= (uint32_t)MT_ROUNDS && !(ga.done && gb.done); round++) {
        const octa::Philox4 r = octa::philox4x32_10(pixel, sample, field, round, k0, k1);
        const float rad = sqrtf(-2.0f * logf(octa::philox_unit(r.v[0])));
        float s, co;
        sincosf(6.283185307179586f * octa::philox_unit(r.v[1]), &s, &co);
        gamma_attempt(ga, rad * co, octa::philox_unit(r.v[2]));
        gamma_attempt(gb, rad * s, octa::philox_unit(r.v[3]));
    }
    return ga.logg - gb.logg;
}

// the variate of log-odds t, as the forward writes it (-t = log G_b - log G_a exactly: a float difference changes sign with its operands)
__device__ __forceinline__ float beta_from_logodds(float t) {
    float x = 1.0f / (1.0f + expf(-t));
    x = fmaxf(x, 0.0f);                    // fmaxf(NaN, 0) = 0
    return fminf(x, 1.0f);
}

__device__ float beta_draw(float a, float b, uint32_t pixel, uint32_t sample, uint32_t field, uint32_t k0, uint32_t k1) {
    return beta_from_logodds(beta_logodds(a, b, pixel, sample, field, k0, k1));
}

struct NoiseArgs {
    const float *img, *bg, *grids, *delta_in, *n_in;
    float *out, *maps, *fields;
    int H, W, gh, gw;
    uint32_t k0, k1, sample0;
    float ld, ls, one_minus_ls, two_lg, one_minus_lg;
};

// the five control grids of sample b into LDS as [5][gh * gw]; the gamma grid already mapped to its range
__device__ __forceinline__ void stage_grids(const NoiseArgs &p, int b, float *cp) {
    const int G = p.gh * p.gw;
    const float *src = p.grids + (size_t)b * 5 * G;
    for (int i = threadIdx.x; i < 5 * G; i += NM_THREADS) {
        float v = src[i];
        if (i >= 4 * G) v = fminf(fmaxf(v, 0.0f), 1.0f) * p.two_lg + p.one_minus_lg;
        cp[i] = v;
    }
    __syncthreads();
}

struct Taps {
    float wy[4], wx[4];
    int iy[4], ix[4];      // iy: row offsets (index * gw)
};

// torch: scale = (float)in / out; source = scale (dst + 0.5) - 0.5, floor, fraction
__device__ __forceinline__ Taps bicubic_taps(const NoiseArgs &p, int y, int x) {
    Taps t;
    const float sy = ((float)p.gh / (float)p.H) * ((float)y + 0.5f) - 0.5f;
    const float sx = ((float)p.gw / (float)p.W) * ((float)x + 0.5f) - 0.5f;
    const float fy = floorf(sy), fx = floorf(sx);
    cubic_weights(sy - fy, t.wy);
    cubic_weights(sx - fx, t.wx);
    for (int k = 0; k < 4; k++) {
        t.iy[k] = clampi((int)fy - 1 + k, 0, p.gh - 1) * p.gw;
        t.ix[k] = clampi((int)fx - 1 + k, 0, p.gw - 1);
    }
    return t;
}

__device__ __forceinline__ float bicubic_at(const float *g, const Taps &t) {
    float acc = 0.0f;
    for (int j = 0; j < 4; j++) {
        const float *row = g + t.iy[j];
        const float r = row[t.ix[0]] * t.wx[0] + row[t.ix[1]] * t.wx[1] + row[t.ix[2]] * t.wx[2] + row[t.ix[3]] * t.wx[3];
        acc += r * t.wy[j];
    }
    return acc;
}

__global__ void __launch_bounds__(NM_THREADS) noise_model_kernel(NoiseArgs p) {
    extern __shared__ __align__(16) float cp[];      // [5][gh * gw]: alpha_v, beta_v, alpha_s, beta_s, gamma (already mapped to its range)
    const int b = blockIdx.y, G = p.gh * p.gw;
    stage_grids(p, b, cp);
    const int HW = p.H * p.W;
    const int pix = blockIdx.x * NM_THREADS + threadIdx.x;
    if (pix >= HW) return;
    const int y = pix / p.W, x = pix - y * p.W;
    const Taps taps = bicubic_taps(p, y, x);
    float m[5];
    for (int f = 0; f < 5; f++) {
        const float acc = bicubic_at(cp + f * G, taps);
        m[f] = f < 4 ? fmaxf(acc, 1e-3f) : acc;
    }
    const size_t i = (size_t)b * HW + pix;
    const uint32_t sample = p.sample0 + (uint32_t)b;
    const float delta = p.delta_in ? p.delta_in[i] : beta_draw(m[0], m[1], (uint32_t)pix, sample, 0u, p.k0, p.k1);
    const float n = p.n_in ? p.n_in[i] : beta_draw(m[2], m[3], (uint32_t)pix, sample, 1u, p.k0, p.k1);

    const float d = p.bg[i] * p.ld * delta;
    float v = fmaxf(p.img[i], d);
    v = v * (p.ls * n + p.one_minus_ls);
    p.out[i] = powf(v + 1e-6f, m[4]);
    if (p.maps)
        for (int f = 0; f < 5; f++) p.maps[((size_t)b * 5 + f) * HW + pix] = m[f];
    if (p.fields) {
        p.fields[((size_t)b * 2 + 0) * HW + pix] = delta;
        p.fields[((size_t)b * 2 + 1) * HW + pix] = n;
    }
}

// ---- backward ----------------------------------------------------------------------------------------------------------------------------
// dGrids of sum(out dOut). Nothing is saved by the forward: the draws are a pure function of (pixel, sample, field, seed), so the pixel pass
// regenerates the log-odds of Delta and N with beta_logodds above -- the forward's own code -- and gets the forward's bits.
//
// Pass 1, one thread per pixel (the forward's geometry): the chain  out = pow(u, Gamma), u = v s + 1e-6, v = max(I, d), d = I_d ld Delta,
// s = ls N + (1 - ls)  backwards as torch's autograd takes it (pow: Gamma u^(Gamma - 1) and out log u; maximum: the larger side, half each at
// a tie; clamp(min = 1e-3): where the bicubic value is >= 1e-3), the reparameterised Beta gradient dx/dA, dx/dB (below), and the five map
// gradients of the pixel to dmaps [B][5][H][W].
// Pass 2, one block per (control point, grid, sample): the adjoint of the bicubic upsampling as a GATHER over the control point's support
// (the pixels one of whose four taps per axis lands on it, about (4 H / gh) x (4 W / gw)), each thread a fixed strided subset in a fixed
// order, summed in double, then a fixed LDS tree. No atomics: the same bits every run, for every batch size and launch order.
//
// Reparameterised Beta gradient: what torch.distributions.Beta.rsample back-propagates, torch._dirichlet_grad on the two-simplex followed by
// _Dirichlet_backward's projection: dx/dA = D(x, A, B) (1 - x), dx/dB = -D(1 - x, B, A) x with D = -(d cdf / d alpha) / pdf / (1 - x),
// torch's piecewise method (ATen/native/Distributions.h, BSD: series in x near 0, series in 1 - x near 1, a Rice saddle-point expansion for
// two large shapes, a rational correction to x (psi(a + b) - psi(a)) / b elsewhere) restated in double, with x AND 1 - x taken from the
// log-odds: x = 1 / (1 + e^-t), 1 - x = 1 / (1 + e^t). Every loop has a constant trip count; a non-finite result (and x in {0, 1}) gives 0.

__device__ double digamma_pos(double x) {      // Cephes' psi for x > 0 as torch restates it (digamma_one); shapes here are >= 1e-3
    if (!(x > 0.0)) return INFINITY;
    double result = 0.0;
    for (int k = 0; k < 10 && x < 10.0; k++) {
        result -= 1.0 / x;
        x += 1.0;
    }
    if (x == 10.0) return result + 2.25175258906672110764;
    double y = 0.0;
    if (x < 1.0e17) {
        const double z = 1.0 / (x * x);
        y = z * ((((((8.33333333333333333333E-2 * z - 2.10927960927960927961E-2) * z + 7.57575757575757575758E-3) * z - 4.16666666666666666667E-3) * z +
                   3.96825396825396825397E-3) * z - 8.33333333333333333333E-3) * z + 8.33333333333333333333E-2);
    }
    return result + log(x) - 0.5 / x - y;
}

// x near 0 (xc = 1 - x)
__device__ double beta_grad_alpha_small(double x, double xc, double alpha, double beta) {
    const double factor = digamma_pos(alpha) - digamma_pos(alpha + beta) - log(x);
    double numer = 1.0, series = numer / alpha * (factor + 1.0 / alpha);
    for (int i = 1; i <= 10; i++) {
        numer *= ((double)i - beta) * x / (double)i;
        const double denom = alpha + (double)i;
        series += numer / denom * (factor + 1.0 / denom);
    }
    return x * pow(xc, -beta) * series;
}

__device__ double beta_grad_beta_small(double x, double xc, double alpha, double beta) {
    const double factor = digamma_pos(alpha + beta) - digamma_pos(beta);
    double numer = 1.0, betas = 1.0, dbetas = 0.0, series = factor / alpha;
    for (int i = 1; i <= 8; i++) {
        numer *= -x / (double)i;
        dbetas = dbetas * (beta - (double)i) + betas;
        betas = betas * (beta - (double)i);
        series += numer / (alpha + (double)i) * (dbetas + factor * betas);
    }
    return -pow(xc, 1.0 - beta) * series;
}

// both shapes large: Rice saddle-point expansion; x - 1 is -xc
__device__ double beta_grad_alpha_mid(double x, double xc, double alpha, double beta) {
    const double total = alpha + beta, mean = alpha / total, sd = sqrt(alpha * beta / (total + 1.0)) / total;
    if (mean - 0.1 * sd <= x && x <= mean + 0.1 * sd) {      // the singularity at x = mean
        const double b2 = beta * beta;
        const double poly = 47.0 * x * b2 * b2 + alpha * ((43.0 + 20.0 * (16.0 + 27.0 * beta) * x) * b2 * beta + alpha * (
                            3.0 * (59.0 + 180.0 * beta - 90.0 * x) * b2 + alpha * ((453.0 + 1620.0 * beta * xc - 455.0 * x) * beta + alpha * (
                            8.0 * xc * (135.0 * beta - 11.0)))));
        const double prefactor_num = (1.0 + 12.0 * alpha) * (1.0 + 12.0 * beta) / (total * total);
        const double prefactor_den = 12960.0 * alpha * alpha * alpha * b2 * (1.0 + 12.0 * total);
        return prefactor_num / xc * poly / prefactor_den;
    }
    const double prefactor = -x / sqrt(2.0 * alpha * beta / total);
    const double stirling = (1.0 + 1.0 / (12.0 * alpha) + 1.0 / (288.0 * alpha * alpha)) * (1.0 + 1.0 / (12.0 * beta) + 1.0 / (288.0 * beta * beta)) /
                            (1.0 + 1.0 / (12.0 * total) + 1.0 / (288.0 * total * total));
    const double term1_num = -2.0 * (alpha * alpha) * xc - alpha * beta * xc - x * (beta * beta);
    const double axbx = beta * x - alpha * xc;
    const double term1 = term1_num / (sqrt(2.0 * alpha / beta) * pow(total, 1.5) * axbx * axbx);
    const double term2 = 0.5 * log(alpha / (total * x));
    const double term3 = sqrt(8.0 * alpha * beta / total) / axbx;
    const double term4 = pow(beta * log(beta / (total * xc)) + alpha * log(alpha / (total * x)), -1.5);
    return stirling * prefactor * (term1 + term2 * (term3 + (x < mean ? term4 : -term4)));
}

__constant__ double BETA_GRAD_RATIONAL[2][3][3][4] = {
    {{{1.003668233, -0.01061107488, -0.0657888334, 0.01201642863},
      {0.6336835991, -0.3557432599, 0.05486251648, -0.001465281033},
      {-0.03276231906, 0.004474107445, 0.002429354597, -0.0001557569013}},
     {{0.221950385, -0.3187676331, 0.01799915743, 0.01074823814},
      {-0.2951249643, 0.06219954479, 0.01535556598, 0.001550077057},
      {0.02155310298, 0.004170831599, 0.001292462449, 6.976601077e-05}},
     {{-0.05980841433, 0.008441916499, 0.01085618172, 0.002319392565},
      {0.02911413504, 0.01400243777, -0.002721828457, 0.000751041181},
      {0.005900514878, -0.001936558688, -9.495446725e-06, 5.385558597e-05}}},
    {{{1, -0.02924021934, -0.04438342661, 0.007285809825},
      {0.6357567472, -0.3473456711, 0.05454656494, -0.002407477521},
      {-0.03301322327, 0.004845219414, 0.00231480583, -0.0002307248149}},
     {{0.5925320577, -0.1757678135, 0.01505928619, 0.000564515273},
      {0.1014815858, -0.06589186703, 0.01272886114, -0.0007316646956},
      {-0.007258481865, 0.001096195486, 0.0003934994223, -4.12701925e-05}},
     {{0.06469649321, -0.0236701437, 0.002902096474, -5.896963079e-05},
      {0.001925008108, -0.002869809258, 0.0008000589141, -6.063713228e-05},
      {-0.0003477407336, 6.959756487e-05, 1.097287507e-05, -1.650964693e-06}}},
};

// D(x, alpha, beta) = -(d cdf(x; alpha, beta) / d alpha) / pdf(x; alpha, beta) / (1 - x); xc = 1 - x
__device__ double dirichlet_grad_one(double x, double xc, double alpha, double beta) {
    const double total = alpha + beta, boundary = total * x * xc;
    if (x <= 0.5 && boundary < 2.5) return beta_grad_alpha_small(x, xc, alpha, beta);
    if (x >= 0.5 && boundary < 0.75) return -beta_grad_beta_small(xc, x, beta, alpha);
    if (alpha > 6.0 && beta > 6.0) return beta_grad_alpha_mid(x, xc, alpha, beta);
    const double u = log(x), a = log(alpha) - u, b = log(total) - a;
    const double pow_u[3] = {1.0, u, u * u}, pow_a[3] = {1.0, a, a * a};
    double p = 0.0, q = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double ua = pow_u[i] * pow_a[j];
            const double *c0 = BETA_GRAD_RATIONAL[0][i][j], *c1 = BETA_GRAD_RATIONAL[1][i][j];
            p += ua * (c0[0] + b * (c0[1] + b * (c0[2] + b * c0[3])));
            q += ua * (c1[0] + b * (c1[1] + b * (c1[2] + b * c1[3])));
        }
    return p / q * (x * (digamma_pos(total) - digamma_pos(alpha)) / beta);
}

// dx/da, dx/db of the Beta(a, b) variate of log-odds t
__device__ void beta_rsample_grad(float t, float a, float b, float &dxda, float &dxdb) {
    const double td = (double)t, x = 1.0 / (1.0 + exp(-td)), xc = 1.0 / (1.0 + exp(td));
    dxda = dxdb = 0.0f;
    if (!(x > 0.0 && xc > 0.0)) return;      // x in {0, 1}, NaN log-odds
    const float ga = (float)(dirichlet_grad_one(x, xc, (double)a, (double)b) * xc);
    const float gb = (float)(-dirichlet_grad_one(xc, x, (double)b, (double)a) * x);
    dxda = isfinite(ga) ? ga : 0.0f;
    dxdb = isfinite(gb) ? gb : 0.0f;
}

struct NoiseBwdArgs {
    NoiseArgs f;               // f.out / f.maps (optional): the re-run forward's output and maps
    const float *dout;
    float *dgrids, *dmaps, *logodds, *bgrad;
};

__global__ void __launch_bounds__(NM_THREADS) noise_model_bwd_pixel_kernel(NoiseBwdArgs q) {
    extern __shared__ __align__(16) float cp[];
    const NoiseArgs &p = q.f;
    const int b = blockIdx.y, G = p.gh * p.gw;
    stage_grids(p, b, cp);
    const int HW = p.H * p.W;
    const int pix = blockIdx.x * NM_THREADS + threadIdx.x;
    if (pix >= HW) return;
    const int y = pix / p.W, x = pix - y * p.W;
    const Taps taps = bicubic_taps(p, y, x);
    float m[5];
    bool open[4];              // the clamp at 1e-3 passes the gradient (torch.clamp: where the value is >= min)
    for (int f = 0; f < 5; f++) {
        const float acc = bicubic_at(cp + f * G, taps);
        if (f < 4) open[f] = acc >= 1e-3f;
        m[f] = f < 4 ? fmaxf(acc, 1e-3f) : acc;
    }
    const size_t i = (size_t)b * HW + pix;
    const uint32_t sample = p.sample0 + (uint32_t)b;
    float t[2] = {0.0f, 0.0f}, field[2], g[4] = {0.0f, 0.0f, 0.0f, 0.0f};      // g: dDelta/dA_v, dDelta/dB_v, dN/dA_s, dN/dB_s
    for (int k = 0; k < 2; k++) {
        const float *given = k == 0 ? p.delta_in : p.n_in;
        if (given) {
            field[k] = given[i];                                               // an injected field does not depend on the grids
        } else {
            t[k] = beta_logodds(m[2 * k], m[2 * k + 1], (uint32_t)pix, sample, (uint32_t)k, p.k0, p.k1);
            field[k] = beta_from_logodds(t[k]);
            beta_rsample_grad(t[k], m[2 * k], m[2 * k + 1], g[2 * k], g[2 * k + 1]);
        }
    }
    const float img = p.img[i], bl = p.bg[i] * p.ld;
    const float d = bl * field[0];
    const float v = fmaxf(img, d);
    const float s = p.ls * field[1] + p.one_minus_ls;
    const float u = v * s + 1e-6f;
    const float out = powf(u, m[4]);
    const float go = q.dout[i];
    const float du = go * (m[4] * powf(u, m[4] - 1.0f));
    const float dd = (du * s) * (d > img ? 1.0f : (d == img ? 0.5f : 0.0f));
    const float ddelta = dd * bl, dn = (du * v) * p.ls;
    float gm[5];
    gm[0] = open[0] ? ddelta * g[0] : 0.0f;
    gm[1] = open[1] ? ddelta * g[1] : 0.0f;
    gm[2] = open[2] ? dn * g[2] : 0.0f;
    gm[3] = open[3] ? dn * g[3] : 0.0f;
    gm[4] = go * (out * logf(u));
    for (int f = 0; f < 5; f++) q.dmaps[((size_t)b * 5 + f) * HW + pix] = gm[f];
    if (p.out) p.out[i] = out;
    if (p.maps)
        for (int f = 0; f < 5; f++) p.maps[((size_t)b * 5 + f) * HW + pix] = m[f];
    if (q.logodds)
        for (int k = 0; k < 2; k++) q.logodds[((size_t)b * 2 + k) * HW + pix] = t[k];
    if (q.bgrad)
        for (int k = 0; k < 4; k++) q.bgrad[((size_t)b * 4 + k) * HW + pix] = g[k];
}

// the weight with which output position `o` of an axis (n_in control points -> n_out pixels) reads control point c: the forward's taps, the ones
// the index clamp merged summed
__device__ __forceinline__ float axis_weight(int o, int n_in, int n_out, int c) {
    const float s = ((float)n_in / (float)n_out) * ((float)o + 0.5f) - 0.5f;
    const float fl = floorf(s);
    float w[4];
    cubic_weights(s - fl, w);
    float sum = 0.0f;
    for (int k = 0; k < 4; k++)
        if (clampi((int)fl - 1 + k, 0, n_in - 1) == c) sum += w[k];
    return sum;
}

// the output positions that can read control point c: source coordinate in [c - 2, c + 2), one position of slack each side (positions in the range
// that do not read c get weight 0 from axis_weight). The float32 source coordinate of axis_weight is off by about n_out 2^-23 positions
// at most, inside the slack for n_out <= 2^20, which octa_noise_model_backward enforces
__device__ __forceinline__ void axis_support(int c, int n_in, int n_out, int &lo, int &hi) {
    const double r = (double)n_out / (double)n_in;
    const double a = floor(((double)c - 1.5) * r - 0.5) - 1.0, b = ceil(((double)c + 2.5) * r - 0.5) + 1.0;
    lo = a < 0.0 ? 0 : (int)a;
    hi = b > (double)(n_out - 1) ? n_out - 1 : (int)b;
}

__global__ void __launch_bounds__(NM_THREADS) noise_model_bwd_gather_kernel(NoiseBwdArgs q) {
    __shared__ double part[NM_THREADS];
    const NoiseArgs &p = q.f;
    const int c = blockIdx.x, f = blockIdx.y, b = blockIdx.z, G = p.gh * p.gw;
    const int cy = c / p.gw, cx = c - cy * p.gw;
    int y0, y1, x0, x1;
    axis_support(cy, p.gh, p.H, y0, y1);
    axis_support(cx, p.gw, p.W, x0, x1);
    const int nx = x1 - x0 + 1;
    const int64_t count = (int64_t)(y1 - y0 + 1) * nx;
    const float *src = q.dmaps + ((size_t)b * 5 + f) * ((size_t)p.H * p.W);
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < count; i += NM_THREADS) {
        const int yy = y0 + (int)(i / nx), xx = x0 + (int)(i % nx);
        const float w = axis_weight(yy, p.gh, p.H, cy) * axis_weight(xx, p.gw, p.W, cx);
        if (w != 0.0f) acc += (double)w * (double)src[(size_t)yy * p.W + xx];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int half = NM_THREADS / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) part[threadIdx.x] += part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float r = (float)part[0];
        if (f == 4) {              // gamma: clamp(g, 0, 1) 2 lg + (1 - lg); torch.clamp passes the gradient on the closed interval
            const float gv = p.grids[((size_t)b * 5 + 4) * G + c];
            r = (gv >= 0.0f && gv <= 1.0f) ? r * p.two_lg : 0.0f;
        }
        q.dgrids[((size_t)b * 5 + f) * G + c] = r;
    }
}

}  // namespace

extern "C" void octa_philox4x32_10(const uint32_t *counter4, const uint32_t *key2, uint32_t *out4) {
    const octa::Philox4 r = octa::philox4x32_10(counter4[0], counter4[1], counter4[2], counter4[3], key2[0], key2[1]);
    for (int k = 0; k < 4; k++) out4[k] = r.v[k];
}

static const char *fill_noise_args(NoiseArgs &p, const float *d_img, const float *d_background, const float *d_grids, int B, int H, int W, int gh, int gw,
                                   uint64_t seed, uint32_t sample_offset, double lambda_delta, double lambda_speckle, double lambda_gamma,
                                   const float *d_delta_in, const float *d_n_in) {
    if (!d_img || !d_background || !d_grids || B <= 0 || H <= 0 || W <= 0 || B > 65535 || (int64_t)H * W > (int64_t)1 << 30 || gh < 1 || gw < 1 ||
        (int64_t)gh * gw > MAX_GRID_POINTS)
        return "bad arguments";
    p.img = d_img; p.bg = d_background; p.grids = d_grids; p.delta_in = d_delta_in; p.n_in = d_n_in;
    p.out = nullptr; p.maps = nullptr; p.fields = nullptr;
    p.H = H; p.W = W; p.gh = gh; p.gw = gw;
    p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32); p.sample0 = sample_offset;
    // the reference multiplies float32 tensors by Python floats: each scalar is formed in double, then rounded to float32 once
    p.ld = (float)lambda_delta; p.ls = (float)lambda_speckle; p.one_minus_ls = (float)(1.0 - lambda_speckle);
    p.two_lg = (float)(2.0 * lambda_gamma); p.one_minus_lg = (float)(1.0 - lambda_gamma);
    return nullptr;
}

extern "C" int octa_noise_model(octa_ctx *ctx, const float *d_img, const float *d_background, const float *d_grids, int B, int H, int W, int gh,
                                int gw, uint64_t seed, uint32_t sample_offset, double lambda_delta, double lambda_speckle, double lambda_gamma,
                                const float *d_delta_in, const float *d_n_in, float *d_out, float *d_maps, float *d_fields, void *stream_) {
    NoiseArgs p;
    if (!ctx || !d_out || d_out == d_img || d_out == d_background ||
        fill_noise_args(p, d_img, d_background, d_grids, B, H, W, gh, gw, seed, sample_offset, lambda_delta, lambda_speckle, lambda_gamma, d_delta_in, d_n_in)) {
        octa::set_error("octa_noise_model: bad arguments (B <= 65535, H W <= 2^30, gh gw <= %d, out must not alias an input)", MAX_GRID_POINTS);
        return -2;
    }
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    p.out = d_out; p.maps = d_maps; p.fields = d_fields;
    const dim3 grid((unsigned)(((int64_t)H * W + NM_THREADS - 1) / NM_THREADS), (unsigned)B);
    hipLaunchKernelGGL(noise_model_kernel, grid, dim3(NM_THREADS), (size_t)5 * gh * gw * sizeof(float), (hipStream_t)stream_, p);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int octa_noise_model_backward(octa_ctx *ctx, const float *d_dout, const float *d_img, const float *d_background, const float *d_grids, int B, int H,
                                         int W, int gh, int gw, uint64_t seed, uint32_t sample_offset, double lambda_delta, double lambda_speckle,
                                         double lambda_gamma, const float *d_delta_in, const float *d_n_in, float *d_dgrids, float *d_dmaps, float *d_out,
                                         float *d_maps, float *d_logodds, float *d_bgrad, void *stream_) {
    NoiseBwdArgs q;
    // H, W <= 2^20 each: the gather finds a control point's support in double with one pixel of slack, the taps' source coordinate is float32
    // (error about n_out 2^-23 pixels): within the slack up to there
    if (!ctx || !d_dout || !d_dgrids || !d_dmaps || H > (1 << 20) || W > (1 << 20) ||
        fill_noise_args(q.f, d_img, d_background, d_grids, B, H, W, gh, gw, seed, sample_offset, lambda_delta, lambda_speckle, lambda_gamma, d_delta_in, d_n_in)) {
        octa::set_error("octa_noise_model_backward: bad arguments (B <= 65535, H, W <= 2^20, H W <= 2^30, gh gw <= %d, dgrids and dmaps are required)", MAX_GRID_POINTS);
        return -2;
    }
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    q.f.out = d_out; q.f.maps = d_maps;
    q.dout = d_dout; q.dgrids = d_dgrids; q.dmaps = d_dmaps; q.logodds = d_logodds; q.bgrad = d_bgrad;
    const dim3 grid((unsigned)(((int64_t)H * W + NM_THREADS - 1) / NM_THREADS), (unsigned)B);
    hipLaunchKernelGGL(noise_model_bwd_pixel_kernel, grid, dim3(NM_THREADS), (size_t)5 * gh * gw * sizeof(float), (hipStream_t)stream_, q);
    OCTA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(noise_model_bwd_gather_kernel, dim3((unsigned)(gh * gw), 5u, (unsigned)B), dim3(NM_THREADS), 0, (hipStream_t)stream_, q);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
