// noise_model.hip -- the reference's handcrafted noise model (models/noise_model.py NoiseModel.forward with adversarial=False, behind
// data/data_transforms.py NoiseModeld) as ONE fused pass over a mini-batch in HBM:
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

// one Beta(a, b) variate for (pixel, sample, field) under key (k0, k1)
__device__ float beta_draw(float a, float b, uint32_t pixel, uint32_t sample, uint32_t field, uint32_t k0, uint32_t k1) {
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
    float x = 1.0f / (1.0f + expf(gb.logg - ga.logg));
    x = fmaxf(x, 0.0f);                    // fmaxf(NaN, 0) = 0
    return fminf(x, 1.0f);
}

struct NoiseArgs {
    const float *img, *bg, *grids, *delta_in, *n_in;
    float *out, *maps, *fields;
    int H, W, gh, gw;
    uint32_t k0, k1, sample0;
    float ld, ls, one_minus_ls, two_lg, one_minus_lg;
};

__global__ void __launch_bounds__(NM_THREADS) noise_model_kernel(NoiseArgs p) {
    extern __shared__ __align__(16) float cp[];      // [5][gh * gw]: alpha_v, beta_v, alpha_s, beta_s, gamma (already mapped to its range)
    const int b = blockIdx.y, G = p.gh * p.gw;
    const float *src = p.grids + (size_t)b * 5 * G;
    for (int i = threadIdx.x; i < 5 * G; i += NM_THREADS) {
        float v = src[i];
        if (i >= 4 * G) v = fminf(fmaxf(v, 0.0f), 1.0f) * p.two_lg + p.one_minus_lg;
        cp[i] = v;
    }
    __syncthreads();
    const int HW = p.H * p.W;
    const int pix = blockIdx.x * NM_THREADS + threadIdx.x;
    if (pix >= HW) return;
    const int y = pix / p.W, x = pix - y * p.W;

    // torch: scale = (float)in / out; source = scale (dst + 0.5) - 0.5, floor, fraction
    float wy[4], wx[4];
    int iy[4], ix[4];
    {
        const float sy = ((float)p.gh / (float)p.H) * ((float)y + 0.5f) - 0.5f;
        const float sx = ((float)p.gw / (float)p.W) * ((float)x + 0.5f) - 0.5f;
        const float fy = floorf(sy), fx = floorf(sx);
        cubic_weights(sy - fy, wy);
        cubic_weights(sx - fx, wx);
        for (int k = 0; k < 4; k++) {
            iy[k] = clampi((int)fy - 1 + k, 0, p.gh - 1) * p.gw;
            ix[k] = clampi((int)fx - 1 + k, 0, p.gw - 1);
        }
    }
    float m[5];
    for (int f = 0; f < 5; f++) {
        const float *g = cp + f * G;
        float acc = 0.0f;
        for (int j = 0; j < 4; j++) {
            const float *row = g + iy[j];
            const float r = row[ix[0]] * wx[0] + row[ix[1]] * wx[1] + row[ix[2]] * wx[2] + row[ix[3]] * wx[3];
            acc += r * wy[j];
        }
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

}  // namespace

extern "C" void octa_philox4x32_10(const uint32_t *counter4, const uint32_t *key2, uint32_t *out4) {
    const octa::Philox4 r = octa::philox4x32_10(counter4[0], counter4[1], counter4[2], counter4[3], key2[0], key2[1]);
    for (int k = 0; k < 4; k++) out4[k] = r.v[k];
}

extern "C" int octa_noise_model(octa_ctx *ctx, const float *d_img, const float *d_background, const float *d_grids, int B, int H, int W, int gh,
                                int gw, uint64_t seed, uint32_t sample_offset, double lambda_delta, double lambda_speckle, double lambda_gamma,
                                const float *d_delta_in, const float *d_n_in, float *d_out, float *d_maps, float *d_fields, void *stream_) {
    if (!ctx || !d_img || !d_background || !d_grids || !d_out || B <= 0 || H <= 0 || W <= 0 || B > 65535 || (int64_t)H * W > (int64_t)1 << 30 ||
        gh < 1 || gw < 1 || (int64_t)gh * gw > MAX_GRID_POINTS || d_out == d_img || d_out == d_background) {
        octa::set_error("octa_noise_model: bad arguments (B <= 65535, H W <= 2^30, gh gw <= %d, out must not alias an input)", MAX_GRID_POINTS);
        return -2;
    }
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    NoiseArgs p;
    p.img = d_img; p.bg = d_background; p.grids = d_grids; p.delta_in = d_delta_in; p.n_in = d_n_in;
    p.out = d_out; p.maps = d_maps; p.fields = d_fields;
    p.H = H; p.W = W; p.gh = gh; p.gw = gw;
    p.k0 = (uint32_t)seed; p.k1 = (uint32_t)(seed >> 32); p.sample0 = sample_offset;
    // the reference multiplies float32 tensors by Python floats: each scalar is formed in double, then rounded to float32 once
    p.ld = (float)lambda_delta; p.ls = (float)lambda_speckle; p.one_minus_ls = (float)(1.0 - lambda_speckle);
    p.two_lg = (float)(2.0 * lambda_gamma); p.one_minus_lg = (float)(1.0 - lambda_gamma);
    const dim3 grid((unsigned)(((int64_t)H * W + NM_THREADS - 1) / NM_THREADS), (unsigned)B);
    hipLaunchKernelGGL(noise_model_kernel, grid, dim3(NM_THREADS), (size_t)5 * gh * gw * sizeof(float), (hipStream_t)stream_, p);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
