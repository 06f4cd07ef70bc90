// conv_f32.hip -- single-precision convolution on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32: fp32 operands, fp32
// accumulation -- no bf16 / xf32 rounding anywhere), NCHW, for the paths of the reference that run WITHOUT mixed precision:
//   * test.py:79 and validate.py (model.inference outside torch.cuda.amp.autocast): every convolution of DynUNet
//     (models/networks.py:6 -> MONAI DynUNet: 3x3 stride 1 / 2, 2x2 stride-2 and 1x1 transposed, 1x1 head with bias);
//   * `General.amp: false` forward passes that need no gradient;
//   * round 6: the same for the GAN networks -- test.py with `General.inference: G` and the frozen generator of the docker pipeline
//     (test.py:75-82, docker/dockershell.sh:14-16) run ResnetGenerator in fp32: 7x7 stem / head behind a reflection pad, 3x3 layers with
//     zero padding or none (behind ReflectionPad2d(1)); NLayerDiscriminator's 4x4 stride-1 layers.
// north_star asks for segmentation logits within 1e-4 of the reference's fp32 CPU path: with exact fp32 products and fp32 sums the
// only difference left is the summation order (tests/test_conv_f32_gpu.py: 1x1x1216x1216 DynUNet logits against the CPU modules).
//
// Implicit GEMM, D[co][pixel] += W[co][ci, tap] * X[ci][pixel + tap]: a 256-thread workgroup owns 32 * MB output channels x an
// 8 x 32 output-pixel tile; a wave owns two tile rows (two 32-pixel N-blocks) x MB M-blocks. Per slice of KC = 8 (stride 2: 4) input channels
// the halo tile [KC][IH][IW] and the weight slice [KC][K*K][32 * MB] are staged in LDS (zero-filled outside the image / beyond Cin /
// beyond Cout); an MFMA consumes two input channels of one tap: lane l supplies W[co = l % 32][ci + l / 32] and
// X[ci + l / 32][pixel l % 32] (one ds_read_b32 each, conflict-free: consecutive lanes read consecutive words). The accumulator
// fragment holds, per register, 32 consecutive pixels of one output channel, so the NCHW stores are 128-byte rows straight from
// registers. A 2x2 stride-2 transposed convolution is four 1x1 launches with a scattered store (osc = 2: one output parity each).
//
// `General.amp: false` training: the data gradient is this kernel on dy with re-packed weights (a 3x3 stride-2 layer as four
// output-parity classes, 1x1 and 2x2 stride-1 products stored scattered), the weight gradient a kernel of its own below
// (conv_f32_wgrad_kernel: per-chunk partials in a workspace slab, added in a fixed order -- deterministic, no atomics).
//
// Roofline: MFMA-bound on paper (dense fp32 matrix peak 157 TFLOP/s, MI355X_MICROARCH.md); algorithmic HBM bytes = input + output
// activations once (fp32) + weights. Measured figures: DESIGN.md section 4.2c'.

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int F_TH = 8, F_TW = 32, F_THREADS = 256;

// X: [N][Cin][H][W]; Wp: [Cin][K*K][CoutW] (packed by the caller: output channel innermost); Y: [N][CoutY][Hy][Wy] written at
// (oy * osc + ooy, ox * osc + oox) for oy < Ho, ox < Wo (Hy = Ho * osc except for the parity classes of a stride-2 data gradient on odd sizes). out(co, oy, ox) = bias[co] + sum_{ci, r, s} X(ci, oy * S + r - pad, ox * S + s - pad) * Wp[ci][r * K + s][co].
template <int K, int S, int MB, bool TR = false>
__global__ void __launch_bounds__(F_THREADS)
conv_f32_kernel(const float *__restrict__ X, const float *__restrict__ Wp, const float *__restrict__ bias, float *__restrict__ Y,
                int Cin, int H, int W, int Cout, int CoutW, int Ho, int Wo, int pad, int tiles_x, int osc, int ooy, int oox, int Hy, int Wy,
                const float *__restrict__ zero) {
    // input channels per slice (stride 2: the halo tile is 4x the output tile, half the depth keeps the prefetch in registers; the 4x4 and 7x7
    // layers of the GAN networks, round 6: 16 / 49 taps per channel -- 4 / 2 channels keep the weight slice at 16 / 25 KB of LDS)
    constexpr int KC = K >= 7 ? 2 : ((S == 2 || K >= 4) ? 4 : 8);
    constexpr int IH = (F_TH - 1) * S + K, IW = (F_TW - 1) * S + K;
    constexpr int IWP = IW | 1;                          // odd row pitch: the two half-waves (channels ci, ci + 1) start on different banks
    constexpr int BM = 32 * MB, KK = K * K;
    constexpr int IN_FLOATS = KC * IH * IWP, W_FLOATS = KC * KK * BM;
    __shared__ float s_in[IN_FLOATS];
    __shared__ float s_w[W_FLOATS];
    static_assert(!TR || (K == 1 && S == 1 && MB == 2), "the fused 2x2 transposed convolution is a 1x1 product with two M-blocks");
    // TR: one launch of a 2x2 stride-2 transposed convolution. blockIdx.y = (block of 32 output channels, output row parity ta);
    // M-block mb holds the SAME 32 channels for output column parity mb, so a lane owns both pixels of an output pair (8-byte stores).
    const int tile = blockIdx.x, n = blockIdx.z, co0 = TR ? (blockIdx.y >> 1) * 32 : blockIdx.y * BM, ta = TR ? (blockIdx.y & 1) : 0;
    const int ty0 = (tile / tiles_x) * F_TH, tx0 = (tile % tiles_x) * F_TW;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = lane & 31, kg = lane >> 5;
    const int iy0 = ty0 * S - pad, ix0 = tx0 * S - pad;
    const float *img = X + (size_t)n * Cin * H * W;

    f32x16 acc[2][MB];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < MB; b++)
#pragma unroll
            for (int k = 0; k < 16; k++) acc[a][b][k] = 0.f;

    // A slice is fetched into REGISTERS one slice ahead (all loads of a thread issued back to back, nothing waits on them until the
    // MFMAs of the current slice have been issued) and written to LDS after the compute: the first version loaded and stored element
    // by element in a loop, ~20 dependent global-load latencies per slice against ~2 us of MFMA work.
    constexpr int NIN = (KC * IH * IW + F_THREADS - 1) / F_THREADS, NW = (W_FLOATS + F_THREADS - 1) / F_THREADS;
    float pin[NIN], pw[NW];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int j = 0; j < NIN; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            const int c = i / (IH * IW), rem = i % (IH * IW), hy = rem / IW, hx = rem % IW;
            const int ci = c0 + c, yy = iy0 + hy, xx = ix0 + hx;
            const bool ok = i < KC * IH * IW && ci < Cin && yy >= 0 && yy < H && xx >= 0 && xx < W;
            pin[j] = *(ok ? img + ((ci * H + yy) * W + xx) : zero);   // padding reads a zero word: the predicate dies before the load is issued (Cin * H * W < 2^31: entry point)
        }
#pragma unroll
        for (int j = 0; j < NW; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            const int row = i / BM, mm = i % BM;                      // row = channel of the slice * K*K + tap (BM is a power of two)
            const int col = TR ? co0 + (mm & 31) : co0 + mm;           // TR: Wp is [Cin][tap 2 ta + mb][Cout]
            const bool ok = i < W_FLOATS && row < (Cin - c0) * KK && col < Cout;
            pw[j] = *(ok ? Wp + ((size_t)(c0 * KK + row) * CoutW + (TR ? (2 * ta + (mm >> 5)) * Cout : 0) + col) : zero);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < NIN; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            const int c = i / (IH * IW), rem = i % (IH * IW), hy = rem / IW, hx = rem % IW;
            if (i < KC * IH * IW) s_in[(c * IH + hy) * IWP + hx] = pin[j];
        }
#pragma unroll
        for (int j = 0; j < NW; j++)
            if (W_FLOATS % F_THREADS == 0 || threadIdx.x + j * F_THREADS < W_FLOATS) s_w[threadIdx.x + j * F_THREADS] = pw[j];
    };

    fetch(0);
    for (int c0 = 0; c0 < Cin; c0 += KC) {
        stash();
        __syncthreads();
        if (c0 + KC < Cin) fetch(c0 + KC);
#pragma unroll
        for (int cp = 0; cp < KC; cp += 2) {
            const int c = cp + kg;                        // this lane's input channel of the pair
#pragma unroll
            for (int r = 0; r < K; r++)
#pragma unroll
                for (int s = 0; s < K; s++) {
                    float a[MB], b[2];
#pragma unroll
                    for (int mb = 0; mb < MB; mb++) a[mb] = s_w[(c * KK + r * K + s) * BM + mb * 32 + m];
#pragma unroll
                    for (int rr = 0; rr < 2; rr++) b[rr] = s_in[(c * IH + (2 * wv + rr) * S + r) * IWP + m * S + s];
#pragma unroll
                    for (int rr = 0; rr < 2; rr++)
#pragma unroll
                        for (int mb = 0; mb < MB; mb++)
                            acc[rr][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb], b[rr], acc[rr][mb], 0, 0, 0);
                }
        }
        __syncthreads();                                  // the slice has been consumed
    }
    // D[co][pixel]: register k of lane (m, kg) holds output channel (k & 3) + 8 * (k >> 2) + 4 * kg of the M-block, pixel column m
    const int ox = tx0 + m;
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        const int oy = ty0 + 2 * wv + rr;
        if (oy >= Ho || ox >= Wo) continue;
        if constexpr (TR) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int co = co0 + (k & 3) + 8 * (k >> 2) + 4 * kg;
                if (co < Cout)
                    *reinterpret_cast<float2 *>(Y + (((size_t)n * Cout + co) * Hy + (oy * 2 + ta)) * Wy + ox * 2) = make_float2(acc[rr][0][k], acc[rr][1][k]);
            }
            continue;
        }
#pragma unroll
        for (int mb = 0; mb < MB; mb++)
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int co = co0 + mb * 32 + (k & 3) + 8 * (k >> 2) + 4 * kg;
                if (co < Cout) {
                    const float v = acc[rr][mb][k] + (bias ? bias[co] : 0.f);
                    Y[(((size_t)n * Cout + co) * Hy + (oy * osc + ooy)) * Wy + ox * osc + oox] = v;
                }
            }
    }
}

template <int K, int S, int MB, bool TR = false>
int launch_f32(const float *zero, const float *X, const float *Wp, const float *bias, float *Y, int N, int Cin, int H, int W, int Cout, int CoutW, int Ho, int Wo, int pad,
               int osc, int ooy, int oox, int Hy, int Wy, hipStream_t stream) {
    const int tiles_x = (Wo + F_TW - 1) / F_TW, tiles_y = (Ho + F_TH - 1) / F_TH;
    dim3 grid((unsigned)(tiles_x * tiles_y), TR ? (unsigned)(2 * ((Cout + 31) / 32)) : (unsigned)((Cout + 32 * MB - 1) / (32 * MB)), (unsigned)N);
    hipLaunchKernelGGL((conv_f32_kernel<K, S, MB, TR>), grid, dim3(F_THREADS), 0, stream, X, Wp, bias, Y, Cin, H, W, Cout, CoutW, Ho, Wo, pad, tiles_x, osc, ooy, oox, Hy, Wy, zero);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

// what the padding lanes of a slice fetch read
const float *zero_word(octa_ctx *ctx) { return static_cast<const float *>(ctx->zeros("conv_f32")); }

// Picks the workgroup width and the (K, stride) instance. The gradient entry points launch the same kernel: the data gradient of
// a stride-1 layer is a forward product of dy with re-packed weights, the transposed layers' and the parity classes' of a stride-2 layer
// are the 2x2 instances.
int dispatch_f32(octa_ctx *ctx, const float *zero, const float *d_x, const float *d_wp, const float *d_bias, float *d_y, int N, int Cin, int H, int W,
                 int Cout, int cout_w, int K, int stride, int pad, int Ho, int Wo, int osc, int ooy, int oox, int Hy, int Wy, hipStream_t stream, const char *who) {
    // 64 output channels per workgroup halve the input staging per product, but the workgroups of a launch are all resident at once
    // and share the CUs' matrix pipes: 380 workgroups on 256 CUs run at the pace of the CUs that hold two (74 %), 760 of half the
    // size at 99 %. Take the narrow variant when it balances the CUs better by more than its extra staging costs.
    auto balance = [&](int mb) {
        const long wgs = (long)((Wo + F_TW - 1) / F_TW) * ((Ho + F_TH - 1) / F_TH) * ((Cout + 32 * mb - 1) / (32 * mb)) * N;
        const long cus = ctx->num_cus > 0 ? ctx->num_cus : 256;
        return (double)wgs / (double)(cus * ((wgs + cus - 1) / cus));
    };
    const bool wide = Cout > 32 && (stride != 1 || balance(2) >= 0.9 * balance(1));     // stride 2 (half-depth slices) measured slower when narrow
#define OCTA_F32_CASE(KK_, SS_)                                                                                                              \
    if (K == KK_ && stride == SS_)                                                                                                           \
        return wide ? launch_f32<KK_, SS_, 2>(zero, d_x, d_wp, d_bias, d_y, N, Cin, H, W, Cout, cout_w, Ho, Wo, pad, osc, ooy, oox, Hy, Wy, stream)       \
                    : launch_f32<KK_, SS_, 1>(zero, d_x, d_wp, d_bias, d_y, N, Cin, H, W, Cout, cout_w, Ho, Wo, pad, osc, ooy, oox, Hy, Wy, stream);
    OCTA_F32_CASE(1, 1)
    OCTA_F32_CASE(3, 1)
    OCTA_F32_CASE(3, 2)
    OCTA_F32_CASE(4, 1)          // PatchGAN (models/networks.py:445-506: 4x4, stride 1, padding 1)
    OCTA_F32_CASE(7, 1)          // the generator's stem and head (models/networks.py:404-421: 7x7 behind ReflectionPad2d(3))
    OCTA_F32_CASE(2, 1)          // data gradient of a 3x3 stride-2 layer: the parity classes with two taps per axis
    OCTA_F32_CASE(2, 2)          // data gradient of a 2x2 stride-2 transposed convolution
#undef OCTA_F32_CASE
    octa::set_error("%s: kernel size %d with stride %d is not instantiated (1/1, 3/1, 3/2, 4/1, 7/1, 2/1, 2/2)", who, K, stride);
    return -2;
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------
// dW[co][ci][r * K + s] = sum_{n, oy, ox} DY[n][co][oy][ox] * X[n][ci][oy * S + r - pad][ox * S + s - pad]: a GEMM with M = Cout,
// N = Cin * K^2 and the reduction over every output pixel of the batch. A workgroup owns 32 output x 32 input channels (all taps) and
// the pixel tiles t = chunk, chunk + nchunks, ... of the batch (tiles of TH x 32 output pixels); a wave owns a quarter of a
// tile's pixel pairs and keeps one 32x32 accumulator fragment per tap. An MFMA consumes two pixels: lane (m, kg) supplies
// DY[co = m][pixel kg] (A) and X[ci = m][pixel kg shifted by the tap] (B), both one conflict-free ds_read_b32 from channel-innermost
// LDS tiles (pitch 33). At the end the four waves add their fragments in the order 0, 1, 2, 3 through the LDS and the workgroup
// stores its partial [tap][32 co][32 ci] to the slab; wgrad_fold adds the chunks' partials in chunk order. No atomics: the bits depend
// on the shapes only (the chunk count is a function of the shape, not of the device).
constexpr int G_TW = 32, G_CP = 33, G_TARGET_WGS = 1024, DB_CHUNKS = 64;

template <int K, int S> struct wgrad_geom {
    static constexpr int TH = S == 1 ? 8 : 2;           // stride 2: the halo tile is twice as wide; 4 rows spilled the prefetch registers
    static constexpr int IH = (TH - 1) * S + K, IW = (G_TW - 1) * S + K, KK = K * K;
    static constexpr int X_FLOATS = IH * IW * G_CP, D_FLOATS = TH * G_TW * G_CP;
    static_assert(KK * 1024 <= X_FLOATS + D_FLOATS, "the wave fold reuses the staging LDS");
};

template <int K, int S>
__global__ void __launch_bounds__(F_THREADS)
conv_f32_wgrad_kernel(const float *__restrict__ X, const float *__restrict__ DY, float *__restrict__ slab, int Cin, int H, int W, int Cout, int Ho,
                      int Wo, int pad, int tiles_x, int tiles_per_img, int total_tiles, int nchunks, int ci_blocks, const float *__restrict__ zero) {
    using G = wgrad_geom<K, S>;
    constexpr int TH = G::TH, IH = G::IH, IW = G::IW, KK = G::KK;
    __shared__ float s_mem[G::X_FLOATS + G::D_FLOATS];
    float *s_x = s_mem, *s_d = s_mem + G::X_FLOATS;       // s_x[(hy * IW + hx) * 33 + ci], s_d[pixel * 33 + co]
    const int chunk = blockIdx.x, cib = blockIdx.y % ci_blocks, cob = blockIdx.y / ci_blocks;
    const int ci0 = cib * 32, co0 = cob * 32;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int m = lane & 31, kg = lane >> 5;

    f32x16 acc[KK];
#pragma unroll
    for (int t = 0; t < KK; t++)
#pragma unroll
        for (int k = 0; k < 16; k++) acc[t][k] = 0.f;

    constexpr int NX = (32 * IH * IW + F_THREADS - 1) / F_THREADS, ND = 32 * TH * G_TW / F_THREADS;
    float px[NX], pd[ND];
    auto fetch = [&](int t) {
        const int n = t / tiles_per_img, rem = t % tiles_per_img;
        const int ty0 = (rem / tiles_x) * TH, tx0 = (rem % tiles_x) * G_TW;
        const int iy0 = ty0 * S - pad, ix0 = tx0 * S - pad;
        const float *xi = X + (size_t)n * Cin * H * W, *di = DY + (size_t)n * Cout * Ho * Wo;
#pragma unroll
        for (int j = 0; j < NX; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            const int c = i / (IH * IW), r = i % (IH * IW), hy = r / IW, hx = r % IW;
            const int ci = ci0 + c, yy = iy0 + hy, xx = ix0 + hx;
            const bool ok = i < 32 * IH * IW && ci < Cin && yy >= 0 && yy < H && xx >= 0 && xx < W;
            px[j] = *(ok ? xi + ((ci * H + yy) * W + xx) : zero);   // Cin * H * W < 2^31: entry point
        }
#pragma unroll
        for (int j = 0; j < ND; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            const int c = i / (TH * G_TW), p = i % (TH * G_TW);
            const int co = co0 + c, oy = ty0 + p / G_TW, ox = tx0 + p % G_TW;
            const bool ok = co < Cout && oy < Ho && ox < Wo;           // pixels beyond the map contribute dy = 0 (and x = 0: no 0 * NaN)
            pd[j] = *(ok ? di + ((co * Ho + oy) * Wo + ox) : zero);
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int j = 0; j < NX; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            const int c = i / (IH * IW), r = i % (IH * IW);
            if (i < 32 * IH * IW) s_x[r * G_CP + c] = px[j];
        }
#pragma unroll
        for (int j = 0; j < ND; j++) {
            const int i = threadIdx.x + j * F_THREADS;
            s_d[(i % (TH * G_TW)) * G_CP + i / (TH * G_TW)] = pd[j];
        }
    };

    if (chunk < total_tiles) fetch(chunk);
    for (int t = chunk; t < total_tiles; t += nchunks) {
        stash();
        __syncthreads();
        if (t + nchunks < total_tiles) fetch(t + nchunks);
        constexpr int PPW = TH * G_TW / 8;                                  // pixel pairs per wave
#pragma unroll 4
        for (int qq = wv * PPW; qq < (wv + 1) * PPW; qq++) {
                const int rr = qq / (G_TW / 2), p = 2 * (qq % (G_TW / 2)) + kg;   // this lane's pixel of the pair
                const float a = s_d[(rr * G_TW + p) * G_CP + m];
#pragma unroll
                for (int r = 0; r < K; r++)
#pragma unroll
                    for (int s = 0; s < K; s++) {
                        const float b = s_x[((rr * S + r) * IW + p * S + s) * G_CP + m];
                        acc[r * K + s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[r * K + s], 0, 0, 0);
                    }
            }
        __syncthreads();                                                    // the tile has been consumed
    }
    // register k of lane (m, kg): output channel co0 + (k & 3) + 8 * (k >> 2) + 4 * kg, input channel ci0 + m
    float *red = s_mem;
    float *out = slab + ((size_t)chunk * gridDim.y + blockIdx.y) * KK * 1024;
    for (int w = 0; w < 4; w++) {
        if (wv == w) {
#pragma unroll
            for (int t = 0; t < KK; t++)
#pragma unroll
                for (int k = 0; k < 16; k++) {
                    const int idx = (t * 32 + (k & 3) + 8 * (k >> 2) + 4 * kg) * 32 + m;
                    const float v = w == 0 ? acc[t][k] : red[idx] + acc[t][k];
                    if (w == 3) out[idx] = v;
                    else red[idx] = v;
                }
        }
        if (w < 3) __syncthreads();
    }
}

// dW (layout [Cout][Cin][K*K]) = the chunks' partials added in chunk order; one thread per slab entry of a chunk (coalesced reads).
__global__ void __launch_bounds__(256)
conv_f32_wgrad_fold(const float *__restrict__ slab, float *__restrict__ dw, int Cin, int Cout, int KK, int nchunks, int ci_blocks, int per_chunk) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= per_chunk) return;
    const int blk = i / (KK * 1024), r = i % (KK * 1024), tap = r / 1024, col = (r % 1024) / 32, ci = (blk % ci_blocks) * 32 + r % 32;
    const int co = (blk / ci_blocks) * 32 + col;
    if (co >= Cout || ci >= Cin) return;
    float s = 0.f;
    for (int c = 0; c < nchunks; c++) s += slab[(size_t)c * per_chunk + i];
    dw[((size_t)co * Cin + ci) * KK + tap] = s;
}

// Bias gradient, db[co] = sum of DY[n][co][:][:]: workgroup (co, chunk) adds a fixed contiguous range of the channel's pixels (per
// thread in order, then a fixed tree), conv_f32_bias_fold adds the DB_CHUNKS partials in order.
__global__ void __launch_bounds__(256)
conv_f32_bias_partial(const float *__restrict__ DY, float *__restrict__ part, int N, int Cout, int HW) {
    const int co = blockIdx.x, chunk = blockIdx.y;
    const long total = (long)N * HW, per = (total + DB_CHUNKS - 1) / DB_CHUNKS;
    const long b = chunk * per, e = b + per < total ? b + per : total;
    float s = 0.f;
    for (long i = b + threadIdx.x; i < e; i += 256) {
        const long n = i / HW, p = i % HW;
        s += DY[((size_t)n * Cout + co) * HW + p];
    }
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[co * DB_CHUNKS + chunk] = red[0];
}

__global__ void conv_f32_bias_fold(const float *__restrict__ part, float *__restrict__ db, int Cout) {
    const int co = blockIdx.x * 256 + threadIdx.x;
    if (co >= Cout) return;
    float s = 0.f;
    for (int c = 0; c < DB_CHUNKS; c++) s += part[co * DB_CHUNKS + c];
    db[co] = s;
}

struct wgrad_plan {
    int tiles_x, tiles_per_img, total_tiles, ci_blocks, co_blocks, nchunks;
    size_t slab_floats, bytes;
};

// The workspace depends on the shapes only: the chunk count aims at G_TARGET_WGS workgroups per launch.
wgrad_plan plan_wgrad(int N, int Cin, int Cout, int K, int stride, int Ho, int Wo) {
    wgrad_plan p;
    const int th = stride == 1 ? wgrad_geom<3, 1>::TH : wgrad_geom<3, 2>::TH;
    p.tiles_x = (Wo + G_TW - 1) / G_TW;
    p.tiles_per_img = p.tiles_x * ((Ho + th - 1) / th);
    p.total_tiles = p.tiles_per_img * N;
    p.ci_blocks = (Cin + 31) / 32;
    p.co_blocks = (Cout + 31) / 32;
    const int blocks = p.ci_blocks * p.co_blocks;
    p.nchunks = (G_TARGET_WGS + blocks - 1) / blocks;
    if (p.nchunks > p.total_tiles) p.nchunks = p.total_tiles;
    p.slab_floats = (size_t)p.nchunks * blocks * K * K * 1024;
    p.bytes = (p.slab_floats + (size_t)Cout * DB_CHUNKS) * sizeof(float);
    return p;
}

template <int K, int S>
int launch_wgrad(const wgrad_plan &p, const float *zero, const float *X, const float *DY, float *slab, float *dw, int N, int Cin, int H, int W,
                 int Cout, int Ho, int Wo, int pad, hipStream_t stream) {
    dim3 grid((unsigned)p.nchunks, (unsigned)(p.ci_blocks * p.co_blocks));
    hipLaunchKernelGGL((conv_f32_wgrad_kernel<K, S>), grid, dim3(F_THREADS), 0, stream, X, DY, slab, Cin, H, W, Cout, Ho, Wo, pad, p.tiles_x,
                       p.tiles_per_img, p.total_tiles, p.nchunks, p.ci_blocks, zero);
    OCTA_HIP_CHECK(hipGetLastError());
    const int per_chunk = p.ci_blocks * p.co_blocks * K * K * 1024;
    hipLaunchKernelGGL(conv_f32_wgrad_fold, dim3((unsigned)((per_chunk + 255) / 256)), dim3(256), 0, stream, slab, dw, Cin, Cout, K * K, p.nchunks,
                       p.ci_blocks, per_chunk);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

// Single-precision convolution, NCHW (see the file header). d_wp: weights packed as [Cin][K*K][cout_w] with cout_w >= Cout (a
// view of a larger packed tensor may be passed: rows are cout_w apart); d_bias: [Cout] or NULL. K / stride in {1/1, 3/1, 3/2, 4/1, 7/1}.
// The output tensor is [N][Cout][Ho * osc][Wo * osc]; osc = 1 writes it densely, osc = 2 writes the pixels of
// parity (ooy, oox) only (one of the four 1x1 products of a 2x2 stride-2 transposed convolution).
extern "C" int octa_conv2d_f32_nchw(octa_ctx *ctx, const float *d_x, const float *d_wp, const float *d_bias, float *d_y, int N, int Cin, int H, int W,
                                    int Cout, int cout_w, int K, int stride, int pad, int Ho, int Wo, int osc, int ooy, int oox, void *stream_) {
    if (!ctx || !d_x || !d_wp || !d_y || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || cout_w < Cout || Ho <= 0 || Wo <= 0 || pad < 0) {
        octa::set_error("octa_conv2d_f32_nchw: bad arguments");
        return -2;
    }
    if ((osc != 1 && osc != 2) || ooy < 0 || ooy >= osc || oox < 0 || oox >= osc) { octa::set_error("octa_conv2d_f32_nchw: bad output scatter"); return -2; }
    if ((long)(Ho - 1) * stride + K - pad > (long)H + pad || (long)(Wo - 1) * stride + K - pad > (long)W + pad) {
        octa::set_error("octa_conv2d_f32_nchw: output size %dx%d reads beyond the padded input", Ho, Wo);
        return -2;
    }
    if ((long)Cin * H * W >= (1L << 31)) { octa::set_error("octa_conv2d_f32_nchw: one image of the input exceeds 2^31 elements"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const float *zero = zero_word(ctx);
    if (!zero) return -1;
    return dispatch_f32(ctx, zero, d_x, d_wp, d_bias, d_y, N, Cin, H, W, Cout, cout_w, K, stride, pad, Ho, Wo, osc, ooy, oox, Ho * osc, Wo * osc, stream,
                        "octa_conv2d_f32_nchw");
}

// 2x2 stride-2 transposed convolution (torch.nn.ConvTranspose2d(Cin, Cout, 2, 2, bias=False): DynUNet's upsampling, MONAI
// UnetUpBlock.transp_conv) in ONE launch: d_wp = the weights packed [Cin][4][Cout] (tap 2 a + b, output channel innermost),
// d_y [N][Cout][2H][2W], y(co, 2 y + a, 2 x + b) = sum_ci x(ci, y, x) w(ci, co, a, b). Four 1x1 launches of octa_conv2d_f32_nchw with
// osc = 2 give the same numbers (same products, same summation order) with 4-byte stores two pixels apart.
extern "C" int octa_convtranspose2x2_f32_nchw(octa_ctx *ctx, const float *d_x, const float *d_wp, float *d_y, int N, int Cin, int H, int W, int Cout, void *stream_) {
    if (!ctx || !d_x || !d_wp || !d_y || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) { octa::set_error("octa_convtranspose2x2_f32_nchw: bad arguments"); return -2; }
    if ((long)Cin * H * W >= (1L << 31)) { octa::set_error("octa_convtranspose2x2_f32_nchw: one image of the input exceeds 2^31 elements"); return -2; }
    if (((uintptr_t)d_y & 7) != 0) { octa::set_error("octa_convtranspose2x2_f32_nchw: the output must be 8-byte aligned"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const float *zero = zero_word(ctx);
    if (!zero) return -1;
    return launch_f32<1, 1, 2, true>(zero, d_x, d_wp, nullptr, d_y, N, Cin, H, W, Cout, 4 * Cout, H, W, 0, 2, 0, 0, 2 * H, 2 * W, stream);
}

// ---- gradients of the fp32 layers (General.amp: false training) -----------------------------------------------------------------
// Layer geometry as in the forward pass: x [N][Cin][H][W], dy [N][Cout][Ho][Wo] (transposed layers: Ho = K H). d_wd: the weights in the
// data-gradient layout, packed by the caller (models/conv_f32.py _dgrad_layout), output = input channel of the layer innermost:
//   Conv2d, stride 1 (1x1 pad 0, 3x3 pad 1):  [Cout][K*K][Cin], taps flipped: wd[co][r K + s][ci] = w[co][ci][K-1-r][K-1-s]
//                                             (dx = the forward kernel on dy with padding K - 1 - pad);
//   Conv2d 3x3 stride 2 pad 1:                [4 parities a b][Cout][4 taps t u][Cin]: dx(2i + a, 2j + b) = sum over t, u in {0, 1} of
//                                             dy(i + t, j + u) wd[2a + b][co][2t + u][ci], wd = w[co][ci][R(a, t)][R(b, u)] with
//                                             R(0, 0) = 1, R(1, 0) = 2, R(1, 1) = 0 and a zero tap for (0, 1). Parity (0, 0) has one
//                                             tap and runs as a 1x1 product (tap slot 0); the other three as 2x2 products, stored
//                                             scattered (osc = 2). dy is never zero-inserted;
//   ConvTranspose2d k = stride in {1, 2}:     [Cout][k*k][Cin], wd[co][2a + b][ci] = w[ci][co][a][b] (dx = a k x k stride-k pad-0
//                                             convolution of dy).
extern "C" int octa_conv2d_f32_dgrad_nchw(octa_ctx *ctx, const float *d_dy, const float *d_wd, float *d_dx, int N, int Cin, int H, int W, int Cout,
                                          int K, int stride, int pad, int Ho, int Wo, int transposed, void *stream_) {
    if (!ctx || !d_dy || !d_wd || !d_dx || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || pad < 0) {
        octa::set_error("octa_conv2d_f32_dgrad_nchw: bad arguments");
        return -2;
    }
    const bool conv_ok = !transposed && ((K == 1 && stride == 1 && pad == 0) || (K == 3 && stride == 1 && pad == 1) || (K == 3 && stride == 2 && pad == 1));
    const bool tr_ok = transposed && (K == 1 || K == 2) && stride == K && pad == 0;
    if (!conv_ok && !tr_ok) {
        octa::set_error("octa_conv2d_f32_dgrad_nchw: layer k%d s%d p%d%s is not covered (Conv2d 1/1/0, 3/1/1, 3/2/1; ConvTranspose2d 1/1/0, 2/2/0)", K,
                        stride, pad, transposed ? " transposed" : "");
        return -2;
    }
    const long eho = transposed ? (long)H * K : ((long)H + 2 * pad - K) / stride + 1, ewo = transposed ? (long)W * K : ((long)W + 2 * pad - K) / stride + 1;
    if (Ho != eho || Wo != ewo) { octa::set_error("octa_conv2d_f32_dgrad_nchw: dy is %dx%d, the layer gives %ldx%ld", Ho, Wo, eho, ewo); return -2; }
    if ((long)Cout * Ho * Wo >= (1L << 31) || (long)Cin * H * W >= (1L << 31)) {
        octa::set_error("octa_conv2d_f32_dgrad_nchw: one image of dy or dx exceeds 2^31 elements");
        return -2;
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const float *zero = zero_word(ctx);
    if (!zero) return -1;
    const char *who = "octa_conv2d_f32_dgrad_nchw";
    if (transposed && K == 2)
        return dispatch_f32(ctx, zero, d_dy, d_wd, nullptr, d_dx, N, Cout, Ho, Wo, Cin, Cin, 2, 2, 0, H, W, 1, 0, 0, H, W, stream, who);
    if (stride == 1)
        return dispatch_f32(ctx, zero, d_dy, d_wd, nullptr, d_dx, N, Cout, Ho, Wo, Cin, Cin, K, 1, K - 1 - pad, H, W, 1, 0, 0, H, W, stream, who);
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const int hp = (H - a + 1) / 2, wp = (W - b + 1) / 2, kp = (a | b) ? 2 : 1;
            if (hp <= 0 || wp <= 0) continue;                               // a map one pixel high / wide has no odd rows / columns
            const int rc = dispatch_f32(ctx, zero, d_dy, d_wd + (size_t)(2 * a + b) * Cout * 4 * Cin, nullptr, d_dx, N, Cout, Ho, Wo, Cin,
                                        kp == 1 ? 4 * Cin : Cin, kp, 1, 0, hp, wp, 2, a, b, H, W, stream, who);
            if (rc) return rc;
        }
    return 0;
}

// Bytes of the workspace octa_conv2d_f32_wgrad_nchw needs for this shape (the caller allocates it: a torch tensor in the binding).
extern "C" int octa_conv2d_f32_wgrad_workspace(int N, int Cin, int H, int W, int Cout, int K, int stride, int pad, int Ho, int Wo, size_t *bytes) {
    if (!bytes || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || pad < 0 || K <= 0 || stride <= 0) {
        octa::set_error("octa_conv2d_f32_wgrad_workspace: bad arguments");
        return -2;
    }
    *bytes = plan_wgrad(N, Cin, Cout, K, stride, Ho, Wo).bytes;
    return 0;
}

// Weight (and bias) gradient: d_dw [Cout][Cin][K][K] = sum_{n, oy, ox} dy[n][co][oy][ox] x[n][ci][oy stride + r - pad][ox stride + s - pad]
// (overwritten), d_db [Cout] = sum of dy (overwritten; NULL: not computed). x [N][Cin][H][W], dy [N][Cout][Ho][Wo]. K / stride in
// {1/1, 3/1, 3/2, 2/2}; a transposed layer passes its dy as x and its x as dy (d_dw is then its [Cin][Cout][k][k] weight). d_ws: at
// least octa_conv2d_f32_wgrad_workspace bytes. Deterministic: partial sums over pixel chunks meet in a slab and are added in a fixed
// order, never with atomics.
extern "C" int octa_conv2d_f32_wgrad_nchw(octa_ctx *ctx, const float *d_x, const float *d_dy, float *d_dw, float *d_db, void *d_ws, size_t ws_bytes,
                                          int N, int Cin, int H, int W, int Cout, int K, int stride, int pad, int Ho, int Wo, void *stream_) {
    if (!ctx || !d_x || !d_dy || !d_dw || !d_ws || N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0 || Ho <= 0 || Wo <= 0 || pad < 0 || pad >= K) {
        octa::set_error("octa_conv2d_f32_wgrad_nchw: bad arguments");
        return -2;
    }
    if ((long)(Ho - 1) * stride + K - pad > (long)H + pad || (long)(Wo - 1) * stride + K - pad > (long)W + pad) {
        octa::set_error("octa_conv2d_f32_wgrad_nchw: output size %dx%d reads beyond the padded input", Ho, Wo);
        return -2;
    }
    if ((long)Cin * H * W >= (1L << 31) || (long)Cout * Ho * Wo >= (1L << 31)) {
        octa::set_error("octa_conv2d_f32_wgrad_nchw: one image of x or dy exceeds 2^31 elements");
        return -2;
    }
    const wgrad_plan p = plan_wgrad(N, Cin, Cout, K, stride, Ho, Wo);
    if (ws_bytes < p.bytes) { octa::set_error("octa_conv2d_f32_wgrad_nchw: workspace of %zu bytes, %zu needed", ws_bytes, p.bytes); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const float *zero = zero_word(ctx);
    if (!zero) return -1;
    float *slab = (float *)d_ws;
    int rc = -3;
    if (K == 1 && stride == 1) rc = launch_wgrad<1, 1>(p, zero, d_x, d_dy, slab, d_dw, N, Cin, H, W, Cout, Ho, Wo, pad, stream);
    else if (K == 3 && stride == 1) rc = launch_wgrad<3, 1>(p, zero, d_x, d_dy, slab, d_dw, N, Cin, H, W, Cout, Ho, Wo, pad, stream);
    else if (K == 3 && stride == 2) rc = launch_wgrad<3, 2>(p, zero, d_x, d_dy, slab, d_dw, N, Cin, H, W, Cout, Ho, Wo, pad, stream);
    else if (K == 2 && stride == 2) rc = launch_wgrad<2, 2>(p, zero, d_x, d_dy, slab, d_dw, N, Cin, H, W, Cout, Ho, Wo, pad, stream);
    if (rc == -3) {
        octa::set_error("octa_conv2d_f32_wgrad_nchw: kernel size %d with stride %d is not instantiated (1/1, 3/1, 3/2, 2/2)", K, stride);
        return -2;
    }
    if (rc || !d_db) return rc;
    float *part = slab + p.slab_floats;
    hipLaunchKernelGGL(conv_f32_bias_partial, dim3((unsigned)Cout, DB_CHUNKS), dim3(256), 0, stream, d_dy, part, N, Cout, Ho * Wo);
    OCTA_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(conv_f32_bias_fold, dim3((unsigned)((Cout + 255) / 256)), dim3(256), 0, stream, part, d_db, Cout);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
