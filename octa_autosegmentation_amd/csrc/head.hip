// head.hip -- 1x1 convolution head to N output channels (UnetOutBlock with out_channels > 1) on the matrix cores.
//
//   forward   y[n][o][q]  = bias[o] + sum_c x[n][q][c] w[o][c]          x NHWC bf16, y CHANNEL-FIRST bf16
//   backward  dx[n][q][c] = sum_o dy[n][o][q] w[o][c]                   dy channel-first bf16, dx NHWC bf16
//             dw[o][c]    = sum_{n,q} dy[n][o][q] x[n][q][c]            float32
//             db[o]       = sum_{n,q} dy[n][o][q]                       float32
//
// Everything after the head is channel-first (the loss's per-(sample, channel) rows, sigmoid, per-channel small-object removal), so the
// kernels write / read [N][Cout][hw] directly: an output tile is transposed through LDS and leaves as whole pixel runs per channel.
//
// A workgroup (4 waves) takes tiles of HEAD_TP = 256 consecutive pixels of the flat [N*hw] pixel axis; a tile may straddle images and
// hw may be odd, so a channel row of a tile is moved in groups of four pixels: one 8-byte access when the four pixels lie in one image
// and the address is 8-byte aligned (always the case when hw % 4 == 0), one 4-byte access per pair when it is 4-byte aligned, else
// element by element. Cout is padded to a multiple of 16 (forward) / 32 (the backward's K) with zero weights; padding is never stored.
//
// v_mfma_f32_16x16x32_bf16 lane maps (lane l, g = l >> 4, r = l & 15): A[row r][k = 8g + j], B[k = 8g + j][col r], j = 0..7;
// D[row = 4g + reg][col = r].
//   forward:  A = x (row = pixel: one 16-byte global load per lane), B = w (col = channel), D: a lane holds 4 consecutive pixels of
//             one channel -> one 8-byte LDS write into the [channel][pixel] tile.
//   dx:       A = w^T (row = input channel), B = dy (k = output channel, col = pixel: 2-byte LDS reads of the staged [o][pixel]
//             tile), D: a lane holds 4 consecutive input channels of one pixel -> 8-byte global stores, 1 KB contiguous per wave.
//   dw:       A = dy (row = o, k = pixel: 16-byte LDS reads), B = x^T (k = pixel, col = c: 16-byte reads of an LDS tile written
//             transposed while staging), accumulated in registers over all tiles of the workgroup. db rides along as the same
//             product with a B operand of ones.
// dw / db: per-workgroup partials (waves summed in LDS in wave order) go to context scratch and a second kernel adds them in a fixed
// order -- no float atomics, two runs are bit-identical.
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short frag_ab;
typedef __attribute__((ext_vector_type(4))) float frag_cd;

constexpr int HEAD_TP = 256;              // pixels per tile
constexpr int HEAD_LD = HEAD_TP + 8;      // LDS row stride in elements (528 bytes: 16-byte aligned rows)
constexpr int HEAD_RED_SPLIT = 16;        // partial sums per output element in the reduction kernel

__device__ __forceinline__ unsigned head_pack(float lo, float hi) { return octa_pack_bf16x2(lo, hi); }

// where the four pixels 4 * lane .. + 3 of the tile that starts at flat pixel p0 live
struct HeadGroup {
    int n, q;          // image and pixel-in-image of the group's first pixel
    int valid;         // how many of the four pixels are < npix (0..4)
    bool one_image;    // all four valid and in image n
};

__device__ __forceinline__ HeadGroup head_group(long p0, int j, long npix, int hw) {
    HeadGroup gq;
    const int p = (int)(p0 + j);                  // N * hw < 2^30 (headn_check)
    const long left = npix - p;
    gq.valid = left >= 4 ? 4 : (left > 0 ? (int)left : 0);
    gq.n = p / hw;
    gq.q = p - gq.n * hw;
    gq.one_image = gq.valid == 4 && gq.q + 3 < hw;
    return gq;
}

// element i of a group -> (image, pixel) when the group crosses an image boundary (hw may be smaller than 4)
__device__ __forceinline__ void head_step(const HeadGroup &gq, int i, int hw, int &n, int &q) {
    n = gq.n;
    q = gq.q + i;
    while (q >= hw) { q -= hw; n++; }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
template <int CIN, int NT>      // NT = padded Cout / 16
__global__ void __launch_bounds__(256)
headn_fwd_kernel(const unsigned short *__restrict__ x, const float *__restrict__ w, const float *__restrict__ bias, long npix, int hw,
                 int Cout, unsigned short *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) unsigned short s_out[];      // [NT * 16][HEAD_LD]
    constexpr int KS = CIN / 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;

    // B fragments: w[o = 16 nt + r][c = 32 ks + 8 g + j], rounded to bf16; zero columns for the channel padding
    frag_ab bw[NT][KS];
    float bv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) {
        const int o = nt * 16 + r;
        bv[nt] = (bias && o < Cout) ? bias[o] : 0.f;
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            unsigned u[4] = {0u, 0u, 0u, 0u};
            if (o < Cout) {
                const float *pw = w + (long)o * CIN + ks * 32 + g * 8;
#pragma unroll
                for (int k = 0; k < 4; k++) u[k] = head_pack(pw[2 * k], pw[2 * k + 1]);
            }
            bw[nt][ks] = __builtin_bit_cast(frag_ab, make_uint4(u[0], u[1], u[2], u[3]));
        }
    }

    const long ntiles = (npix + HEAD_TP - 1) / HEAD_TP;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long p0 = tile * HEAD_TP;
        // a wave owns 64 pixels = 4 row tiles of 16
        frag_ab a[4][KS];
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            const long p = p0 + wave * 64 + mt * 16 + r;
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (p < npix) v = *reinterpret_cast<const uint4 *>(x + p * CIN + ks * 32 + g * 8);
                a[mt][ks] = __builtin_bit_cast(frag_ab, v);
            }
        }
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
#pragma unroll
            for (int nt = 0; nt < NT; nt++) {
                frag_cd acc = {bv[nt], bv[nt], bv[nt], bv[nt]};
#pragma unroll
                for (int ks = 0; ks < KS; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[mt][ks], bw[nt][ks], acc, 0, 0, 0);
                // D[row = pixel 4g + reg][col = channel r]
                const uint2 pk = make_uint2(head_pack(acc[0], acc[1]), head_pack(acc[2], acc[3]));
                *reinterpret_cast<uint2 *>(&s_out[(nt * 16 + r) * HEAD_LD + wave * 64 + mt * 16 + g * 4]) = pk;
            }
        }
        __syncthreads();
        // channel rows out: wave w takes channels w, w + 4, ...; lane takes pixels 4 lane .. 4 lane + 3 of the tile
        const HeadGroup gq = head_group(p0, 4 * lane, npix, hw);
        for (int o = wave; o < Cout; o += 4) {
            const uint2 v = *reinterpret_cast<const uint2 *>(&s_out[o * HEAD_LD + 4 * lane]);
            if (gq.one_image) {
                unsigned short *dst = y + ((long)gq.n * Cout + o) * hw + gq.q;
                const unsigned al = (unsigned)(reinterpret_cast<uintptr_t>(dst) & 7u);
                if (al == 0) {
                    *reinterpret_cast<uint2 *>(dst) = v;
                } else if (al == 4) {
                    reinterpret_cast<unsigned *>(dst)[0] = v.x;
                    reinterpret_cast<unsigned *>(dst)[1] = v.y;
                } else {
                    dst[0] = (unsigned short)(v.x & 0xffffu);
                    dst[1] = (unsigned short)(v.x >> 16);
                    dst[2] = (unsigned short)(v.y & 0xffffu);
                    dst[3] = (unsigned short)(v.y >> 16);
                }
            } else {
                const unsigned short e[4] = {(unsigned short)(v.x & 0xffffu), (unsigned short)(v.x >> 16), (unsigned short)(v.y & 0xffffu),
                                             (unsigned short)(v.y >> 16)};
                for (int i = 0; i < gq.valid; i++) {
                    int n, q;
                    head_step(gq, i, hw, n, q);
                    y[((long)n * Cout + o) * hw + q] = e[i];
                }
            }
        }
        __syncthreads();
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// partial layout per workgroup: [KT * 32 * CIN] dw (row o, column c) then [KT * 32] db
template <int CIN, int KT>      // KT = padded Cout / 32 (K steps of dx; 2 KT row tiles of dw)
__global__ void __launch_bounds__(256)
headn_bwd_kernel(const unsigned short *__restrict__ x, const unsigned short *__restrict__ dy, const float *__restrict__ w, long npix,
                 int hw, int Cout, unsigned short *__restrict__ dx, float *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) unsigned short s_mem[];
    constexpr int KP = KT * 32, MO = KT * 2, NC = CIN / 16;
    unsigned short *s_dy = s_mem;                      // [KP][HEAD_LD]   dy tile, [o][pixel]; rows >= Cout stay zero
    unsigned short *s_xt = s_mem + KP * HEAD_LD;       // [CIN][HEAD_LD]  x tile transposed, [c][pixel]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;

    for (int i = threadIdx.x; i < KP * HEAD_LD / 2; i += 256) reinterpret_cast<unsigned *>(s_dy)[i] = 0u;

    // A fragments of dx: w^T[row c = 16 nc + r][k = o = 32 ks + 8 g + j]
    frag_ab aw[NC][KT];
#pragma unroll
    for (int nc = 0; nc < NC; nc++) {
#pragma unroll
        for (int ks = 0; ks < KT; ks++) {
            unsigned u[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int o0 = ks * 32 + g * 8 + 2 * k;
                const float lo = o0 < Cout ? w[(long)o0 * CIN + nc * 16 + r] : 0.f;
                const float hi = o0 + 1 < Cout ? w[(long)(o0 + 1) * CIN + nc * 16 + r] : 0.f;
                u[k] = head_pack(lo, hi);
            }
            aw[nc][ks] = __builtin_bit_cast(frag_ab, make_uint4(u[0], u[1], u[2], u[3]));
        }
    }
    const frag_ab ones = __builtin_bit_cast(frag_ab, make_uint4(0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u));

    frag_cd dwacc[MO][NC], dbacc[MO];
#pragma unroll
    for (int mo = 0; mo < MO; mo++) {
        dbacc[mo] = frag_cd{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int nc = 0; nc < NC; nc++) dwacc[mo][nc] = frag_cd{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();

    const long ntiles = (npix + HEAD_TP - 1) / HEAD_TP;
    for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long p0 = tile * HEAD_TP;
        // stage dy: wave w takes rows w, w + 4, ...; lane takes pixels 4 lane .. + 3 (zeros past npix)
        const HeadGroup gq = head_group(p0, 4 * lane, npix, hw);
        for (int o = wave; o < Cout; o += 4) {
            uint2 v = make_uint2(0u, 0u);
            if (gq.one_image) {
                const unsigned short *src = dy + ((long)gq.n * Cout + o) * hw + gq.q;
                const unsigned al = (unsigned)(reinterpret_cast<uintptr_t>(src) & 7u);
                if (al == 0) {
                    v = *reinterpret_cast<const uint2 *>(src);
                } else if (al == 4) {
                    v.x = reinterpret_cast<const unsigned *>(src)[0];
                    v.y = reinterpret_cast<const unsigned *>(src)[1];
                } else {
                    v.x = (unsigned)src[0] | ((unsigned)src[1] << 16);
                    v.y = (unsigned)src[2] | ((unsigned)src[3] << 16);
                }
            } else {
                unsigned e[4] = {0u, 0u, 0u, 0u};
                for (int i = 0; i < gq.valid; i++) {
                    int n, q;
                    head_step(gq, i, hw, n, q);
                    e[i] = dy[((long)n * Cout + o) * hw + q];
                }
                v.x = e[0] | (e[1] << 16);
                v.y = e[2] | (e[3] << 16);
            }
            *reinterpret_cast<uint2 *>(&s_dy[o * HEAD_LD + 4 * lane]) = v;
        }
        // stage x transposed: thread -> (pixel t / (CIN / 8) + 256 / (CIN / 8) * it, 8-channel chunk t % (CIN / 8))
        {
            constexpr int CH = CIN / 8, PPI = 256 / CH;
#pragma unroll
            for (int it = 0; it < CH; it++) {
                const int pix = it * PPI + threadIdx.x / CH, ch = threadIdx.x % CH;
                const long p = p0 + pix;
                uint4 v = make_uint4(0u, 0u, 0u, 0u);
                if (p < npix) v = *reinterpret_cast<const uint4 *>(x + p * CIN + ch * 8);
                const unsigned u[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    s_xt[(ch * 8 + 2 * k) * HEAD_LD + pix] = (unsigned short)(u[k] & 0xffffu);
                    s_xt[(ch * 8 + 2 * k + 1) * HEAD_LD + pix] = (unsigned short)(u[k] >> 16);
                }
            }
        }
        __syncthreads();

        // dx: a wave owns 64 pixels = 4 column tiles of 16
#pragma unroll
        for (int mt = 0; mt < 4; mt++) {
            const int pix = wave * 64 + mt * 16 + r;
            frag_ab b[KT];
#pragma unroll
            for (int ks = 0; ks < KT; ks++) {
                unsigned u[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int o0 = ks * 32 + g * 8 + 2 * k;
                    u[k] = (unsigned)s_dy[o0 * HEAD_LD + pix] | ((unsigned)s_dy[(o0 + 1) * HEAD_LD + pix] << 16);
                }
                b[ks] = __builtin_bit_cast(frag_ab, make_uint4(u[0], u[1], u[2], u[3]));
            }
            const long p = p0 + pix;
#pragma unroll
            for (int nc = 0; nc < NC; nc++) {
                frag_cd acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int ks = 0; ks < KT; ks++) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aw[nc][ks], b[ks], acc, 0, 0, 0);
                // D[row = c = 16 nc + 4 g + reg][col = pixel r]
                if (p < npix)
                    *reinterpret_cast<uint2 *>(dx + p * CIN + nc * 16 + g * 4) = make_uint2(head_pack(acc[0], acc[1]), head_pack(acc[2], acc[3]));
            }
        }
        // dw, db: K = the wave's 64 pixels, two steps of 32
#pragma unroll
        for (int ks = 0; ks < 2; ks++) {
            const int pk = wave * 64 + ks * 32 + g * 8;
            frag_ab bx[NC];
#pragma unroll
            for (int nc = 0; nc < NC; nc++) bx[nc] = __builtin_bit_cast(frag_ab, *reinterpret_cast<const uint4 *>(&s_xt[(nc * 16 + r) * HEAD_LD + pk]));
#pragma unroll
            for (int mo = 0; mo < MO; mo++) {
                const frag_ab ad = __builtin_bit_cast(frag_ab, *reinterpret_cast<const uint4 *>(&s_dy[(mo * 16 + r) * HEAD_LD + pk]));
                dbacc[mo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, ones, dbacc[mo], 0, 0, 0);
#pragma unroll
                for (int nc = 0; nc < NC; nc++) dwacc[mo][nc] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ad, bx[nc], dwacc[mo][nc], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // the four waves' sums, added in wave order in LDS (the tile buffers are free now), then out as this workgroup's partial
    float *s_red = reinterpret_cast<float *>(s_mem);           // [KP * CIN + KP] floats <= the tile buffers
    for (int wv = 0; wv < 4; wv++) {
        if (wave == wv) {
#pragma unroll
            for (int mo = 0; mo < MO; mo++) {
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int o = mo * 16 + g * 4 + reg;
#pragma unroll
                    for (int nc = 0; nc < NC; nc++) {
                        const int idx = o * CIN + nc * 16 + r;
                        s_red[idx] = wv == 0 ? dwacc[mo][nc][reg] : s_red[idx] + dwacc[mo][nc][reg];
                    }
                    if (r == 0) s_red[KP * CIN + o] = wv == 0 ? dbacc[mo][reg] : s_red[KP * CIN + o] + dbacc[mo][reg];
                }
            }
        }
        __syncthreads();
    }
    float *out = partials + (long)blockIdx.x * (KP * CIN + KP);
    for (int i = threadIdx.x; i < KP * CIN + KP; i += 256) out[i] = s_red[i];
}

// dw[o][c] / db[o] = sum over the workgroups' partials: thread (element e, split s) adds partials s, s + 16, ... in order, the 16
// splits are added in order
__global__ void __launch_bounds__(256)
headn_reduce_kernel(const float *__restrict__ partials, int nparts, int pstride, int kp, int Cin, int Cout, float *__restrict__ dw,
                    float *__restrict__ db) {
    __shared__ float s[HEAD_RED_SPLIT][16];
    const int el = threadIdx.x & 15, sp = threadIdx.x >> 4;
    const int e = blockIdx.x * 16 + el, total = Cout * Cin + Cout;
    float acc = 0.f;
    if (e < total) {
        const int src = e < Cout * Cin ? e : kp * Cin + (e - Cout * Cin);       // rows o < Cout are the leading rows of the padded partial
        for (int b = sp; b < nparts; b += HEAD_RED_SPLIT) acc += partials[(long)b * pstride + src];
    }
    s[sp][el] = acc;
    __syncthreads();
    if (sp == 0 && e < total) {
        float t = s[0][el];
        for (int k = 1; k < HEAD_RED_SPLIT; k++) t += s[k][el];
        if (e < Cout * Cin) dw[e] = t;
        else if (db) db[e - Cout * Cin] = t;
    }
}

int headn_check(const char *who, int N, int64_t hw, int Cin, int Cout) {
    if (N <= 0 || hw <= 0 || (Cin != 32 && Cin != 64) || Cout < 2 || Cout > 64) {
        octa::set_error("%s: unsupported shape N = %d, hw = %lld, Cin = %d, Cout = %d (Cin must be 32 or 64, 2 <= Cout <= 64)", who, N, (long long)hw, Cin, Cout);
        return -2;
    }
    if (hw > INT32_MAX / 2 || (int64_t)N * hw > INT32_MAX / 2) {
        octa::set_error("%s: N * hw = %lld pixels is beyond the kernel's 2^30 limit", who, (long long)N * (long long)hw);
        return -2;
    }
    return 0;
}

template <int CIN, int NT>
int launch_fwd(const octa_ctx *ctx, const unsigned short *x, const float *w, const float *bias, long npix, int hw, int Cout, unsigned short *y,
               hipStream_t stream) {
    const long ntiles = (npix + HEAD_TP - 1) / HEAD_TP;
    const long blocks = ntiles < 4L * ctx->num_cus ? ntiles : 4L * ctx->num_cus;
    const size_t lds = (size_t)NT * 16 * HEAD_LD * sizeof(unsigned short);
    hipLaunchKernelGGL((headn_fwd_kernel<CIN, NT>), dim3((unsigned)blocks), dim3(256), lds, stream, x, w, bias, npix, hw, Cout, y);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

template <int CIN, int KT>
int launch_bwd(octa_ctx *ctx, const unsigned short *x, const unsigned short *dy, const float *w, long npix, int hw, int Cout, unsigned short *dx,
               float *dw, float *db, hipStream_t stream) {
    const long ntiles = (npix + HEAD_TP - 1) / HEAD_TP;
    const long blocks = ntiles < 2L * ctx->num_cus ? ntiles : 2L * ctx->num_cus;
    constexpr int KP = KT * 32, PSTRIDE = KP * CIN + KP;
    float *ws = ctx->wgrad_ws.take<float>((size_t)blocks * PSTRIDE);
    if (!ws) return -1;
    const size_t lds = (size_t)(KP + CIN) * HEAD_LD * sizeof(unsigned short);
    static_assert((size_t)PSTRIDE * sizeof(float) <= (size_t)(KP + CIN) * HEAD_LD * sizeof(unsigned short), "the wave reduction reuses the tile buffers");
    if (lds > 64 * 1024)      // 64 -> more than 32 channels: 66 KB of the CU's 160 KB
        OCTA_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(&headn_bwd_kernel<CIN, KT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((headn_bwd_kernel<CIN, KT>), dim3((unsigned)blocks), dim3(256), lds, stream, x, dy, w, npix, hw, Cout, dx, ws);
    OCTA_HIP_CHECK(hipGetLastError());
    const int total = Cout * CIN + Cout;
    hipLaunchKernelGGL(headn_reduce_kernel, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, stream, ws, (int)blocks, PSTRIDE, KP, CIN, Cout, dw, db);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" int octa_headn_nhwc_fwd(octa_ctx *ctx, const void *d_x, const float *d_w, const float *d_bias, int N, int64_t hw, int Cin, int Cout,
                                   void *d_y, void *stream_) {
    if (!ctx || !d_x || !d_w || !d_y) { octa::set_error("octa_headn_nhwc_fwd: null pointer"); return -2; }
    if (headn_check("octa_headn_nhwc_fwd", N, hw, Cin, Cout)) return -2;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned short *x = static_cast<const unsigned short *>(d_x);
    unsigned short *y = static_cast<unsigned short *>(d_y);
    const long npix = (long)N * hw;
    const int nt = (Cout + 15) / 16;
#define OCTA_HEADN_FWD(CIN_, NT_) if (Cin == CIN_ && nt == NT_) return launch_fwd<CIN_, NT_>(ctx, x, d_w, d_bias, npix, (int)hw, Cout, y, stream)
    OCTA_HEADN_FWD(32, 1); OCTA_HEADN_FWD(32, 2); OCTA_HEADN_FWD(32, 3); OCTA_HEADN_FWD(32, 4);
    OCTA_HEADN_FWD(64, 1); OCTA_HEADN_FWD(64, 2); OCTA_HEADN_FWD(64, 3); OCTA_HEADN_FWD(64, 4);
#undef OCTA_HEADN_FWD
    octa::set_error("octa_headn_nhwc_fwd: no kernel for Cin = %d, Cout = %d", Cin, Cout);
    return -2;
}

extern "C" int octa_headn_nhwc_bwd(octa_ctx *ctx, const void *d_x, const void *d_dy, const float *d_w, int N, int64_t hw, int Cin, int Cout,
                                   void *d_dx, float *d_dw, float *d_db, void *stream_) {
    if (!ctx || !d_x || !d_dy || !d_w || !d_dx || !d_dw) { octa::set_error("octa_headn_nhwc_bwd: null pointer"); return -2; }
    if (headn_check("octa_headn_nhwc_bwd", N, hw, Cin, Cout)) return -2;
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const unsigned short *x = static_cast<const unsigned short *>(d_x), *dy = static_cast<const unsigned short *>(d_dy);
    unsigned short *dx = static_cast<unsigned short *>(d_dx);
    const long npix = (long)N * hw;
    const int kt = (Cout + 31) / 32;
#define OCTA_HEADN_BWD(CIN_, KT_) if (Cin == CIN_ && kt == KT_) return launch_bwd<CIN_, KT_>(ctx, x, dy, d_w, npix, (int)hw, Cout, dx, d_dw, d_db, stream)
    OCTA_HEADN_BWD(32, 1); OCTA_HEADN_BWD(32, 2); OCTA_HEADN_BWD(64, 1); OCTA_HEADN_BWD(64, 2);
#undef OCTA_HEADN_BWD
    octa::set_error("octa_headn_nhwc_bwd: no kernel for Cin = %d, Cout = %d", Cin, Cout);
    return -2;
}
