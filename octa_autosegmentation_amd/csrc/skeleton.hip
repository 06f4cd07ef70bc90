// skeleton.hip -- Zhang & Suen (1984) parallel thinning for the clDice metric of the validation phase.
//
// Replaces `skimage.morphology.skeletonize` (2-D) of the reference's utils/cldice.py for a batch of masks resident in HBM.
// The rule, for a foreground pixel P1 with neighbours P2 = N, P3 = NE, P4 = E, P5 = SE, P6 = S, P7 = SW, P8 = W, P9 = NW (outside the
// image = background), B = number of set neighbours, A = number of 0 -> 1 steps in the cyclic sequence P2 .. P9, P2:
//   removable when 2 <= B <= 6 and A == 1 and   first sub-iteration:  P2 P4 P6 == 0 and P4 P6 P8 == 0
//                                                second sub-iteration: P2 P4 P8 == 0 and P2 P6 P8 == 0
// every sub-iteration decides on the image as it was when it began; (first, second) repeats until a double pass removes nothing.
//
// Layout: the masks are packed 64 pixels to a uint64 (bit i of word xw = pixel x = 64 xw + i; bits past W stay zero), two packed
// copies A and B per image. One launch per sub-iteration, one lane per word: first reads A and writes B, second reads B and writes
// A, so no lane can see a value of the sub-iteration it is in (ordering between sub-iterations is the launch boundary on the stream,
// nothing waits inside a kernel). A lane loads the 3 x 3 words around its own, builds the eight neighbour planes with shifts and the
// carry bits of the adjacent words, and evaluates the rule as bitwise logic on all 64 pixels at once (a bit-sliced counter for B, "at
// least one / at least two" planes for A). A packed 1216^2 mask is 185 KB: the passes run out of L2.
//
// Termination: flag[d][b] is set (plain store of 1) by any lane that removes a pixel of image b in double pass d. The lanes of double
// pass d + 1 leave at once when flag[d][b] is 0 -- the image is at its fixed point, A holds it, and its later flags stay 0 -- so a
// converged image costs nothing but the empty lanes. The host reads the flags once per chunk of SKEL_CHUNK double passes.

#include "common.h"

namespace {

typedef unsigned long long u64;

// double passes between two host reads of the flags. Chosen by counting, PROVISIONAL until the costs are measured: a
// read makes the host wait for the stream, so K must be well above 1; with K = 8 the 1216^2 vessel masks (16 .. 24 double passes) take
// 2 .. 3 reads for 34 .. 50 launches, and the overshoot is at most 7 double passes of lanes that leave at once.
constexpr int SKEL_CHUNK = 8;

__global__ void __launch_bounds__(256)
skel_pack_kernel(const unsigned char *__restrict__ in, u64 *__restrict__ A, int H, int W, int Wq, long n_words) {
    // one wave per word: lane i holds pixel 64 xw + i, the ballot is the word
    const long word = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (word >= n_words) return;                                   // wave-uniform
    const int lane = threadIdx.x & 63;
    const int xw = (int)(word % Wq);
    const long row = word / Wq;                                    // b * H + y
    const int x = xw * 64 + lane;
    const bool on = x < W && in[row * W + x] != 0;
    const u64 bits = __ballot(on);
    if (lane == 0) A[word] = bits;
}

__global__ void __launch_bounds__(256)
skel_unpack_kernel(const u64 *__restrict__ A, unsigned char *__restrict__ out, int W, int Wq, long n_pixels) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pixels) return;
    const long row = i / W;
    const int x = (int)(i - row * W);
    out[i] = (unsigned char)((A[row * Wq + (x >> 6)] >> (x & 63)) & 1ull);
}

// SECOND = false: first sub-iteration, true: second. prev_flag: flags of the previous double pass (nullptr in the first one).
template <bool SECOND>
__global__ void __launch_bounds__(256)
skel_sub_kernel(const u64 *__restrict__ src, u64 *__restrict__ dst, const int *__restrict__ prev_flag, int *__restrict__ flag, int H,
                int Wq, long n_words) {
    const long word = (long)blockIdx.x * 256 + threadIdx.x;
    if (word >= n_words) return;
    const long words_per_image = (long)H * Wq;
    const int b = (int)(word / words_per_image);
    if (prev_flag && prev_flag[b] == 0) return;                    // fixed point reached: A is final, B is not read again
    const long in_image = word - (long)b * words_per_image;
    const int y = (int)(in_image / Wq), xw = (int)(in_image - (long)y * Wq);
    const bool has_l = xw > 0, has_r = xw + 1 < Wq;
    const u64 *c = src + word;

    const u64 C = c[0];
    u64 keep = C;
    if (C) {
        const u64 Cl = has_l ? c[-1] : 0ull, Cr = has_r ? c[1] : 0ull;
        u64 N = 0, Nl = 0, Nr = 0, S = 0, Sl = 0, Sr = 0;
        if (y > 0) {
            N = c[-Wq];
            Nl = has_l ? c[-Wq - 1] : 0ull;
            Nr = has_r ? c[-Wq + 1] : 0ull;
        }
        if (y + 1 < H) {
            S = c[Wq];
            Sl = has_l ? c[Wq - 1] : 0ull;
            Sr = has_r ? c[Wq + 1] : 0ull;
        }
        // bit i = pixel x: the pixel to the east (x + 1) is bit i + 1, so its plane is the word shifted DOWN, with bit 0 of the right word
        const u64 p2 = N, p3 = (N >> 1) | (Nr << 63), p4 = (C >> 1) | (Cr << 63), p5 = (S >> 1) | (Sr << 63);
        const u64 p6 = S, p7 = (S << 1) | (Sl >> 63), p8 = (C << 1) | (Cl >> 63), p9 = (N << 1) | (Nl >> 63);
        const u64 p[8] = {p2, p3, p4, p5, p6, p7, p8, p9};
        u64 b0 = 0, b1 = 0, b2 = 0, b3 = 0;                       // bit-sliced B
        u64 one = 0, two = 0;                                       // A >= 1, A >= 2
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const u64 q = p[k];
            const u64 c0 = b0 & q;
            b0 ^= q;
            const u64 c1 = b1 & c0;
            b1 ^= c0;
            const u64 c2 = b2 & c1;
            b2 ^= c1;
            b3 |= c2;
            const u64 step = ~q & p[(k + 1) & 7];
            two |= one & step;
            one |= step;
        }
        const u64 b_ok = ~b3 & (b1 | b2) & ~(b0 & b1 & b2);      // not 8, not 0 / 1, not 7
        const u64 a_ok = one & ~two;
        const u64 cond = SECOND ? (~(p2 & p4 & p8) & ~(p2 & p6 & p8)) : (~(p2 & p4 & p6) & ~(p4 & p6 & p8));
        const u64 gone = C & b_ok & a_ok & cond;
        keep = C & ~gone;
        if (gone) flag[b] = 1;
    }
    dst[word] = keep;
}

}  // namespace

extern "C" int octa_skeletonize(octa_ctx *ctx, const uint8_t *d_in, int B, int H, int W, uint8_t *d_out, int *passes, void *stream_) {
    if (!ctx || !d_in || !d_out || B <= 0 || H <= 0 || W <= 0) { octa::set_error("octa_skeletonize: bad arguments"); return -2; }
    const long n_pixels = (long)B * H * W;
    if (n_pixels > 0x7fffffffL) { octa::set_error("octa_skeletonize: more than 2^31 pixels in one batch"); return -2; }
    {   // the input is read after the output is written (pack, passes, unpack): no overlap at all
        const uintptr_t i0 = (uintptr_t)d_in, o0 = (uintptr_t)d_out;
        if (i0 < o0 + (uintptr_t)n_pixels && o0 < i0 + (uintptr_t)n_pixels) { octa::set_error("octa_skeletonize: d_out must not alias d_in"); return -2; }
    }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    const int Wq = (W + 63) / 64;
    const long n_words = (long)B * H * Wq;
    // hard bound of the host loop, in double passes. H + W is a heuristic, not a theorem: blobs lose a layer per removing pass (at
    // most min(H, W) / 2 of them), but a long diagonal staircase unzips from its ends a few pixels per pass (100 x 101: 50 passes), and
    // no proof covers every shape. Running into it is a loud -3 on a call that was still converging, never a wrong skeleton.
    const int bound = H + W + SKEL_CHUNK;
    const int max_chunks = (bound + SKEL_CHUNK - 1) / SKEL_CHUNK;
    u64 *A = ctx->work[2].take<u64>(2 * (size_t)n_words);
    // flags of two chunks, alternating: a chunk's first double pass reads the last flags of the chunk before it
    int *flags = ctx->work[1].take<int>((size_t)SKEL_CHUNK * B * 2);
    if (!A || !flags) return -1;
    u64 *Bp = A + n_words;
    std::vector<int> h_flags((size_t)SKEL_CHUNK * B);

    hipLaunchKernelGGL(skel_pack_kernel, dim3((unsigned)((n_words + 3) / 4)), dim3(256), 0, stream, d_in, A, H, W, Wq, n_words);
    const unsigned blocks = (unsigned)((n_words + 255) / 256);
    int removing = 0;
    bool converged = false;
    for (int chunk = 0; chunk < max_chunks && !converged; ++chunk) {
        int *cur = flags + (size_t)(chunk & 1) * SKEL_CHUNK * B;
        const int *last_of_prev = flags + (size_t)((chunk & 1) ^ 1) * SKEL_CHUNK * B + (size_t)(SKEL_CHUNK - 1) * B;
        OCTA_HIP_CHECK(hipMemsetAsync(cur, 0, sizeof(int) * (size_t)SKEL_CHUNK * B, stream));
        for (int k = 0; k < SKEL_CHUNK; ++k) {
            const int *prev = k > 0 ? cur + (size_t)(k - 1) * B : (chunk > 0 ? last_of_prev : nullptr);
            int *f = cur + (size_t)k * B;
            hipLaunchKernelGGL(skel_sub_kernel<false>, dim3(blocks), dim3(256), 0, stream, (const u64 *)A, Bp, prev, f, H, Wq, n_words);
            hipLaunchKernelGGL(skel_sub_kernel<true>, dim3(blocks), dim3(256), 0, stream, (const u64 *)Bp, A, prev, f, H, Wq, n_words);
        }
        OCTA_HIP_CHECK(hipGetLastError());
        OCTA_HIP_CHECK(hipMemcpyAsync(h_flags.data(), cur, sizeof(int) * (size_t)SKEL_CHUNK * B, hipMemcpyDeviceToHost, stream));
        OCTA_HIP_CHECK(hipStreamSynchronize(stream));
        for (int k = 0; k < SKEL_CHUNK; ++k) {
            bool any = false;
            for (int b = 0; b < B; ++b) any = any || h_flags[(size_t)k * B + b] != 0;
            if (any) removing = chunk * SKEL_CHUNK + k + 1;
            else { converged = true; break; }                       // later double passes of the chunk were no-ops
        }
    }
    if (!converged) {
        octa::set_error("octa_skeletonize: no fixed point after %d double passes (H + W = %d)", max_chunks * SKEL_CHUNK, H + W);
        return -3;
    }
    hipLaunchKernelGGL(skel_unpack_kernel, dim3((unsigned)((n_pixels + 255) / 256)), dim3(256), 0, stream, (const u64 *)A, d_out, W, Wq, n_pixels);
    OCTA_HIP_CHECK(hipGetLastError());
    if (passes) *passes = removing + 1;                             // the removing double passes and the one that found nothing to remove
    return 0;
}
