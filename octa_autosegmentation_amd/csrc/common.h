// common.h -- context, error reporting and scratch management shared by the HIP sources.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/octa_hip.h"

namespace octa {

void set_error(const char *fmt, ...);

#define OCTA_HIP_CHECK(expr)                                                                   \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            octa::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                            __LINE__);                                                         \
            return -1;                                                                         \
        }                                                                                      \
    } while (0)

// grow-only device buffer
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    int reserve(size_t bytes) {
        if (bytes <= cap) return 0;
        if (p) {
            // kernels launched a moment ago may still read the old buffer (on any stream of this context's owner): wait
            // for the device explicitly instead of relying on hipFree's implicit synchronisation
            hipError_t e = hipDeviceSynchronize();
            e = hipFree(p);
            (void)e;
            p = nullptr;
            cap = 0;
        }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            set_error("hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
            p = nullptr;
            return -1;
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p) {
            hipError_t e = hipFree(p);
            (void)e;
        }
        p = nullptr;
        cap = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
    // room for `count` elements of T, then the buffer as T*; nullptr with the error set when the allocation fails
    template <class T> T *take(size_t count) { return reserve(sizeof(T) * count) ? nullptr : as<T>(); }
    DevBuf &operator=(const DevBuf &) = delete;    // an owner: assigning a struct that holds one (`plan = RasterPlan()`) must not compile
};

}  // namespace octa

#if defined(__HIPCC__)
// fp32 -> bf16, round to nearest even, on gfx950's v_cvt_pk_bf16_f32 (one instruction per PAIR; the integer formulation costs
// five per value, which shows in the VALU-bound epilogues and streaming kernels). Bit-identical to it for every non-NaN input.
__device__ __forceinline__ unsigned octa_pack_bf16x2(float lo, float hi) {
    typedef __attribute__((ext_vector_type(2))) float octa_f2;
    typedef __attribute__((ext_vector_type(2))) __bf16 octa_bf2;
    const octa_f2 v = {lo, hi};
    const octa_bf2 r = __builtin_convertvector(v, octa_bf2);
    return __builtin_bit_cast(unsigned, r);
}
__device__ __forceinline__ unsigned short octa_f2bf(float f) { return (unsigned short)(octa_pack_bf16x2(f, 0.f) & 0xffffu); }
#endif

namespace octa {

// The rasteriser's device counters, zeroed by every plan. The kernels of raster.hip address them through `int *err_flag` (error at int 0,
// the profile counters of an OCTA_RASTER_PROF build at ints 2 / 4 / 6) and `long *total_out`: the asserts below pin that layout.
struct RasterCounters {
    int error;          // a RasterError, 0 = none; written with atomicExch, the last writer wins
    int pad;
    long prof[3];       // 100 MHz ticks summed over workgroups: edge binning, stroke tessellation, ordered fold
    long side_total;    // polygon sides of all edges: the plan half sizes the side array from it
};
static_assert(offsetof(RasterCounters, error) == 0 && offsetof(RasterCounters, prof) == 2 * sizeof(int) &&
              offsetof(RasterCounters, prof[1]) == 4 * sizeof(int) && offsetof(RasterCounters, prof[2]) == 6 * sizeof(int) &&
              offsetof(RasterCounters, side_total) == 4 * sizeof(long), "raster.hip's kernels index the counters as int 0, ints 2 / 4 / 6 and long 4");
// Nothing in production reads `error` back: only octa_raster_prof returns it, to a timing tool ("Context scratch").
enum RasterError {
    RASTER_ERR_EDGE_SKIPPED = 1,    // a single edge does not fit the render workgroup's LDS pool and was left out
    RASTER_ERR_TESS_OVERFLOW = 2,   // clipping gave an edge more extra side pieces than its spare slots hold; the surplus was dropped
    RASTER_ERR_SIDE_TOTAL = 3,      // the side total left the 32-bit offset range
};

// HELD: what octa_rasterize_2d_plan leaves for octa_rasterize_2d_draw (raster.hip). A context holds one plan; only raster.hip names these.
struct RasterPlan {
    bool valid = false, rowbin = false; int B = 0, W = 0, H = 0; long n_total = 0;
    DevBuf edge_off;   // long [B + 1]
    DevBuf meta;        // EdgeMeta [n_total + 1]
    DevBuf bbox;        // BBox16 [n_total + 1] per-edge pixel boxes
    DevBuf side_off;    // int [n_total + 1] side offsets, local to a scan block
    DevBuf block_sums;  // int [scan blocks + 1] scan block sums -> bases
    DevBuf counters;    // RasterCounters
};

}  // namespace octa

struct octa_ctx {
    int device = 0;
    int num_cus = 256;
    octa::RasterPlan plan;
    // TRANSIENT: work buffers any entry point may take; their contents are dead once it returns (one context = one stream at a time).
    //   0: rasteriser sides (int4), voxeliser byte volume
    //   1: rasteriser row records (RowRec); component counts and roots (postproc, cc3d); skeleton pass flags
    //   2: rasteriser per-row counts; component labels (postproc, cc3d); skeleton bit planes
    //   3: fp64 partial sums (norm); best-component records (cc3d); voxeliser per-edge image index
    // octa_rasterize_2d_plan RESERVES slots 0 - 2 for the draw half, which must not touch the allocator, and the draw half takes its
    // pointers when it runs: only the capacity has to survive a call in between, and a grow-only buffer keeps that.
    octa::DevBuf work[4];
    octa::DevBuf wgrad_ws;      // TRANSIENT, kept apart from the slots: per-workgroup partial weight gradients (conv.hip, head.hip), stream-ordered like the rest
    octa::DevBuf read_back_flag;  // TRANSIENT: int, octa_edges_read_back's count of unhandled rows (graphio.hip)
    octa::DevBuf zero_page;     // HELD: 256 zero bytes: source of the padding pixels of the DMA-staged convolutions (conv.hip, conv_f32.hip)
    // the zero page, filled on first use; nullptr on failure. `who` opens the error text
    const void *zeros(const char *who) {
        if (!zero_page.p) {
            if (zero_page.reserve(256)) return nullptr;
            // hipMemset on device memory may return before the fill has run, and it runs on the NULL stream, which torch's (non-blocking) streams do
            // not wait for: the first DMA-staged launch of a fresh context could fetch its padding from an uncleared page. Wait for the device once.
            if (hipMemset(zero_page.p, 0, zero_page.cap) != hipSuccess || hipDeviceSynchronize() != hipSuccess) { octa::set_error("%s: zero page memset failed", who); zero_page.release(); return nullptr; }
        }
        return zero_page.p;
    }
    // HELD: ring of pre-zeroed accumulator slots (norm.hip statistics): ONE memset per lap instead of one per launch. Stream-ordered
    // like every other scratch buffer of the context (one context = one stream at a time).
    octa::DevBuf zero_ring;
    size_t zero_ring_pos = 0;
    // returns `bytes` (multiple of 256 after rounding) of zeros that the caller may dirty; nullptr on failure
    void *zeroed(size_t bytes, hipStream_t stream) {
        bytes = (bytes + 255) & ~(size_t)255;
        const size_t want = bytes * 64 > ((size_t)4 << 20) ? bytes * 64 : ((size_t)4 << 20);
        if (zero_ring.cap < want) {
            if (zero_ring.reserve(want)) return nullptr;
            zero_ring_pos = zero_ring.cap;            // force a clearing lap
        }
        if (zero_ring_pos + bytes > zero_ring.cap) {
            if (hipMemsetAsync(zero_ring.p, 0, zero_ring.cap, stream) != hipSuccess) { octa::set_error("zero ring memset failed"); return nullptr; }
            zero_ring_pos = 0;
        }
        void *r = static_cast<char *>(zero_ring.p) + zero_ring_pos;
        zero_ring_pos += bytes;
        return r;
    }
    // THE list of the context's device buffers: octa_ctx_destroy and scratch_bytes() walk it, so a new buffer is added here and nowhere else
    template <class Ctx, class F> static void each_buffer(Ctx &c, F f) {
        for (auto *b : {&c.plan.edge_off, &c.plan.meta, &c.plan.bbox, &c.plan.side_off, &c.plan.block_sums, &c.plan.counters, &c.work[0], &c.work[1],
                        &c.work[2], &c.work[3], &c.wgrad_ws, &c.read_back_flag, &c.zero_page, &c.zero_ring})
            f(*b);
    }
    size_t scratch_bytes() const {
        size_t n = 0;
        each_buffer(*this, [&](const octa::DevBuf &b) { n += b.cap; });
        return n;
    }
};
