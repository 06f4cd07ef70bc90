// cc3d.hip -- 3-D connected components for the volume post-processing: keep the components with at least
// min_size voxels, or the largest one per volume (RemoveOuterNoise / KeepLargestConnectedComponent of the reference's
// data/data_transforms.py:418-432, MONAI -> skimage.measure.label + bincount + argmax).
//
// The volume is cut into bricks of 4 x 8 x 64 voxels (W fastest, so a brick row is one 64-byte run of the input). Five passes:
//   local   one workgroup per brick: foreground -> LDS, union-find over the brick in LDS only (ids are the 11-bit positions in the
//           brick, kept in 32-bit LDS words because the LDS min is a 32-bit operation), members counted per local root in LDS;
//           writes each voxel's provisional label (the global flat index of its local root, -1 = background) and, per
//           foreground voxel, the member count of its local root at the root and 0 elsewhere
//   seam    the voxels on a brick's faces unite with their forward neighbours in the adjacent bricks: larger root under the
//           smaller one (atomic min), so links strictly decrease and every root ends as the smallest flat index of its component;
//           interior voxels do nothing
//   resolve per brick: every voxel's label becomes its final root; the counts of the brick's local roots that are not final roots are
//           added per final root in LDS, then one global integer add per (brick, root)
//   roots   per volume: number of roots, 64-bit max over (count << 32) | (0xffffffff - root index in the volume), reduced in
//           registers, per wave and per workgroup first: most voxels win, ties go to the component whose first voxel comes first in C order
//   filter  a voxel survives if its root's count reaches min_size (mode 0) or its root is the volume's winner (mode 1)
// Integer work only; minimum, integer sum and maximum do not depend on the order they are applied in, so the output is a pure
// function of the input. The neighbour tests use coordinates inside one volume, so volumes of a batch are never united.

#include "common.h"

namespace {

constexpr int BX = 64, BY = 8, BZ = 4, BV = BX * BY * BZ, NT = 256, VPT = BV / NT;
constexpr int ROOTS_SPAN = 1024, ROOTS_GRID = 2048;     // roots pass: at least this many voxels per workgroup, about this many workgroups

// Union-find on an int array (LDS: workgroup scope, HBM: agent scope -- the relaxed agent-scope loads bypass the CU's L1, which
// another CU's atomics never refresh). L[x] <= x always, roots have L[r] == r.
template <int SCOPE>
__device__ __forceinline__ int uf_find(int *L, int x) {
    while (true) {
        const int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
        if (p == x) return x;
        const int g = __hip_atomic_load(L + p, __ATOMIC_RELAXED, SCOPE);
        if (g != p) __hip_atomic_store(L + x, g, __ATOMIC_RELAXED, SCOPE);   // path halving; benign race: only ever moves x closer to its root
        x = p;
    }
}

template <int SCOPE>
__device__ __forceinline__ void uf_union(int *L, int a, int b) {
    while (true) {
        a = uf_find<SCOPE>(L, a);
        b = uf_find<SCOPE>(L, b);
        if (a == b) return;
        if (a > b) { const int t = a; a = b; b = t; }
        const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, SCOPE);   // link root b under a (a < b)
        if (old == b) return;                  // b was still a root: linked
        b = old;                               // someone linked b elsewhere meanwhile: unite with that instead
    }
}

// read-only walk to the root (the forest is final)
__device__ __forceinline__ int uf_root(const int *L, int x) {
    while (true) {
        const int p = L[x];
        if (p == x) return x;
        x = p;
    }
}

// The 13 forward neighbours (after the voxel in C order), numbered o = 0 .. 12 in C order of (dz, dy, dx): (0,0,1), (0,1,-1), ..., (1,1,1).
constexpr int NOFF = 13;
__device__ __forceinline__ constexpr int off_dz(int o) { return (o + 5) / 9; }
__device__ __forceinline__ constexpr int off_dy(int o) { return (o + 5) % 9 / 3 - 1; }
__device__ __forceinline__ constexpr int off_dx(int o) { return (o + 5) % 3 - 1; }
// in the 6- / 18- / 26-neighbourhood (conn 1 / 2 / 3)?
__device__ __forceinline__ constexpr bool off_in(int o, int conn) {
    return off_dz(o) + (off_dy(o) < 0 ? -off_dy(o) : off_dy(o)) + (off_dx(o) < 0 ? -off_dx(o) : off_dx(o)) <= conn;
}
// Both brick kernels first collect a thread's pairs to unite in a bit set -- bit (j & 3) * 13 + o of word j >> 2 for its voxel j and
// offset o, the neighbours read without a branch so that the reads overlap -- and then unite them in ONE loop: the lanes of a wave work
// on their pairs side by side, and a wave takes as long as its busiest lane, not as long as all (voxel, offset) steps one after another.
__device__ __forceinline__ int pop_pair(unsigned long long (&pend)[2], int &j) {
    const int h = pend[0] ? 0 : 1;
    const int q = __ffsll((long long)pend[h]) - 1;
    pend[h] &= pend[h] - 1;
    j = h * 4 + q / NOFF;
    return q % NOFF;
}

struct Brick { int x0, y0, z0; long vbase; };

__device__ __forceinline__ Brick brick_of(unsigned b, int D, int H, int W, int nbx, int nby, int nbz) {
    Brick k;
    k.x0 = (int)(b % (unsigned)nbx) * BX; b /= (unsigned)nbx;
    k.y0 = (int)(b % (unsigned)nby) * BY; b /= (unsigned)nby;
    k.z0 = (int)(b % (unsigned)nbz) * BZ; b /= (unsigned)nbz;
    k.vbase = (long)b * D * H * W;
    return k;
}

template <int CONN>
__global__ void __launch_bounds__(NT)
cc3_local_kernel(const unsigned char *__restrict__ in, int *__restrict__ Lg, int *__restrict__ cnt, int D, int H, int W, int nbx, int nby, int nbz,
                 unsigned bricks) {
    __shared__ int P[BV];     // parent (position in the brick), -1 = background or outside the volume
    __shared__ int C[BV];     // members per local root
    for (unsigned brick = blockIdx.x; brick < bricks; brick += gridDim.x) {      // one brick per workgroup unless the grid was capped
        const Brick k = brick_of(brick, D, H, W, nbx, nby, nbz);
        const int t = threadIdx.x;
        // thread t owns positions l = j * 256 + t: lx = t & 63 for all of them, one 64-byte row of the input per wave and j
        const int lx = t & (BX - 1), x = k.x0 + lx;
        unsigned fg = 0;
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int l = j * NT + t, ly = (l >> 6) & (BY - 1), lz = l >> 9;
            const int y = k.y0 + ly, z = k.z0 + lz;
            bool f = false;
            if (x < W && y < H && z < D) f = in[k.vbase + ((long)z * H + y) * W + x] != 0;
            P[l] = f ? l : -1;
            C[l] = 0;
            fg |= (unsigned)f << j;
        }
        __syncthreads();
        unsigned long long pend[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int l = j * NT + t, ly = (l >> 6) & (BY - 1), lz = l >> 9;
#pragma unroll
            for (int o = 0; o < NOFF; ++o) {
                if (!off_in(o, CONN)) continue;
                const int nx = lx + off_dx(o), ny = ly + off_dy(o), nz = lz + off_dz(o);
                const bool valid = ((fg >> j) & 1u) && nx >= 0 && nx < BX && ny >= 0 && ny < BY && nz < BZ;
                const int n = P[valid ? (nz * BY + ny) * BX + nx : l];       // foreground or not: the unions of other threads do not change it
                if (valid && n >= 0) pend[j >> 2] |= 1ull << ((j & 3) * NOFF + o);
            }
        }
        while (pend[0] | pend[1]) {
            int j;
            const int o = pop_pair(pend, j);
            const int l = j * NT + t;
            uf_union<__HIP_MEMORY_SCOPE_WORKGROUP>(P, l, l + (off_dz(o) * BY + off_dy(o)) * BX + off_dx(o));
        }
        __syncthreads();
        int root[VPT];
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            root[j] = -1;
            if (!((fg >> j) & 1u)) continue;
            root[j] = uf_root(P, j * NT + t);
            atomicAdd(&C[root[j]], 1);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int l = j * NT + t, ly = (l >> 6) & (BY - 1), lz = l >> 9;
            const int y = k.y0 + ly, z = k.z0 + lz;
            if (x >= W || y >= H || z >= D) continue;
            const long g = k.vbase + ((long)z * H + y) * W + x;
            const int r = root[j];
            if (r < 0) { Lg[g] = -1; continue; }
            // the order of the positions in a brick is the C order of the volume: the local root is the component's first voxel here
            const int rx = r & (BX - 1), ry = (r >> 6) & (BY - 1), rz = r >> 9;
            Lg[g] = (int)(k.vbase + ((long)(k.z0 + rz) * H + (k.y0 + ry)) * W + (k.x0 + rx));
            cnt[g] = C[l];        // the members at the local root, 0 at every other foreground voxel (background entries are never read)
        }
        __syncthreads();
    }
}

template <int CONN>
__global__ void __launch_bounds__(NT)
cc3_seam_kernel(int *Lg, int D, int H, int W, int nbx, int nby, int nbz, unsigned bricks) {
    for (unsigned brick = blockIdx.x; brick < bricks; brick += gridDim.x) {
        const Brick k = brick_of(brick, D, H, W, nbx, nby, nbz);
        const int t = threadIdx.x;
        const int lx = t & (BX - 1), x = k.x0 + lx;
        unsigned fg = 0;          // bit j: voxel j is inside the volume, on a face of the brick, and foreground
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int l = j * NT + t, ly = (l >> 6) & (BY - 1), lz = l >> 9;
            const int y = k.y0 + ly, z = k.z0 + lz;
            const bool face = lx == 0 || lx == BX - 1 || ly == 0 || ly == BY - 1 || lz == 0 || lz == BZ - 1;
            if (face && x < W && y < H && z < D) fg |= (unsigned)(Lg[k.vbase + ((long)z * H + y) * W + x] >= 0) << j;
        }
        unsigned long long pend[2] = {0, 0};
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            if (!__any((fg >> j) & 1u)) continue;       // the rows inside the brick have work in lanes 0 and 63 only, and seldom
            const int l = j * NT + t, ly = (l >> 6) & (BY - 1), lz = l >> 9;
            const int y = k.y0 + ly, z = k.z0 + lz;
            const long g = (fg >> j) & 1u ? k.vbase + ((long)z * H + y) * W + x : k.vbase;
            int prev = -1;
#pragma unroll
            for (int o = 0; o < NOFF; ++o) {
                if (!off_in(o, CONN)) continue;
                const int dz = off_dz(o), dy = off_dy(o), dx = off_dx(o);
                const bool leaves = lx + dx < 0 || lx + dx >= BX || ly + dy < 0 || ly + dy >= BY || lz + dz >= BZ;      // else: united in LDS
                const bool valid = ((fg >> j) & 1u) && leaves && x + dx >= 0 && x + dx < W && y + dy >= 0 && y + dy < H && z + dz < D;
                const int n = Lg[valid ? g + ((long)dz * H + dy) * W + dx : g];
                // two neighbours seen under the same label are in one component, whatever the other workgroups do meanwhile: one union
                // serves both (across a dense face a voxel's nine neighbours are mostly one local component of the next brick)
                if (valid && n >= 0 && n != prev) { pend[j >> 2] |= 1ull << ((j & 3) * NOFF + o); prev = n; }
            }
        }
        while (pend[0] | pend[1]) {
            int j;
            const int o = pop_pair(pend, j);
            const int l = j * NT + t, ly = (l >> 6) & (BY - 1), lz = l >> 9;
            const long g = k.vbase + ((long)(k.z0 + lz) * H + (k.y0 + ly)) * W + x;
            uf_union<__HIP_MEMORY_SCOPE_AGENT>(Lg, (int)g, (int)(g + ((long)off_dz(o) * H + off_dy(o)) * W + off_dx(o)));
        }
    }
}

// One workgroup per brick again. Every voxel's label becomes its final root. A local root that is not the final root hands its count
// on: the counts of a brick that go to the same root are added in an LDS table first (open addressing, one slot per position: a
// brick has at most BV / 2 local roots, the table cannot fill), then ONE global add per (brick, root) -- a component of millions of
// voxels receives an add per brick it passes through, not one per local root.
__global__ void __launch_bounds__(NT)
cc3_resolve_kernel(int *Lg, int *cnt, int D, int H, int W, int nbx, int nby, int nbz, unsigned bricks) {
    __shared__ int K[BV];     // root, -1 = free slot
    __shared__ int S[BV];     // count to add to it
    for (unsigned brick = blockIdx.x; brick < bricks; brick += gridDim.x) {
        const Brick k = brick_of(brick, D, H, W, nbx, nby, nbz);
        const int t = threadIdx.x;
        const int x = k.x0 + (t & (BX - 1));
#pragma unroll
        for (int j = 0; j < VPT; ++j) { K[j * NT + t] = -1; S[j * NT + t] = 0; }
        __syncthreads();
        // the first two steps of every walk and the counts are read for all eight voxels at once (outside the volume and on background:
        // the volume's first voxel instead, ignored), so that the reads overlap
        long g[VPT];
        int p[VPT], q[VPT], c[VPT];
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            const int l = j * NT + t, y = k.y0 + ((l >> 6) & (BY - 1)), z = k.z0 + (l >> 9);
            const bool inside = x < W && y < H && z < D;
            g[j] = inside ? k.vbase + ((long)z * H + y) * W + x : k.vbase;
            p[j] = Lg[g[j]];
            if (!inside) p[j] = -1;
        }
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            q[j] = Lg[p[j] >= 0 ? (long)p[j] : k.vbase];
            c[j] = cnt[p[j] >= 0 ? g[j] : k.vbase];       // > 0: a local root; under another root it receives no add itself, so this is its own count
        }
#pragma unroll
        for (int j = 0; j < VPT; ++j) {
            if (p[j] < 0) continue;
            const int r = q[j] == p[j] ? p[j] : uf_root(Lg, q[j]);
            if (r != p[j]) Lg[g[j]] = r;         // others may be walking through this voxel: they find r from the old value as well
            if (c[j] > 0 && r != (int)g[j]) {
                unsigned h = ((unsigned)r * 2654435761u) >> 21;      // 11 bits
                while (true) {
                    const int old = atomicCAS(&K[h], -1, r);
                    if (old == -1 || old == r) break;
                    h = (h + 1) & (BV - 1);
                }
                atomicAdd(&S[h], c[j]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < VPT; ++j)
            if (K[j * NT + t] >= 0) atomicAdd(&cnt[K[j * NT + t]], S[j * NT + t]);
        __syncthreads();
    }
}

// per volume: best[vol] = max key, ncomp[vol] += roots. per_vol workgroups stride through a volume; maximum and count are kept in
// registers, reduced per wave by shuffles and per workgroup in LDS: two global atomics per workgroup, a few thousand in all.
__global__ void __launch_bounds__(NT)
cc3_roots_kernel(const int *__restrict__ Lg, const int *__restrict__ cnt, unsigned long long *__restrict__ best, unsigned long long *__restrict__ ncomp,
                 long n_vol, unsigned per_vol) {
    __shared__ unsigned long long s_best[NT / 64];
    __shared__ unsigned s_n[NT / 64];
    const unsigned vol = blockIdx.x / per_vol;
    const long vbase = (long)vol * n_vol;
    unsigned long long key = 0;
    unsigned n = 0;
#pragma unroll 4
    for (long v = (long)(blockIdx.x % per_vol) * NT + threadIdx.x; v < n_vol; v += (long)per_vol * NT) {
        if (Lg[vbase + v] != (int)(vbase + v)) continue;
        const unsigned long long k = ((unsigned long long)(unsigned)cnt[vbase + v] << 32) | (unsigned long long)(0xffffffffu - (unsigned)v);
        key = k > key ? k : key;
        ++n;
    }
    for (int s = 32; s; s >>= 1) {
        const unsigned long long other = __shfl_xor(key, s, 64);
        key = other > key ? other : key;
        n += __shfl_xor(n, s, 64);
    }
    if ((threadIdx.x & 63) == 0) { s_best[threadIdx.x >> 6] = key; s_n[threadIdx.x >> 6] = n; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < NT / 64; ++w) { key = s_best[w] > key ? s_best[w] : key; n += s_n[w]; }
        if (n) {
            atomicMax(&best[vol], key);
            atomicAdd(&ncomp[vol], (unsigned long long)n);
        }
    }
}

__global__ void __launch_bounds__(NT)
cc3_filter_kernel(const int *__restrict__ Lg, const int *__restrict__ cnt, const unsigned long long *__restrict__ best, unsigned char *__restrict__ out,
                  long n_vol, long n_total, int mode, int min_size, unsigned char on_value) {
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= n_total) return;
    const int r = Lg[i];
    bool keep = false;
    if (r >= 0) {
        if (mode == 0) {
            keep = cnt[r] >= min_size;
        } else {
            const long vol = i / n_vol;
            const unsigned long long key = best[vol];      // non-zero: this volume has foreground
            keep = (long)r == vol * n_vol + (long)(0xffffffffu - (unsigned)(key & 0xffffffffu));
        }
    }
    out[i] = keep ? on_value : (unsigned char)0;
}

__global__ void cc3_info_kernel(const unsigned long long *__restrict__ best, const unsigned long long *__restrict__ ncomp, long long *__restrict__ info, int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const unsigned long long key = best[b];
    info[3 * b + 0] = (long long)ncomp[b];
    info[3 * b + 1] = (long long)(key >> 32);
    info[3 * b + 2] = key ? (long long)(0xffffffffu - (unsigned)(key & 0xffffffffu)) : -1;
}

}  // namespace

extern "C" int octa_cc3d_filter(octa_ctx *ctx, const uint8_t *d_in, int B, int D, int H, int W, int connectivity, int mode, int min_size,
                                uint8_t on_value, uint8_t *d_out, int64_t *d_info, void *stream_) {
    if (!ctx || !d_in || !d_out) { octa::set_error("octa_cc3d_filter: bad pointers"); return -2; }
    if (B <= 0 || D <= 0 || H <= 0 || W <= 0) { octa::set_error("octa_cc3d_filter: B, D, H, W must be positive"); return -2; }
    if (connectivity < 1 || connectivity > 3) { octa::set_error("octa_cc3d_filter: connectivity must be 1 (6-), 2 (18-) or 3 (26-neighbourhood)"); return -2; }
    if (mode < 0 || mode > 1) { octa::set_error("octa_cc3d_filter: mode must be 0 (size filter) or 1 (largest component)"); return -2; }
    const long n_plane = (long)H * W, n_vol = n_plane <= 0x7fffffffL ? n_plane * D : n_plane;     // no product leaves 63 bits
    if (n_vol > 0x7fffffffL || n_vol * B > 0x7fffffffL) { octa::set_error("octa_cc3d_filter: more than 2^31 - 1 voxels in one batch"); return -2; }
    const long n_total = n_vol * B;
    if (d_in < d_out + n_total && d_out < d_in + n_total) { octa::set_error("octa_cc3d_filter: bad pointers (d_out overlaps d_in)"); return -2; }
    hipStream_t stream = (hipStream_t)stream_;
    OCTA_HIP_CHECK(hipSetDevice(ctx->device));
    int *Lg = ctx->work[2].take<int>((size_t)n_total), *cnt = ctx->work[1].take<int>((size_t)n_total);
    unsigned long long *best = ctx->work[3].take<unsigned long long>(2 * (size_t)B);
    if (!Lg || !cnt || !best) return -1;
    unsigned long long *ncomp = best + B;
    const int nbx = (W + BX - 1) / BX, nby = (H + BY - 1) / BY, nbz = (D + BZ - 1) / BZ;
    const unsigned bricks = (unsigned)((long)nbx * nby * nbz * B);      // <= n_total
    const unsigned blocks = (unsigned)((n_total + NT - 1) / NT);
    const unsigned bgrid = bricks < (1u << 23) ? bricks : (1u << 23);     // grid x threads stays below 2^32 for thin volumes too
    if (connectivity == 1) {
        hipLaunchKernelGGL(cc3_local_kernel<1>, dim3(bgrid), dim3(NT), 0, stream, d_in, Lg, cnt, D, H, W, nbx, nby, nbz, bricks);
        hipLaunchKernelGGL(cc3_seam_kernel<1>, dim3(bgrid), dim3(NT), 0, stream, Lg, D, H, W, nbx, nby, nbz, bricks);
    } else if (connectivity == 2) {
        hipLaunchKernelGGL(cc3_local_kernel<2>, dim3(bgrid), dim3(NT), 0, stream, d_in, Lg, cnt, D, H, W, nbx, nby, nbz, bricks);
        hipLaunchKernelGGL(cc3_seam_kernel<2>, dim3(bgrid), dim3(NT), 0, stream, Lg, D, H, W, nbx, nby, nbz, bricks);
    } else {
        hipLaunchKernelGGL(cc3_local_kernel<3>, dim3(bgrid), dim3(NT), 0, stream, d_in, Lg, cnt, D, H, W, nbx, nby, nbz, bricks);
        hipLaunchKernelGGL(cc3_seam_kernel<3>, dim3(bgrid), dim3(NT), 0, stream, Lg, D, H, W, nbx, nby, nbz, bricks);
    }
    hipLaunchKernelGGL(cc3_resolve_kernel, dim3(bgrid), dim3(NT), 0, stream, Lg, cnt, D, H, W, nbx, nby, nbz, bricks);
    if (mode == 1 || d_info) {
        OCTA_HIP_CHECK(hipMemsetAsync(best, 0, sizeof(unsigned long long) * 2 * (size_t)B, stream));
        const long want = (n_vol + ROOTS_SPAN - 1) / ROOTS_SPAN, cap = ROOTS_GRID / B > 0 ? ROOTS_GRID / B : 1;
        const unsigned per_vol = (unsigned)(want < cap ? want : cap);
        hipLaunchKernelGGL(cc3_roots_kernel, dim3(per_vol * (unsigned)B), dim3(NT), 0, stream, Lg, cnt, best, ncomp, n_vol, per_vol);
        if (d_info) hipLaunchKernelGGL(cc3_info_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, best, ncomp, (long long *)d_info, B);
    }
    hipLaunchKernelGGL(cc3_filter_kernel, dim3(blocks), dim3(NT), 0, stream, Lg, cnt, best, d_out, n_vol, n_total, mode, min_size, on_value);
    OCTA_HIP_CHECK(hipGetLastError());
    return 0;
}
