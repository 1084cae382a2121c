// binens.hip (libbinens.so, include/binens.h) — the two streaming kernels of the test-time self-ensemble (bin_amd/ensemble.py):
//   ens_orient_kernel : one read of a frame, up to 8 flipped copies of it written (the oriented inputs of the network);
//   ens_merge_kernel  : M network outputs un-flipped on the fly, summed as a balanced pairwise tree and scaled by 1/M.
// Both are HBM-bound element-wise kernels with an index map: no LDS, no reuse.  Items (a handful of pointers each) travel BY VALUE
// in the kernel-argument segment; blockIdx.y picks the item, blockIdx.x grid-strides over its elements with 64-bit indices.
// Data paths: an item whose pointers are all 16-byte aligned, at W % 4 == 0, moves float4s — the mirror image of the float4 at
// column x is the float4 at column W-4-x, aligned too, with its components reversed in registers; any other item moves single
// floats.  Both paths apply the same index map and the same adds in the same order, so they agree bit for bit.
// The adds and the scale are written with the rounding intrinsics: nothing may be contracted or re-associated, the order of the
// tree is the contract (binens.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binens.h"

namespace {
constexpr int ENS_THREADS = 256;
constexpr int64_t ENS_MAX_BLOCKS = 2048;                         // per launch, over all items (8 workgroups per CU); beyond that blocks stride
constexpr int64_t ENS_MAX_ELEMS = (int64_t)1 << 40;

struct OrientItem {                                              // BinEnsOrient with its flips packed, 8 bits each, into one word
    const float* src;
    float* dst[BINENS_MAX_ORIENT];
    uint64_t flips;
    int32_t n_dst;
};
struct OrientTable {
    OrientItem item[BINENS_MAX_SOURCES];
    uint32_t vec_mask;                                           // bit i: item i takes the 16 B path
};
struct MergeTable {
    BinEnsMerge item[BINENS_MAX_SLOTS];
    uint8_t flip_of[BINENS_MAX_ORIENT];
    uint32_t vec_mask;
};
static_assert(sizeof(BinEnsOrient) == 88, "BinEnsOrient layout");
static_assert(sizeof(BinEnsMerge) == 72, "BinEnsMerge layout");
static_assert(sizeof(OrientTable) + 16 <= 3840 && sizeof(MergeTable) + 16 <= 3840, "the tables must fit the by-value argument limit");

// v, or v with its components reversed: the float4 as it reads in a row mirrored along W (component selects: nothing is indexed)
__device__ __forceinline__ float4 reversed_if(bool rev, float4 v) {
    return make_float4(rev ? v.w : v.x, rev ? v.z : v.y, rev ? v.y : v.z, rev ? v.x : v.w);
}

// Where unit `u` (a float on the 4 B path with Wu = W, a float4 on the 16 B path with Wu = W / 4) goes under a flip: u + dx when
// mirrored along W, + dy when mirrored along H.  The (row, column) split is taken once per unit, whatever the number of flips; the
// map is its own inverse.  Tensors below 2^31 units (all but the largest) divide in 32 bits.
struct Mirror {
    int64_t u, dx, dy;
    __device__ __forceinline__ Mirror(int64_t u_, int H, int Wu, bool small) : u(u_) {
        int x, y;
        if (small) {
            const uint32_t row = (uint32_t)u_ / (uint32_t)Wu;
            x = (int)((uint32_t)u_ - row * (uint32_t)Wu);
            y = (int)(row % (uint32_t)H);
        } else {
            const int64_t row = u_ / Wu;
            x = (int)(u_ - row * Wu);
            y = (int)(row % H);
        }
        dx = Wu - 1 - 2 * x;
        dy = (int64_t)(H - 1 - 2 * y) * Wu;
    }
    __device__ __forceinline__ int64_t at(unsigned flip) const {
        return u + ((flip & BINENS_FLIP_W) ? dx : 0) + ((flip & BINENS_FLIP_H) ? dy : 0);
    }
};

template <int M> __device__ __forceinline__ float tree_mean(float (&x)[M]) {
#pragma unroll
    for (int m = M; m > 1; m >>= 1)
#pragma unroll
        for (int i = 0; i < m / 2; ++i) x[i] = __fadd_rn(x[2 * i], x[2 * i + 1]);
    return __fmul_rn(x[0], 1.0f / M);
}
}  // namespace

__global__ void __launch_bounds__(ENS_THREADS)
ens_orient_kernel(const OrientTable tab, const int64_t total, const int H, const int W) {
    const OrientItem& it = tab.item[blockIdx.y];
    const int nd = it.n_dst;
    const uint64_t flips = it.flips;
    const int64_t stride = (int64_t)gridDim.x * ENS_THREADS;
    const bool small = total < ((int64_t)1 << 31);
    if ((tab.vec_mask >> blockIdx.y) & 1u) {
        const int W4 = W >> 2;
        const int64_t units = total >> 2;                        // W % 4 == 0: total is a multiple of 4
        const float4* __restrict__ src = reinterpret_cast<const float4*>(it.src);
        for (int64_t u = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x; u < units; u += stride) {
            const float4 v = src[u];
            const Mirror m(u, H, W4, small);
#pragma unroll
            for (int j = 0; j < BINENS_MAX_ORIENT; ++j)          // (a constant trip count: the item stays in the argument segment)
                if (j < nd) {
                    const unsigned f = (unsigned)(flips >> (8 * j)) & 3u;
                    reinterpret_cast<float4*>(it.dst[j])[m.at(f)] = reversed_if(f & BINENS_FLIP_W, v);
                }
        }
    } else {
        for (int64_t e = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x; e < total; e += stride) {
            const float v = it.src[e];
            const Mirror m(e, H, W, small);
#pragma unroll
            for (int j = 0; j < BINENS_MAX_ORIENT; ++j)
                if (j < nd) it.dst[j][m.at((unsigned)(flips >> (8 * j)) & 3u)] = v;
        }
    }
}

template <int M>
__global__ void __launch_bounds__(ENS_THREADS)
ens_merge_kernel(const MergeTable tab, const int64_t total, const int H, const int W) {
    const BinEnsMerge& it = tab.item[blockIdx.y];
    const int64_t stride = (int64_t)gridDim.x * ENS_THREADS;
    const bool small = total < ((int64_t)1 << 31);
    if ((tab.vec_mask >> blockIdx.y) & 1u) {
        const int W4 = W >> 2;
        const int64_t units = total >> 2;
        for (int64_t u = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x; u < units; u += stride) {
            const Mirror m(u, H, W4, small);
            float4 v[M];
#pragma unroll
            for (int o = 0; o < M; ++o)                          // all M loads in flight before the first add
                v[o] = reinterpret_cast<const float4*>(it.src[o])[m.at(tab.flip_of[o])];
            float a[M], b[M], c[M], d[M];
#pragma unroll
            for (int o = 0; o < M; ++o) {
                const float4 t = reversed_if(tab.flip_of[o] & BINENS_FLIP_W, v[o]);
                a[o] = t.x; b[o] = t.y; c[o] = t.z; d[o] = t.w;
            }
            reinterpret_cast<float4*>(it.dst)[u] = make_float4(tree_mean<M>(a), tree_mean<M>(b), tree_mean<M>(c), tree_mean<M>(d));
        }
    } else {
        for (int64_t e = (int64_t)blockIdx.x * ENS_THREADS + threadIdx.x; e < total; e += stride) {
            const Mirror m(e, H, W, small);
            float x[M];
#pragma unroll
            for (int o = 0; o < M; ++o) x[o] = it.src[o][m.at(tab.flip_of[o])];
            it.dst[e] = tree_mean<M>(x);
        }
    }
}

namespace {
struct Range { uintptr_t lo; bool written; };

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// E_ARG when a written buffer overlaps any other buffer of the call (every buffer is `bytes` long)
bool overlap(const Range* r, int n, uintptr_t bytes) {
    for (int i = 0; i < n; ++i) {
        if (!r[i].written) continue;
        for (int j = 0; j < n; ++j)
            if (j != i && r[i].lo < r[j].lo + bytes && r[j].lo < r[i].lo + bytes) return true;
    }
    return false;
}

int check_shape(int planes, int H, int W, int64_t* total) {
    if (planes < 1 || H < 1 || W < 1) return BINENS_E_ARG;
    const int64_t rows = (int64_t)planes * H;                    // < 2^62
    if (rows > ENS_MAX_ELEMS / W) return BINENS_E_SHAPE;         // rows * W would pass 2^40
    *total = rows * W;
    return 0;
}

// the grid is sized from the element count: one lane per float4 when every item takes the 16 B path, one per float otherwise (a
// 16 B item in such a mixed launch simply leaves its later blocks idle), capped where a block starts to stride
dim3 grid_for(int64_t total, bool all_vec, int n) {
    const int64_t units = all_vec ? total / 4 : total;
    const int64_t blocks = (units + ENS_THREADS - 1) / ENS_THREADS;
    const int64_t cap = ENS_MAX_BLOCKS / n > 0 ? ENS_MAX_BLOCKS / n : 1;
    return dim3((unsigned)(blocks < cap ? blocks : cap), (unsigned)n);
}
}  // namespace

int binens_version(void) { return BINENS_VERSION; }

int binens_orient(const BinEnsOrient* items, int n, int planes, int H, int W, void* stream) {
    if (n < 0 || n > BINENS_MAX_SOURCES || (n > 0 && !items)) return BINENS_E_ARG;
    int64_t total = 0;
    if (int rc = check_shape(planes, H, W, &total)) return rc;
    if (n == 0) return 0;
    OrientTable tab = {};
    Range ranges[BINENS_MAX_SOURCES * (BINENS_MAX_ORIENT + 1)];
    int nr = 0, n_vec = 0;
    for (int i = 0; i < n; ++i) {
        const BinEnsOrient& it = items[i];
        if (!it.src || !aligned(it.src, 4) || it.n_dst < 1 || it.n_dst > BINENS_MAX_ORIENT) return BINENS_E_ARG;
        bool vec = (W % 4 == 0) && aligned(it.src, 16);
        ranges[nr++] = Range{(uintptr_t)it.src, false};
        tab.item[i].src = it.src;
        tab.item[i].n_dst = it.n_dst;
        for (int j = 0; j < it.n_dst; ++j) {
            if (!it.dst[j] || !aligned(it.dst[j], 4) || (it.flip[j] & ~(BINENS_FLIP_W | BINENS_FLIP_H))) return BINENS_E_ARG;
            vec = vec && aligned(it.dst[j], 16);
            ranges[nr++] = Range{(uintptr_t)it.dst[j], true};
            tab.item[i].dst[j] = it.dst[j];
            tab.item[i].flips |= (uint64_t)it.flip[j] << (8 * j);
        }
        if (vec) { tab.vec_mask |= 1u << i; ++n_vec; }
    }
    if (overlap(ranges, nr, (uintptr_t)total * 4)) return BINENS_E_ARG;
    hipLaunchKernelGGL(ens_orient_kernel, grid_for(total, n_vec == n, n), dim3(ENS_THREADS), 0, (hipStream_t)stream,
                       tab, total, H, W);
    return (int)hipGetLastError();
}

int binens_merge(const BinEnsMerge* items, int n, int M, const uint8_t* flip_of, int planes, int H, int W, void* stream) {
    if (n < 0 || n > BINENS_MAX_SLOTS || (n > 0 && !items)) return BINENS_E_ARG;
    if ((M != 1 && M != 2 && M != 4 && M != 8) || !flip_of) return BINENS_E_ARG;
    int64_t total = 0;
    if (int rc = check_shape(planes, H, W, &total)) return rc;
    MergeTable tab = {};
    for (int o = 0; o < M; ++o) {
        if (flip_of[o] & ~(BINENS_FLIP_W | BINENS_FLIP_H)) return BINENS_E_ARG;
        tab.flip_of[o] = flip_of[o];
    }
    if (n == 0) return 0;
    Range ranges[BINENS_MAX_SLOTS * (BINENS_MAX_ORIENT + 1)];
    int nr = 0, n_vec = 0;
    for (int i = 0; i < n; ++i) {
        const BinEnsMerge& it = items[i];
        if (!it.dst || !aligned(it.dst, 4)) return BINENS_E_ARG;
        bool vec = (W % 4 == 0) && aligned(it.dst, 16);
        ranges[nr++] = Range{(uintptr_t)it.dst, true};
        tab.item[i].dst = it.dst;
        for (int o = 0; o < M; ++o) {
            if (!it.src[o] || !aligned(it.src[o], 4)) return BINENS_E_ARG;
            vec = vec && aligned(it.src[o], 16);
            ranges[nr++] = Range{(uintptr_t)it.src[o], false};
            tab.item[i].src[o] = it.src[o];
        }
        if (vec) { tab.vec_mask |= 1u << i; ++n_vec; }
    }
    if (overlap(ranges, nr, (uintptr_t)total * 4)) return BINENS_E_ARG;
    const dim3 grid = grid_for(total, n_vec == n, n), block(ENS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    switch (M) {
    case 1: hipLaunchKernelGGL(ens_merge_kernel<1>, grid, block, 0, s, tab, total, H, W); break;
    case 2: hipLaunchKernelGGL(ens_merge_kernel<2>, grid, block, 0, s, tab, total, H, W); break;
    case 4: hipLaunchKernelGGL(ens_merge_kernel<4>, grid, block, 0, s, tab, total, H, W); break;
    default: hipLaunchKernelGGL(ens_merge_kernel<8>, grid, block, 0, s, tab, total, H, W); break;
    }
    return (int)hipGetLastError();
}
