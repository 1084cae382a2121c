// bingrad_norm.hip (libbingrad.so, include/bingrad.h) — the gradient guard of the training step: the global L2 norm of all
// gradients, the clip coefficient of torch.nn.utils.clip_grad_norm_ and the in-place scale, for a whole parameter set in a handful
// of launches and without a host round trip.
// The rows travel BY VALUE (the idiom of adam_step_kernel, binopt_adam.hip): no device-side table, no copy, no allocation.
//   grad_sumsq_kernel  a workgroup owns one GN_CHUNK-element chunk of one row; the table carries the first workgroup of every row and
//                      a workgroup finds its row by a binary search over those (wave-uniform: loads from the kernel arguments).  Each
//                      element is converted to double, squared (exact: 24 x 24 bits) and accumulated in double; the lanes' sums are
//                      reduced within the wave by shuffles, across the waves through LDS, both in a fixed order, and lane 0 stores the
//                      workgroup's sum to ITS slot of the workspace.  Nothing is accumulated across workgroups here, so the result does
//                      not depend on the order in which workgroups run.
//   grad_final_kernel  one workgroup sums the slots in a fixed order (lane t takes slots t, t + 256, ...; then a tree through LDS),
//                      reads the status word and writes the 32-byte record.
//   grad_scale_kernel  the work split of the first kernel; reads coef from the record on the device, returns when it is exactly 1.0f,
//                      otherwise g *= coef in fp32, everything a lane owns loaded before its first store ("Epilogues and
//                      vmcnt").
// A row whose pointer is 16-byte aligned moves 16 B per lane in every whole chunk; its last, partial chunk, and every row with a
// misaligned pointer (the gradients of FlatGradAllReduce are views at any 4-byte offset), take 4 B per lane with clamped, unpredicated
// loads.  HBM-bound: 4 B read per element for the norm, 8 B for a scale that clips.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bingrad.h"

#include <math.h>

namespace {
constexpr int GN_THREADS = 256;
constexpr int GN_UNROLL = 4;                                     // float4 (or, on the scalar path, 4 single floats) per lane
constexpr int GN_CHUNK = GN_THREADS * GN_UNROLL * 4;             // 4096 elements = 16 KB per workgroup, 64 B in flight per lane
constexpr int GN_WAVES = GN_THREADS / 64;
constexpr int64_t GN_MAX_BLOCKS = (1 << 24) - 1;                 // workgroups per launch: 256 x that many threads stay below 2^32 in a grid

struct GradTable {
    BinGradTensor row[BINGRAD_MAX_TENSORS];
    int first_block[BINGRAD_MAX_TENSORS + 1];                    // row r owns workgroups first_block[r] .. first_block[r + 1] - 1
    int n;
};
// the launch's arguments travel in the kernel-argument segment: keep table + scalars well under 4 KB
static_assert(sizeof(BinGradTensor) == 16, "BinGradTensor layout");
static_assert(sizeof(BinGradRecord) == 32 && offsetof(BinGradRecord, flags) == 16, "BinGradRecord layout");
static_assert(sizeof(GradTable) + 4 * sizeof(void*) <= 3072, "the table must fit the by-value argument limit");

// the row of this workgroup: largest r with first_block[r] <= blockIdx.x  (first_block[0] = 0, first_block[n] = gridDim.x)
__device__ __forceinline__ int find_row(const GradTable& tab) {
    int lo = 0, hi = tab.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double square_add(float x, double acc) {
    const double d = (double)x;
    return fma(d, d, acc);                                       // the product of two converted floats is exact in double
}

int64_t chunks_of(int64_t numel) { return (numel + GN_CHUNK - 1) / GN_CHUNK; }

// -1 / -2 for a bad table, else the number of workgroups (= workspace slots) all rows take
int64_t check_rows(const BinGradTensor* items, int n) {
    if (n < 0 || (n > 0 && !items)) return BINGRAD_E_ARG;
    int64_t total = 0;
    for (int i = 0; i < n; ++i) {
        if (!items[i].g || items[i].numel < 1) return BINGRAD_E_ARG;
        if (chunks_of(items[i].numel) > GN_MAX_BLOCKS) return BINGRAD_E_SHAPE;
        total += chunks_of(items[i].numel);
    }
    return total;
}

// rows [i, i + k) into `tab`, as many as one launch takes; returns k and the launch's workgroup count
int fill_table(GradTable& tab, const BinGradTensor* items, int i, int n, int64_t& blocks) {
    blocks = 0;
    int k = 0;
    for (; k < BINGRAD_MAX_TENSORS && i + k < n; ++k) {
        const int64_t nb = chunks_of(items[i + k].numel);
        if (blocks + nb > GN_MAX_BLOCKS) break;                       // the rest goes into the next launch
        tab.row[k] = items[i + k];
        tab.first_block[k] = (int)blocks;
        blocks += nb;
    }
    for (int j = k; j <= BINGRAD_MAX_TENSORS; ++j) tab.first_block[j] = (int)blocks;
    for (int j = k; j < BINGRAD_MAX_TENSORS; ++j) tab.row[j] = BinGradTensor{};
    tab.n = k;
    return k;
}
}  // namespace

__global__ void __launch_bounds__(GN_THREADS)
grad_sumsq_kernel(const GradTable tab, double* __restrict__ slots) {
    const int row = find_row(tab);
    const float* __restrict__ G = tab.row[row].g;
    const int64_t numel = tab.row[row].numel;
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[row]) * GN_CHUNK;
    const int t = threadIdx.x;
    double acc = 0.0;
    if ((((uintptr_t)G) & 15) == 0 && base + GN_CHUNK <= numel) { // a whole chunk of an aligned row: 16 B per lane, nothing predicated
        float4 g[GN_UNROLL];
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) g[k] = *(const float4*)(G + base + 4 * (k * GN_THREADS + t));
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) {
            acc = square_add(g[k].x, acc);
            acc = square_add(g[k].y, acc);
            acc = square_add(g[k].z, acc);
            acc = square_add(g[k].w, acc);
        }
    } else {
        // 4 B per lane, consecutive lanes on consecutive floats.  The loads are not predicated (a lane past the end re-reads the row's
        // last element, numel >= 1), so all of them are in flight at once; what a lane past the end read is dropped by a select.
        constexpr int U = GN_UNROLL * 4;
        float g[U];
#pragma unroll
        for (int k = 0; k < U; ++k) g[k] = G[min(base + k * GN_THREADS + t, numel - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k) acc = (base + k * GN_THREADS + t < numel) ? square_add(g[k], acc) : acc;
    }
    // lanes of a wave: a shuffle tree, the same pairs every run
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double wave_sum[GN_WAVES];
    if ((t & 63) == 0) wave_sum[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double s = wave_sum[0];
#pragma unroll
        for (int w = 1; w < GN_WAVES; ++w) s += wave_sum[w];
        slots[blockIdx.x] = s;
    }
}

__global__ void __launch_bounds__(GN_THREADS)
grad_final_kernel(const double* __restrict__ slots, int64_t n_slots, float max_norm, const uint32_t* __restrict__ status_word,
                  uint32_t status_mask, BinGradRecord* __restrict__ record) {
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int64_t i = t; i < n_slots; i += GN_THREADS) acc += slots[i];
    __shared__ double part[GN_THREADS];
    part[t] = acc;
    __syncthreads();
    for (int s = GN_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) part[t] += part[t + s];
        __syncthreads();
    }
    if (t == 0) {
        const double sumsq = part[0];
        const double norm = sqrt(sumsq);
        const uint32_t status = status_word ? (*status_word & status_mask) : 0u;
        const bool bad = !isfinite(sumsq);
        float coef = 1.0f;
        if (max_norm != 0.f && !bad) coef = (float)fmin(1.0, (double)max_norm / (norm + 1e-6));
        BinGradRecord r;
        r.sumsq = sumsq;
        r.norm = (float)norm;
        r.coef = coef;
        r.flags = (bad ? BINGRAD_FLAG_NONFINITE : 0) | (status ? BINGRAD_FLAG_STATUS : 0);
        r.status = status;
        r.reserved[0] = r.reserved[1] = 0;
        *record = r;
    }
}

__global__ void __launch_bounds__(GN_THREADS)
grad_scale_kernel(const GradTable tab, const BinGradRecord* __restrict__ record) {
    const float coef = record->coef;                             // uniform over the grid
    if (coef == 1.0f) return;                                    // not clipped (or not finite): nothing is written
    const int row = find_row(tab);
    float* __restrict__ G = tab.row[row].g;
    const int64_t numel = tab.row[row].numel;
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[row]) * GN_CHUNK;
    const int t = threadIdx.x;
    if ((((uintptr_t)G) & 15) == 0 && base + GN_CHUNK <= numel) {
        float4 g[GN_UNROLL];
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) g[k] = *(const float4*)(G + base + 4 * (k * GN_THREADS + t));
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) {
            g[k].x *= coef; g[k].y *= coef; g[k].z *= coef; g[k].w *= coef;
        }
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) *(float4*)(G + base + 4 * (k * GN_THREADS + t)) = g[k];
    } else {
        constexpr int U = GN_UNROLL * 4;
        float g[U];
#pragma unroll
        for (int k = 0; k < U; ++k) g[k] = G[min(base + k * GN_THREADS + t, numel - 1)];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t e = base + k * GN_THREADS + t;
            if (e < numel) G[e] = g[k] * coef;
        }
    }
}

int bingrad_version(void) { return BINGRAD_VERSION; }

int64_t bingrad_norm_workspace_bytes(const BinGradTensor* items, int n) {
    const int64_t total = check_rows(items, n);
    if (total < 0) return total;
    return (int64_t)sizeof(double) * (total > 0 ? total : 1);
}

int bingrad_norm(const BinGradTensor* items, int n, float max_norm, const uint32_t* status_word, uint32_t status_mask, void* workspace,
                 BinGradRecord* record, void* stream) {
    const int64_t total = check_rows(items, n);                  // everything is checked before anything is launched
    if (total < 0) return (int)total;
    if (!(max_norm >= 0.f) || !workspace || !record) return BINGRAD_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    double* slots = (double*)workspace;
    int64_t slot = 0;
    int i = 0;
    while (i < n) {                                              // launches of at most BINGRAD_MAX_TENSORS rows, disjoint slots
        GradTable tab;
        int64_t blocks = 0;
        const int k = fill_table(tab, items, i, n, blocks);
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, s, tab, slots + slot);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        slot += blocks;
        i += k;
    }
    hipLaunchKernelGGL(grad_final_kernel, dim3(1), dim3(GN_THREADS), 0, s, (const double*)slots, slot, max_norm, status_word, status_mask,
                       record);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int bingrad_scale(const BinGradTensor* items, int n, const BinGradRecord* record, void* stream) {
    const int64_t total = check_rows(items, n);
    if (total < 0) return (int)total;
    if (!record) return BINGRAD_E_ARG;
    hipStream_t s = (hipStream_t)stream;
    int i = 0;
    while (i < n) {
        GradTable tab;
        int64_t blocks = 0;
        const int k = fill_table(tab, items, i, n, blocks);
        hipLaunchKernelGGL(grad_scale_kernel, dim3((unsigned)blocks), dim3(GN_THREADS), 0, s, tab, record);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        i += k;
    }
    return 0;
}
