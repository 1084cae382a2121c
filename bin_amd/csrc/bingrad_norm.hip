// bingrad_norm.hip (libbingrad.so, include/bingrad.h) — the gradient guard of the training step: the global L2 norm of all
// gradients, the clip coefficient of torch.nn.utils.clip_grad_norm_ and the in-place scale, for a whole parameter set in a handful
// of launches and without a host round trip.
// The rows travel BY VALUE and the work split is binhip_multi_tensor.h's: the table, the row search, the launch packing and the
// two-path chunk walk (walk_chunk) live there; this file keeps the arithmetic, the reductions, the argument checks and the entry points.
//   grad_sumsq_kernel  a workgroup owns one GN_CHUNK-element chunk of one row and finds its row by a binary search over the table.  Each
//                      element is converted to double, squared (exact: 24 x 24 bits) and accumulated in double; the lanes' sums are
//                      reduced within the wave by shuffles, across the waves through LDS, both in a fixed order, and lane 0 stores the
//                      workgroup's sum to ITS slot of the workspace.  Nothing is accumulated across workgroups here, so the result does
//                      not depend on the order in which workgroups run.
//   grad_final_kernel  one workgroup sums the slots in a fixed order (lane t takes slots t, t + 256, ...; then a tree through LDS),
//                      reads the status word and writes the 32-byte record.
//   grad_scale_kernel  the work split of the first kernel; reads coef from the record on the device, returns when it is exactly 1.0f,
//                      otherwise g *= coef in fp32, everything a lane owns loaded before its first store.
// A row whose pointer is 16-byte aligned moves 16 B per lane in every whole chunk; its last, partial chunk, and every row with a
// misaligned pointer (the gradients of FlatGradAllReduce are views at any 4-byte offset), take 4 B per lane with clamped, unpredicated
// loads.  HBM-bound: 4 B read per element for the norm, 8 B for a scale that clips.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/bingrad.h"
#include "binhip_multi_tensor.h"

#include <math.h>

namespace {
constexpr int GN_THREADS = 256;
constexpr int GN_UNROLL = 4;                                     // float4 (or, on the scalar path, 4 single floats) per lane
constexpr int GN_CHUNK = GN_THREADS * GN_UNROLL * 4;             // 4096 elements = 16 KB per workgroup, 64 B in flight per lane
constexpr int GN_WAVES = GN_THREADS / 64;
constexpr int64_t GN_MAX_BLOCKS = (1 << 24) - 1;                 // workgroups per launch: 256 x that many threads stay below 2^32 in a grid

using GradTable = multi_tensor::RowTable<BinGradTensor, BINGRAD_MAX_TENSORS>;
using GradLaunches = multi_tensor::Launches<GN_CHUNK, GN_MAX_BLOCKS>;
// the launch's arguments travel in the kernel-argument segment: keep table + scalars well under 4 KB
static_assert(sizeof(BinGradTensor) == 16, "BinGradTensor layout");
static_assert(sizeof(BinGradRecord) == 32 && offsetof(BinGradRecord, flags) == 16, "BinGradRecord layout");
static_assert(sizeof(GradTable) + 4 * sizeof(void*) <= 3072, "the table must fit the by-value argument limit");
static_assert(BINGRAD_E_ARG == multi_tensor::E_ARG && BINGRAD_E_SHAPE == multi_tensor::E_SHAPE, "the shared checks return these");

__device__ __forceinline__ double square_add(float x, double acc) {
    const double d = (double)x;
    return fma(d, d, acc);                                       // the product of two converted floats is exact in double
}

struct SquareAdd {                                               // walk_chunk's functor: what a lane past the end read is dropped by a select
    double& acc;
    __device__ __forceinline__ void operator()(float (&x)[1], bool valid) const { acc = valid ? square_add(x[0], acc) : acc; }
};

struct Scale {
    float coef;
    __device__ __forceinline__ void operator()(float (&x)[1], bool) const { x[0] *= coef; }
};

// -1 / -2 for a bad table, else the number of workgroups (= workspace slots) all rows take
int64_t check_rows(const BinGradTensor* items, int n) {
    return GradLaunches::check_rows(items, n, [](const BinGradTensor& r) { return r.g != nullptr; });
}
}  // namespace

__global__ void __launch_bounds__(GN_THREADS)
grad_sumsq_kernel(const GradTable tab, double* __restrict__ slots) {
    const int row = find_row(tab);
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[row]) * GN_CHUNK;
    const int t = threadIdx.x;
    double acc = 0.0;
    multi_tensor::walk_chunk<GN_THREADS, GN_UNROLL, 0>(tab.row[row].numel, base, SquareAdd{acc}, tab.row[row].g);   // nothing written
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
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[row]) * GN_CHUNK;
    multi_tensor::walk_chunk<GN_THREADS, GN_UNROLL, 0b1>(tab.row[row].numel, base, Scale{coef}, tab.row[row].g);   // g written
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
    int64_t slot = 0;                                            // launches of at most BINGRAD_MAX_TENSORS rows, disjoint slots
    const int rc = GradLaunches::for_each_launch<GradTable>(items, n, [&](const GradTable& tab, unsigned blocks) {
        hipLaunchKernelGGL(grad_sumsq_kernel, dim3(blocks), dim3(GN_THREADS), 0, s, tab, slots + slot);
        slot += blocks;
    });
    if (rc != 0) return rc;
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
    return GradLaunches::for_each_launch<GradTable>(items, n, [&](const GradTable& tab, unsigned blocks) {
        hipLaunchKernelGGL(grad_scale_kernel, dim3(blocks), dim3(GN_THREADS), 0, s, tab, record);
    });
}
