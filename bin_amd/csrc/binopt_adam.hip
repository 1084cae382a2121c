// binopt_adam.hip (libbinopt.so, include/binopt.h) — the Adam update of the training step (torch.optim.Adam's non-capturable single-tensor path,
// torch/optim/adam.py _single_tensor_adam) for a whole parameter group in a handful of launches.
// One elementwise kernel walks a table of tensors passed BY VALUE (the idiom of score_tile_kernel<FramePairs> and the
// multi_loss kernels): no device-side table, no host-to-device copy, no allocation.  Per element, in fp32:
//     g' = g + weight_decay * p                       (skipped when weight_decay == 0)
//     m' = m + (1 - beta1) * (g' - m)
//     v' = beta2 * v + (1 - beta2) * g' * g'
//     p' = p - step_size * m' / (sqrtf(v') * inv_sqrt_bc2 + eps)
// with IEEE sqrtf and division.  step_size = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) sit in the row, computed by
// the caller in double and rounded once: t may differ between parameters (one that got its first gradient late).
// HBM-bound at 28 B per element (p, g, m, v read; p, m, v written).
// Work split (binhip_multi_tensor.h's): a workgroup owns one AD_CHUNK-element chunk of one row and finds its row by a binary search
// over the table.  So a 3-element bias costs one workgroup that exits after one predicated element, and a 221 184-element weight is
// 108 workgroups.  A row whose four pointers are all 16-byte aligned moves 16 B per lane in every whole chunk; its last, partial
// chunk, and every row with a misaligned pointer, take 4 B per lane.  Both paths load all four operands of everything a lane owns
// before their first store: the walk lives in walk_chunk, this file keeps the arithmetic, the argument checks and the entry point.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binopt.h"
#include "binhip_multi_tensor.h"

#include <math.h>

namespace {
constexpr int AD_THREADS = 256;
constexpr int AD_UNROLL = 2;                                     // float4 (or, on the scalar path, 4 single floats) per lane
constexpr int AD_CHUNK = AD_THREADS * AD_UNROLL * 4;             // 2048 elements per workgroup

using AdamTable = multi_tensor::RowTable<BinAdamTensor, BINOPT_ADAM_MAX_TENSORS>;
using AdamLaunches = multi_tensor::Launches<AD_CHUNK, 0x7fffffff>;
// the launch's arguments travel in the kernel-argument segment: keep table + scalars well under 4 KB
static_assert(sizeof(BinAdamTensor) == 48, "BinAdamTensor layout");
static_assert(sizeof(AdamTable) + 5 * sizeof(float) <= 3840, "the table must fit the by-value argument limit");
static_assert(BINOPT_E_ARG == multi_tensor::E_ARG && BINOPT_E_SHAPE == multi_tensor::E_SHAPE, "the shared checks return these");

struct AdamCoef { float w1, beta2, w2, eps, weight_decay; };     // w1 = 1 - beta1, w2 = 1 - beta2 (rounded once from double)

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamCoef& c, float step_size,
                                            float inv_sqrt_bc2) {
    if (c.weight_decay != 0.f) g = g + c.weight_decay * p;
    m = m + c.w1 * (g - m);
    v = c.beta2 * v + (c.w2 * g) * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + c.eps;
    p = p - step_size * (m / denom);
}

struct AdamElement {                                             // walk_chunk's functor over one element's {p, g, m, v}
    const AdamCoef& c;
    float step_size, inv_sqrt_bc2;
    __device__ __forceinline__ void operator()(float (&x)[4], bool) const { adam_update(x[0], x[1], x[2], x[3], c, step_size, inv_sqrt_bc2); }
};
}  // namespace

__global__ void __launch_bounds__(AD_THREADS)
adam_step_kernel(const AdamTable tab, const AdamCoef c) {
    const int row = find_row(tab);
    const BinAdamTensor& r = tab.row[row];
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[row]) * AD_CHUNK;
    multi_tensor::walk_chunk<AD_THREADS, AD_UNROLL, 0b1101>(r.numel, base, AdamElement{c, r.step_size, r.inv_sqrt_bc2}, r.p, r.g, r.m, r.v);   // p, m, v written
}

int binopt_version(void) { return BINOPT_VERSION; }

int binopt_adam_step(const BinAdamTensor* items, int n, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return BINOPT_E_ARG;   // before the rows: E_SHAPE comes last
    const int64_t total = AdamLaunches::check_rows(items, n, [](const BinAdamTensor& r) { return r.p && r.g && r.m && r.v; });
    if (total < 0) return (int)total;                            // everything is checked before anything is launched
    AdamCoef c;
    c.w1 = (float)(1.0 - multi_tensor::shortest_decimal(beta1));
    c.beta2 = beta2;
    c.w2 = (float)(1.0 - multi_tensor::shortest_decimal(beta2));
    c.eps = eps;
    c.weight_decay = weight_decay;
    hipStream_t s = (hipStream_t)stream;
    return AdamLaunches::for_each_launch<AdamTable>(items, n, [&](const AdamTable& tab, unsigned blocks) {
        hipLaunchKernelGGL(adam_step_kernel, dim3(blocks), dim3(AD_THREADS), 0, s, tab, c);
    });
}
