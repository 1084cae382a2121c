// binema_step.hip (libbinema.so, include/binema.h) — the exponential moving average of the weights (train.ema_decay) for a whole
// network in a handful of launches.  One elementwise kernel walks a table of tensors passed BY VALUE (the idiom of
// adam_step_kernel): no device-side table, no host-to-device copy, no allocation.  Per element, in fp32:
//     e' = e + w * (p - e),      w = 1 - decay (rounded once from double)
// HBM-bound at 12 B per element (e, p read; e written), and at the size of this network launch-bound: so a launch takes as many
// rows as the by-value argument limit lets it.
// Work split (binhip_multi_tensor.h's): a workgroup owns one EM_CHUNK-element chunk of one row and finds its row by a binary search
// over the table.  A row whose two pointers are 16-byte aligned moves 16 B per lane in every whole chunk; its last, partial chunk,
// and every row with a misaligned pointer, take 4 B per lane.  Both paths load both operands of everything a lane owns before their
// first store, and both compute the one expression of ema_update, so they agree bit for bit: the walk lives in walk_chunk, this file
// keeps the arithmetic, the argument checks and the entry point.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binema.h"
#include "binhip_multi_tensor.h"

#include <math.h>

namespace {
constexpr int EM_THREADS = 256;
constexpr int EM_UNROLL = 2;                                     // float4 (or, on the scalar path, 4 single floats) per lane
constexpr int EM_CHUNK = EM_THREADS * EM_UNROLL * 4;             // 2048 elements per workgroup

using EmaTable = multi_tensor::RowTable<BinEmaTensor, BINEMA_MAX_TENSORS>;
using EmaLaunches = multi_tensor::Launches<EM_CHUNK, 0x7fffffff>;
// the launch's arguments travel in the kernel-argument segment: keep table + scalar well under 4 KB
static_assert(sizeof(BinEmaTensor) == 24, "BinEmaTensor layout");
static_assert(sizeof(EmaTable) + sizeof(float) <= 3840, "the table must fit the by-value argument limit");
static_assert(BINEMA_E_ARG == multi_tensor::E_ARG && BINEMA_E_SHAPE == multi_tensor::E_SHAPE, "the shared checks return these");

__device__ __forceinline__ float ema_update(float e, float p, float w) { return e + w * (p - e); }

struct EmaElement {                                              // walk_chunk's functor over one element's {e, p}
    float w;
    __device__ __forceinline__ void operator()(float (&x)[2], bool) const { x[0] = ema_update(x[0], x[1], w); }
};
}  // namespace

__global__ void __launch_bounds__(EM_THREADS)
ema_step_kernel(const EmaTable tab, const float w) {
    const int row = find_row(tab);
    const BinEmaTensor& r = tab.row[row];
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[row]) * EM_CHUNK;
    multi_tensor::walk_chunk<EM_THREADS, EM_UNROLL, 0b01>(r.numel, base, EmaElement{w}, r.e, r.p);   // e written
}

int binema_version(void) { return BINEMA_VERSION; }

int binema_step(const BinEmaTensor* items, int n, float decay, void* stream) {
    // A decay = 0.9999 arrives as the float 0.99989998…, and 1 - that is off from 1e-4 by 1.7e-4 relative: w comes from the decimal
    // the caller wrote.
    if (!(decay >= 0.f && decay < 1.f)) return BINEMA_E_ARG;     // before the rows: E_SHAPE comes last
    const int64_t total = EmaLaunches::check_rows(items, n, [](const BinEmaTensor& r) { return r.e && r.p; });
    if (total < 0) return (int)total;                            // everything is checked before anything is launched
    const float w = (float)(1.0 - multi_tensor::shortest_decimal(decay));
    hipStream_t s = (hipStream_t)stream;
    return EmaLaunches::for_each_launch<EmaTable>(items, n, [&](const EmaTable& tab, unsigned blocks) {
        hipLaunchKernelGGL(ema_step_kernel, dim3(blocks), dim3(EM_THREADS), 0, s, tab, w);
    });
}
