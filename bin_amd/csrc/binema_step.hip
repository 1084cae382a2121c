// binema_step.hip (libbinema.so, include/binema.h) — the exponential moving average of the weights (train.ema_decay) for a whole
// network in a handful of launches.  One elementwise kernel walks a table of tensors passed BY VALUE (the idiom of
// adam_step_kernel): no device-side table, no host-to-device copy, no allocation.  Per element, in fp32:
//     e' = e + w * (p - e),      w = 1 - decay (rounded once from double)
// HBM-bound at 12 B per element (e, p read; e written), and at the size of this network launch-bound: so a launch takes as many
// rows as the by-value argument limit lets it.
// Work split (binopt_adam.hip's): a workgroup owns one EM_CHUNK-element chunk of one row; the table carries the first workgroup of
// every row, and a workgroup finds its row by a binary search over those (wave-uniform: scalar loads from the kernel arguments).
// A row whose two pointers are 16-byte aligned moves 16 B per lane in every whole chunk; its last, partial chunk, and every row
// with a misaligned pointer, take 4 B per lane.  Both paths load both operands of everything a lane owns before their first store
// ("Epilogues and vmcnt"), and both compute the one expression of ema_update, so they agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binema.h"

#include <math.h>

namespace {
constexpr int EM_THREADS = 256;
constexpr int EM_UNROLL = 2;                                     // float4 (or, on the scalar path, 4 single floats) per lane
constexpr int EM_CHUNK = EM_THREADS * EM_UNROLL * 4;             // 2048 elements per workgroup

struct EmaTable {
    BinEmaTensor row[BINEMA_MAX_TENSORS];
    int first_block[BINEMA_MAX_TENSORS + 1];                     // row r owns workgroups first_block[r] .. first_block[r + 1] - 1
    int n;
};
// the launch's arguments travel in the kernel-argument segment: keep table + scalar well under 4 KB
static_assert(sizeof(BinEmaTensor) == 24, "BinEmaTensor layout");
static_assert(sizeof(EmaTable) + sizeof(float) <= 3840, "the table must fit the by-value argument limit");

__device__ __forceinline__ float ema_update(float e, float p, float w) { return e + w * (p - e); }

// The shortest decimal that rounds to the float `b` (what printing a float32 shows), as a double: binopt_adam.hip's.  A caller's
// decay = 0.9999 arrives as the float 0.99989998…, and 1 - that is off from 1e-4 by 1.7e-4 relative — far outside fp32 rounding of
// the update; the decimal the caller wrote is recovered instead.  For a float that is no short decimal this returns a double within
// half a float ulp of it.
double shortest_decimal(float b) {
    double scale = 1.0;
    for (int k = 1; k <= 9; ++k) {
        scale *= 10.0;                                           // exact in double
        const double d = nearbyint((double)b * scale) / scale;  // an integer over an exact power of ten: correctly rounded
        if ((float)d == b) return d;
    }
    return (double)b;
}
}  // namespace

__global__ void __launch_bounds__(EM_THREADS)
ema_step_kernel(const EmaTable tab, const float w) {
    // the row of this workgroup: largest r with first_block[r] <= blockIdx.x  (first_block[0] = 0, first_block[n] = gridDim.x)
    int lo = 0, hi = tab.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const BinEmaTensor& r = tab.row[lo];
    float* __restrict__ E = r.e;
    const float* __restrict__ P = r.p;
    const int64_t numel = r.numel;
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[lo]) * EM_CHUNK;
    const int t = threadIdx.x;
    const bool aligned = ((((uintptr_t)E | (uintptr_t)P) & 15) == 0);   // wave-uniform

    if (aligned && base + EM_CHUNK <= numel) {                   // a whole chunk of an aligned row: 16 B per lane, nothing predicated
        float4 e[EM_UNROLL], p[EM_UNROLL];
#pragma unroll
        for (int k = 0; k < EM_UNROLL; ++k) {
            const int64_t i = base + 4 * (k * EM_THREADS + t);
            e[k] = *(const float4*)(E + i);
            p[k] = *(const float4*)(P + i);
        }
#pragma unroll
        for (int k = 0; k < EM_UNROLL; ++k) {
            e[k].x = ema_update(e[k].x, p[k].x, w);
            e[k].y = ema_update(e[k].y, p[k].y, w);
            e[k].z = ema_update(e[k].z, p[k].z, w);
            e[k].w = ema_update(e[k].w, p[k].w, w);
        }
#pragma unroll
        for (int k = 0; k < EM_UNROLL; ++k) {
            const int64_t i = base + 4 * (k * EM_THREADS + t);
            *(float4*)(E + i) = e[k];
        }
    } else {
        // 4 B per lane, consecutive lanes on consecutive floats: a row with a misaligned pointer, and the last, partial chunk of
        // every row.  The loads are not predicated (a lane past the end re-reads the row's last element, numel >= 1), so all of
        // them are in flight at once; only the stores are.
        constexpr int U = EM_UNROLL * 4;
        float e[U], p[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t i = min(base + k * EM_THREADS + t, numel - 1);
            e[k] = E[i]; p[k] = P[i];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) e[k] = ema_update(e[k], p[k], w);
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t i = base + k * EM_THREADS + t;
            if (i < numel) E[i] = e[k];
        }
    }
}

int binema_version(void) { return BINEMA_VERSION; }

int binema_step(const BinEmaTensor* items, int n, float decay, void* stream) {
    if (n < 0 || (n > 0 && !items)) return BINEMA_E_ARG;
    if (!(decay >= 0.f && decay < 1.f)) return BINEMA_E_ARG;
    const int64_t max_blocks = 0x7fffffff;
    for (int i = 0; i < n; ++i) {                                // everything is checked before anything is launched
        if (!items[i].e || !items[i].p || items[i].numel < 1) return BINEMA_E_ARG;
        if ((items[i].numel - 1) / EM_CHUNK + 1 > max_blocks) return BINEMA_E_SHAPE;
    }
    const float w = (float)(1.0 - shortest_decimal(decay));
    hipStream_t s = (hipStream_t)stream;
    int i = 0;
    while (i < n) {                                              // launches of at most BINEMA_MAX_TENSORS rows
        EmaTable tab;
        int64_t blocks = 0;
        int k = 0;
        for (; k < BINEMA_MAX_TENSORS && i + k < n; ++k) {
            const int64_t nb = (items[i + k].numel - 1) / EM_CHUNK + 1;
            if (blocks + nb > max_blocks) break;                 // the rest goes into the next launch
            tab.row[k] = items[i + k];
            tab.first_block[k] = (int)blocks;
            blocks += nb;
        }
        for (int j = k; j <= BINEMA_MAX_TENSORS; ++j) tab.first_block[j] = (int)blocks;
        for (int j = k; j < BINEMA_MAX_TENSORS; ++j) tab.row[j] = BinEmaTensor{};
        tab.n = k;
        hipLaunchKernelGGL(ema_step_kernel, dim3((unsigned)blocks), dim3(EM_THREADS), 0, s, tab, w);
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return (int)err;
        i += k;
    }
    return 0;
}
