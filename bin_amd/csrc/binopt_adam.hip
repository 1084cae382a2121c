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
// Work split: a workgroup owns one AD_CHUNK-element chunk of one row; the table carries the first workgroup of every row, and a
// workgroup finds its row by a binary search over those (wave-uniform: scalar loads from the kernel arguments).  So a 3-element
// bias costs one workgroup that exits after one predicated element, and a 221 184-element weight is 108 workgroups.
// A row whose four pointers are all 16-byte aligned moves 16 B per lane in every whole chunk; its last, partial chunk, and every
// row with a misaligned pointer (the gradients of FlatGradAllReduce are views at any 4-byte offset), take 4 B per lane.  Both
// paths load all four operands of everything a lane owns before their first store ("Epilogues and vmcnt").
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binopt.h"

#include <math.h>

namespace {
constexpr int AD_THREADS = 256;
constexpr int AD_UNROLL = 2;                                     // float4 (or, on the scalar path, 4 single floats) per lane
constexpr int AD_CHUNK = AD_THREADS * AD_UNROLL * 4;             // 2048 elements per workgroup

struct AdamTable {
    BinAdamTensor row[BINOPT_ADAM_MAX_TENSORS];
    int first_block[BINOPT_ADAM_MAX_TENSORS + 1];                // row r owns workgroups first_block[r] .. first_block[r + 1] - 1
    int n;
};
// the launch's arguments travel in the kernel-argument segment: keep table + scalars well under 4 KB
static_assert(sizeof(BinAdamTensor) == 48, "BinAdamTensor layout");
static_assert(sizeof(AdamTable) + 5 * sizeof(float) <= 3840, "the table must fit the by-value argument limit");

struct AdamCoef { float w1, beta2, w2, eps, weight_decay; };     // w1 = 1 - beta1, w2 = 1 - beta2 (rounded once from double)

__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, const AdamCoef& c, float step_size,
                                            float inv_sqrt_bc2) {
    if (c.weight_decay != 0.f) g = g + c.weight_decay * p;
    m = m + c.w1 * (g - m);
    v = c.beta2 * v + (c.w2 * g) * g;
    const float denom = sqrtf(v) * inv_sqrt_bc2 + c.eps;
    p = p - step_size * (m / denom);
}

// The shortest decimal that rounds to the float `b` (what printing a float32 shows), as a double.  A caller's beta2 = 0.999 arrives as
// the float 0.99900001287…, and 1 - that is off from 0.001 by 1.3e-5 relative — far outside fp32 rounding of the v update; the decimal
// the caller wrote is recovered instead, so that 1 - beta carries full fp32 precision (torch casts its double 1 - beta2 the same way).
// For a float that is no short decimal this returns a double within half a float ulp of it.
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

__global__ void __launch_bounds__(AD_THREADS)
adam_step_kernel(const AdamTable tab, const AdamCoef c) {
    // the row of this workgroup: largest r with first_block[r] <= blockIdx.x  (first_block[0] = 0, first_block[n] = gridDim.x)
    int lo = 0, hi = tab.n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tab.first_block[mid] <= (int)blockIdx.x) lo = mid; else hi = mid;
    }
    const BinAdamTensor& r = tab.row[lo];
    float* __restrict__ P = r.p;
    const float* __restrict__ G = r.g;
    float* __restrict__ M = r.m;
    float* __restrict__ V = r.v;
    const int64_t numel = r.numel;
    const float step_size = r.step_size, inv_sqrt_bc2 = r.inv_sqrt_bc2;
    const int64_t base = (int64_t)((int)blockIdx.x - tab.first_block[lo]) * AD_CHUNK;
    const int t = threadIdx.x;
    const bool aligned = ((((uintptr_t)P | (uintptr_t)G | (uintptr_t)M | (uintptr_t)V) & 15) == 0);   // wave-uniform

    if (aligned && base + AD_CHUNK <= numel) {                   // a whole chunk of an aligned row: 16 B per lane, nothing predicated
        float4 p[AD_UNROLL], g[AD_UNROLL], m[AD_UNROLL], v[AD_UNROLL];
#pragma unroll
        for (int k = 0; k < AD_UNROLL; ++k) {
            const int64_t e = base + 4 * (k * AD_THREADS + t);
            p[k] = *(const float4*)(P + e);
            g[k] = *(const float4*)(G + e);
            m[k] = *(const float4*)(M + e);
            v[k] = *(const float4*)(V + e);
        }
#pragma unroll
        for (int k = 0; k < AD_UNROLL; ++k) {
            adam_update(p[k].x, g[k].x, m[k].x, v[k].x, c, step_size, inv_sqrt_bc2);
            adam_update(p[k].y, g[k].y, m[k].y, v[k].y, c, step_size, inv_sqrt_bc2);
            adam_update(p[k].z, g[k].z, m[k].z, v[k].z, c, step_size, inv_sqrt_bc2);
            adam_update(p[k].w, g[k].w, m[k].w, v[k].w, c, step_size, inv_sqrt_bc2);
        }
#pragma unroll
        for (int k = 0; k < AD_UNROLL; ++k) {
            const int64_t e = base + 4 * (k * AD_THREADS + t);
            *(float4*)(P + e) = p[k];
            *(float4*)(M + e) = m[k];
            *(float4*)(V + e) = v[k];
        }
    } else {
        // 4 B per lane, consecutive lanes on consecutive floats: a row with a misaligned pointer, and the last, partial chunk of
        // every row.  The loads are not predicated (a lane past the end re-reads the row's last element, numel >= 1), so all of
        // them are in flight at once; only the stores are.
        constexpr int U = AD_UNROLL * 4;
        float p[U], g[U], m[U], v[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t e = min(base + k * AD_THREADS + t, numel - 1);
            p[k] = P[e]; g[k] = G[e]; m[k] = M[e]; v[k] = V[e];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) adam_update(p[k], g[k], m[k], v[k], c, step_size, inv_sqrt_bc2);
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t e = base + k * AD_THREADS + t;
            if (e < numel) { P[e] = p[k]; M[e] = m[k]; V[e] = v[k]; }
        }
    }
}

int binopt_version(void) { return BINOPT_VERSION; }

int binopt_adam_step(const BinAdamTensor* items, int n, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (n < 0 || (n > 0 && !items)) return BINOPT_E_ARG;
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return BINOPT_E_ARG;
    const int64_t max_blocks = 0x7fffffff;
    for (int i = 0; i < n; ++i) {                                // everything is checked before anything is launched
        if (!items[i].p || !items[i].g || !items[i].m || !items[i].v || items[i].numel < 1) return BINOPT_E_ARG;
        if ((items[i].numel + AD_CHUNK - 1) / AD_CHUNK > max_blocks) return BINOPT_E_SHAPE;
    }
    AdamCoef c;
    c.w1 = (float)(1.0 - shortest_decimal(beta1));
    c.beta2 = beta2;
    c.w2 = (float)(1.0 - shortest_decimal(beta2));
    c.eps = eps;
    c.weight_decay = weight_decay;
    hipStream_t s = (hipStream_t)stream;
    int i = 0;
    while (i < n) {                                              // launches of at most BINOPT_ADAM_MAX_TENSORS rows
        AdamTable tab;
        int64_t blocks = 0;
        int k = 0;
        for (; k < BINOPT_ADAM_MAX_TENSORS && i + k < n; ++k) {
            const int64_t nb = (items[i + k].numel + AD_CHUNK - 1) / AD_CHUNK;
            if (blocks + nb > max_blocks) break;                 // the rest goes into the next launch
            tab.row[k] = items[i + k];
            tab.first_block[k] = (int)blocks;
            blocks += nb;
        }
        for (int j = k; j <= BINOPT_ADAM_MAX_TENSORS; ++j) tab.first_block[j] = (int)blocks;
        for (int j = k; j < BINOPT_ADAM_MAX_TENSORS; ++j) tab.row[j] = BinAdamTensor{};
        tab.n = k;
        hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)blocks), dim3(AD_THREADS), 0, s, tab, c);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
        i += k;
    }
    return 0;
}
