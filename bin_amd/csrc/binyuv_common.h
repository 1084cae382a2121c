// binyuv_common.h — what the frame <-> YUV kernels of libbinyuv.so (binyuv.hip) and libbinrate.so (binrate.hip) share: the
// coefficients of a format, the per-pixel expressions, the item split and the launch geometry.  ONE definition of the arithmetic:
// a frame that goes through binrate_blend_to_yuv with w == 0 gives the bytes binyuv_from_frame gives.  The arithmetic is written
// with fmaf and the rounding intrinsics: nothing is left to contraction.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binyuv.h"

namespace {
constexpr int YUV_THREADS = 256;
constexpr int64_t YUV_MAX_BLOCKS = 2048;                         // 8 workgroups per CU; beyond that blocks stride
constexpr int64_t YUV_MAX_ELEMS = (int64_t)1 << 40;

struct ToCoef {                                                  // R = y + rv v, G = y + gu u + gv v, B = y + bu u, with
    float y_off, y_scale, rv, gu, gv, bu;                        // y = (Y - y_off) y_scale, u = U - 128, v = V - 128
};
struct FromCoef {                                                // y = kr R + kg G + kb B, pb = (B - y) ipb, pr = (R - y) ipr
    float kr, kg, kb, ipb, ipr, y_scale, y_off, c_scale;         // Y = y y_scale + y_off, U = pb c_scale + 128
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// ---- the per-pixel expressions: ONE definition for both data paths
__device__ __forceinline__ void yuv_pixel(uint32_t Y, uint32_t U, uint32_t V, const ToCoef& k, float& r, float& g, float& b) {
    const float y = __fmul_rn(__fsub_rn((float)Y, k.y_off), k.y_scale);
    const float u = __fsub_rn((float)U, 128.f), v = __fsub_rn((float)V, 128.f);
    r = clamp01(fmaf(k.rv, v, y));
    g = clamp01(fmaf(k.gv, v, fmaf(k.gu, u, y)));
    b = clamp01(fmaf(k.bu, u, y));
}
__device__ __forceinline__ void rgb_pixel(float r, float g, float b, const FromCoef& k, float& y, float& pb, float& pr) {
    r = clamp01(r); g = clamp01(g); b = clamp01(b);
    y = fmaf(k.kb, b, fmaf(k.kg, g, __fmul_rn(k.kr, r)));
    pb = __fmul_rn(__fsub_rn(b, y), k.ipb);
    pr = __fmul_rn(__fsub_rn(r, y), k.ipr);
}
__device__ __forceinline__ uint32_t quantise(float v, float scale, float off) {
    return (uint32_t)fminf(fmaxf(rintf(fmaf(v, scale, off)), 0.f), 255.f);
}
// mean over the pixels of a 2x2 block that exist: (p00 + p01) + (p10 + p11), then a power-of-two scale
__device__ __forceinline__ float block_mean(float p00, float p01, float p10, float p11, bool col1, bool row1) {
    const float s0 = col1 ? __fadd_rn(p00, p01) : p00, s1 = col1 ? __fadd_rn(p10, p11) : p10;
    const float s = row1 ? __fadd_rn(s0, s1) : s0;
    return __fmul_rn(s, (col1 ? 0.5f : 1.f) * (row1 ? 0.5f : 1.f));
}
__device__ __forceinline__ uint32_t pack4(const uint32_t (&q)[4]) { return q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24); }

// item -> (row, column group); items below 2^31 (all but the largest) divide in 32 bits
__device__ __forceinline__ void split(int64_t item, int ng, bool small, int& row, int& grp) {
    if (small) {
        const uint32_t r = (uint32_t)item / (uint32_t)ng;
        row = (int)r; grp = (int)((uint32_t)item - r * (uint32_t)ng);
    } else {
        const int64_t r = item / ng;
        row = (int)r; grp = (int)(item - r * ng);
    }
}

// ---- host side
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
inline bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

// Kr, Kb of the matrix and the scales of the range, in double; the kernels get them rounded to fp32 once
inline int coefficients(const BinYuvFormat* f, ToCoef* to, FromCoef* from) {
    if (!f || (f->chroma != BINYUV_CHROMA_420 && f->chroma != BINYUV_CHROMA_444)) return BINYUV_E_ARG;
    if (f->matrix != BINYUV_MATRIX_BT601 && f->matrix != BINYUV_MATRIX_BT709) return BINYUV_E_ARG;
    if (f->range != BINYUV_RANGE_LIMITED && f->range != BINYUV_RANGE_FULL) return BINYUV_E_ARG;
    const double kr = f->matrix == BINYUV_MATRIX_BT601 ? 0.299 : 0.2126, kb = f->matrix == BINYUV_MATRIX_BT601 ? 0.114 : 0.0722;
    const double kg = 1.0 - kr - kb;
    const bool full = f->range == BINYUV_RANGE_FULL;
    const double ys = full ? 255.0 : 219.0, yo = full ? 0.0 : 16.0, cs = full ? 255.0 : 224.0;
    if (to) {
        to->y_off = (float)yo;
        to->y_scale = (float)(1.0 / ys);
        to->rv = (float)(2.0 * (1.0 - kr) / cs);
        to->bu = (float)(2.0 * (1.0 - kb) / cs);
        to->gu = (float)(-kb * 2.0 * (1.0 - kb) / kg / cs);
        to->gv = (float)(-kr * 2.0 * (1.0 - kr) / kg / cs);
    }
    if (from) {
        from->kr = (float)kr; from->kg = (float)kg; from->kb = (float)kb;
        from->ipb = (float)(1.0 / (2.0 * (1.0 - kb)));
        from->ipr = (float)(1.0 / (2.0 * (1.0 - kr)));
        from->y_scale = (float)ys; from->y_off = (float)yo; from->c_scale = (float)cs;
    }
    return 0;
}

// the grid is sized from the item count (one lane per item), capped where a block starts to stride
inline dim3 grid_for(int64_t items) {
    const int64_t blocks = (items + YUV_THREADS - 1) / YUV_THREADS;
    return dim3((unsigned)(blocks < YUV_MAX_BLOCKS ? blocks : YUV_MAX_BLOCKS));
}
}  // namespace
