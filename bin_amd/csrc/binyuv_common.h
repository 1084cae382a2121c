// binyuv_common.h — what the YUV kernels of libbinyuv.so (binyuv.hip), libbinrate.so (binrate.hip) and libbinclip.so (binclip.hip)
// share, each written ONCE:
//   - the coefficients of a format and the per-pixel expressions (yuv_pixel, rgb_pixel, quantise, block_mean);
//   - the item split (split);
//   - the stages a kernel is composed of: load_yuv4_vec / load_yuv4_bytes (8-bit planes -> a lane's registers, one per data path: the
//     kernel decides per column group and clamps its own columns), load_rgb4 (the crop of an fp32 planar frame -> a lane's
//     registers) and store_yuv (quantise, 4:2:0 block mean, the plane stores with their edge guards);
//   - the host side: chroma_size, the geometry and checks of a frame -> YUV call (yuv_out_geometry), the grid (grid_for) and
//     the launch (launch).  The pick of a kernel's <VEC, C420> instance stays with each entry point: two lines that name the kernel.
// A kernel reads: split the item, load, apply the per-pixel function, store.  Data paths: VEC moves dwords / 16-bit chroma pairs /
// float4s, the other path bytes and single floats; both fill the same registers, so they agree bit for bit, and so do the libraries: a
// frame that goes through binrate_blend_to_yuv with w == 0 gives the bytes binyuv_from_frame gives, binclip_yuv_to_bgr the bytes of
// binyuv_to_frame's values.  The arithmetic is written with fmaf and the rounding intrinsics: nothing is left to contraction.
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

// ---- the stages.  Their pointer parameters are plain on purpose (the kernels' own are __restrict__): with __restrict__ on store_yuv's
// planes the compiler no longer unrolls the grid-stride loop of the <VEC, 4:4:4> kernels three times, which is another kernel.
__device__ __forceinline__ void unpack4(uint32_t w, uint32_t (&q)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (w >> (8 * i)) & 255u;
}

// The two data paths of a YUV load, of the luma rows sy[] and the chroma row at crow (both clamped by the caller).  Columns sx0 ..
// sx0+3, sx0 a multiple of 4 inside the row and the planes dword-aligned: one dword per luma row and a 16-bit pair (4:2:0) or a dword
// (4:4:4) per chroma plane ...
template <bool C420, int R>
__device__ __forceinline__ void load_yuv4_vec(const uint8_t* Yp, const uint8_t* Up, const uint8_t* Vp, int W, const int (&sy)[R],
                                              int64_t crow, int sx0, uint32_t (&yv)[R][4], uint32_t (&uv)[4], uint32_t (&vv)[4]) {
#pragma unroll
    for (int r = 0; r < R; ++r) unpack4(*reinterpret_cast<const uint32_t*>(Yp + (int64_t)sy[r] * W + sx0), yv[r]);
    if (C420) {
        const uint32_t wu = *reinterpret_cast<const uint16_t*>(Up + crow + (sx0 >> 1));
        const uint32_t wv = *reinterpret_cast<const uint16_t*>(Vp + crow + (sx0 >> 1));
#pragma unroll
        for (int i = 0; i < 4; ++i) { uv[i] = (wu >> (8 * (i >> 1))) & 255u; vv[i] = (wv >> (8 * (i >> 1))) & 255u; }
    } else {
        unpack4(*reinterpret_cast<const uint32_t*>(Up + crow + sx0), uv);
        unpack4(*reinterpret_cast<const uint32_t*>(Vp + crow + sx0), vv);
    }
}
// ... and the columns sx[] (any four, clamped to the row by the caller) as bytes
template <bool C420, int R>
__device__ __forceinline__ void load_yuv4_bytes(const uint8_t* Yp, const uint8_t* Up, const uint8_t* Vp, int W, const int (&sy)[R],
                                                int64_t crow, const int (&sx)[4], uint32_t (&yv)[R][4], uint32_t (&uv)[4],
                                                uint32_t (&vv)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int r = 0; r < R; ++r) yv[r][i] = Yp[(int64_t)sy[r] * W + sx[i]];
        const int cx = C420 ? sx[i] >> 1 : sx[i];
        uv[i] = Up[crow + cx];
        vv[i] = Vp[crow + cx];
    }
}

// Crop columns x0 .. x0+3 of crop rows y0 .. y0+R-1 of the frame x ([3, Hp, Wp], plane = Hp * Wp, the crop at (top, left)): float4s
// (VEC: Wp, left and x0 multiples of 4, x 16-byte aligned) or single floats.  Rows and columns past the crop's edge clamp to it.
template <bool VEC, int R>
__device__ __forceinline__ void load_rgb4(const float* x, int64_t plane, int Wp, int top, int left, int H, int W, int x0, int y0,
                                          float (&cr)[R][4], float (&cg)[R][4], float (&cb)[R][4]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int yy = y0 + r < H ? y0 + r : H - 1;
        const float* p = x + (int64_t)(top + yy) * Wp + left;
        if (VEC) {
            const float4 a = *reinterpret_cast<const float4*>(p + x0);
            const float4 b = *reinterpret_cast<const float4*>(p + plane + x0);
            const float4 c = *reinterpret_cast<const float4*>(p + 2 * plane + x0);
            cr[r][0] = a.x; cr[r][1] = a.y; cr[r][2] = a.z; cr[r][3] = a.w;
            cg[r][0] = b.x; cg[r][1] = b.y; cg[r][2] = b.z; cg[r][3] = b.w;
            cb[r][0] = c.x; cb[r][1] = c.y; cb[r][2] = c.z; cb[r][3] = c.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int xx = x0 + i < W ? x0 + i : W - 1;
                cr[r][i] = p[xx]; cg[r][i] = p[plane + xx]; cb[r][i] = p[2 * plane + xx];
            }
        }
    }
}

// Item (j, g) of an H x W picture: luma ly and chroma pb, pr of crop columns x0 = 4g .. and crop rows y0 = R j .. -> the bytes of the
// Y, U and V planes (chroma row j; 4:2:0: chroma columns 2g, 2g+1 as the mean of their block).  VEC (W a multiple of 4, the planes
// dword-aligned): a dword per luma row, a 16-bit pair or a dword per chroma plane; else bytes.  Nothing is stored past the edge.
template <bool VEC, bool C420, int R>
__device__ __forceinline__ void store_yuv(const float (&ly)[R][4], const float (&pb)[R][4], const float (&pr)[R][4], const FromCoef& k,
                                          int x0, int y0, int j, int g, int H, int W, int cw, uint8_t* Yp, uint8_t* Up, uint8_t* Vp) {
    uint32_t qy[R][4], qu[4], qv[4];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) qy[r][i] = quantise(ly[r][i], k.y_scale, k.y_off);
    if (C420) {
        const bool row1 = y0 + 1 < H;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const bool col1 = x0 + 2 * c + 1 < W;
            qu[c] = quantise(block_mean(pb[0][2 * c], pb[0][2 * c + 1], pb[R - 1][2 * c], pb[R - 1][2 * c + 1], col1, row1), k.c_scale, 128.f);
            qv[c] = quantise(block_mean(pr[0][2 * c], pr[0][2 * c + 1], pr[R - 1][2 * c], pr[R - 1][2 * c + 1], col1, row1), k.c_scale, 128.f);
        }
        qu[2] = qu[3] = qv[2] = qv[3] = 0;
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) { qu[i] = quantise(pb[0][i], k.c_scale, 128.f); qv[i] = quantise(pr[0][i], k.c_scale, 128.f); }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (y0 + r >= H) continue;
        uint8_t* o = Yp + (int64_t)(y0 + r) * W + x0;
        if (VEC) {
            *reinterpret_cast<uint32_t*>(o) = pack4(qy[r]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) o[i] = (uint8_t)qy[r][i];
        }
    }
    if (C420) {
        const int64_t at = (int64_t)j * cw + 2 * g;
        if (VEC) {
            *reinterpret_cast<uint16_t*>(Up + at) = (uint16_t)(qu[0] | (qu[1] << 8));
            *reinterpret_cast<uint16_t*>(Vp + at) = (uint16_t)(qv[0] | (qv[1] << 8));
        } else {
#pragma unroll
            for (int c = 0; c < 2; ++c)
                if (x0 + 2 * c < W) { Up[at + c] = (uint8_t)qu[c]; Vp[at + c] = (uint8_t)qv[c]; }
        }
    } else {
        const int64_t at = (int64_t)j * cw + x0;
        if (VEC) {
            *reinterpret_cast<uint32_t*>(Up + at) = pack4(qu);
            *reinterpret_cast<uint32_t*>(Vp + at) = pack4(qv);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) { Up[at + i] = (uint8_t)qu[i]; Vp[at + i] = (uint8_t)qv[i]; }
        }
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

// rows and columns of a chroma plane of an H x W picture (in 64 bits: H + 1 need not fit an int)
inline void chroma_size(bool c420, int H, int W, int& ch, int& cw) {
    ch = c420 ? (int)(((int64_t)H + 1) / 2) : H;
    cw = c420 ? (int)(((int64_t)W + 1) / 2) : W;
}

// What the frame -> YUV entry points (binyuv_from_frame, binrate_blend_to_yuv) check and compute alike, in their order: the output
// planes, the sizes and the crop (E_ARG), the frame's size (E_SHAPE), then y, u, v against each other (E_ARG).  The caller checks its
// own input pointers before this, and their overlap with the planes (overlaps_planes) and their alignment after it.
struct YuvOutGeometry {
    bool c420, vec;                                              // vec: the sizes and the output planes allow the vector path
    int ch, cw, ng;
    int64_t items;
    uint64_t in_bytes, y_bytes, c_bytes;
};
inline int yuv_out_geometry(int Hp, int Wp, int top, int left, int H, int W, const BinYuvFormat* f, const uint8_t* y, const uint8_t* u,
                            const uint8_t* v, YuvOutGeometry* q) {
    if (!y || !u || !v) return BINYUV_E_ARG;
    if (Hp < 1 || Wp < 1 || H < 1 || W < 1 || top < 0 || left < 0) return BINYUV_E_ARG;
    if ((int64_t)top + H > Hp || (int64_t)left + W > Wp) return BINYUV_E_ARG;
    if (3 * (int64_t)Hp > YUV_MAX_ELEMS / Wp) return BINYUV_E_SHAPE;
    q->c420 = f->chroma == BINYUV_CHROMA_420;
    chroma_size(q->c420, H, W, q->ch, q->cw);
    q->in_bytes = (uint64_t)3 * Hp * Wp * 4; q->y_bytes = (uint64_t)H * W; q->c_bytes = (uint64_t)q->ch * q->cw;
    if (overlap(y, q->y_bytes, u, q->c_bytes) || overlap(y, q->y_bytes, v, q->c_bytes) || overlap(u, q->c_bytes, v, q->c_bytes))
        return BINYUV_E_ARG;
    q->vec = W % 4 == 0 && Wp % 4 == 0 && left % 4 == 0 && aligned(y, 4) && aligned(u, 4) && aligned(v, 4);
    q->ng = (W + 3) / 4;
    q->items = (int64_t)q->ch * q->ng;
    return 0;
}
inline bool overlaps_planes(const float* x, const YuvOutGeometry& q, const uint8_t* y, const uint8_t* u, const uint8_t* v) {
    return overlap(x, q.in_bytes, y, q.y_bytes) || overlap(x, q.in_bytes, u, q.c_bytes) || overlap(x, q.in_bytes, v, q.c_bytes);
}

// the grid is sized from the item count (one lane per item), capped where a block starts to stride
inline dim3 grid_for(int64_t items) {
    const int64_t blocks = (items + YUV_THREADS - 1) / YUV_THREADS;
    return dim3((unsigned)(blocks < YUV_MAX_BLOCKS ? blocks : YUV_MAX_BLOCKS));
}
// the launch of a kernel instance on `stream`; returns its status
template <class Kernel, class... Args>
inline int launch(Kernel kernel, dim3 grid, void* stream, Args... args) {
    hipLaunchKernelGGL(kernel, grid, dim3(YUV_THREADS), 0, (hipStream_t)stream, args...);
    return (int)hipGetLastError();
}
}  // namespace
