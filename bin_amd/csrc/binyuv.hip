// binyuv.hip (libbinyuv.so, include/binyuv.h) — the two streaming kernels of the video path (bin_amd/video.py):
//   yuv_to_frame_kernel   : 8-bit planar YUV (4:2:0 / 4:4:4, BT.601 / BT.709, limited / full) -> replicate-padded fp32 planar RGB;
//   yuv_from_frame_kernel : the crop of an fp32 planar RGB frame -> 8-bit planar YUV, 4:2:0 chroma as the box mean of its block.
// Both are HBM-bound element-wise kernels: no LDS, no reuse beyond a lane's own registers.  A lane owns 4 consecutive pixels of a
// row, of two rows at 4:2:0 (a chroma pair is loaded once); blockIdx.x grid-strides over (row or row pair, column group) items with
// 64-bit indices.  Data paths (binyuv.h): VEC moves dwords / 16-bit chroma pairs / float4s, the other path bytes and single floats;
// both fill the same registers and call the same per-pixel functions (binyuv_common.h, shared with binrate.hip), so they agree bit
// for bit.  The arithmetic is written with fmaf and the rounding intrinsics: nothing is left to contraction.  All of a lane's loads
// come before its first store.
#include "binyuv_common.h"

static_assert(sizeof(BinYuvFormat) == 12, "BinYuvFormat layout");

// Item (j, g): output columns 4g .. 4g+3 of output row j (4:4:4) or of output rows 2j - (pt & 1), 2j - (pt & 1) + 1 (4:2:0: the pair
// is aligned to the SOURCE rows, so both take one chroma row also under an odd top pad).  Pad lanes clamp their source coordinate.
template <bool VEC, bool C420>
__global__ void __launch_bounds__(YUV_THREADS)
yuv_to_frame_kernel(const uint8_t* __restrict__ Yp, const uint8_t* __restrict__ Up, const uint8_t* __restrict__ Vp, const int H,
                    const int W, const int cw, const int pl, const int pt, const int Hp, const int Wp, const int ng,
                    const int64_t items, const ToCoef k, float* __restrict__ out) {
    constexpr int R = C420 ? 2 : 1;
    const int64_t plane = (int64_t)Hp * Wp, stride = (int64_t)gridDim.x * YUV_THREADS;
    const bool small = items < ((int64_t)1 << 31);
    const int row_off = C420 ? (pt & 1) : 0;
    for (int64_t item = (int64_t)blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += stride) {
        int j, g;
        split(item, ng, small, j, g);
        const int ox0 = 4 * g, oy0 = R * j - row_off;
        int sy[R];
#pragma unroll
        for (int r = 0; r < R; ++r) sy[r] = clampi(oy0 + r - pt, H - 1);
        const int64_t crow = (int64_t)(C420 ? sy[0] >> 1 : sy[0]) * cw;
        uint32_t yv[R][4], uv[4], vv[4];
        if (VEC && ox0 >= pl && ox0 - pl < W) {                  // an interior group: pl, W multiples of 4, so all of it is
            const int sx0 = ox0 - pl;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(Yp + (int64_t)sy[r] * W + sx0);
#pragma unroll
                for (int i = 0; i < 4; ++i) yv[r][i] = (w >> (8 * i)) & 255u;
            }
            if (C420) {
                const uint32_t wu = *reinterpret_cast<const uint16_t*>(Up + crow + (sx0 >> 1));
                const uint32_t wv = *reinterpret_cast<const uint16_t*>(Vp + crow + (sx0 >> 1));
#pragma unroll
                for (int i = 0; i < 4; ++i) { uv[i] = (wu >> (8 * (i >> 1))) & 255u; vv[i] = (wv >> (8 * (i >> 1))) & 255u; }
            } else {
                const uint32_t wu = *reinterpret_cast<const uint32_t*>(Up + crow + sx0);
                const uint32_t wv = *reinterpret_cast<const uint32_t*>(Vp + crow + sx0);
#pragma unroll
                for (int i = 0; i < 4; ++i) { uv[i] = (wu >> (8 * i)) & 255u; vv[i] = (wv >> (8 * i)) & 255u; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int sx = clampi(ox0 + i - pl, W - 1);
#pragma unroll
                for (int r = 0; r < R; ++r) yv[r][i] = Yp[(int64_t)sy[r] * W + sx];
                const int cx = C420 ? sx >> 1 : sx;
                uv[i] = Up[crow + cx];
                vv[i] = Vp[crow + cx];
            }
        }
        float cr[R][4], cg[R][4], cb[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) yuv_pixel(yv[r][i], uv[i], vv[i], k, cr[r][i], cg[r][i], cb[r][i]);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int oy = oy0 + r;
            if (oy < 0 || oy >= Hp) continue;
            float* o = out + (int64_t)oy * Wp + ox0;
            if (VEC) {
                *reinterpret_cast<float4*>(o) = make_float4(cr[r][0], cr[r][1], cr[r][2], cr[r][3]);
                *reinterpret_cast<float4*>(o + plane) = make_float4(cg[r][0], cg[r][1], cg[r][2], cg[r][3]);
                *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(cb[r][0], cb[r][1], cb[r][2], cb[r][3]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (ox0 + i < Wp) { o[i] = cr[r][i]; o[plane + i] = cg[r][i]; o[2 * plane + i] = cb[r][i]; }
            }
        }
    }
}

// Item (j, g): crop columns 4g .. 4g+3 of crop row j (4:4:4) or of crop rows 2j, 2j+1 (4:2:0: chroma row j, chroma columns 2g, 2g+1).
// Lanes past the crop's edge clamp their source coordinate to it and store nothing there.
template <bool VEC, bool C420>
__global__ void __launch_bounds__(YUV_THREADS)
yuv_from_frame_kernel(const float* __restrict__ x, const int Hp, const int Wp, const int top, const int left, const int H,
                      const int W, const int cw, const int ng, const int64_t items, const FromCoef k, uint8_t* __restrict__ Yp,
                      uint8_t* __restrict__ Up, uint8_t* __restrict__ Vp) {
    constexpr int R = C420 ? 2 : 1;
    const int64_t plane = (int64_t)Hp * Wp, stride = (int64_t)gridDim.x * YUV_THREADS;
    const bool small = items < ((int64_t)1 << 31);
    for (int64_t item = (int64_t)blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += stride) {
        int j, g;
        split(item, ng, small, j, g);
        const int x0 = 4 * g, y0 = R * j;
        float cr[R][4], cg[R][4], cb[R][4];
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
        float ly[R][4], pb[R][4], pr[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) rgb_pixel(cr[r][i], cg[r][i], cb[r][i], k, ly[r][i], pb[r][i], pr[r][i]);
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
}

int binyuv_version(void) { return BINYUV_VERSION; }

int binyuv_to_frame(const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W, const BinYuvFormat* format, int pad_left,
                    int pad_right, int pad_top, int pad_bottom, float* out_chw, void* stream) {
    ToCoef k;
    if (int rc = coefficients(format, &k, nullptr)) return rc;
    if (!y || !u || !v || !out_chw || !aligned(out_chw, 4)) return BINYUV_E_ARG;
    if (H < 1 || W < 1 || pad_left < 0 || pad_right < 0 || pad_top < 0 || pad_bottom < 0) return BINYUV_E_ARG;
    const int64_t Hp = (int64_t)H + pad_top + pad_bottom, Wp = (int64_t)W + pad_left + pad_right;
    if (Hp > INT32_MAX || Wp > INT32_MAX || 3 * Hp > YUV_MAX_ELEMS / Wp) return BINYUV_E_SHAPE;
    const bool c420 = format->chroma == BINYUV_CHROMA_420;
    const int ch = c420 ? (H + 1) / 2 : H, cw = c420 ? (W + 1) / 2 : W;
    const uint64_t out_bytes = (uint64_t)(3 * Hp * Wp) * 4, c_bytes = (uint64_t)ch * cw;
    if (overlap(out_chw, out_bytes, y, (uint64_t)H * W) || overlap(out_chw, out_bytes, u, c_bytes) || overlap(out_chw, out_bytes, v, c_bytes))
        return BINYUV_E_ARG;
    const bool vec = W % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 && aligned(out_chw, 16) && aligned(y, 4) && aligned(u, 4) && aligned(v, 4);
    const int ng = (int)((Wp + 3) / 4);
    const int64_t rows = c420 ? (Hp + (pad_top & 1) + 1) / 2 : Hp, items = rows * ng;
    const dim3 grid = grid_for(items), block(YUV_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const auto kernel = vec ? (c420 ? yuv_to_frame_kernel<true, true> : yuv_to_frame_kernel<true, false>)
                            : (c420 ? yuv_to_frame_kernel<false, true> : yuv_to_frame_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, y, u, v, H, W, cw, pad_left, pad_top, (int)Hp, (int)Wp, ng, items, k, out_chw);
    return (int)hipGetLastError();
}

int binyuv_from_frame(const float* chw, int Hp, int Wp, int top, int left, int H, int W, const BinYuvFormat* format, uint8_t* y,
                      uint8_t* u, uint8_t* v, void* stream) {
    FromCoef k;
    if (int rc = coefficients(format, nullptr, &k)) return rc;
    if (!chw || !y || !u || !v || !aligned(chw, 4)) return BINYUV_E_ARG;
    if (Hp < 1 || Wp < 1 || H < 1 || W < 1 || top < 0 || left < 0) return BINYUV_E_ARG;
    if ((int64_t)top + H > Hp || (int64_t)left + W > Wp) return BINYUV_E_ARG;
    if (3 * (int64_t)Hp > YUV_MAX_ELEMS / Wp) return BINYUV_E_SHAPE;
    const bool c420 = format->chroma == BINYUV_CHROMA_420;
    const int ch = c420 ? (H + 1) / 2 : H, cw = c420 ? (W + 1) / 2 : W;
    const uint64_t in_bytes = (uint64_t)3 * Hp * Wp * 4, y_bytes = (uint64_t)H * W, c_bytes = (uint64_t)ch * cw;
    if (overlap(chw, in_bytes, y, y_bytes) || overlap(chw, in_bytes, u, c_bytes) || overlap(chw, in_bytes, v, c_bytes) ||
        overlap(y, y_bytes, u, c_bytes) || overlap(y, y_bytes, v, c_bytes) || overlap(u, c_bytes, v, c_bytes))
        return BINYUV_E_ARG;
    const bool vec = W % 4 == 0 && Wp % 4 == 0 && left % 4 == 0 && aligned(chw, 16) && aligned(y, 4) && aligned(u, 4) && aligned(v, 4);
    const int ng = (W + 3) / 4;
    const int64_t items = (int64_t)ch * ng;
    const dim3 grid = grid_for(items), block(YUV_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const auto kernel = vec ? (c420 ? yuv_from_frame_kernel<true, true> : yuv_from_frame_kernel<true, false>)
                            : (c420 ? yuv_from_frame_kernel<false, true> : yuv_from_frame_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, chw, Hp, Wp, top, left, H, W, cw, ng, items, k, y, u, v);
    return (int)hipGetLastError();
}
