// binyuv.hip (libbinyuv.so, include/binyuv.h) — the two streaming kernels of the video path (bin_amd/video.py):
//   yuv_to_frame_kernel   : 8-bit planar YUV (4:2:0 / 4:4:4, BT.601 / BT.709, limited / full) -> replicate-padded fp32 planar RGB;
//   yuv_from_frame_kernel : the crop of an fp32 planar RGB frame -> 8-bit planar YUV, 4:2:0 chroma as the box mean of its block.
// Both are HBM-bound element-wise kernels: no LDS, no reuse beyond a lane's own registers.  A lane owns 4 consecutive pixels of a
// row, of two rows at 4:2:0 (a chroma pair is loaded once); blockIdx.x grid-strides over (row or row pair, column group) items with
// 64-bit indices.  The load and store stages, the per-pixel functions and the two data paths (binyuv.h) are binyuv_common.h's; what
// is written here is each kernel's item geometry and the padded float4 store.  All of a lane's loads come before its first store.
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
        // an interior group: pl, W multiples of 4, so all of it is
        if (VEC && ox0 >= pl && ox0 - pl < W) {
            load_yuv4_vec<C420, R>(Yp, Up, Vp, W, sy, crow, ox0 - pl, yv, uv, vv);
        } else {
            int sx[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sx[i] = clampi(ox0 + i - pl, W - 1);
            load_yuv4_bytes<C420, R>(Yp, Up, Vp, W, sy, crow, sx, yv, uv, vv);
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
        load_rgb4<VEC, R>(x, plane, Wp, top, left, H, W, x0, y0, cr, cg, cb);
        float ly[R][4], pb[R][4], pr[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) rgb_pixel(cr[r][i], cg[r][i], cb[r][i], k, ly[r][i], pb[r][i], pr[r][i]);
        store_yuv<VEC, C420, R>(ly, pb, pr, k, x0, y0, j, g, H, W, cw, Yp, Up, Vp);
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
    int ch, cw;
    chroma_size(c420, H, W, ch, cw);
    const uint64_t out_bytes = (uint64_t)(3 * Hp * Wp) * 4, c_bytes = (uint64_t)ch * cw;
    if (overlap(out_chw, out_bytes, y, (uint64_t)H * W) || overlap(out_chw, out_bytes, u, c_bytes) || overlap(out_chw, out_bytes, v, c_bytes))
        return BINYUV_E_ARG;
    const bool vec = W % 4 == 0 && pad_left % 4 == 0 && Wp % 4 == 0 && aligned(out_chw, 16) && aligned(y, 4) && aligned(u, 4) && aligned(v, 4);
    const int ng = (int)((Wp + 3) / 4);
    const int64_t rows = c420 ? (Hp + (pad_top & 1) + 1) / 2 : Hp;
    const auto kernel = vec ? (c420 ? yuv_to_frame_kernel<true, true> : yuv_to_frame_kernel<true, false>)
                            : (c420 ? yuv_to_frame_kernel<false, true> : yuv_to_frame_kernel<false, false>);
    return launch(kernel, grid_for(rows * ng), stream, y, u, v, H, W, cw, pad_left, pad_top, (int)Hp, (int)Wp, ng, rows * ng, k, out_chw);
}

int binyuv_from_frame(const float* chw, int Hp, int Wp, int top, int left, int H, int W, const BinYuvFormat* format, uint8_t* y,
                      uint8_t* u, uint8_t* v, void* stream) {
    FromCoef k;
    YuvOutGeometry q;
    if (int rc = coefficients(format, nullptr, &k)) return rc;
    if (!chw || !aligned(chw, 4)) return BINYUV_E_ARG;
    if (int rc = yuv_out_geometry(Hp, Wp, top, left, H, W, format, y, u, v, &q)) return rc;
    if (overlaps_planes(chw, q, y, u, v)) return BINYUV_E_ARG;
    const bool vec = q.vec && aligned(chw, 16);
    const auto kernel = vec ? (q.c420 ? yuv_from_frame_kernel<true, true> : yuv_from_frame_kernel<true, false>)
                            : (q.c420 ? yuv_from_frame_kernel<false, true> : yuv_from_frame_kernel<false, false>);
    return launch(kernel, grid_for(q.items), stream, chw, Hp, Wp, top, left, H, W, q.cw, q.ng, q.items, k, y, u, v);
}
