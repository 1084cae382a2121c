// binclip.hip (libbinclip.so, include/binclip.h) — the streaming kernel that fills the device frame cache from video
// (bin_amd/data/video_dataset.py):
//   yuv_to_bgr_kernel : the 8-bit planar YUV payloads of n frames (4:2:0 / 4:4:4, BT.601 / BT.709, limited / full) -> uint8 HWC BGR.
// An HBM-bound element-wise kernel of binyuv.hip's shape: no LDS, no reuse beyond a lane's own registers.  A lane owns 4 consecutive
// pixels of a row, of two rows at 4:2:0; blockIdx.x grid-strides over (frame, row or row pair, column group) items with 64-bit
// indices.  The load stage and the per-pixel function are binyuv_common.h's (load_yuv4_vec / load_yuv4_bytes, yuv_pixel:
// yuv_to_frame_kernel's, so the bytes are those of binyuv_to_frame's values); what is written here is the three-level item split and
// the store: VEC (binclip.h) one 12-byte store per row, the other path bytes.  All of a lane's loads come before its first store.
#include "binyuv_common.h"
#include "../../include/binclip.h"

static_assert(sizeof(BinYuvFormat) == 12, "BinYuvFormat layout");
static_assert(BINCLIP_E_ARG == BINYUV_E_ARG && BINCLIP_E_SHAPE == BINYUV_E_SHAPE, "one set of codes");

namespace {
struct __attribute__((packed, aligned(4))) Bgr4 {                // 4 BGR pixels: 12 bytes at a 4-byte aligned address
    uint32_t a, b, c;
};

// the byte binhip_frame_to_u8 stores for a channel that is in [0, 1] already
__device__ __forceinline__ uint32_t to_byte(float c) { return (uint32_t)rintf(__fmul_rn(c, 255.f)); }
}  // namespace

// Item (f, j, g): columns 4g .. 4g+3 of row j (4:4:4) or of rows 2j, 2j+1 (4:2:0: chroma row j) of frame f.  Lanes past the right or
// the bottom edge (byte path, odd H) clamp their source coordinate to it and store nothing there.
template <bool VEC, bool C420>
__global__ void __launch_bounds__(YUV_THREADS)
yuv_to_bgr_kernel(const uint8_t* __restrict__ payloads, const int64_t payload_stride, const int H, const int W, const int cw,
                  const int64_t c_bytes, const int rows, const int ng, const int64_t items, const ToCoef k,
                  uint8_t* __restrict__ out) {
    constexpr int R = C420 ? 2 : 1;
    const int64_t y_bytes = (int64_t)H * W, stride = (int64_t)gridDim.x * YUV_THREADS;
    const bool small = items < ((int64_t)1 << 31);
    for (int64_t item = (int64_t)blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += stride) {
        int f, j, g;
        if (small) {                                             // frame * rows + row fits 32 bits with the item
            int fj;
            split(item, ng, true, fj, g);
            split(fj, rows, true, f, j);
        } else {
            const int64_t fj = item / ng, fl = fj / rows;
            g = (int)(item - fj * ng); f = (int)fl; j = (int)(fj - fl * rows);
        }
        const uint8_t* Yp = payloads + (int64_t)f * payload_stride;
        const uint8_t* Up = Yp + y_bytes;
        const uint8_t* Vp = Up + c_bytes;
        const int x0 = 4 * g, y0 = R * j;
        int sy[R];
#pragma unroll
        for (int r = 0; r < R; ++r) sy[r] = y0 + r < H ? y0 + r : H - 1;
        const int64_t crow = (int64_t)j * cw;
        uint32_t yv[R][4], uv[4], vv[4];
        if (VEC) {
            load_yuv4_vec<C420, R>(Yp, Up, Vp, W, sy, crow, x0, yv, uv, vv);
        } else {
            int sx[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) sx[i] = x0 + i < W ? x0 + i : W - 1;
            load_yuv4_bytes<C420, R>(Yp, Up, Vp, W, sy, crow, sx, yv, uv, vv);
        }
        uint32_t qb[R][4], qg[R][4], qr[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float cr, cg, cb;
                yuv_pixel(yv[r][i], uv[i], vv[i], k, cr, cg, cb);
                qb[r][i] = to_byte(cb); qg[r][i] = to_byte(cg); qr[r][i] = to_byte(cr);
            }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (y0 + r >= H) continue;
            uint8_t* o = out + (((int64_t)f * H + (y0 + r)) * W + x0) * 3;
            if (VEC) {
                Bgr4 v;
                v.a = qb[r][0] | (qg[r][0] << 8) | (qr[r][0] << 16) | (qb[r][1] << 24);
                v.b = qg[r][1] | (qr[r][1] << 8) | (qb[r][2] << 16) | (qg[r][2] << 24);
                v.c = qr[r][2] | (qb[r][3] << 8) | (qg[r][3] << 16) | (qr[r][3] << 24);
                *reinterpret_cast<Bgr4*>(o) = v;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x0 + i < W) { o[3 * i] = (uint8_t)qb[r][i]; o[3 * i + 1] = (uint8_t)qg[r][i]; o[3 * i + 2] = (uint8_t)qr[r][i]; }
            }
        }
    }
}

int binclip_version(void) { return BINCLIP_VERSION; }

int binclip_yuv_to_bgr(const uint8_t* payloads, int n, int64_t payload_stride, int H, int W, const BinYuvFormat* format,
                       uint8_t* bgr_hwc, void* stream) {
    ToCoef k;
    if (int rc = coefficients(format, &k, nullptr)) return rc;
    if (!payloads || !bgr_hwc || n < 1 || H < 1 || W < 1 || payload_stride < 1) return BINCLIP_E_ARG;
    const bool c420 = format->chroma == BINYUV_CHROMA_420;
    int ch, cw;
    chroma_size(c420, H, W, ch, cw);
    const uint64_t pixels = (uint64_t)H * W, c_bytes = (uint64_t)ch * cw, frame_bytes = pixels + 2 * c_bytes;   // below 2^64
    if ((uint64_t)payload_stride < frame_bytes) return BINCLIP_E_ARG;
    const uint64_t limit = (uint64_t)YUV_MAX_ELEMS;
    if (pixels > limit || 3 * pixels * (uint64_t)n > limit) return BINCLIP_E_SHAPE;                             // (below 2^40 * 2^33)
    if ((uint64_t)payload_stride > limit || (uint64_t)payload_stride * (uint64_t)n > limit) return BINCLIP_E_SHAPE;
    const uint64_t out_bytes = 3 * pixels * (uint64_t)n, in_bytes = (uint64_t)(n - 1) * (uint64_t)payload_stride + frame_bytes;
    if (overlap(bgr_hwc, out_bytes, payloads, in_bytes)) return BINCLIP_E_ARG;
    // W % 4 == 0 makes H * W and ch * cw multiples of 4 and 2: with an aligned base and stride every plane row of every frame is
    const bool vec = W % 4 == 0 && payload_stride % 4 == 0 && aligned(payloads, 4) && aligned(bgr_hwc, 4);
    const int ng = (int)(((int64_t)W + 3) / 4);
    const int64_t items = (int64_t)n * ch * ng;
    const auto kernel = vec ? (c420 ? yuv_to_bgr_kernel<true, true> : yuv_to_bgr_kernel<true, false>)
                            : (c420 ? yuv_to_bgr_kernel<false, true> : yuv_to_bgr_kernel<false, false>);
    return launch(kernel, grid_for(items), stream, payloads, payload_stride, H, W, cw, (int64_t)c_bytes, ch, ng, items, k, bgr_hwc);
}
