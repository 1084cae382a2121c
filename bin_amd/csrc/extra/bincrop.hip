// bincrop.hip (libbincrop.so, include/bincrop.h) — the streaming kernel that decodes a batch's crops out of a device frame cache kept
// in YUV (bin_amd/data/video_dataset.py, `device_cache_format: yuv`):
//   yuv_crops_to_bgr_kernel : per table row the ch x cw crop of one 8-bit planar YUV frame of a byte arena -> uint8 HWC BGR.
// An HBM-bound element-wise kernel of binclip.hip's shape: no LDS, no reuse beyond a lane's own registers.  A lane owns 4 consecutive
// output columns of one output row; blockIdx.x grid-strides over (table row, crop row, column group) items with 64-bit indices.  The
// load stages and the per-pixel function are binyuv_common.h's (load_yuv4_vec / load_yuv4_bytes, yuv_pixel: the ones
// yuv_to_bgr_kernel of binclip.hip compiles, so the bytes are binclip_yuv_to_bgr's); what is written here is the row record, the
// per-row pick of the load path, and the store: OUTVEC (bincrop.h) one 12-byte store, the other path bytes.  All of a lane's loads
// come before its first store.
#include "../binyuv_common.h"
#include "../../../include/bincrop.h"

static_assert(sizeof(BinCropRow) == 32, "BinCropRow layout");
static_assert(BINCROP_E_ARG == BINYUV_E_ARG && BINCROP_E_SHAPE == BINYUV_E_SHAPE, "one set of codes");
static_assert(BINCROP_FORMATS == 4, "2 matrices x 2 ranges");

namespace {
struct __attribute__((packed, aligned(4))) Bgr4 {                // 4 BGR pixels: 12 bytes at a 4-byte aligned address
    uint32_t a, b, c;
};
struct Coef4 {                                                   // the coefficients of format index 2 * matrix + range, by value
    ToCoef k[BINCROP_FORMATS];
};

// the byte binhip_frame_to_u8 stores for a channel that is in [0, 1] already (binclip.hip's)
__device__ __forceinline__ uint32_t to_byte(float c) { return (uint32_t)rintf(__fmul_rn(c, 255.f)); }

// k[f] without an indexed copy of the kernel argument: four selects per coefficient
__device__ __forceinline__ float pick(float a, float b, float c, float d, int f) { return f == 0 ? a : f == 1 ? b : f == 2 ? c : d; }
__device__ __forceinline__ ToCoef pick(const Coef4& q, int f) {
    ToCoef k;
    k.y_off = pick(q.k[0].y_off, q.k[1].y_off, q.k[2].y_off, q.k[3].y_off, f);
    k.y_scale = pick(q.k[0].y_scale, q.k[1].y_scale, q.k[2].y_scale, q.k[3].y_scale, f);
    k.rv = pick(q.k[0].rv, q.k[1].rv, q.k[2].rv, q.k[3].rv, f);
    k.gu = pick(q.k[0].gu, q.k[1].gu, q.k[2].gu, q.k[3].gu, f);
    k.gv = pick(q.k[0].gv, q.k[1].gv, q.k[2].gv, q.k[3].gv, f);
    k.bu = pick(q.k[0].bu, q.k[1].bu, q.k[2].bu, q.k[3].bu, f);
    return k;
}
}  // namespace

// Item (r, j, g): output columns 4g .. 4g+3 of output row j of table row r.  The record is clamped, never trusted: a frame of at least
// 1 x 1, an offset that keeps the payload inside the arena, source coordinates inside the frame.  A payload larger than the arena
// (which no validated table holds) is not read at all: its crop is stored as zeros.
template <bool C420, bool OUTVEC>
__global__ void __launch_bounds__(YUV_THREADS)
yuv_crops_to_bgr_kernel(const uint8_t* __restrict__ arena, const int64_t arena_bytes, const BinCropRow* __restrict__ rows, const int ch,
                        const int cw, const int ng, const int64_t items, const Coef4 coef, uint8_t* __restrict__ out) {
    const int64_t stride = (int64_t)gridDim.x * YUV_THREADS;
    const bool small = items < ((int64_t)1 << 31);
    for (int64_t item = (int64_t)blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += stride) {
        int r, j, g;
        if (small) {                                             // table row * ch + crop row fits 32 bits with the item
            int rj;
            split(item, ng, true, rj, g);
            split(rj, ch, true, r, j);
        } else {
            const int64_t rj = item / ng, rl = rj / ch;
            g = (int)(item - rj * ng); r = (int)rl; j = (int)(rj - rl * ch);
        }
        const BinCropRow rec = rows[r];
        const int H = rec.H > 1 ? rec.H : 1, W = rec.W > 1 ? rec.W : 1;
        const int chh = C420 ? (int)(((int64_t)H + 1) >> 1) : H, cww = C420 ? (int)(((int64_t)W + 1) >> 1) : W;
        const int64_t y_bytes = (int64_t)H * W, c_bytes = (int64_t)chh * cww, frame_bytes = y_bytes + 2 * c_bytes;
        const bool fits = frame_bytes <= arena_bytes;
        const int64_t last = arena_bytes - frame_bytes;
        const int64_t off = !fits || rec.offset < 0 ? 0 : (rec.offset > last ? last : rec.offset);
        const uint8_t* Yp = arena + off;
        const uint8_t* Up = Yp + y_bytes;
        const uint8_t* Vp = Up + c_bytes;
        const int y0 = clampi(rec.y0, H - 1), x0 = clampi(rec.x0, W - 1);
        const int sy[1] = {(int64_t)y0 + j < H ? y0 + j : H - 1};
        const int64_t crow = (int64_t)(C420 ? sy[0] >> 1 : sy[0]) * cww;
        const int64_t sx0 = (int64_t)x0 + 4 * (int64_t)g;
        // the row's pick: dwords and 16-bit chroma pairs where every plane row of this payload is aligned and the crop starts on a
        // dword; the lane's columns must lie inside the row (they do for every validated row: x0 + cw <= W and W % 4 == 0)
        const bool vec = (((uintptr_t)Yp | (uintptr_t)(uint32_t)W | (uintptr_t)(uint32_t)x0) & 3) == 0 && sx0 + 3 < W;
        uint32_t yv[1][4] = {{0, 0, 0, 0}}, uv[4] = {128, 128, 128, 128}, vv[4] = {128, 128, 128, 128};
        if (fits) {
            if (vec) {
                load_yuv4_vec<C420, 1>(Yp, Up, Vp, W, sy, crow, (int)sx0, yv, uv, vv);
            } else {
                int sx[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) sx[i] = sx0 + i < W ? (int)(sx0 + i) : W - 1;
                load_yuv4_bytes<C420, 1>(Yp, Up, Vp, W, sy, crow, sx, yv, uv, vv);
            }
        }
        const ToCoef k = pick(coef, rec.format & (BINCROP_FORMATS - 1));
        uint32_t qb[4], qg[4], qr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            float cr, cg, cb;
            yuv_pixel(yv[0][i], uv[i], vv[i], k, cr, cg, cb);
            qb[i] = fits ? to_byte(cb) : 0; qg[i] = fits ? to_byte(cg) : 0; qr[i] = fits ? to_byte(cr) : 0;
        }
        uint8_t* o = out + (((int64_t)r * ch + j) * cw + 4 * (int64_t)g) * 3;
        if (OUTVEC) {
            Bgr4 v;
            v.a = qb[0] | (qg[0] << 8) | (qr[0] << 16) | (qb[1] << 24);
            v.b = qg[1] | (qr[1] << 8) | (qb[2] << 16) | (qg[2] << 24);
            v.c = qr[2] | (qb[3] << 8) | (qg[3] << 16) | (qr[3] << 24);
            *reinterpret_cast<Bgr4*>(o) = v;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * g + i < cw) { o[3 * i] = (uint8_t)qb[i]; o[3 * i + 1] = (uint8_t)qg[i]; o[3 * i + 2] = (uint8_t)qr[i]; }
        }
    }
}

int bincrop_version(void) { return BINCROP_VERSION; }

int bincrop_yuv_crops_to_bgr(const uint8_t* arena, int64_t arena_bytes, const BinCropRow* rows, int n_rows, int ch, int cw, int chroma,
                             uint8_t* out, void* stream) {
    if (!arena || !rows || !out || n_rows < 1 || ch < 1 || cw < 1 || arena_bytes < 1) return BINCROP_E_ARG;
    if (chroma != BINYUV_CHROMA_420 && chroma != BINYUV_CHROMA_444) return BINCROP_E_ARG;
    if (!aligned(rows, 8)) return BINCROP_E_ARG;
    Coef4 coef;
    for (int m = 0; m < 2; ++m)
        for (int g = 0; g < 2; ++g) {
            const BinYuvFormat f = {chroma, m ? BINYUV_MATRIX_BT709 : BINYUV_MATRIX_BT601, g ? BINYUV_RANGE_FULL : BINYUV_RANGE_LIMITED};
            if (int rc = coefficients(&f, &coef.k[2 * m + g], nullptr)) return rc;
        }
    const uint64_t limit = (uint64_t)YUV_MAX_ELEMS;
    const uint64_t pixels = (uint64_t)ch * (uint64_t)cw;                                                         // below 2^62
    if (pixels > limit || 3 * pixels * (uint64_t)n_rows > limit) return BINCROP_E_SHAPE;                         // (below 2^42 * 2^31)
    if ((uint64_t)arena_bytes > limit) return BINCROP_E_SHAPE;
    const uint64_t out_bytes = 3 * pixels * (uint64_t)n_rows;
    const uint64_t table_bytes = (uint64_t)n_rows * sizeof(BinCropRow);
    if (overlap(out, out_bytes, arena, (uint64_t)arena_bytes) || overlap(out, out_bytes, rows, table_bytes)) return BINCROP_E_ARG;
    const bool c420 = chroma == BINYUV_CHROMA_420;
    const bool outvec = cw % 4 == 0 && aligned(out, 4);
    const int ng = (int)(((int64_t)cw + 3) / 4);
    const int64_t items = (int64_t)n_rows * ch * ng;
    const auto kernel = c420 ? (outvec ? yuv_crops_to_bgr_kernel<true, true> : yuv_crops_to_bgr_kernel<true, false>)
                             : (outvec ? yuv_crops_to_bgr_kernel<false, true> : yuv_crops_to_bgr_kernel<false, false>);
    return launch(kernel, grid_for(items), stream, arena, arena_bytes, rows, ch, cw, ng, items, coef, out);
}
