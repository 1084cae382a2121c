// binrate.hip (libbinrate.so, include/binrate.h) — the streaming kernel of the frame-rate resampler (bin_amd/rate.py):
//   blend_to_yuv_kernel : the crops of two fp32 planar RGB frames, mixed as ca + w (cb - ca) on clamped values -> 8-bit planar YUV.
// The twin of yuv_from_frame_kernel (binyuv.hip) with a second input: HBM-bound and element-wise, no LDS, no reuse beyond a lane's
// own registers.  A lane owns 4 consecutive pixels of a row, of two rows at 4:2:0; blockIdx.x grid-strides over (row or row pair,
// column group) items with 64-bit indices.  Data paths (binrate.h): VEC moves float4s / dwords / 16-bit chroma pairs, the other path
// single floats and bytes; both fill the same registers and call the same per-pixel functions (binyuv_common.h, shared with
// binyuv.hip: the conversion is written once), so they agree bit for bit.  The mix is written with the rounding intrinsics: nothing
// is left to contraction.  All of a lane's loads come before its first store.
#include "binyuv_common.h"
#include "../../include/binrate.h"

static_assert(sizeof(BinYuvFormat) == 12, "BinYuvFormat layout");
static_assert(BINRATE_E_ARG == BINYUV_E_ARG && BINRATE_E_SHAPE == BINYUV_E_SHAPE, "one set of error codes");

namespace {
// clamp first (NaN -> 0, -inf -> 0, +inf -> 1), then the mix: w == 0 and a == b both give clamp01(a), whatever a and b hold
__device__ __forceinline__ float mix(float a, float b, float w) {
    const float ca = clamp01(a), cb = clamp01(b);
    return __fadd_rn(ca, __fmul_rn(w, __fsub_rn(cb, ca)));
}
}  // namespace

// Item (j, g): crop columns 4g .. 4g+3 of crop row j (4:4:4) or of crop rows 2j, 2j+1 (4:2:0: chroma row j, chroma columns 2g, 2g+1).
// Lanes past the crop's edge clamp their source coordinate to it and store nothing there.
template <bool VEC, bool C420>
__global__ void __launch_bounds__(YUV_THREADS)
blend_to_yuv_kernel(const float* __restrict__ xa, const float* __restrict__ xb, const float w, const int Hp, const int Wp,
                    const int top, const int left, const int H, const int W, const int cw, const int ng, const int64_t items,
                    const FromCoef k, uint8_t* __restrict__ Yp, uint8_t* __restrict__ Up, uint8_t* __restrict__ Vp) {
    constexpr int R = C420 ? 2 : 1;
    const int64_t plane = (int64_t)Hp * Wp, stride = (int64_t)gridDim.x * YUV_THREADS;
    const bool small = items < ((int64_t)1 << 31);
    for (int64_t item = (int64_t)blockIdx.x * YUV_THREADS + threadIdx.x; item < items; item += stride) {
        int j, g;
        split(item, ng, small, j, g);
        const int x0 = 4 * g, y0 = R * j;
        float ar[R][4], ag[R][4], ab[R][4], br[R][4], bg[R][4], bb[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int yy = y0 + r < H ? y0 + r : H - 1;
            const int64_t at = (int64_t)(top + yy) * Wp + left;
            const float *sa = xa + at, *sb = xb + at;
            if (VEC) {
                const float4 a0 = *reinterpret_cast<const float4*>(sa + x0);
                const float4 a1 = *reinterpret_cast<const float4*>(sa + plane + x0);
                const float4 a2 = *reinterpret_cast<const float4*>(sa + 2 * plane + x0);
                const float4 b0 = *reinterpret_cast<const float4*>(sb + x0);
                const float4 b1 = *reinterpret_cast<const float4*>(sb + plane + x0);
                const float4 b2 = *reinterpret_cast<const float4*>(sb + 2 * plane + x0);
                ar[r][0] = a0.x; ar[r][1] = a0.y; ar[r][2] = a0.z; ar[r][3] = a0.w;
                ag[r][0] = a1.x; ag[r][1] = a1.y; ag[r][2] = a1.z; ag[r][3] = a1.w;
                ab[r][0] = a2.x; ab[r][1] = a2.y; ab[r][2] = a2.z; ab[r][3] = a2.w;
                br[r][0] = b0.x; br[r][1] = b0.y; br[r][2] = b0.z; br[r][3] = b0.w;
                bg[r][0] = b1.x; bg[r][1] = b1.y; bg[r][2] = b1.z; bg[r][3] = b1.w;
                bb[r][0] = b2.x; bb[r][1] = b2.y; bb[r][2] = b2.z; bb[r][3] = b2.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int xx = x0 + i < W ? x0 + i : W - 1;
                    ar[r][i] = sa[xx]; ag[r][i] = sa[plane + xx]; ab[r][i] = sa[2 * plane + xx];
                    br[r][i] = sb[xx]; bg[r][i] = sb[plane + xx]; bb[r][i] = sb[2 * plane + xx];
                }
            }
        }
        float ly[R][4], pb[R][4], pr[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rgb_pixel(mix(ar[r][i], br[r][i], w), mix(ag[r][i], bg[r][i], w), mix(ab[r][i], bb[r][i], w), k, ly[r][i], pb[r][i],
                          pr[r][i]);
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

int binrate_version(void) { return BINRATE_VERSION; }

int binrate_blend_to_yuv(const float* a_chw, const float* b_chw, float w, int Hp, int Wp, int top, int left, int H, int W,
                         const BinYuvFormat* format, uint8_t* y, uint8_t* u, uint8_t* v, void* stream) {
    FromCoef k;
    if (int rc = coefficients(format, nullptr, &k)) return rc;
    if (!a_chw || !b_chw || !y || !u || !v || !aligned(a_chw, 4) || !aligned(b_chw, 4)) return BINRATE_E_ARG;
    if (!(w >= 0.f && w < 1.f)) return BINRATE_E_ARG;            // (NaN compares false)
    if (Hp < 1 || Wp < 1 || H < 1 || W < 1 || top < 0 || left < 0) return BINRATE_E_ARG;
    if ((int64_t)top + H > Hp || (int64_t)left + W > Wp) return BINRATE_E_ARG;
    if (3 * (int64_t)Hp > YUV_MAX_ELEMS / Wp) return BINRATE_E_SHAPE;
    const bool c420 = format->chroma == BINYUV_CHROMA_420;
    const int ch = c420 ? (H + 1) / 2 : H, cw = c420 ? (W + 1) / 2 : W;
    const uint64_t in_bytes = (uint64_t)3 * Hp * Wp * 4, y_bytes = (uint64_t)H * W, c_bytes = (uint64_t)ch * cw;
    for (const float* x : {a_chw, b_chw})
        if (overlap(x, in_bytes, y, y_bytes) || overlap(x, in_bytes, u, c_bytes) || overlap(x, in_bytes, v, c_bytes)) return BINRATE_E_ARG;
    if (overlap(y, y_bytes, u, c_bytes) || overlap(y, y_bytes, v, c_bytes) || overlap(u, c_bytes, v, c_bytes)) return BINRATE_E_ARG;
    const bool vec = W % 4 == 0 && Wp % 4 == 0 && left % 4 == 0 && aligned(a_chw, 16) && aligned(b_chw, 16) && aligned(y, 4) &&
                     aligned(u, 4) && aligned(v, 4);
    const int ng = (W + 3) / 4;
    const int64_t items = (int64_t)ch * ng;
    const dim3 grid = grid_for(items), block(YUV_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const auto kernel = vec ? (c420 ? blend_to_yuv_kernel<true, true> : blend_to_yuv_kernel<true, false>)
                            : (c420 ? blend_to_yuv_kernel<false, true> : blend_to_yuv_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, a_chw, b_chw, w, Hp, Wp, top, left, H, W, cw, ng, items, k, y, u, v);
    return (int)hipGetLastError();
}
