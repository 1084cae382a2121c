// binrate.hip (libbinrate.so, include/binrate.h) — the streaming kernel of the frame-rate resampler (bin_amd/rate.py):
//   blend_to_yuv_kernel : the crops of two fp32 planar RGB frames, mixed as ca + w (cb - ca) on clamped values -> 8-bit planar YUV.
// yuv_from_frame_kernel (binyuv.hip) with a second input: the same item geometry, the same stages of binyuv_common.h (load_rgb4
// once per frame, rgb_pixel, store_yuv), and between the loads and the conversion the mix, which is what is written here.  The mix
// uses the rounding intrinsics: nothing is left to contraction.  All of a lane's loads come before its first store.
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

// Item (j, g): as yuv_from_frame_kernel's.
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
        load_rgb4<VEC, R>(xa, plane, Wp, top, left, H, W, x0, y0, ar, ag, ab);
        load_rgb4<VEC, R>(xb, plane, Wp, top, left, H, W, x0, y0, br, bg, bb);
        float ly[R][4], pb[R][4], pr[R][4];
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                rgb_pixel(mix(ar[r][i], br[r][i], w), mix(ag[r][i], bg[r][i], w), mix(ab[r][i], bb[r][i], w), k, ly[r][i], pb[r][i],
                          pr[r][i]);
        store_yuv<VEC, C420, R>(ly, pb, pr, k, x0, y0, j, g, H, W, cw, Yp, Up, Vp);
    }
}

int binrate_version(void) { return BINRATE_VERSION; }

int binrate_blend_to_yuv(const float* a_chw, const float* b_chw, float w, int Hp, int Wp, int top, int left, int H, int W,
                         const BinYuvFormat* format, uint8_t* y, uint8_t* u, uint8_t* v, void* stream) {
    FromCoef k;
    YuvOutGeometry q;
    if (int rc = coefficients(format, nullptr, &k)) return rc;
    if (!a_chw || !b_chw || !aligned(a_chw, 4) || !aligned(b_chw, 4)) return BINRATE_E_ARG;
    if (!(w >= 0.f && w < 1.f)) return BINRATE_E_ARG;            // (NaN compares false)
    if (int rc = yuv_out_geometry(Hp, Wp, top, left, H, W, format, y, u, v, &q)) return rc;
    if (overlaps_planes(a_chw, q, y, u, v) || overlaps_planes(b_chw, q, y, u, v)) return BINRATE_E_ARG;
    const bool vec = q.vec && aligned(a_chw, 16) && aligned(b_chw, 16);
    const auto kernel = vec ? (q.c420 ? blend_to_yuv_kernel<true, true> : blend_to_yuv_kernel<true, false>)
                            : (q.c420 ? blend_to_yuv_kernel<false, true> : blend_to_yuv_kernel<false, false>);
    return launch(kernel, grid_for(q.items), stream, a_chw, b_chw, w, Hp, Wp, top, left, H, W, q.cw, q.ng, q.items, k, y, u, v);
}
