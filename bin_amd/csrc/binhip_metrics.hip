// binhip_metrics.hip — image-quality scores of the evaluation loop (test.py:404-456, utils/util.py:201-251):
//   per pair of HWC uint8 images: sum of squared and of absolute differences (exact), the Gaussian 11x11 SSIM of
//   utils/util.py:211-251 and the 7x7 uniform SSIM of skimage compare_ssim(multichannel=True), which test.py:31-36 uses.
// One tile walk serves all four, binhip_score_walk.h's (shared with libbinscore.so, whose loader reads the u8 planes of a YUV
// payload): a workgroup owns SC_TH image rows x 226 interleaved elements (element e = 3 x + channel, so a same-channel neighbour
// is 3 elements away and the 5-pixel halo is 15 elements).  Partial sums go to a fixed workspace slot per workgroup; a second
// launch adds the slots of an image in a fixed order, so two calls give the same bits.
// The walk is a template on its loader.  U8Pairs reads the interleaved u8 images above (binhip_image_score).  FramePairs
// (binhip_frame_score, the validation loop of models/bin_model.py:564-589) reads planar fp32 [3][H][W] frames through a table
// of pointers passed by value and quantises every value on load with tensor2img's expression (frame_to_u8_kernel), so the u8
// image exists in the LDS tiles only: one grid slice per (pair, channel), a same-channel neighbour 1 element away, a 5-column
// halo and 246 output columns per 256-thread row.
#include "binhip_internal.h"
#include "binhip_score_walk.h"

namespace {
static_assert(BINHIP_SCORE_SSIM_G11 == SC_FLAG_G11 && BINHIP_SCORE_SSIM_U7 == SC_FLAG_U7, "the header's flags are the walk's");
static_assert(sizeof(BinImageScore) == 32, "BinImageScore layout");

// Loaders of the tile walk.  STRIDE = distance in elements between same-channel neighbours of a row; a row of the walk has
// row_elems(W) elements, a 5-pixel halo of HALO elements on each side and TE output elements per 256-thread tile row.
struct U8Pairs {                                     // [n][H][W][3] u8, element e = 3 x + channel; grid z = pair
    static constexpr int STRIDE = 3, HALO = 5 * STRIDE, TE = SC_THREADS - 2 * HALO;      // 226 output elements
    const uint8_t *a, *b;
    __host__ __device__ static int row_elems(int W) { return 3 * W; }
    __device__ static int slice_flags(int, int flags) { return flags; }
    __device__ void load(int z, int gi, int e, int H, int W, uint8_t& xa, uint8_t& xb) const {
        const size_t o = ((size_t)z * H + gi) * (3 * (size_t)W) + e;
        xa = a[o];
        xb = b[o];
    }
};
struct FramePairs {                                  // planar fp32 [3][H][W] frames; grid z = 3 pair + channel
    static constexpr int STRIDE = 1, HALO = 5 * STRIDE, TE = SC_THREADS - 2 * HALO;      // 246 output columns
    const float* x[BINHIP_SCORE_MAX_PAIRS];
    const float* y[BINHIP_SCORE_MAX_PAIRS];
    __host__ __device__ static int row_elems(int W) { return W; }
    __device__ static int slice_flags(int, int flags) { return flags; }
    // tensor2img (utils/util.py:113-137), the expression of frame_to_u8_kernel: NaN -> 0, -inf -> 0, +inf -> 255
    __device__ static uint8_t quantise(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }
    __device__ void load(int z, int gi, int e, int H, int W, uint8_t& xa, uint8_t& xb) const {
        const int pair = z / 3, c = z - 3 * pair;
        const size_t o = ((size_t)c * H + gi) * (size_t)W + e;
        xa = quantise(x[pair][o]);
        xb = quantise(y[pair][o]);
    }
};
}  // namespace

// one workgroup per image pair: the slots of pair blockIdx.x in a fixed order, then the metrics
__global__ void __launch_bounds__(256)
image_score_final_kernel(const ScorePartial* __restrict__ part, int slots, int H, int W, int flags, BinImageScore* __restrict__ out) {
    __shared__ double sd[6][256];
    __shared__ long long sl[2][256];
    const int t = threadIdx.x;
    const ScorePartial* p = part + (size_t)blockIdx.x * slots;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    long long sse = 0, sad = 0;
    for (int s = t; s < slots; s += 256) {
        sse += p[s].sse;
        sad += p[s].sad;
        for (int c = 0; c < 3; ++c) {
            acc[c] += p[s].g11[c];
            acc[3 + c] += p[s].u7[c];
        }
    }
    for (int c = 0; c < 6; ++c) sd[c][t] = acc[c];
    sl[0][t] = sse;
    sl[1][t] = sad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            for (int c = 0; c < 6; ++c) sd[c][t] += sd[c][t + o];
            sl[0][t] += sl[0][t + o];
            sl[1][t] += sl[1][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double nan = __builtin_nan("");
        BinImageScore r;
        r.sse = sl[0][0];
        r.sad = sl[1][0];
        // per channel: mean of the valid map; then the mean of the three channels (util.calculate_ssim, compare_ssim)
        const double ng = (double)(H - 10) * (double)(W - 10), nu = (double)(H - 6) * (double)(W - 6);
        r.ssim_g11 = (flags & BINHIP_SCORE_SSIM_G11) ? (sd[0][0] / ng + sd[1][0] / ng + sd[2][0] / ng) / 3.0 : nan;
        r.ssim_u7 = (flags & BINHIP_SCORE_SSIM_U7) ? (sd[3][0] / nu + sd[4][0] / nu + sd[5][0] / nu) / 3.0 : nan;
        out[blockIdx.x] = r;
    }
}

static int score_shape(int n, int n_max, int H, int W, int flags) {
    if (flags & ~(BINHIP_SCORE_SSIM_G11 | BINHIP_SCORE_SSIM_U7)) return BINHIP_E_ARG;
    if (n <= 0 || n > n_max || H <= 0 || W <= 0 || H > 65535 || W > 65535) return BINHIP_E_SHAPE;
    if ((flags & BINHIP_SCORE_SSIM_G11) && (H < 11 || W < 11)) return BINHIP_E_SHAPE;
    if ((flags & BINHIP_SCORE_SSIM_U7) && (H < 7 || W < 7)) return BINHIP_E_SHAPE;
    return 0;
}

size_t binhip_image_score_workspace_bytes(int n, int H, int W, int flags) {
    if (score_shape(n, 65535, H, W, flags) != 0) return 0;
    return (size_t)n * sc_tiles_y(H) * sc_tiles_x<U8Pairs>(W) * sizeof(ScorePartial);
}

int binhip_image_score(const uint8_t* a, const uint8_t* b, int n, int H, int W, int flags, const double* g11_taps, void* ws,
                       size_t ws_bytes, BinImageScore* out, void* stream) {
    if (!a || !b || !ws || !out) return BINHIP_E_ARG;
    if ((flags & BINHIP_SCORE_SSIM_G11) && !g11_taps) return BINHIP_E_ARG;
    const int rc = score_shape(n, 65535, H, W, flags);
    if (rc != 0) return rc;
    if (ws_bytes < binhip_image_score_workspace_bytes(n, H, W, flags)) return BINHIP_E_WORKSPACE;
    ScoreTaps taps{};
    if (g11_taps)
        for (int k = 0; k < 11; ++k) taps.w[k] = g11_taps[k];
    hipStream_t s = (hipStream_t)stream;
    const int tx = sc_tiles_x<U8Pairs>(W), ty = sc_tiles_y(H);
    ScorePartial* part = (ScorePartial*)ws;
    const U8Pairs ld{a, b};
    hipLaunchKernelGGL(score_tile_kernel<U8Pairs>, dim3(tx, ty, n), dim3(SC_THREADS), 0, s, ld, H, W, flags, taps, part);
    hipLaunchKernelGGL(image_score_final_kernel, dim3(n), dim3(256), 0, s, part, tx * ty, H, W, flags, out);
    BH_CHECK_LAUNCH();
    return 0;
}

size_t binhip_frame_score_workspace_bytes(int n, int H, int W, int flags) {
    if (score_shape(n, BINHIP_SCORE_MAX_PAIRS, H, W, flags) != 0) return 0;
    return (size_t)n * 3 * sc_tiles_y(H) * sc_tiles_x<FramePairs>(W) * sizeof(ScorePartial);
}

int binhip_frame_score(const float* const* x, const float* const* y, int n, int H, int W, int flags, const double* g11_taps,
                       void* ws, size_t ws_bytes, BinImageScore* out, void* stream) {
    if (!x || !y || !ws || !out) return BINHIP_E_ARG;
    if ((flags & BINHIP_SCORE_SSIM_G11) && !g11_taps) return BINHIP_E_ARG;
    const int rc = score_shape(n, BINHIP_SCORE_MAX_PAIRS, H, W, flags);
    if (rc != 0) return rc;
    FramePairs ld{};
    for (int i = 0; i < n; ++i) {
        if (!x[i] || !y[i]) return BINHIP_E_ARG;
        ld.x[i] = x[i];
        ld.y[i] = y[i];
    }
    if (ws_bytes < binhip_frame_score_workspace_bytes(n, H, W, flags)) return BINHIP_E_WORKSPACE;
    ScoreTaps taps{};
    if (g11_taps)
        for (int k = 0; k < 11; ++k) taps.w[k] = g11_taps[k];
    hipStream_t s = (hipStream_t)stream;
    const int tx = sc_tiles_x<FramePairs>(W), ty = sc_tiles_y(H);
    ScorePartial* part = (ScorePartial*)ws;
    // slices 3 i .. 3 i + 2 are pair i's channels, so its 3 tx ty slots are consecutive: the final launch is the u8 path's
    hipLaunchKernelGGL(score_tile_kernel<FramePairs>, dim3(tx, ty, 3 * n), dim3(SC_THREADS), 0, s, ld, H, W, flags, taps, part);
    hipLaunchKernelGGL(image_score_final_kernel, dim3(n), dim3(256), 0, s, part, 3 * tx * ty, H, W, flags, out);
    BH_CHECK_LAUNCH();
    return 0;
}
