// binhip_metrics.hip — image-quality scores of the evaluation loop (test.py:404-456, utils/util.py:201-251):
//   per pair of HWC uint8 images: sum of squared and of absolute differences (exact), the Gaussian 11x11 SSIM of
//   utils/util.py:211-251 and the 7x7 uniform SSIM of skimage compare_ssim(multichannel=True), which test.py:31-36 uses.
// One tile walk serves all four: a workgroup owns SC_TH image rows x 226 interleaved elements (element e = 3 x + channel,
// so a same-channel neighbour is 3 elements away and the 5-pixel halo is 15 elements); it stages both u8 tiles with their
// halo in LDS, runs the vertical pass of its own column, publishes that row of column sums in LDS and runs the horizontal pass
// from there.  Partial sums go to a fixed workspace slot per workgroup; a second launch adds the slots of an image in a fixed
// order, so two calls give the same bits.
// The walk is a template on its loader.  U8Pairs reads the interleaved u8 images above (binhip_image_score).  FramePairs
// (binhip_frame_score, the validation loop of models/bin_model.py:564-589) reads planar fp32 [3][H][W] frames through a table
// of pointers passed by value and quantises every value on load with tensor2img's expression (frame_to_u8_kernel), so the u8
// image exists in the LDS tiles only: one grid slice per (pair, channel), a same-channel neighbour 1 element away, a 5-column
// halo and 246 output columns per 256-thread row.
#include "binhip_internal.h"

namespace {
constexpr int SC_THREADS = 256;
constexpr int SC_TH = 16;                            // output rows per tile
constexpr int SC_ROWS = SC_TH + 10;                  // staged rows: the tile and 5 halo rows above and below

struct ScoreTaps { double w[11]; };
struct ScorePartial { long long sse, sad; double g11[3], u7[3]; };
static_assert(sizeof(ScorePartial) == 64, "workspace slot");
static_assert(sizeof(BinImageScore) == 32, "BinImageScore layout");

// Loaders of the tile walk.  STRIDE = distance in elements between same-channel neighbours of a row; a row of the walk has
// row_elems(W) elements, a 5-pixel halo of HALO elements on each side and TE output elements per 256-thread tile row.
struct U8Pairs {                                     // [n][H][W][3] u8, element e = 3 x + channel; grid z = pair
    static constexpr int STRIDE = 3, HALO = 5 * STRIDE, TE = SC_THREADS - 2 * HALO;      // 226 output elements
    const uint8_t *a, *b;
    __host__ __device__ static int row_elems(int W) { return 3 * W; }
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
    // tensor2img (utils/util.py:113-137), the expression of frame_to_u8_kernel: NaN -> 0, -inf -> 0, +inf -> 255
    __device__ static uint8_t quantise(float v) { return (uint8_t)rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f); }
    __device__ void load(int z, int gi, int e, int H, int W, uint8_t& xa, uint8_t& xb) const {
        const int pair = z / 3, c = z - 3 * pair;
        const size_t o = ((size_t)c * H + gi) * (size_t)W + e;
        xa = quantise(x[pair][o]);
        xb = quantise(y[pair][o]);
    }
};

template <class L> int sc_tiles_x(int W) { return (L::row_elems(W) + L::TE - 1) / L::TE; }
int sc_tiles_y(int H) { return (H + SC_TH - 1) / SC_TH; }

// utils/util.py ssim(): m = ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)), C = (K 255)^2
__device__ __forceinline__ double ssim_g11(double mx, double my, double mxx, double myy, double mxy) {
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double s1 = mxx - mx * mx, s2 = myy - my * my, s12 = mxy - mx * my;
    return ((2.0 * mx * my + C1) * (2.0 * s12 + C2)) / ((mx * mx + my * my + C1) * (s1 + s2 + C2));
}
// skimage compare_ssim for uint8 (R = 255, K1 0.01, K2 0.03, sample covariance 49/48) from the exact 7x7 window sums
__device__ __forceinline__ double ssim_u7(int sx, int sy, int sxx, int syy, int sxy) {
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    const double NP = 49.0, cov_norm = NP / (NP - 1.0);
    const double ux = sx / NP, uy = sy / NP, uxx = sxx / NP, uyy = syy / NP, uxy = sxy / NP;
    const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
    const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
    return (A1 * A2) / (B1 * B2);
}
}  // namespace

// grid (tiles_x, tiles_y, slices of the loader); one workgroup = SC_TH rows x L::TE elements of one slice
template <class L>
__global__ void __launch_bounds__(SC_THREADS)
score_tile_kernel(const L ld, int H, int W, int flags, ScoreTaps taps, ScorePartial* __restrict__ part) {
    constexpr int SC_HALO = L::HALO, SC_TE = L::TE, SC_STRIDE = L::STRIDE;
    __shared__ uint8_t sa[SC_ROWS][SC_THREADS], sb[SC_ROWS][SC_THREADS];
    __shared__ double vg[2][5][SC_THREADS];          // column sums of one row, double-buffered: one barrier per row
    __shared__ int vu[2][5][SC_THREADS];
    __shared__ double rg[SC_THREADS], ru[SC_THREADS];
    __shared__ long long rs[SC_THREADS], rd[SC_THREADS];
    const int t = threadIdx.x;
    const int RW = L::row_elems(W);
    const int i0 = blockIdx.y * SC_TH, e0 = blockIdx.x * SC_TE;
    const int e = e0 - SC_HALO + t;                  // this thread's element column
    const bool ecol = e >= 0 && e < RW;
    const bool g11 = (flags & BINHIP_SCORE_SSIM_G11) != 0, u7 = (flags & BINHIP_SCORE_SSIM_U7) != 0;

    // stage rows i0-5 .. i0+SC_TH+4 of both images; zero outside (no counted window reaches them)
    for (int r = 0; r < SC_ROWS; ++r) {
        const int gi = i0 - 5 + r;
        uint8_t xa = 0, xb = 0;
        if (ecol && gi >= 0 && gi < H) ld.load(blockIdx.z, gi, e, H, W, xa, xb);
        sa[r][t] = xa;
        sb[r][t] = xb;
    }
    // (a thread reads back only its own column: no barrier before the vertical pass)

    const bool outcol = ecol && t >= SC_HALO && t < SC_HALO + SC_TE;
    const int j = e / SC_STRIDE;                     // pixel column (meaningful where ecol)
    const bool gcol = g11 && outcol && j >= 5 && j <= W - 6;
    const bool ucol = u7 && outcol && j >= 3 && j <= W - 4;
    double gacc = 0.0, uacc = 0.0;
    int sse = 0, sad = 0;                            // <= SC_TH x 65025
    const int rows = min(SC_TH, H - i0);
    for (int ro = 0; ro < rows; ++ro) {
        const int i = i0 + ro, buf = ro & 1;
        // vertical pass: staged rows ro .. ro+10 are image rows i-5 .. i+5
        if (g11 && ecol) {                           // (a column outside the row feeds no counted window)
            double gx = 0.0, gy = 0.0, gxx = 0.0, gyy = 0.0, gxy = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const int x = sa[ro + k][t], y = sb[ro + k][t];
                const double w = taps.w[k];
                gx += w * (double)x;
                gy += w * (double)y;
                gxx += w * (double)(x * x);
                gyy += w * (double)(y * y);
                gxy += w * (double)(x * y);
            }
            vg[buf][0][t] = gx; vg[buf][1][t] = gy; vg[buf][2][t] = gxx; vg[buf][3][t] = gyy; vg[buf][4][t] = gxy;
        }
        if (u7 && ecol) {
            int ux = 0, uy = 0, uxx = 0, uyy = 0, uxy = 0;
#pragma unroll
            for (int k = 2; k < 9; ++k) {            // image rows i-3 .. i+3
                const int x = sa[ro + k][t], y = sb[ro + k][t];
                ux += x; uy += y; uxx += x * x; uyy += y * y; uxy += x * y;
            }
            vu[buf][0][t] = ux; vu[buf][1][t] = uy; vu[buf][2][t] = uxx; vu[buf][3][t] = uyy; vu[buf][4][t] = uxy;
        }
        __syncthreads();
        if (outcol) {
            const int d = (int)sa[ro + 5][t] - (int)sb[ro + 5][t];
            sse += d * d;
            sad += d < 0 ? -d : d;
            // horizontal pass: same-channel neighbours at t + SC_STRIDE (k - 5)
            if (gcol && i >= 5 && i <= H - 6) {
                double mx = 0.0, my = 0.0, mxx = 0.0, myy = 0.0, mxy = 0.0;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const int s = t + SC_STRIDE * (k - 5);
                    const double w = taps.w[k];
                    mx += w * vg[buf][0][s]; my += w * vg[buf][1][s];
                    mxx += w * vg[buf][2][s]; myy += w * vg[buf][3][s]; mxy += w * vg[buf][4][s];
                }
                gacc += ssim_g11(mx, my, mxx, myy, mxy);
            }
            if (ucol && i >= 3 && i <= H - 4) {
                int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
                for (int k = -3; k <= 3; ++k) {
                    const int s = t + SC_STRIDE * k;
                    sx += vu[buf][0][s]; sy += vu[buf][1][s]; sxx += vu[buf][2][s]; syy += vu[buf][3][s]; sxy += vu[buf][4][s];
                }
                uacc += ssim_u7(sx, sy, sxx, syy, sxy);
            }
        }
    }

    // the tile's sums, per channel, in a fixed order
    rg[t] = gacc; ru[t] = uacc; rs[t] = sse; rd[t] = sad;
    __syncthreads();
    ScorePartial* p = part + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if constexpr (SC_STRIDE == 3) {
        if (t < 3) {                                 // channel t: output columns whose element % 3 == t
            double g = 0.0, u = 0.0;
            for (int s = SC_HALO + (t - e0 % 3 + 3) % 3; s < SC_HALO + SC_TE; s += 3) {
                g += rg[s];
                u += ru[s];
            }
            p->g11[t] = g;
            p->u7[t] = u;
        } else if (t == 3 || t == 4) {
            const long long* src = t == 3 ? rs : rd;
            long long v = 0;
            for (int s = 0; s < SC_THREADS; ++s) v += src[s];
            if (t == 3) p->sse = v; else p->sad = v;
        }
    } else {                                         // one channel per slice: a tree over the row (the halo columns hold 0)
        for (int o = SC_THREADS / 2; o > 0; o >>= 1) {
            if (t < o) {
                rg[t] += rg[t + o];
                ru[t] += ru[t + o];
                rs[t] += rs[t + o];
                rd[t] += rd[t + o];
            }
            __syncthreads();
        }
        if (t < 3) {                                 // the slice's channel; the other two add 0 in the final launch
            const bool mine = t == (int)(blockIdx.z % 3);
            p->g11[t] = mine ? rg[0] : 0.0;
            p->u7[t] = mine ? ru[0] : 0.0;
        } else if (t == 3) {
            p->sse = rs[0];
        } else if (t == 4) {
            p->sad = rd[0];
        }
    }
}

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
