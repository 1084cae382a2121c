// binhip_score_walk.h — the tile walk of the image-quality scores, ONE definition for libbinhip.so (binhip_metrics.hip: interleaved
// u8 images and planar fp32 frames) and libbinscore.so (binscore.hip: single u8 planes of a YUV payload).  Needs the HIP runtime
// only; each file that includes it brings its loaders, its final kernel and its record.
// Per pair of u8 images: the sum of squared and of absolute differences (exact), the Gaussian 11x11 SSIM of utils/util.py:211-251
// and the 7x7 uniform SSIM of skimage compare_ssim.  A workgroup owns SC_TH rows x L::TE elements of one slice of its loader; it
// stages both u8 tiles with their halo in LDS, runs the vertical pass of its own column, publishes that row of column sums in LDS
// and runs the horizontal pass from there.  Partial sums go to a fixed workspace slot per workgroup; a final launch of the
// including file adds the slots in a fixed order, so two calls give the same bits.
// A loader L has: STRIDE (distance in elements between same-channel neighbours of a row), HALO = 5 STRIDE, TE = SC_THREADS - 2 HALO
// output elements per 256-thread tile row, row_elems(W) elements per row, slice_flags(z, flags) (the SSIMs slice z is scored
// with) and load(z, gi, e, H, W, xa, xb): element e of row gi of slice z (grid z) of both images.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {
constexpr int SC_THREADS = 256;
constexpr int SC_TH = 16;                            // output rows per tile
constexpr int SC_ROWS = SC_TH + 10;                  // staged rows: the tile and 5 halo rows above and below
constexpr int SC_FLAG_G11 = 1, SC_FLAG_U7 = 2;       // the `flags` of the walk: the values of both libraries' headers

struct ScoreTaps { double w[11]; };
struct ScorePartial { long long sse, sad; double g11[3], u7[3]; };
static_assert(sizeof(ScorePartial) == 64, "workspace slot");

template <class L> int sc_tiles_x(int W) { return (L::row_elems(W) + L::TE - 1) / L::TE; }
inline int sc_tiles_y(int H) { return (H + SC_TH - 1) / SC_TH; }

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
    flags = ld.slice_flags(blockIdx.z, flags);
    const bool g11 = (flags & SC_FLAG_G11) != 0, u7 = (flags & SC_FLAG_U7) != 0;

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
