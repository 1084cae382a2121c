// binssim.hip (libbinssim.so, include/binssim.h) — the SSIM term of the training criterion `cb+ssim`: its value and its gradient
// over up to 24 (x, y) pairs of fp32 planes in one call.  The arithmetic is the header's specification: window statistics, the
// SSIM formula, the coefficient maps and their spreading in double (the gradient's three summands cancel by a factor up to
// 2 / C2), fp32 only at the loads and the final stores.
// Forward: the tile walk of binhip_score_walk.h on fp32 data.  A workgroup owns SF_TH rows x SF_TE columns of windows of one plane
// of one term; it stages both tiles with their 10 extra rows and columns in LDS, runs the vertical pass of its own column,
// publishes that row of column sums in LDS and runs the horizontal pass from there.  Its sum goes to its own workspace slot; the
// final launch adds a term's slots in a fixed order.
// Backward: a workgroup owns SB_TH x SB_TW pixels of one plane of one term and recomputes the statistics of every window that
// reaches them (centres within 5 pixels of the tile, inputs within 10).  Centre rows are walked SB_R at a time: column sums ->
// window statistics and the four coefficients a_x, a_y, b, c -> their spread along the row into `hm`; the spread down the columns
// and the combination with x_p, y_p follow once all rows are there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/binssim.h"

namespace {
constexpr int SF_THREADS = 128;
constexpr int SF_TH = BINSSIM_FWD_TILE_H, SF_TE = BINSSIM_FWD_TILE_W;
constexpr int SF_ROWS = SF_TH + 10;                  // staged rows: a window's 11 rows start at its own
static_assert(SF_TE == SF_THREADS - 10, "thread t owns input column t of the tile; windows start at columns 0 .. SF_TE - 1");
constexpr int SF_FINAL_THREADS = 256;

constexpr int SB_THREADS = 256;
constexpr int SB_TH = BINSSIM_BWD_TILE_H, SB_TW = BINSSIM_BWD_TILE_W;
constexpr int SB_CH = SB_TH + 10, SB_CW = SB_TW + 10;    // window centres that reach the tile: rows, columns
constexpr int SB_SW = SB_TW + 20;                        // input columns those windows read
constexpr int SB_R = 4;                                  // centre rows per pass
static_assert(SB_R * SB_SW <= SB_THREADS && SB_R * SB_CW <= SB_THREADS, "one item per thread in the statistics passes");
static_assert((4 * SB_R * SB_TW) % SB_THREADS == 0 && (SB_TH * SB_TW) % SB_THREADS == 0, "whole rounds in the spreading passes");
static_assert((5 * SB_R * SB_SW + 4 * SB_R * SB_CW + 4 * SB_CH * SB_TW) * sizeof(double) <= 64 * 1024, "static LDS");

struct SsimTaps { double w[11]; };

constexpr double SSIM_C1 = 0.01 * 0.01, SSIM_C2 = 0.03 * 0.03;

inline int sf_tiles_x(int W) { return (W - 10 + SF_TE - 1) / SF_TE; }
inline int sf_tiles_y(int H) { return (H - 10 + SF_TH - 1) / SF_TH; }
inline int sb_tiles_x(int W) { return (W + SB_TW - 1) / SB_TW; }
inline int sb_tiles_y(int H) { return (H + SB_TH - 1) / SB_TH; }
}  // namespace

// grid (planes * tiles_y * tiles_x, n_terms); one workgroup = SF_TH x SF_TE windows of one plane of one term
__global__ void __launch_bounds__(SF_THREADS)
ssim_fwd_tile_kernel(const BinSsimTerms terms, int H, int W, int tiles_x, int tiles_y, SsimTaps taps, double* __restrict__ part) {
    __shared__ float sx[SF_ROWS][SF_THREADS], sy[SF_ROWS][SF_THREADS];
    __shared__ double vg[2][5][SF_THREADS];          // column sums of one row, double-buffered: one barrier per row
    __shared__ double red[SF_THREADS];
    const int t = threadIdx.x, term = blockIdx.y;
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)tiles_x);
    b /= (unsigned)tiles_x;
    const int ty = (int)(b % (unsigned)tiles_y);
    const size_t plane = b / (unsigned)tiles_y;
    const float* __restrict__ x = terms.x[term] + plane * H * W;
    const float* __restrict__ y = terms.y[term] + plane * H * W;
    const int i0 = ty * SF_TH;                       // first window row of the tile = its first input row
    const int e = tx * SF_TE + t;                    // this thread's input column
    const bool ecol = e < W;

    // stage input rows i0 .. i0 + SF_ROWS - 1; zero outside (no counted window reaches them)
    for (int r = 0; r < SF_ROWS; ++r) {
        const int gi = i0 + r;
        float xv = 0.f, yv = 0.f;
        if (ecol && gi < H) {
            xv = x[(size_t)gi * W + e];
            yv = y[(size_t)gi * W + e];
        }
        sx[r][t] = xv;
        sy[r][t] = yv;
    }
    // (a thread reads back only its own column: no barrier before the vertical pass)

    const bool outcol = t < SF_TE && e <= W - 11;    // a window starts at this column
    const int rows = min(SF_TH, H - 10 - i0);
    double acc = 0.0;
    for (int ro = 0; ro < rows; ++ro) {
        const int buf = ro & 1;
        if (ecol) {                                  // vertical pass: staged rows ro .. ro + 10
            double gx = 0.0, gy = 0.0, gxx = 0.0, gyy = 0.0, gxy = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double xv = (double)sx[ro + k][t], yv = (double)sy[ro + k][t];
                const double w = taps.w[k];
                gx += w * xv;
                gy += w * yv;
                gxx += w * (xv * xv);
                gyy += w * (yv * yv);
                gxy += w * (xv * yv);
            }
            vg[buf][0][t] = gx; vg[buf][1][t] = gy; vg[buf][2][t] = gxx; vg[buf][3][t] = gyy; vg[buf][4][t] = gxy;
        }
        __syncthreads();
        if (outcol) {                                // horizontal pass: columns t .. t + 10, all inside the row
            double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
            for (int k = 0; k < 11; ++k) {
                const double w = taps.w[k];
                mx += w * vg[buf][0][t + k]; my += w * vg[buf][1][t + k];
                exx += w * vg[buf][2][t + k]; eyy += w * vg[buf][3][t + k]; exy += w * vg[buf][4][t + k];
            }
            const double sxx = exx - mx * mx, syy = eyy - my * my, sxy = exy - mx * my;
            const double A1 = 2.0 * mx * my + SSIM_C1, A2 = 2.0 * sxy + SSIM_C2;
            const double B1 = mx * mx + my * my + SSIM_C1, B2 = sxx + syy + SSIM_C2;
            acc += (A1 * A2) / (B1 * B2);
        }
    }

    // the tile's sum: a tree over the columns (those without a window hold 0)
    red[t] = acc;
    __syncthreads();
    for (int o = SF_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) part[(size_t)term * gridDim.x + blockIdx.x] = red[0];
}

// grid (n_terms); adds the `slots` partial sums of a term in a fixed order
__global__ void __launch_bounds__(SF_FINAL_THREADS)
ssim_fwd_final_kernel(const double* __restrict__ part, unsigned slots, double count, float* __restrict__ ssim) {
    __shared__ double red[SF_FINAL_THREADS];
    const int t = threadIdx.x;
    const double* p = part + (size_t)blockIdx.x * slots;
    double acc = 0.0;
    for (unsigned s = t; s < slots; s += SF_FINAL_THREADS) acc += p[s];
    red[t] = acc;
    __syncthreads();
    for (int o = SF_FINAL_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) ssim[blockIdx.x] = (float)(red[0] / count);
}

// grid (planes * tiles_y * tiles_x, n_terms); one workgroup = SB_TH x SB_TW pixels of one plane of one term
__global__ void __launch_bounds__(SB_THREADS)
ssim_bwd_kernel(const BinSsimTerms terms, int H, int W, int tiles_x, int tiles_y, SsimTaps taps, double inv_count,
                const float* __restrict__ g) {
    __shared__ double vs[5][SB_R][SB_SW];            // column sums of SB_R centre rows
    __shared__ double cm[4][SB_R][SB_CW];            // a_x, a_y, b, c of those rows' windows
    __shared__ double hm[4][SB_CH][SB_TW];           // the same, spread along the row onto the tile's columns
    const int t = threadIdx.x, term = blockIdx.y;
    unsigned bid = blockIdx.x;
    const int tx = (int)(bid % (unsigned)tiles_x);
    bid /= (unsigned)tiles_x;
    const int ty = (int)(bid % (unsigned)tiles_y);
    const size_t plane = bid / (unsigned)tiles_y;
    const size_t base = plane * H * W;
    const float* __restrict__ x = terms.x[term] + base;
    const float* __restrict__ y = terms.y[term] + base;
    const int i0 = ty * SB_TH, j0 = tx * SB_TW;

    for (int r0 = 0; r0 < SB_CH; r0 += SB_R) {
        // column sums: centre row ci = i0 - 5 + r, input column j0 - 10 + c; zero where no counted window reads them
        if (t < SB_R * SB_SW) {
            const int rr = t / SB_SW, c = t - rr * SB_SW;
            const int ci = i0 - 5 + r0 + rr, col = j0 - 10 + c;
            double gx = 0.0, gy = 0.0, gxx = 0.0, gyy = 0.0, gxy = 0.0;
            if (r0 + rr < SB_CH && ci >= 5 && ci <= H - 6 && col >= 0 && col < W) {
                const float* px = x + (size_t)(ci - 5) * W + col;
                const float* py = y + (size_t)(ci - 5) * W + col;
                float xr[11], yr[11];
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    xr[k] = px[(size_t)k * W];
                    yr[k] = py[(size_t)k * W];
                }
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const double xv = (double)xr[k], yv = (double)yr[k];
                    const double w = taps.w[k];
                    gx += w * xv;
                    gy += w * yv;
                    gxx += w * (xv * xv);
                    gyy += w * (yv * yv);
                    gxy += w * (xv * yv);
                }
            }
            vs[0][rr][c] = gx; vs[1][rr][c] = gy; vs[2][rr][c] = gxx; vs[3][rr][c] = gyy; vs[4][rr][c] = gxy;
        }
        __syncthreads();
        // window statistics and coefficients: centre column cj = j0 - 5 + s reads sums s .. s + 10; zero for a window that is not counted
        if (t < SB_R * SB_CW) {
            const int rr = t / SB_CW, s = t - rr * SB_CW;
            const int ci = i0 - 5 + r0 + rr, cj = j0 - 5 + s;
            double ax = 0.0, ay = 0.0, cb = 0.0, cc = 0.0;
            if (r0 + rr < SB_CH && ci >= 5 && ci <= H - 6 && cj >= 5 && cj <= W - 6) {
                double mx = 0.0, my = 0.0, exx = 0.0, eyy = 0.0, exy = 0.0;
#pragma unroll
                for (int k = 0; k < 11; ++k) {
                    const double w = taps.w[k];
                    mx += w * vs[0][rr][s + k]; my += w * vs[1][rr][s + k];
                    exx += w * vs[2][rr][s + k]; eyy += w * vs[3][rr][s + k]; exy += w * vs[4][rr][s + k];
                }
                const double sxx = exx - mx * mx, syy = eyy - my * my, sxy = exy - mx * my;
                const double A1 = 2.0 * mx * my + SSIM_C1, A2 = 2.0 * sxy + SSIM_C2;
                const double B1 = mx * mx + my * my + SSIM_C1, B2 = sxx + syy + SSIM_C2;
                const double rB1 = 1.0 / B1, rB2 = 1.0 / B2, rBB = 1.0 / (B1 * B2);
                const double S = (A1 * A2) * rBB;
                const double u = 2.0 * (A2 - A1) * rBB, v = 2.0 * S * (rB2 - rB1);
                ax = my * u + mx * v;
                ay = mx * u + my * v;
                cb = -2.0 * S * rB2;
                cc = 2.0 * A1 * rBB;
            }
            cm[0][rr][s] = ax; cm[1][rr][s] = ay; cm[2][rr][s] = cb; cm[3][rr][s] = cc;
        }
        __syncthreads();
        // spread along the row: pixel column j takes centre s = j + k with the weight the window gives it, w[10 - k]
#pragma unroll
        for (int it = 0; it < 4 * SB_R * SB_TW / SB_THREADS; ++it) {
            const int idx = it * SB_THREADS + t;
            const int m = idx / (SB_R * SB_TW), rem = idx - m * (SB_R * SB_TW);
            const int rr = rem / SB_TW, j = rem - rr * SB_TW;
            if (r0 + rr < SB_CH) {
                double acc = 0.0;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc += taps.w[10 - k] * cm[m][rr][j + k];
                hm[m][r0 + rr][j] = acc;
            }
        }
        // (the next pass writes `vs` behind this pass's second barrier and `cm` behind its own first: no barrier here)
    }
    __syncthreads();

    // spread down the columns, combine with the pixel's own values, round once
    const double scale = (double)g[term] * inv_count;
    float* __restrict__ gxo = terms.gx[term];
    float* __restrict__ gyo = terms.gy[term];
#pragma unroll
    for (int it = 0; it < SB_TH * SB_TW / SB_THREADS; ++it) {
        const int idx = it * SB_THREADS + t;
        const int i = idx / SB_TW, j = idx - i * SB_TW;
        const int pi = i0 + i, pj = j0 + j;
        if (pi >= H || pj >= W) continue;
        double tax = 0.0, tay = 0.0, tb = 0.0, tc = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const double w = taps.w[10 - k];
            tax += w * hm[0][i + k][j]; tay += w * hm[1][i + k][j];
            tb += w * hm[2][i + k][j]; tc += w * hm[3][i + k][j];
        }
        const size_t off = (size_t)pi * W + pj;
        const double xv = (double)x[off], yv = (double)y[off];
        if (gxo) gxo[base + off] = (float)(scale * (tax + xv * tb + yv * tc));
        if (gyo) gyo[base + off] = (float)(scale * (tay + yv * tb + xv * tc));
    }
}

namespace {
// whether [a, a + an) and [b, b + bn) share a byte
inline bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa <= pb ? pb - pa < an : pa - pb < bn;
}
inline bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// what both entry points check of the terms and the shape; 0, or the refusal
int check_terms(const BinSsimTerms* terms, const double* taps11) {
    if (!terms || !taps11) return BINSSIM_E_ARG;
    if (terms->n_terms < 1 || terms->n_terms > BINSSIM_MAX_TERMS) return BINSSIM_E_ARG;
    for (int t = 0; t < terms->n_terms; ++t) {
        if (!terms->x[t] || !terms->y[t]) return BINSSIM_E_ARG;
        if (misaligned(terms->x[t], 4) || misaligned(terms->y[t], 4)) return BINSSIM_E_ARG;
    }
    return 0;
}
bool bad_shape(int planes, int H, int W) {
    return planes < 1 || H < 11 || W < 11 || (long long)planes * H > 0x7fffffffLL || (long long)planes * H * W > 0x7fffffffLL;
}
// whether an output of `bytes` bytes at `out` overlaps an input plane stack of any used term
bool overlaps_an_input(const BinSsimTerms* terms, size_t plane_bytes, const void* out, size_t bytes) {
    for (int t = 0; t < terms->n_terms; ++t)
        if (ranges_overlap(out, bytes, terms->x[t], plane_bytes) || ranges_overlap(out, bytes, terms->y[t], plane_bytes)) return true;
    return false;
}
SsimTaps load_taps(const double* taps11) {
    SsimTaps taps;
    for (int k = 0; k < 11; ++k) taps.w[k] = taps11[k];
    return taps;
}
}  // namespace

int binssim_version(void) { return BINSSIM_VERSION; }

size_t binssim_workspace_bytes(int n_terms, int planes, int H, int W) {
    if (n_terms < 1 || n_terms > BINSSIM_MAX_TERMS || bad_shape(planes, H, W)) return 0;
    return sizeof(double) * (size_t)n_terms * (size_t)planes * (size_t)sf_tiles_y(H) * (size_t)sf_tiles_x(W);
}

int binssim_forward(const BinSsimTerms* terms, int planes, int H, int W, const double* taps11, void* ws, size_t ws_bytes, float* ssim,
                    void* stream) {
    if (const int rc = check_terms(terms, taps11)) return rc;
    if (!ws || !ssim || misaligned(ws, 8) || misaligned(ssim, 4)) return BINSSIM_E_ARG;
    if (bad_shape(planes, H, W)) return BINSSIM_E_SHAPE;
    const int n = terms->n_terms;
    const size_t need = binssim_workspace_bytes(n, planes, H, W), plane_bytes = sizeof(float) * (size_t)planes * H * W;
    if (overlaps_an_input(terms, plane_bytes, ssim, sizeof(float) * n) || overlaps_an_input(terms, plane_bytes, ws, need) ||
        ranges_overlap(ssim, sizeof(float) * n, ws, need))
        return BINSSIM_E_ARG;
    if (ws_bytes < need) return BINSSIM_E_WORKSPACE;
    const int tiles_x = sf_tiles_x(W), tiles_y = sf_tiles_y(H);
    const unsigned slots = (unsigned)((size_t)planes * tiles_y * tiles_x);   // <= planes * H * W
    const double count = (double)planes * (double)(H - 10) * (double)(W - 10);
    hipLaunchKernelGGL(ssim_fwd_tile_kernel, dim3(slots, n), dim3(SF_THREADS), 0, (hipStream_t)stream, *terms, H, W, tiles_x, tiles_y,
                       load_taps(taps11), (double*)ws);
    hipLaunchKernelGGL(ssim_fwd_final_kernel, dim3(n), dim3(SF_FINAL_THREADS), 0, (hipStream_t)stream, (const double*)ws, slots, count,
                       ssim);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int binssim_backward(const BinSsimTerms* terms, int planes, int H, int W, const double* taps11, const float* g, void* stream) {
    if (const int rc = check_terms(terms, taps11)) return rc;
    if (!g || misaligned(g, 4)) return BINSSIM_E_ARG;
    const int n = terms->n_terms;
    for (int t = 0; t < n; ++t) {
        if (!terms->gx[t] && !terms->gy[t]) return BINSSIM_E_ARG;
        if (misaligned(terms->gx[t], 4) || misaligned(terms->gy[t], 4)) return BINSSIM_E_ARG;
    }
    if (bad_shape(planes, H, W)) return BINSSIM_E_SHAPE;
    const size_t plane_bytes = sizeof(float) * (size_t)planes * H * W;
    const float* outs[2 * BINSSIM_MAX_TERMS];
    int n_outs = 0;
    for (int t = 0; t < n; ++t) {
        if (terms->gx[t]) outs[n_outs++] = terms->gx[t];
        if (terms->gy[t]) outs[n_outs++] = terms->gy[t];
    }
    for (int a = 0; a < n_outs; ++a) {
        if (overlaps_an_input(terms, plane_bytes, outs[a], plane_bytes) || ranges_overlap(outs[a], plane_bytes, g, sizeof(float) * n))
            return BINSSIM_E_ARG;
        for (int b = 0; b < a; ++b)
            if (ranges_overlap(outs[a], plane_bytes, outs[b], plane_bytes)) return BINSSIM_E_ARG;
    }
    const int tiles_x = sb_tiles_x(W), tiles_y = sb_tiles_y(H);
    const unsigned blocks = (unsigned)((size_t)planes * tiles_y * tiles_x);  // <= planes * H * W
    const double inv_count = 1.0 / ((double)planes * (double)(H - 10) * (double)(W - 10));
    hipLaunchKernelGGL(ssim_bwd_kernel, dim3(blocks, n), dim3(SB_THREADS), 0, (hipStream_t)stream, *terms, H, W, tiles_x, tiles_y,
                       load_taps(taps11), inv_count, g);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
