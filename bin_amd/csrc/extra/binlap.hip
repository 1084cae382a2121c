// binlap.hip (libbinlap.so, include/binlap.h) — the Laplacian-pyramid term of the training criterion `cb+lap`: its value and its
// gradient over up to 24 (x, y) pairs of fp32 planes in one call.  The arithmetic is the header's specification, all of it in
// double; fp32 only at the loads of x, y, g and at the final stores.  Level 0 (d = x - y) is never materialised: the kernels that
// read it form it from x and y.
// Two tile geometries, each a kernel template:
//   down: a workgroup owns LD_TH x LD_TW COARSE pixels of one plane of one term and stages the (2 LD_TH + 3) x (2 LD_TW + 3) fine
//         pixels its five stride-2 taps reach, even and odd columns in LDS arrays of their own so that the row pass reads at stride 1
//         (stride 2 in doubles is a two-way bank conflict); row pass, then column pass.  Forward: R, fine values staged with the
//         clamp.  Adjoint: E^T r_l, the staged values r_l (0 outside the plane), subtracted from G_{l+1} in place.
//   up:   a workgroup owns LU_TH x LU_TW FINE pixels and stages the (LU_TH / 2 + 3) x (LU_TW / 2 + 3) coarse pixels E and R^T reach
//         (g_{l+1} with the clamp; G_{l+1} - E^T r_l with 0 outside the plane).  Forward: the band and its Charbonnier sum, one
//         workspace slot per workgroup.  Adjoint: G_l = r_l + R^T(...), at level 0 scaled by g[t] and stored as gx, -gy.
// R^T and E^T have constant weights except in the first and last row / column, where the generic weight functions count the taps
// that the clamp folds there.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/binlap.h"

namespace {
constexpr int LP_THREADS = 256;
constexpr int LD_TH = BINLAP_DOWN_TILE_H, LD_TW = BINLAP_DOWN_TILE_W;
constexpr int LD_FH = 2 * LD_TH + 3, LD_FW = 2 * LD_TW + 3;    // staged fine rows, columns: fine 2 c0 - 2 .. 2 (c0 + T - 1) + 2
constexpr int LD_HW = LD_TW + 2;                               // columns of one parity among them
constexpr int LD_CH = LD_TH + 4, LD_CW = LD_TW + 4;            // adjoint: coarse c0 - 2 .. c0 + T + 1, what E reaches from those
constexpr int LU_TH = BINLAP_UP_TILE_H, LU_TW = BINLAP_UP_TILE_W;
constexpr int LU_CH = LU_TH / 2 + 3, LU_CW = LU_TW / 2 + 3;    // coarse p0 / 2 - 1 .. p0 / 2 + T / 2 + 1
constexpr int LP_FINAL_THREADS = 256;
static_assert(LU_TH % 2 == 0 && LU_TW % 2 == 0, "a tile starts at an even pixel");
static_assert((LU_TH * LU_TW) % LP_THREADS == 0 && LP_THREADS % 64 == 0, "whole rounds, whole waves");
static_assert((LD_FH * 2 * LD_HW + LD_FH * LD_TW + LD_CH * LD_CW) * sizeof(double) <= 64 * 1024, "static LDS");

struct LapLevels {                   // the final launch's view of the slots: per level where they start, how many per term, 1 / n_l
    unsigned long long first[BINLAP_MAX_LEVELS];
    unsigned count[BINLAP_MAX_LEVELS];
    double inv_n[BINLAP_MAX_LEVELS];
    int levels;
};

inline int ld_tiles(int n, int tile) { return (n + tile - 1) / tile; }

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ inline double tap(int a) { return a == 2 ? 0.375 : (a == 1 || a == 3) ? 0.25 : 0.0625; }   // K[a]

// E along one dimension at fine p: the weights of coarse (p - 1) >> 1 and its two successors (the clamp is the staging's)
__device__ inline void expand_weights(int p, double w[3]) {
    const bool even = (p & 1) == 0;
    w[0] = even ? 0.125 : 0.5;
    w[1] = even ? 0.75 : 0.5;
    w[2] = even ? 0.125 : 0.0;
}
// R^T along one dimension at fine j of n (coarse size m): the weights of the same three coarse pixels
__device__ inline void reduce_t_weights(int j, int n, int m, double w[3]) {
    if (j > 0 && j < n - 1) {
        const bool even = (j & 1) == 0;
        w[0] = even ? 0.0625 : 0.25;
        w[1] = even ? 0.375 : 0.25;
        w[2] = even ? 0.0625 : 0.0;
        return;
    }
    const int base = (j - 1) >> 1;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int i = base + k;
        double s = 0.0;
        if (i >= 0 && i < m) {
#pragma unroll
            for (int a = 0; a < 5; ++a)
                if (clampi(2 * i + a - 2, 0, n - 1) == j) s += tap(a);
        }
        w[k] = s;
    }
}
// E^T along one dimension at coarse c of m (fine size n): the weight of fine p = 2 c - 2 + a
__device__ inline double expand_t_weight(int a, int c, int n, int m) {
    if (c > 0 && c < m - 1) return 2.0 * tap(a);
    const int p = 2 * c - 2 + a;
    double s = 0.0;
    if (p >= 0 && p < n) {
#pragma unroll
        for (int b = 0; b < 5; ++b) {
            const int e = p + b - 2;
            if ((e & 1) == 0 && clampi(e >> 1, 0, m - 1) == c) s += 2.0 * tap(b);
        }
    }
    return s;
}
}  // namespace

// grid (planes * tiles_y * tiles_x, n_terms); one workgroup = LD_TH x LD_TW coarse pixels of one plane of one term.
// gf: level l of all terms in double, null = level 0 (x - y).  ADJ = false: out = level l + 1 = R(level l).
// ADJ = true: gc = level l + 1, out = G_{l+1}, replaced in place by G_{l+1} - E^T r_l.
template <bool ADJ>
__global__ void __launch_bounds__(LP_THREADS)
lap_down_kernel(const BinLapTerms terms, int planes, int hf, int wf, int hc, int wc, int tiles_x, int tiles_y,
                const double* __restrict__ gf, const double* __restrict__ gc, double* __restrict__ out, double eps, double inv_n) {
    __shared__ double sf[LD_FH][2][LD_HW];           // [row][column parity][column / 2]
    __shared__ double hp[LD_FH][LD_TW];              // after the row pass
    __shared__ double sc[ADJ ? LD_CH : 1][ADJ ? LD_CW : 1];
    const int t = threadIdx.x, term = blockIdx.y;
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)tiles_x);
    b /= (unsigned)tiles_x;
    const int ty = (int)(b % (unsigned)tiles_y);
    const size_t plane = b / (unsigned)tiles_y;
    const size_t fbase = plane * hf * wf, cbase = ((size_t)term * planes + plane) * hc * wc;
    const float* __restrict__ x = terms.x[term] + fbase;
    const float* __restrict__ y = terms.y[term] + fbase;
    const double* __restrict__ gfp = gf ? gf + (size_t)term * planes * hf * wf + fbase : nullptr;
    const int ci0 = ty * LD_TH, cj0 = tx * LD_TW;

    if (ADJ) {
        const double* __restrict__ gcp = gc + cbase;
        for (int idx = t; idx < LD_CH * LD_CW; idx += LP_THREADS) {
            const int r = idx / LD_CW, c = idx - r * LD_CW;
            sc[r][c] = gcp[(size_t)clampi(ci0 - 2 + r, 0, hc - 1) * wc + clampi(cj0 - 2 + c, 0, wc - 1)];
        }
        __syncthreads();
    }
    for (int idx = t; idx < LD_FH * LD_FW; idx += LP_THREADS) {
        const int r = idx / LD_FW, c = idx - r * LD_FW;
        int pi = 2 * ci0 - 2 + r, pj = 2 * cj0 - 2 + c;
        double v = 0.0;
        if (!ADJ) {                                  // R reads through the clamp
            pi = clampi(pi, 0, hf - 1);
            pj = clampi(pj, 0, wf - 1);
        }
        if (pi >= 0 && pi < hf && pj >= 0 && pj < wf) {
            const size_t off = (size_t)pi * wf + pj;
            v = gfp ? gfp[off] : (double)x[off] - (double)y[off];
            if (ADJ) {                               // r_l = b / sqrt(b^2 + eps) / n_l, b = g_l - E(g_{l+1})
                double wi[3], wj[3];
                expand_weights(pi, wi);
                expand_weights(pj, wj);
                const int lr = ((pi - 1) >> 1) - (ci0 - 2), lc = ((pj - 1) >> 1) - (cj0 - 2);
                double e = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int m = 0; m < 3; ++m) e += (wi[k] * wj[m]) * sc[lr + k][lc + m];
                const double band = v - e;
                v = band / sqrt(band * band + eps) * inv_n;
            }
        }
        sf[r][c & 1][c >> 1] = v;
    }
    __syncthreads();
    // the row pass: coarse column cj reads staged columns 2 cj .. 2 cj + 4
    for (int idx = t; idx < LD_FH * LD_TW; idx += LP_THREADS) {
        const int r = idx / LD_TW, cj = idx - r * LD_TW;
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const double w = ADJ ? expand_t_weight(a, cj0 + cj, wf, wc) : tap(a);
            acc += w * sf[r][a & 1][cj + (a >> 1)];
        }
        hp[r][cj] = acc;
    }
    __syncthreads();
    // the column pass: coarse row ci reads rows 2 ci .. 2 ci + 4
    double* __restrict__ op = out + cbase;
    for (int idx = t; idx < LD_TH * LD_TW; idx += LP_THREADS) {
        const int ci = idx / LD_TW, cj = idx - ci * LD_TW;
        const int gi = ci0 + ci, gj = cj0 + cj;
        if (gi >= hc || gj >= wc) continue;
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a < 5; ++a) {
            const double w = ADJ ? expand_t_weight(a, gi, hf, hc) : tap(a);
            acc += w * hp[2 * ci + a][cj];
        }
        const size_t off = (size_t)gi * wc + gj;
        op[off] = ADJ ? op[off] - acc : acc;
    }
}

// grid (planes * tiles_y * tiles_x, n_terms); one workgroup = LU_TH x LU_TW fine pixels of one plane of one term.
// gf: level l in double, null = level 0; gc: level l + 1, null = l is the last level (b_l = g_l).
// BWD = false: part[term * gridDim.x + blockIdx.x] = the sum of sqrt(b^2 + eps) over the tile.
// BWD = true: qc = G_{l+1} - E^T r_l (null with gc); G_l = r_l + R^T qc goes to gout (double), or with a null gout (level 0) to
// gx[t] = g[t] G_0, gy[t] = -g[t] G_0.  pad: null, or one double that the first workgroup writes as 0.
template <bool BWD>
__global__ void __launch_bounds__(LP_THREADS)
lap_up_kernel(const BinLapTerms terms, int planes, int hf, int wf, int hc, int wc, int tiles_x, int tiles_y,
              const double* __restrict__ gf, const double* __restrict__ gc, const double* __restrict__ qc, double* __restrict__ gout,
              const float* __restrict__ g, double* __restrict__ part, double* __restrict__ pad, double eps, double inv_n) {
    __shared__ double sc[LU_CH][LU_CW];
    __shared__ double sq[BWD ? LU_CH : 1][BWD ? LU_CW : 1];
    __shared__ double red[LP_THREADS / 64];
    const int t = threadIdx.x, term = blockIdx.y;
    unsigned b = blockIdx.x;
    const int tx = (int)(b % (unsigned)tiles_x);
    b /= (unsigned)tiles_x;
    const int ty = (int)(b % (unsigned)tiles_y);
    const size_t plane = b / (unsigned)tiles_y;
    const size_t fbase = plane * hf * wf;
    const float* __restrict__ x = terms.x[term] + fbase;
    const float* __restrict__ y = terms.y[term] + fbase;
    const double* __restrict__ gfp = gf ? gf + (size_t)term * planes * hf * wf + fbase : nullptr;
    const int i0 = ty * LU_TH, j0 = tx * LU_TW;
    const int c0i = i0 / 2 - 1, c0j = j0 / 2 - 1;    // the first staged coarse row, column

    if (gc) {
        const size_t cbase = ((size_t)term * planes + plane) * hc * wc;
        for (int idx = t; idx < LU_CH * LU_CW; idx += LP_THREADS) {
            const int r = idx / LU_CW, c = idx - r * LU_CW;
            const int ci = c0i + r, cj = c0j + c;
            sc[r][c] = gc[cbase + (size_t)clampi(ci, 0, hc - 1) * wc + clampi(cj, 0, wc - 1)];
            if (BWD) sq[r][c] = (ci >= 0 && ci < hc && cj >= 0 && cj < wc) ? qc[cbase + (size_t)ci * wc + cj] : 0.0;
        }
        __syncthreads();
    }
    if (BWD && pad && blockIdx.x == 0 && blockIdx.y == 0 && t == 0) pad[0] = 0.0;

    double scale = 0.0;
    float* __restrict__ gxo = nullptr;
    float* __restrict__ gyo = nullptr;
    double* __restrict__ gop = nullptr;
    if (BWD) {
        if (gout) {
            gop = gout + (size_t)term * planes * hf * wf + fbase;
        } else {
            scale = (double)g[term];
            gxo = terms.gx[term];
            gyo = terms.gy[term];
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int it = 0; it < LU_TH * LU_TW / LP_THREADS; ++it) {
        const int idx = it * LP_THREADS + t;
        const int i = idx / LU_TW, j = idx - i * LU_TW;
        const int pi = i0 + i, pj = j0 + j;
        if (pi >= hf || pj >= wf) continue;
        const size_t off = (size_t)pi * wf + pj;
        double band = gfp ? gfp[off] : (double)x[off] - (double)y[off];
        const int lr = ((pi - 1) >> 1) - c0i, lc = ((pj - 1) >> 1) - c0j;
        if (gc) {
            double wi[3], wj[3];
            expand_weights(pi, wi);
            expand_weights(pj, wj);
            double e = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k)
#pragma unroll
                for (int m = 0; m < 3; ++m) e += (wi[k] * wj[m]) * sc[lr + k][lc + m];
            band -= e;
        }
        const double root = sqrt(band * band + eps);
        if (!BWD) {
            acc += root;
        } else {
            double grad = band / root * inv_n;
            if (gc) {
                double wi[3], wj[3];
                reduce_t_weights(pi, hf, hc, wi);
                reduce_t_weights(pj, wf, wc, wj);
                double s = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k)
#pragma unroll
                    for (int m = 0; m < 3; ++m) s += (wi[k] * wj[m]) * sq[lr + k][lc + m];
                grad += s;
            }
            if (gop) {
                gop[off] = grad;
            } else {
                if (gxo) gxo[fbase + off] = (float)(scale * grad);
                if (gyo) gyo[fbase + off] = (float)(-(scale * grad));
            }
        }
    }
    if (!BWD) {
        // the tile's sum: down each wave by shuffles, then the waves in order (pixels outside the plane added nothing)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
        if ((t & 63) == 0) red[t >> 6] = acc;
        __syncthreads();
        if (t == 0) {
            double s = red[0];
#pragma unroll
            for (int w = 1; w < LP_THREADS / 64; ++w) s += red[w];
            part[(size_t)term * gridDim.x + blockIdx.x] = s;
        }
    }
}

// grid (n_terms); per level the term's slots added in a fixed order, the level means added from level 0 up
__global__ void __launch_bounds__(LP_FINAL_THREADS)
lap_final_kernel(const double* __restrict__ slots, LapLevels lv, float* __restrict__ lap) {
    __shared__ double red[LP_FINAL_THREADS];
    const int t = threadIdx.x;
    double total = 0.0;
    for (int l = 0; l < lv.levels; ++l) {
        const double* p = slots + lv.first[l] + (size_t)blockIdx.x * lv.count[l];
        double acc = 0.0;
        for (unsigned s = t; s < lv.count[l]; s += LP_FINAL_THREADS) acc += p[s];
        red[t] = acc;
        __syncthreads();
        for (int o = LP_FINAL_THREADS / 2; o > 0; o >>= 1) {
            if (t < o) red[t] += red[t + o];
            __syncthreads();
        }
        total += red[0] * lv.inv_n[l];
        __syncthreads();
    }
    if (t == 0) lap[blockIdx.x] = (float)total;
}

namespace {
// whether [a, a + an) and [b, b + bn) share a byte
inline bool ranges_overlap(const void* a, size_t an, const void* b, size_t bn) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa <= pb ? pb - pa < an : pa - pb < bn;
}
inline bool misaligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) != 0; }

// what both entry points check of the terms; 0, or the refusal
int check_terms(const BinLapTerms* terms) {
    if (!terms) return BINLAP_E_ARG;
    if (terms->n_terms < 1 || terms->n_terms > BINLAP_MAX_TERMS) return BINLAP_E_ARG;
    for (int t = 0; t < terms->n_terms; ++t) {
        if (!terms->x[t] || !terms->y[t]) return BINLAP_E_ARG;
        if (misaligned(terms->x[t], 4) || misaligned(terms->y[t], 4)) return BINLAP_E_ARG;
    }
    return 0;
}
bool bad_values(int levels, double eps) { return levels < 1 || levels > BINLAP_MAX_LEVELS || !(eps > 0.0) || !isfinite(eps); }
bool bad_shape(int planes, int H, int W, int levels) {
    const int least = 1 << (levels - 1);
    return planes < 1 || H < least || W < least || (long long)planes * H > 0x7fffffffLL || (long long)planes * H * W > 0x7fffffffLL;
}
// whether `bytes` bytes at `p` overlap an input plane stack of any used term
bool overlaps_an_input(const BinLapTerms* terms, size_t plane_bytes, const void* p, size_t bytes) {
    for (int t = 0; t < terms->n_terms; ++t)
        if (ranges_overlap(p, bytes, terms->x[t], plane_bytes) || ranges_overlap(p, bytes, terms->y[t], plane_bytes)) return true;
    return false;
}

struct Pyramid {                     // a valid geometry: the level sizes and where the levels >= 1 lie in a workspace, in doubles
    int h[BINLAP_MAX_LEVELS], w[BINLAP_MAX_LEVELS];
    size_t at[BINLAP_MAX_LEVELS];    // level l >= 1 of all terms: at[l] .. at[l] + n_terms * planes * h[l] * w[l]
    size_t coarse;                   // the doubles of the levels >= 1 together
    size_t slots;                    // band tiles of all levels and terms
    LapLevels lv;
};
Pyramid pyramid(int n_terms, int planes, int H, int W, int levels) {
    Pyramid p = {};
    p.lv.levels = levels;
    for (int l = 0; l < levels; ++l) {
        p.h[l] = l ? (p.h[l - 1] + 1) / 2 : H;
        p.w[l] = l ? (p.w[l - 1] + 1) / 2 : W;
        p.at[l] = p.coarse;
        if (l) p.coarse += (size_t)n_terms * planes * p.h[l] * p.w[l];
        p.lv.first[l] = p.slots;
        p.lv.count[l] = (unsigned)((size_t)planes * ld_tiles(p.h[l], LU_TH) * ld_tiles(p.w[l], LU_TW));   // <= planes * H * W
        p.lv.inv_n[l] = 1.0 / ((double)planes * (double)p.h[l] * (double)p.w[l]);
        p.slots += (size_t)n_terms * p.lv.count[l];
    }
    return p;
}
bool refused(int n_terms, int planes, int H, int W, int levels) {
    return n_terms < 1 || n_terms > BINLAP_MAX_TERMS || levels < 1 || levels > BINLAP_MAX_LEVELS || bad_shape(planes, H, W, levels);
}

// level l -> l + 1 of the pyramid in `pyr` for all terms
void launch_reduces(const BinLapTerms& terms, int planes, const Pyramid& p, double* pyr, double eps, hipStream_t stream) {
    for (int l = 0; l + 1 < p.lv.levels; ++l) {
        const int tx = ld_tiles(p.w[l + 1], LD_TW), ty = ld_tiles(p.h[l + 1], LD_TH);
        hipLaunchKernelGGL(lap_down_kernel<false>, dim3((unsigned)((size_t)planes * ty * tx), terms.n_terms), dim3(LP_THREADS), 0, stream,
                           terms, planes, p.h[l], p.w[l], p.h[l + 1], p.w[l + 1], tx, ty, l ? (const double*)(pyr + p.at[l]) : nullptr,
                           (const double*)nullptr, pyr + p.at[l + 1], eps, 0.0);
    }
}
}  // namespace

int binlap_version(void) { return BINLAP_VERSION; }

size_t binlap_forward_workspace_bytes(int n_terms, int planes, int H, int W, int levels) {
    if (refused(n_terms, planes, H, W, levels)) return 0;
    const Pyramid p = pyramid(n_terms, planes, H, W, levels);
    return sizeof(double) * (p.coarse + p.slots);
}

size_t binlap_backward_workspace_bytes(int n_terms, int planes, int H, int W, int levels) {
    if (refused(n_terms, planes, H, W, levels)) return 0;
    const Pyramid p = pyramid(n_terms, planes, H, W, levels);
    return sizeof(double) * (p.coarse ? 2 * p.coarse : 1);
}

int binlap_forward(const BinLapTerms* terms, int planes, int H, int W, int levels, double eps, void* ws, size_t ws_bytes, float* lap,
                   void* stream) {
    if (const int rc = check_terms(terms)) return rc;
    if (!ws || !lap || misaligned(ws, 8) || misaligned(lap, 4)) return BINLAP_E_ARG;
    if (bad_values(levels, eps)) return BINLAP_E_ARG;
    if (bad_shape(planes, H, W, levels)) return BINLAP_E_SHAPE;
    const int n = terms->n_terms;
    const size_t need = binlap_forward_workspace_bytes(n, planes, H, W, levels), plane_bytes = sizeof(float) * (size_t)planes * H * W;
    if (overlaps_an_input(terms, plane_bytes, lap, sizeof(float) * n) || overlaps_an_input(terms, plane_bytes, ws, need) ||
        ranges_overlap(lap, sizeof(float) * n, ws, need))
        return BINLAP_E_ARG;
    if (ws_bytes < need) return BINLAP_E_WORKSPACE;
    const Pyramid p = pyramid(n, planes, H, W, levels);
    double* pyr = (double*)ws;
    double* slots = pyr + p.coarse;
    const hipStream_t s = (hipStream_t)stream;
    launch_reduces(*terms, planes, p, pyr, eps, s);
    for (int l = 0; l < levels; ++l) {
        const bool last = l == levels - 1;
        const int tx = ld_tiles(p.w[l], LU_TW), ty = ld_tiles(p.h[l], LU_TH);
        hipLaunchKernelGGL(lap_up_kernel<false>, dim3(p.lv.count[l], n), dim3(LP_THREADS), 0, s, *terms, planes, p.h[l], p.w[l],
                           last ? 0 : p.h[l + 1], last ? 0 : p.w[l + 1], tx, ty, l ? (const double*)(pyr + p.at[l]) : nullptr,
                           last ? nullptr : (const double*)(pyr + p.at[l + 1]), (const double*)nullptr, (double*)nullptr,
                           (const float*)nullptr, slots + p.lv.first[l], (double*)nullptr, eps, 0.0);
    }
    hipLaunchKernelGGL(lap_final_kernel, dim3(n), dim3(LP_FINAL_THREADS), 0, s, (const double*)slots, p.lv, lap);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}

int binlap_backward(const BinLapTerms* terms, int planes, int H, int W, int levels, double eps, const float* g, void* ws,
                    size_t ws_bytes, void* stream) {
    if (const int rc = check_terms(terms)) return rc;
    const int n = terms->n_terms;
    for (int t = 0; t < n; ++t) {
        if (!terms->gx[t] && !terms->gy[t]) return BINLAP_E_ARG;
        if (misaligned(terms->gx[t], 4) || misaligned(terms->gy[t], 4)) return BINLAP_E_ARG;
    }
    if (!g || !ws || misaligned(g, 4) || misaligned(ws, 8)) return BINLAP_E_ARG;
    if (bad_values(levels, eps)) return BINLAP_E_ARG;
    if (bad_shape(planes, H, W, levels)) return BINLAP_E_SHAPE;
    const size_t need = binlap_backward_workspace_bytes(n, planes, H, W, levels), plane_bytes = sizeof(float) * (size_t)planes * H * W;
    const float* outs[2 * BINLAP_MAX_TERMS];
    int n_outs = 0;
    for (int t = 0; t < n; ++t) {
        if (terms->gx[t]) outs[n_outs++] = terms->gx[t];
        if (terms->gy[t]) outs[n_outs++] = terms->gy[t];
    }
    for (int a = 0; a < n_outs; ++a) {
        if (overlaps_an_input(terms, plane_bytes, outs[a], plane_bytes) || ranges_overlap(outs[a], plane_bytes, g, sizeof(float) * n) ||
            ranges_overlap(outs[a], plane_bytes, ws, need))
            return BINLAP_E_ARG;
        for (int b = 0; b < a; ++b)
            if (ranges_overlap(outs[a], plane_bytes, outs[b], plane_bytes)) return BINLAP_E_ARG;
    }
    if (overlaps_an_input(terms, plane_bytes, ws, need) || ranges_overlap(ws, need, g, sizeof(float) * n)) return BINLAP_E_ARG;
    if (ws_bytes < need) return BINLAP_E_WORKSPACE;
    const Pyramid p = pyramid(n, planes, H, W, levels);
    double* pyr = (double*)ws;
    double* adj = pyr + p.coarse;                    // G_l at adj + at[l], l >= 1; with one level the pad double
    const hipStream_t s = (hipStream_t)stream;
    launch_reduces(*terms, planes, p, pyr, eps, s);
    for (int l = levels - 1; l >= 0; --l) {
        const bool last = l == levels - 1;
        if (!last) {                                 // G_{l+1} -> G_{l+1} - E^T r_l, in place
            const int tx = ld_tiles(p.w[l + 1], LD_TW), ty = ld_tiles(p.h[l + 1], LD_TH);
            hipLaunchKernelGGL(lap_down_kernel<true>, dim3((unsigned)((size_t)planes * ty * tx), n), dim3(LP_THREADS), 0, s, *terms, planes,
                               p.h[l], p.w[l], p.h[l + 1], p.w[l + 1], tx, ty, l ? (const double*)(pyr + p.at[l]) : nullptr,
                               (const double*)(pyr + p.at[l + 1]), adj + p.at[l + 1], eps, p.lv.inv_n[l]);
        }
        const int tx = ld_tiles(p.w[l], LU_TW), ty = ld_tiles(p.h[l], LU_TH);
        hipLaunchKernelGGL(lap_up_kernel<true>, dim3(p.lv.count[l], n), dim3(LP_THREADS), 0, s, *terms, planes, p.h[l], p.w[l],
                           last ? 0 : p.h[l + 1], last ? 0 : p.w[l + 1], tx, ty, l ? (const double*)(pyr + p.at[l]) : nullptr,
                           last ? nullptr : (const double*)(pyr + p.at[l + 1]), last ? nullptr : (const double*)(adj + p.at[l + 1]),
                           l ? adj + p.at[l] : nullptr, g, (double*)nullptr, p.coarse ? nullptr : adj, eps, p.lv.inv_n[l]);
    }
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
