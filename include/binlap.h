/*
 * binlap.h — flat C ABI of libbinlap.so: the Laplacian-pyramid term of the training criterion `cb+lap`, value and gradient, on the
 * MI355X (gfx950) from fp32 frames that are on the device already (bin_amd/models/loss.py, `pixel_criterion: cb+lap`).  A library
 * of its own for the same reason as every other small library of the project: no other interface changes with it, and a binder
 * that never trains on the pyramid never loads it.
 *
 * Conventions are those of the other small headers: every pointer is a DEVICE pointer owned by the caller; the library never
 * allocates, frees or retains device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host
 * synchronisation inside; return value 0 = ok, negative = argument / shape / workspace error (returned before any HIP call),
 * positive = hipError_t.  No mutable process-global state; entry points are re-entrant.
 *
 * The function.  x, y: fp32 [planes][H][W], any values.  d = x - y is formed in double (both operands are exact there); the
 * pyramid is linear, so one pyramid of d serves.  K = (1, 4, 6, 4, 1) / 16, applied separably; a tap index that falls outside a
 * row or column is clamped to the edge.  Per dimension, with n the fine size and m = ceil(n / 2) the coarse size:
 *     reduce  R: n -> m,   R(g)[i] = sum_{a = 0..4} K[a] g[clamp(2 i + a - 2, 0, n - 1)]
 *     expand  E: m -> n,   E(c)[p] = sum_{a: (p + a - 2) even} 2 K[a] c[clamp((p + a - 2) / 2, 0, m - 1)]
 * (even p take (1, 6, 1) / 8 of c[p/2 - 1 .. p/2 + 1], odd p take (1, 1) / 2 of their two neighbours; the rows of both operators
 * sum to 1 at every size, odd sizes included).  With L levels (1 .. BINLAP_MAX_LEVELS):
 *     g_0 = d,  g_{l+1} = R(g_l),   b_l = g_l - E(g_{l+1}) for l < L - 1,   b_{L-1} = g_{L-1},
 *     lap(x, y) = sum_l mean_p sqrt(b_l[p]^2 + eps)
 * the mean of a level over all its n_l = planes h_l w_l elements; eps > 0 is not squared (the criterion passes 1e-6).  L = 1 is the
 * Charbonnier mean itself.  The gradient, with r_l = b_l / sqrt(b_l^2 + eps) / n_l:
 *     G_{L-1} = r_{L-1},   G_l = r_l + R^T (G_{l+1} - E^T r_l),   d lap / d x = G_0,   d lap / d y = -G_0.
 * R^T and E^T are gathers, irregular in the first and last rows and columns where the clamp folds taps onto the edge.  All
 * arithmetic is in double: the pyramid levels in the workspace, the bands, the sums and the adjoint; only the loads of x and y and
 * the final stores are fp32, each result rounded once.
 *
 * A call covers up to BINLAP_MAX_TERMS (x, y) pairs of one shape; the number of launches depends on `levels` only (2 L forward,
 * 3 L - 2 backward).  A term's value and gradients are the same bits whatever other terms share the call, and two calls give the
 * same bits: partial sums go to fixed workspace slots and are added in a fixed order, there are no atomics.  Every byte of every
 * output and of the used workspace is written, whatever it held before; nothing outside them is written, nothing outside the
 * planes and the used workspace is read.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINLAP_API) are its ONLY dynamic symbols. */
#define BINLAP_API __attribute__((visibility("default")))

#define BINLAP_VERSION 100          /* what binlap_version() of a matching library returns */

#define BINLAP_E_ARG       (-1)     /* null pointer / bad value   */
#define BINLAP_E_SHAPE     (-2)     /* unsupported shape          */
#define BINLAP_E_WORKSPACE (-3)     /* workspace too small        */

#define BINLAP_MAX_TERMS 24         /* pairs per call */
#define BINLAP_MAX_LEVELS 8         /* pyramid levels */

#define BINLAP_DOWN_TILE_H 16       /* COARSE pixels per workgroup of the kernels that walk a fine level onto the coarser one (R, E^T) */
#define BINLAP_DOWN_TILE_W 32
#define BINLAP_UP_TILE_H 32         /* FINE pixels per workgroup of the kernels that walk a coarse level onto the finer one (E, R^T): */
#define BINLAP_UP_TILE_W 64         /*   the bands, whose partial sums the forward workspace query counts, one per tile              */

typedef struct BinLapTerms {        /* passed by value into the kernels */
    const float* x[BINLAP_MAX_TERMS];
    const float* y[BINLAP_MAX_TERMS];
    float* gx[BINLAP_MAX_TERMS];    /* backward only: d loss / d x of term t, [planes][H][W]; null = not wanted */
    float* gy[BINLAP_MAX_TERMS];    /* backward only: d loss / d y of term t; null = not wanted                 */
    int32_t n_terms;                /* 1 .. BINLAP_MAX_TERMS; entries from n_terms on are ignored */
} BinLapTerms;

BINLAP_API int binlap_version(void);

/* Bytes of workspace binlap_forward needs: the levels 1 .. L - 1 of every term's pyramid in double, and one double per band tile
 * (BINLAP_UP_TILE_H x BINLAP_UP_TILE_W) of every plane of every level of every term.  0 = a term count, a geometry or a level
 * count that binlap_forward refuses. */
BINLAP_API size_t binlap_forward_workspace_bytes(int n_terms, int planes, int H, int W, int levels);

/* Bytes of workspace binlap_backward needs: the levels 1 .. L - 1 of every term's pyramid and of its adjoint G in double; one
 * double (written as 0) when levels = 1, so that 0 always means a refusal.  0 = what binlap_backward refuses of these arguments. */
BINLAP_API size_t binlap_backward_workspace_bytes(int n_terms, int planes, int H, int W, int levels);

/* lap[t] = lap(x[t], y[t]) for t < n_terms, as fp32: L - 1 reduce launches, L band launches and one final launch for all terms.
 * gx / gy are ignored.
 * BINLAP_E_ARG: a null terms, ws or lap; n_terms outside 1 .. BINLAP_MAX_TERMS; a null x or y of a used term; an x, y or lap
 *   that is not 4-byte aligned, a ws that is not 8-byte aligned; levels outside 1 .. BINLAP_MAX_LEVELS; an eps that is not
 *   finite or not > 0; lap or the used workspace overlapping an input or each other.
 * BINLAP_E_SHAPE: planes < 1; min(H, W) < 2^(levels - 1); planes * H * W > 2^31 - 1.
 * BINLAP_E_WORKSPACE: ws_bytes below binlap_forward_workspace_bytes(n_terms, planes, H, W, levels).
 * Checked in this order: pointers and counts, levels and eps, the shape, the overlaps, the workspace size.                        */
BINLAP_API int binlap_forward(const BinLapTerms* terms, int planes, int H, int W, int levels, double eps, void* ws, size_t ws_bytes,
                              float* lap, void* stream);

/* gx[t] = g[t] * d lap(x[t], y[t]) / d x[t] = g[t] G_0 and gy[t] = -g[t] G_0, for every non-null gx[t] / gy[t].  It takes x, y
 * and g only, nothing a forward call left behind: it rebuilds the pyramid.  g: [n_terms] fp32 on the device.
 * BINLAP_E_ARG: a null terms, g or ws; n_terms outside 1 .. BINLAP_MAX_TERMS; a null x or y of a used term; a used term with
 *   neither gx nor gy; an x, y, gx, gy or g that is not 4-byte aligned, a ws that is not 8-byte aligned; levels outside
 *   1 .. BINLAP_MAX_LEVELS; an eps that is not finite or not > 0; an output or the used workspace overlapping an input (x, y of
 *   any term, or g), an output overlapping another output (an output named twice) or the used workspace.
 * BINLAP_E_SHAPE: as binlap_forward.
 * BINLAP_E_WORKSPACE: ws_bytes below binlap_backward_workspace_bytes(n_terms, planes, H, W, levels).
 * Checked in this order: pointers and counts (the terms, then g and ws), levels and eps, the shape, the overlaps, the workspace
 * size.                                                                                                                           */
BINLAP_API int binlap_backward(const BinLapTerms* terms, int planes, int H, int W, int levels, double eps, const float* g,
                               void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
