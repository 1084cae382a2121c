/*
 * binssim.h — flat C ABI of libbinssim.so: the structural-similarity term of the training criterion `cb+ssim`, value and gradient,
 * on the MI355X (gfx950) from fp32 frames that are on the device already (bin_amd/models/loss.py, `pixel_criterion: cb+ssim`).  A
 * library of its own for the same reason as every other small library of the project: no other interface changes with it, and a
 * binder that never trains on SSIM never loads it.
 *
 * Conventions are those of the other small headers: every pointer but `taps11` is a DEVICE pointer owned by the caller; the library
 * never allocates, frees or retains device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously,
 * no host synchronisation inside; return value 0 = ok, negative = argument / shape / workspace error (returned before any HIP
 * call), positive = hipError_t.  No mutable process-global state; entry points are re-entrant.
 *
 * The function.  x, y: fp32 [planes][H][W], any values (they are not assumed to lie in [0, 1]).  w: the separable 11 x 11 window
 * whose 1-D taps the caller passes as `taps11` (11 doubles on the HOST, read during the call; the project passes the normalised
 * Gaussian of sigma 1.5).  Valid windows only: centres 5 <= i <= H - 6, 5 <= j <= W - 6, P = (H - 10)(W - 10) per plane.  With
 * C1 = 0.01^2, C2 = 0.03^2 (data range 1), per window q
 *     mx = sum w x, my = sum w y, exx = sum w x^2, eyy = sum w y^2, exy = sum w x y,
 *     sxx = exx - mx^2, syy = eyy - my^2, sxy = exy - mx my,
 *     A1 = 2 mx my + C1, A2 = 2 sxy + C2, B1 = mx^2 + my^2 + C1, B2 = sxx + syy + C2,   S_q = A1 A2 / (B1 B2)
 * and ssim(x, y) = the mean of S_q over all planes * P windows.  Its gradient, with T(m)(p) = sum_q w_qp m_q (each window's value
 * spread back over its 11 x 11 pixels):
 *     b = -2 S / B2,  c = 2 A1 / (B1 B2),  a_x = 2 my (A2 - A1) / (B1 B2) + 2 mx S (1 / B2 - 1 / B1),  a_y: mx and my exchanged,
 *     d ssim / d x_p = [T(a_x)(p) + x_p T(b)(p) + y_p T(c)(p)] / (planes P),   d ssim / d y_p: x and y exchanged.
 * The three summands cancel heavily (b reaches 2 / C2), so the window statistics, the formula, the coefficient maps and the
 * spreading are all in double; only the loads and the final stores are fp32, each result rounded once.
 *
 * A call covers up to BINSSIM_MAX_TERMS (x, y) pairs of one shape.  A term's value and gradients are the same bits whatever
 * other terms share the call, and two calls give the same bits: partial sums go to fixed workspace slots and are added in a
 * fixed order, there are no atomics.  Every byte of every output and of the used workspace is written, whatever it held before;
 * nothing outside them is written, nothing outside the planes is read.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINSSIM_API) are its ONLY dynamic symbols. */
#define BINSSIM_API __attribute__((visibility("default")))

#define BINSSIM_VERSION 100         /* what binssim_version() of a matching library returns */

#define BINSSIM_E_ARG       (-1)    /* null pointer / bad value   */
#define BINSSIM_E_SHAPE     (-2)    /* unsupported shape          */
#define BINSSIM_E_WORKSPACE (-3)    /* workspace too small        */

#define BINSSIM_MAX_TERMS 24        /* pairs per call */

#define BINSSIM_FWD_TILE_H 16       /* windows per workgroup of the forward: rows, columns (what the workspace query counts) */
#define BINSSIM_FWD_TILE_W 118
#define BINSSIM_BWD_TILE_H 32       /* pixels per workgroup of the backward: rows, columns */
#define BINSSIM_BWD_TILE_W 32

typedef struct BinSsimTerms {       /* passed by value into the kernels */
    const float* x[BINSSIM_MAX_TERMS];
    const float* y[BINSSIM_MAX_TERMS];
    float* gx[BINSSIM_MAX_TERMS];   /* backward only: d loss / d x of term t, [planes][H][W]; null = not wanted */
    float* gy[BINSSIM_MAX_TERMS];   /* backward only: d loss / d y of term t; null = not wanted                 */
    int32_t n_terms;                /* 1 .. BINSSIM_MAX_TERMS; entries from n_terms on are ignored */
} BinSsimTerms;

BINSSIM_API int binssim_version(void);

/* Bytes of workspace binssim_forward needs: one double per forward tile of every plane of every term.  0 = a geometry or a term
 * count that binssim_forward refuses. */
BINSSIM_API size_t binssim_workspace_bytes(int n_terms, int planes, int H, int W);

/* ssim[t] = ssim(x[t], y[t]) for t < n_terms, as fp32: one tile launch and one final launch for all terms.  gx / gy are ignored.
 * BINSSIM_E_ARG: a null terms, taps11, ws or ssim; n_terms outside 1 .. BINSSIM_MAX_TERMS; a null x or y of a used term; an x, y
 *   or ssim that is not 4-byte aligned, a ws that is not 8-byte aligned; ssim or the used workspace overlapping an input or
 *   each other.
 * BINSSIM_E_SHAPE: planes < 1; H < 11 or W < 11; planes * H * W > 2^31 - 1.
 * BINSSIM_E_WORKSPACE: ws_bytes below binssim_workspace_bytes(n_terms, planes, H, W).
 * Checked in this order: pointers and counts, the shape, the overlaps, the workspace size.                                        */
BINSSIM_API int binssim_forward(const BinSsimTerms* terms, int planes, int H, int W, const double* taps11,
                                void* ws, size_t ws_bytes, float* ssim, void* stream);

/* gx[t] = g[t] * d ssim(x[t], y[t]) / d x[t] and gy[t] likewise for y, for every non-null gx[t] / gy[t]: one launch for all terms.
 * It takes x, y, the taps and g only, nothing a forward call left behind.  g: [n_terms] fp32 on the device.
 * BINSSIM_E_ARG: a null terms, taps11 or g; n_terms outside 1 .. BINSSIM_MAX_TERMS; a null x or y of a used term; a used term
 *   with neither gx nor gy; a pointer that is not 4-byte aligned; an output that overlaps an input (x, y of any term, or g) or
 *   another output (an output named twice).
 * BINSSIM_E_SHAPE: as binssim_forward.                                                                                            */
BINSSIM_API int binssim_backward(const BinSsimTerms* terms, int planes, int H, int W, const double* taps11,
                                 const float* g, void* stream);

#ifdef __cplusplus
}
#endif
