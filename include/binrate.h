/*
 * binrate.h — flat C ABI of libbinrate.so: the mix of two fp32 RGB frames converted straight to 8-bit planar YUV on the MI355X
 * (gfx950), the hot step of the frame-rate resampler (bin_amd/rate.py, `python -m bin_amd.test --input_video ... --output_rate N[:D]`).
 * The companion of libbinyuv.so, and a library of its own for the same reason as each of the others: their interfaces are untouched
 * by it, and a binder that never resamples never loads it.
 *
 * Conventions are binyuv.h's: every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains
 * device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host synchronisation inside;
 * return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.  Formats, plane layouts and the frame -> YUV conversion are binyuv.h's.
 *
 * Per channel value, with a and b the two frames' values at one place and 0 <= w < 1 the weight of b, every operation rounded to
 * fp32 on its own (no fused multiply-add):
 *
 *   ca = fminf(fmaxf(a, 0), 1),  cb = fminf(fmaxf(b, 0), 1)         (NaN -> 0, -inf -> 0, +inf -> 1: nothing propagates)
 *   c  = ca + w * (cb - ca)
 *
 * and c goes through binyuv_from_frame's frame -> YUV conversion, the same code.  So w == 0 gives the bytes of
 * binyuv_from_frame(a) for any a and b, and a == b gives them for any w.
 *
 * Data paths are binyuv_from_frame's: a lane owns 4 consecutive pixels of a row (of two rows at 4:2:0); when W % 4 == 0, `left` and
 * Wp keep the fp32 rows 16-byte aligned, BOTH fp32 pointers are 16-byte and every plane pointer 4-byte aligned, fp32 moves as 16
 * bytes, Y and 4:4:4 chroma as dwords and a 4:2:0 chroma pair as one 16-bit word; anything else moves single floats and bytes.  Both
 * paths give the same bits.  Nothing outside the planes and the two crops' rows is read or written; indices are 64-bit.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "binyuv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINRATE_API) are its ONLY dynamic symbols. */
#define BINRATE_API __attribute__((visibility("default")))

#define BINRATE_VERSION 100       /* what binrate_version() of a matching library returns */

#define BINRATE_E_ARG   (-1)      /* null pointer / bad value   (= BINYUV_E_ARG)   */
#define BINRATE_E_SHAPE (-2)      /* unsupported shape          (= BINYUV_E_SHAPE) */

BINRATE_API int binrate_version(void);

/* a_chw, b_chw: fp32 [3][Hp][Wp] each (the same address is allowed); the crop rows [top, top+H), columns [left, left+W) of
 * a + w (b - a), as defined above -> the planes y, u, v of an H x W picture.
 * BINRATE_E_ARG: a null pointer, a_chw or b_chw not 4-byte aligned, w NaN or outside [0, 1), Hp, Wp, H or W < 1, top or left < 0, a
 * crop that leaves the frame, an unknown chroma / matrix / range, a plane overlapping a frame or another plane.
 * BINRATE_E_SHAPE: 3*Hp*Wp beyond 2^40.                                                                                        */
BINRATE_API int binrate_blend_to_yuv(const float* a_chw, const float* b_chw, float w, int Hp, int Wp, int top, int left, int H, int W,
                                     const BinYuvFormat* format, uint8_t* y, uint8_t* u, uint8_t* v, void* stream);

#ifdef __cplusplus
}
#endif
