/*
 * binyuv.h — flat C ABI of libbinyuv.so: 8-bit planar YUV <-> padded fp32 RGB frame on the MI355X (gfx950), the video-side
 * twins of binhip_u8_to_frame / binhip_frame_to_u8 (bin_amd/video.py, `python -m bin_amd.test --input_video`).  The companion of
 * libbinhip.so, libbinopt.so, libbingrad.so, libbinema.so and libbinens.so, and a library of its own for the same reason as each
 * of those: their interfaces are untouched by it, and a binder that never reads video never loads it.
 *
 * Conventions are binens.h's: every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains
 * device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host synchronisation inside;
 * return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.
 *
 * A format is (chroma, matrix, range).  Planes are 8-bit and contiguous: Y[H][W], U[ch][cw], V[ch][cw]; 4:2:0 has ch = ceil(H/2),
 * cw = ceil(W/2), 4:4:4 has ch = H, cw = W.  Odd H and W are legal.  With Kr, Kb of the matrix and Kg = 1 - Kr - Kb, in real
 * numbers (the kernels are fp32 and stay within 2^-20 of this on every element):
 *
 *   YUV -> frame   limited: y = (Y-16)/219, pb = (U-128)/224, pr = (V-128)/224;   full: y = Y/255, pb = (U-128)/255, pr = (V-128)/255
 *                  R = y + 2(1-Kr) pr,  B = y + 2(1-Kb) pb,  G = (y - Kr R - Kb B)/Kg  (R, B unclamped), each then clamped to [0, 1];
 *                  4:2:0 chroma is replicated: pixel (r, c) takes chroma sample (r>>1, c>>1);
 *                  out is fp32 planar RGB [3][H+pt+pb][W+pl+pr] with replicate padding: the tensor binhip_u8_to_frame produces.
 *   frame -> YUV   every value first goes through binhip_frame_to_u8's clamp fminf(fmaxf(v, 0), 1): NaN -> 0, -inf -> 0, +inf -> 1;
 *                  y = Kr R + Kg G + Kb B,  pb = (B-y)/(2(1-Kb)),  pr = (R-y)/(2(1-Kr));
 *                  4:2:0: pb, pr of a chroma sample are the mean over the pixels of its 2x2 block that lie inside the crop (4, 2 at
 *                  an odd edge, 1 at an odd corner), summed ((p00 + p01) + (p10 + p11)) and scaled by a power of two;
 *                  limited: Y = 16 + 219 y, U = 128 + 224 pb, V = 128 + 224 pr;   full: Y = 255 y, U = 128 + 255 pb, V = 128 + 255 pr;
 *                  rounded half to even (rintf) and clamped to 0..255.  No 8-bit RGB in between: one rounding only.
 * Replication up and the box mean down make the pair an exact round trip on every code point whose unclamped RGB lies in [0, 1].
 *
 * Data paths.  A lane owns 4 consecutive pixels of a row (of two rows at 4:2:0, so a chroma pair is loaded once).  When W % 4 == 0,
 * the pads (the crop's `left` and Wp) keep the fp32 rows 16-byte aligned, the fp32 pointer is 16-byte and every plane pointer
 * 4-byte aligned, Y and 4:4:4 chroma move as dwords, a 4:2:0 chroma pair as one 16-bit word and fp32 as 16 bytes; anything else
 * moves bytes and single floats.  Both paths evaluate the same per-pixel function and give the same bits.  (The U and V planes of
 * one contiguous payload start at H*W and H*W + ch*cw: odd sizes reach the byte path by themselves.)
 * Nothing outside the planes and the fp32 tensor is read or written; indices are 64-bit.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINYUV_API) are its ONLY dynamic symbols. */
#define BINYUV_API __attribute__((visibility("default")))

#define BINYUV_VERSION 100        /* what binyuv_version() of a matching library returns */

#define BINYUV_E_ARG   (-1)       /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINYUV_E_SHAPE (-2)       /* unsupported shape          (= BINHIP_E_SHAPE) */

#define BINYUV_CHROMA_420 420
#define BINYUV_CHROMA_444 444
#define BINYUV_MATRIX_BT601 0     /* Kr = 0.299,  Kb = 0.114  */
#define BINYUV_MATRIX_BT709 1     /* Kr = 0.2126, Kb = 0.0722 */
#define BINYUV_RANGE_LIMITED 0
#define BINYUV_RANGE_FULL 1

typedef struct BinYuvFormat {
    int32_t chroma;
    int32_t matrix;
    int32_t range;
} BinYuvFormat;

BINYUV_API int binyuv_version(void);

/* y, u, v: the three planes of an H x W picture (see above) -> out_chw, fp32 [3][H+pad_top+pad_bottom][W+pad_left+pad_right].
 * BINYUV_E_ARG: a null pointer, H or W < 1, a negative pad, an unknown chroma / matrix / range, out_chw not 4-byte aligned, out_chw
 * overlapping a plane.  BINYUV_E_SHAPE: a padded side beyond 2^31 - 1 or 3*Hp*Wp beyond 2^40.                                  */
BINYUV_API int binyuv_to_frame(const uint8_t* y, const uint8_t* u, const uint8_t* v, int H, int W, const BinYuvFormat* format,
                               int pad_left, int pad_right, int pad_top, int pad_bottom, float* out_chw, void* stream);

/* chw: fp32 [3][Hp][Wp]; the crop rows [top, top+H), columns [left, left+W) of it -> the planes y, u, v of an H x W picture.
 * BINYUV_E_ARG: a null pointer, Hp, Wp, H or W < 1, top or left < 0, a crop that leaves the frame, an unknown chroma / matrix /
 * range, chw not 4-byte aligned, a plane overlapping chw or another plane.  BINYUV_E_SHAPE: 3*Hp*Wp beyond 2^40.               */
BINYUV_API int binyuv_from_frame(const float* chw, int Hp, int Wp, int top, int left, int H, int W, const BinYuvFormat* format,
                                 uint8_t* y, uint8_t* u, uint8_t* v, void* stream);

#ifdef __cplusplus
}
#endif
