/*
 * binclip.h — flat C ABI of libbinclip.so: the Y4M payloads of a clip -> the uint8 HWC BGR frames of the device frame cache on the
 * MI355X (gfx950), the fill of a training arena from sharp high-frame-rate video (bin_amd/data/video_dataset.py, dataset mode
 * `BIN_video`).  The companion of libbinhip.so, libbinopt.so, libbingrad.so, libbinema.so, libbinens.so, libbinyuv.so,
 * libbinscene.so, libbinchain.so, libbinrate.so and libbinscore.so, and a library of its own for the same reason as each of those:
 * their interfaces are untouched by it, and a binder that never trains from video never loads it.
 *
 * Conventions are binyuv.h's: every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains
 * device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host synchronisation inside;
 * return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.
 *
 * The format (BinYuvFormat and its BINYUV_* constants) and the plane shapes are binyuv.h's, included here and not redeclared:
 * a payload is Y[H][W], U[ch][cw], V[ch][cw], contiguous, 4:2:0 or 4:4:4; odd H and W are legal.
 *
 * Per pixel: (r, g, b) is binyuv_to_frame's value (same coefficients, same fp32 expressions, clamped to [0, 1]; 4:2:0 chroma is
 * replicated: pixel (y, x) takes sample (y >> 1, x >> 1)), and each byte is (uint8)rintf(channel * 255.f) (one fp32 product, rounded
 * half to even), stored B, G, R.  That is binhip_frame_to_u8 of binyuv_to_frame without pads, byte for byte, in one launch for all
 * n frames and without the fp32 frame in between.
 *
 * Data paths.  A lane owns 4 consecutive pixels of a row (of two rows at 4:2:0, so a chroma pair is loaded once).  When W % 4 == 0,
 * `payloads` and `bgr_hwc` are 4-byte aligned and payload_stride % 4 == 0, every plane row of every frame is 4-byte (a 4:2:0 chroma
 * row 2-byte) aligned: Y and 4:4:4 chroma move as dwords, a 4:2:0 chroma pair as one 16-bit word, and the 4 pixels of a row leave as
 * one 12-byte store.  Anything else moves bytes.  Both paths evaluate the same per-pixel function and give the same bits.
 * Nothing outside the n payloads (the padding between them included) is read, nothing outside bgr_hwc written; indices are 64-bit.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "binyuv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINCLIP_API) are its ONLY dynamic symbols. */
#define BINCLIP_API __attribute__((visibility("default")))

#define BINCLIP_VERSION 100        /* what binclip_version() of a matching library returns */

#define BINCLIP_E_ARG   (-1)       /* null pointer / bad value   (= BINYUV_E_ARG)   */
#define BINCLIP_E_SHAPE (-2)       /* unsupported shape          (= BINYUV_E_SHAPE) */

BINCLIP_API int binclip_version(void);

/* payloads + i * payload_stride, i < n: the payload of frame i of an H x W stream -> bgr_hwc, uint8 [n][H][W][3], contiguous (the
 * arena layout of binhip_gather_windows).
 * BINCLIP_E_ARG: a null pointer, n, H or W < 1, payload_stride below the bytes of a frame, an unknown chroma / matrix / range,
 *   bgr_hwc overlapping the bytes from payloads to the end of the last payload.
 * BINCLIP_E_SHAPE: n * H * W * 3 or n * payload_stride beyond 2^40.                                                            */
BINCLIP_API int binclip_yuv_to_bgr(const uint8_t* payloads, int n, int64_t payload_stride, int H, int W,
                                   const BinYuvFormat* format, uint8_t* bgr_hwc, void* stream);

#ifdef __cplusplus
}
#endif
