/*
 * bincrop.h — flat C ABI of libbincrop.so: crops of 8-bit planar YUV frames that lie in one byte arena -> uint8 HWC BGR crops on the
 * MI355X (gfx950), the per-batch decode of a device frame cache that is kept in YUV (bin_amd/data/video_dataset.py, dataset mode
 * `BIN_video` with `device_cache_format: yuv`).  A library of its own for the same reason as every other small library of the
 * project: no other interface changes with it (binclip.h least of all), and a binder that never trains from a YUV arena never loads it.
 *
 * Conventions are binclip.h's: every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains
 * device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host synchronisation inside;
 * return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.
 *
 * The arena is bytes.  A payload is binyuv.h's: Y[H][W], U[ch][cw], V[ch][cw], contiguous, of ONE chroma layout per call (4:2:0:
 * ceil(H/2) x ceil(W/2) planes; 4:4:4: H x W); odd H and W are legal.  Where a payload lies, how large its frame is, which crop of
 * it is wanted and which matrix and range it is decoded with travel per row of a table (BinCropRow), so frames of different sizes
 * and formats are decoded by one launch.
 *
 * Per pixel: output pixel (j, i) of row r has the three bytes binclip_yuv_to_bgr gives pixel (y0 + j, x0 + i) of that frame, by
 * construction: the coefficients and the per-pixel expressions are the one definition both libraries compile (4:2:0 chroma is
 * replicated: pixel (y, x) takes sample (y >> 1, x >> 1); each byte is (uint8)rintf(channel * 255.f), stored B, G, R).
 *
 * Data paths.  A lane owns 4 consecutive output columns of one output row; items grid-stride with 64-bit indices; all of a lane's
 * loads come before its first store.  Loads: when a row's payload address (arena + offset) is 4-byte aligned, its W % 4 == 0 and
 * its x0 % 4 == 0, the lane's 4 luma bytes move as one dword and its chroma as one 16-bit word (4:2:0) or one dword (4:4:4) per
 * plane; any other row moves bytes.  The choice is made per row, on the device.  Stores: when cw % 4 == 0 and `out` is 4-byte
 * aligned the 4 pixels leave as one 12-byte store, otherwise as bytes.  Every path evaluates the same per-pixel function on the same
 * bytes and gives the same bits.  Nothing outside a row's payload is read (the padding between payloads included), nothing outside
 * `out` is written; every byte of `out` is written, whatever it held before.
 *
 * The kernel only clamps: a source coordinate past a frame's last row or column reads that row or column, an offset that leaves
 * the arena is moved inside it, a format index keeps its low two bits.  A caller validates its table on the host (ops.yuv_crops_to_bgr
 * does), as callers of binhip_gather_windows do.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "binyuv.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINCROP_API) are its ONLY dynamic symbols. */
#define BINCROP_API __attribute__((visibility("default")))

#define BINCROP_VERSION 100        /* what bincrop_version() of a matching library returns */

#define BINCROP_E_ARG   (-1)       /* null pointer / bad value   (= BINYUV_E_ARG)   */
#define BINCROP_E_SHAPE (-2)       /* unsupported shape          (= BINYUV_E_SHAPE) */

#define BINCROP_FORMATS 4          /* format index = 2 * matrix + range (BINYUV_MATRIX_*, BINYUV_RANGE_*) */

typedef struct BinCropRow {        /* one decoded frame; 32 bytes, the table is 8-byte aligned */
    int64_t offset;                /* of the payload's first byte in the arena */
    int32_t H, W;                  /* the frame's own size */
    int32_t y0, x0;                /* the crop's top left pixel: y0 + ch <= H, x0 + cw <= W */
    int32_t format;                /* 0 .. BINCROP_FORMATS - 1 */
    int32_t reserved;              /* 0 */
} BinCropRow;

BINCROP_API int bincrop_version(void);

/* rows[r], r < n_rows: the ch x cw crop at (y0, x0) of the H x W frame whose payload starts at arena + offset -> out, uint8
 * [n_rows][ch][cw][3] BGR, contiguous (the arena layout of binhip_gather_windows).  `chroma`: BINYUV_CHROMA_420 | _444, of every row.
 * BINCROP_E_ARG: a null pointer, n_rows, ch or cw < 1, an unknown chroma, arena_bytes < 1, `rows` not 8-byte aligned, `out`
 *   overlapping the arena or the table.
 * BINCROP_E_SHAPE: arena_bytes or n_rows * ch * cw * 3 beyond 2^40.
 * The rows themselves are device memory and are not read on the host: see "The kernel only clamps" above.                          */
BINCROP_API int bincrop_yuv_crops_to_bgr(const uint8_t* arena, int64_t arena_bytes, const BinCropRow* rows, int n_rows, int ch, int cw,
                                         int chroma, uint8_t* out, void* stream);

#ifdef __cplusplus
}
#endif
