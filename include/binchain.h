/*
 * binchain.h — flat C ABI of libbinchain.so: the hand-off kernel of chained interpolation passes (bin_amd/chain.py, `python -m
 * bin_amd.test --input_video ... --factor 4|8`) on the MI355X (gfx950).  The companion of libbinhip.so, libbinopt.so,
 * libbingrad.so, libbinema.so, libbinens.so, libbinyuv.so and libbinscene.so, and a library of its own for the same reason as each
 * of those: their interfaces are untouched by it, and a binder that never chains passes never loads it.
 *
 * Conventions are binens.h's and binyuv.h's: every pointer inside an item is a DEVICE pointer owned by the caller; the library never
 * allocates, frees or retains device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host
 * synchronisation inside; return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive =
 * hipError_t.  No mutable process-global state; entry points are re-entrant.  Items travel to the kernel BY VALUE.
 *
 * The reframe R turns a padded fp32 output of the generator back into one of its inputs, which is an image in [0, 1] with
 * replicate padding: the crop of the source, every value through binhip_frame_to_u8's clamp fminf(fmaxf(v, 0), 1) (NaN -> 0,
 * -inf -> 0, +inf -> 1; the sign of a zero is not specified), padded again by replication.  With Hd = H + pad_top + pad_bottom and
 * Wd = W + pad_left + pad_right, per plane p:
 *
 *     dst[p][y][x] = clamp( src[p][ top + min(max(y - pad_top, 0), H - 1) ][ left + min(max(x - pad_left, 0), W - 1) ] )
 *
 * Data paths.  When Ws, W and Wd, the offsets `left` and `pad_left` are multiples of 4 and both pointers of an item are 16-byte
 * aligned, the item moves 16 B per lane (a pad lane loads the float4 at its clamped column and broadcasts its edge component);
 * any other item moves 4 B per lane.  Both paths give the same bits.  Nothing outside [src, src + planes*Hs*Ws) is read, nothing
 * outside [dst, dst + planes*Hd*Wd) is written; indices are 64-bit.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINCHAIN_API) are its ONLY dynamic symbols. */
#define BINCHAIN_API __attribute__((visibility("default")))

#define BINCHAIN_VERSION 100      /* what binchain_version() of a matching library returns */

#define BINCHAIN_E_ARG   (-1)     /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINCHAIN_E_SHAPE (-2)     /* unsupported shape          (= BINHIP_E_SHAPE) */

#define BINCHAIN_MAX_ITEMS 24     /* frames per call: the 2 * 8 + 1 level-1 frames of a --batch 8 group are one launch */

BINCHAIN_API int binchain_version(void);

/* Per item, dst = R(src) as above: src is fp32 [planes][Hs][Ws], dst is fp32 [planes][H+pad_top+pad_bottom][W+pad_left+pad_right];
 * the geometry is shared by the n items of a call, one launch covers them all.  n == 0 returns 0 without a launch.
 * BINCHAIN_E_ARG: n < 0 or n > BINCHAIN_MAX_ITEMS, a null `items` with n > 0, planes, Hs, Ws, H or W < 1, a negative pad, top or
 * left < 0, a crop that leaves the source (top + H > Hs, left + W > Ws), a null or not 4-byte aligned pointer, a dst that overlaps
 * any other buffer of the call (its own src included; sources may alias each other, they are only read).
 * BINCHAIN_E_SHAPE: Hd or Wd beyond 2^31 - 1, planes*Hs*Ws or planes*Hd*Wd beyond 2^40.                                         */
typedef struct BinChainItem {
    const float* src;
    float* dst;
} BinChainItem;
BINCHAIN_API int binchain_reframe(const BinChainItem* items /* host array */, int n, int planes, int Hs, int Ws, int top, int left,
                                  int H, int W, int pad_left, int pad_right, int pad_top, int pad_bottom, void* stream);

#ifdef __cplusplus
}
#endif
