/*
 * binscene.h — flat C ABI of libbinscene.so: what a scene-cut detector needs from the 8-bit luma planes of a video stream, measured
 * on the MI355X (gfx950) from planes that are on the device already (bin_amd/scene.py, `python -m bin_amd.test --scene_cut`).  The
 * companion of libbinhip.so, libbinopt.so, libbingrad.so, libbinema.so, libbinens.so and libbinyuv.so, and a library of its own for
 * the same reason as each of those: their interfaces are untouched by it, and a binder that never looks for cuts never loads it.
 *
 * Conventions are binyuv.h's: every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains
 * device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host synchronisation inside;
 * return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.
 *
 * A plane is H*W contiguous bytes, [H][W]: the Y plane of a Y4M payload, 4:2:0 and 4:4:4 alike.  Any base address and any size are
 * legal: the kernel walks the plane as n = H*W bytes, the 16-byte aligned middle of `cur` as 16-byte vectors and the up to 15 bytes
 * before and after it one by one; `prev` moves as vectors when it shares `cur`'s offset within 16 bytes and as bytes otherwise.  Both
 * paths feed the same accumulation.  All results are integer sums, so they are exact and do not depend on the execution order.
 * Nothing outside the planes is read and nothing outside the record is written.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINSCENE_API) are its ONLY dynamic symbols. */
#define BINSCENE_API __attribute__((visibility("default")))

#define BINSCENE_VERSION 100      /* what binscene_version() of a matching library returns */

#define BINSCENE_E_ARG   (-1)     /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINSCENE_E_SHAPE (-2)     /* unsupported shape          (= BINHIP_E_SHAPE) */

#define BINSCENE_BINS 64          /* histogram bins: bin k counts the pixels with value >> 2 == k */

typedef struct BinSceneRecord {
    uint64_t sad;                 /* sum over the plane of |cur - prev|; 0 when prev is NULL */
    uint32_t hist[BINSCENE_BINS]; /* hist[k] = number of pixels of cur with value >> 2 == k   */
} BinSceneRecord;                 /* 264 bytes */

BINSCENE_API int binscene_version(void);

/* cur, prev (may be NULL): H x W planes -> *rec.  The call itself enqueues the clearing of *rec on `stream` before the kernel: the
 * caller need not clear it, and two calls into one record leave the second call's values.
 * BINSCENE_E_ARG: a null cur or rec, H or W < 1, rec not 8-byte aligned, rec overlapping a plane.
 * BINSCENE_E_SHAPE: H*W beyond 2^31 - 1 (the bound that keeps the 32-bit counts safe).                                       */
BINSCENE_API int binscene_luma_stats(const uint8_t* cur, const uint8_t* prev, int H, int W, BinSceneRecord* rec, void* stream);

#ifdef __cplusplus
}
#endif
