/*
 * binens.h — flat C ABI of libbinens.so: the two streaming kernels of the test-time self-ensemble (bin_amd/ensemble.py) on the
 * MI355X (gfx950), the companion of libbinhip.so (binhip.h), libbinopt.so (binopt.h), libbingrad.so (bingrad.h) and libbinema.so
 * (binema.h).  It is a library of its own so that the interfaces of those four (their versions, their entry-point counts) are
 * untouched by it: a binder that never ensembles never loads it.
 *
 * Conventions are binopt.h's: every pointer inside an item is a DEVICE pointer owned by the caller; the library never allocates,
 * frees or retains device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host
 * synchronisation inside; return value 0 = ok, negative = argument / shape error, positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.  Items travel to the kernel BY VALUE (no device table, no copy), and every
 * error is returned before anything is launched.
 *
 * Tensors: fp32, contiguous [planes][H][W] (planes = N*3 for a batch of frames), at any 4-byte offset (batch slices and tensors a
 * cache owns both occur).  Nothing outside [ptr, ptr + planes*H*W) is read or written; indices are 64-bit.  When W % 4 == 0 and
 * every pointer of an item is 16-byte aligned the item moves 16 B per lane (the mirrored float4 of column x sits at column W-4-x,
 * aligned, with its components reversed in registers); any other item moves 4 B per lane.  The two paths give the same bits.
 * inf and NaN are not treated specially: they propagate.
 * Time reversal never reaches the library: it is a permutation of whole tensors, which the host does by handing over other pointers.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINENS_API) are its ONLY dynamic symbols. */
#define BINENS_API __attribute__((visibility("default")))

#define BINENS_VERSION 100        /* what binens_version() of a matching library returns */

#define BINENS_E_ARG   (-1)       /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINENS_E_SHAPE (-2)       /* unsupported shape          (= BINHIP_E_SHAPE) */

#define BINENS_FLIP_W 1           /* mirror along W (columns) */
#define BINENS_FLIP_H 2           /* mirror along H (rows)    */
#define BINENS_MAX_ORIENT 8       /* orientations of a group: destinations of a binens_orient item, sources of a binens_merge item */
#define BINENS_MAX_SOURCES 6      /* binens_orient items per call */
#define BINENS_MAX_SLOTS 14       /* binens_merge items per call  */

BINENS_API int binens_version(void);

/* ---- orient: flipped copies of frames ---------------------------------------------------------------------------------------
 * Per item, every dst[j], j < n_dst, becomes src with flip[j] (an OR of BINENS_FLIP_*) applied, per plane:
 *     dst[j][p][y][x] = src[p][flip[j] & H ? H-1-y : y][flip[j] & W ? W-1-x : x]
 * One read of src, n_dst writes (flip 0 = a copy); one launch covers all n items.  dst[j], j >= n_dst, is not looked at.
 * n == 0 returns 0 without a launch.  BINENS_E_ARG: n < 0 or n > BINENS_MAX_SOURCES, a null `items` with n > 0, planes, H or W
 * < 1, n_dst outside [1, BINENS_MAX_ORIENT], a flip with other bits, a null or not 4-byte aligned pointer, a dst that overlaps any
 * other buffer of the call (a dst equal to its src included).  BINENS_E_SHAPE: planes*H*W beyond 2^40.                          */
typedef struct BinEnsOrient {
    const float* src;
    float* dst[BINENS_MAX_ORIENT];
    uint8_t flip[BINENS_MAX_ORIENT];
    int32_t n_dst;
} BinEnsOrient;
BINENS_API int binens_orient(const BinEnsOrient* items /* host array */, int n, int planes, int H, int W, void* stream);

/* ---- merge: the ensemble estimate -------------------------------------------------------------------------------------------
 * Per item, with x_o = src[o] un-flipped by flip_of[o] (a flip is an involution: un-flipping is the same index map as flipping),
 *     dst = (1/M) * tree-sum over o < M of x_o
 * where the sum is the balanced pairwise tree over the orientation index, ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)) for M = 8, each add
 * rounded to fp32, and 1/M is a power of two (exact short of denormal results).  The tree, unlike a sequential sum, is invariant
 * under any XOR of the index, which is how the orientation group acts on it: the ensemble of an oriented input is the oriented
 * ensemble bit for bit.  All M loads of a lane are issued before the first add; one launch covers all n items.
 * `flip_of`: HOST array of M entries, shared by the items.  src[o], o >= M, is not looked at.
 * n == 0 returns 0 without a launch.  BINENS_E_ARG: n < 0 or n > BINENS_MAX_SLOTS, a null `items` with n > 0, M not in {1, 2, 4, 8},
 * a null `flip_of` or an entry with other bits, planes, H or W < 1, a null or not 4-byte aligned pointer, a dst that overlaps any
 * other buffer of the call (a dst equal to one of its srcs included; sources may alias each other, they are only read).
 * BINENS_E_SHAPE: planes*H*W beyond 2^40.                                                                                       */
typedef struct BinEnsMerge {
    const float* src[BINENS_MAX_ORIENT];
    float* dst;
} BinEnsMerge;
BINENS_API int binens_merge(const BinEnsMerge* items /* host array */, int n, int M, const uint8_t* flip_of /* host, M entries */,
                            int planes, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
