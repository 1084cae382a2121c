/*
 * binema.h — flat C ABI of libbinema.so: the exponential moving average (EMA) of the generator weights on the MI355X (gfx950),
 * the companion of libbinhip.so (binhip.h), libbinopt.so (binopt.h) and libbingrad.so (bingrad.h).  It is a library of its own so
 * that the interfaces of those three (their versions, their entry-point counts) are untouched by it: a binder that does not train
 * with `train.ema_decay` never loads it.
 *
 * Conventions are binopt.h's: every pointer inside a row is a DEVICE pointer owned by the caller; the library never allocates,
 * frees or retains device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host
 * synchronisation inside; return value 0 = ok, negative = argument / shape error, positive = hipError_t.  No mutable
 * process-global state; entry points are re-entrant.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINEMA_API) are its ONLY dynamic symbols. */
#define BINEMA_API __attribute__((visibility("default")))

#define BINEMA_VERSION 100        /* what binema_version() of a matching library returns */

#define BINEMA_E_ARG   (-1)       /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINEMA_E_SHAPE (-2)       /* unsupported shape          (= BINHIP_E_SHAPE) */

BINEMA_API int binema_version(void);

/* ---- one averaging step over a set of tensors ---------------------------------------------------------------------------
 * `items`: HOST array of n rows, one per tensor; the rows travel to the kernel by value (no device table, no copy), so the
 * library splits n into launches of at most BINEMA_MAX_TENSORS rows.  Per element of a row, in fp32 (the multiply-add may be
 * contracted):
 *     e' = e + w * (p - e),      w = 1 - decay
 * e (the average, the "shadow") is updated in place, p (the weight) is only read.  Every buffer is a contiguous run of `numel`
 * floats at any 4-byte offset (a row whose two pointers are 16-byte aligned moves 16 B per lane in its whole chunks, any other
 * row and every last partial chunk 4 B per lane; the two paths give the same bits); the buffers of one call must not overlap.
 * Nothing outside [ptr, ptr + numel) is read or written.
 * `decay` is the fp32 rounding of the caller's hyper-parameter.  1 - decay is needed to full fp32 precision, which the float no
 * longer carries (1 - 0.9999f is off from 1e-4 by 1.7e-4), so the library forms it in double from the shortest decimal that
 * rounds to the float (0.9999f -> 0.9999) and rounds once.
 * Non-finite values are not treated specially: an inf or NaN in p propagates into e and stays there.  No flags are kept;
 * refusing a bad step is the gradient guard's job (bingrad.h), before the optimizer writes p.
 * n == 0 returns 0 without a launch.  Errors, all before anything is launched: BINEMA_E_ARG for n < 0, a null `items` with
 * n > 0, a null pointer or numel < 1 in any row, decay outside [0, 1) (NaN included); BINEMA_E_SHAPE for a row that needs more
 * than 2^31 - 1 workgroups.  Neither allocates nor syncs; re-entrant.                                                       */
#define BINEMA_MAX_TENSORS 136    /* rows per launch: 136 x 24 B + the chunk table stay under the 4 KB kernel-argument limit */
typedef struct BinEmaTensor {
    float* e;
    const float* p;
    int64_t numel;
} BinEmaTensor;
BINEMA_API int binema_step(const BinEmaTensor* items /* host array */, int n, float decay, void* stream);

#ifdef __cplusplus
}
#endif
