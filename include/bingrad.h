/*
 * bingrad.h — flat C ABI of libbingrad.so: the gradient guard of the MI355X (gfx950) training step — the global L2 norm of all
 * gradients in one deterministic pass, the clip coefficient of torch.nn.utils.clip_grad_norm_, and the in-place scale — the
 * companion of libbinhip.so (binhip.h) and libbinopt.so (binopt.h).  It is a library of its own so that the interfaces of the
 * other two (their versions, their entry-point counts) are untouched by it: a binder that trains without `train.grad_clip`
 * and `train.skip_bad_steps` never loads it.
 *
 * Conventions are binhip.h's: every pointer inside a row, `workspace`, `record` and `status_word` are DEVICE pointers owned by
 * the caller; the library never allocates, frees or retains device memory; `stream` is a hipStream_t passed as void*; all
 * work is enqueued asynchronously, no host synchronisation inside; return value 0 = ok, negative = argument / shape error,
 * positive = hipError_t; every argument is checked before anything is launched.  No mutable process-global state; entry
 * points are re-entrant: two host threads on two streams with their own workspace and record get the serial result.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINGRAD_API) are its ONLY dynamic symbols. */
#define BINGRAD_API __attribute__((visibility("default")))

#define BINGRAD_VERSION 100        /* what bingrad_version() of a matching library returns */

#define BINGRAD_E_ARG   (-1)       /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINGRAD_E_SHAPE (-2)       /* unsupported shape          (= BINHIP_E_SHAPE) */

#define BINGRAD_FLAG_NONFINITE 1   /* BinGradRecord.flags: sumsq is not finite, i.e. some gradient element is inf or NaN */
#define BINGRAD_FLAG_STATUS    2   /* BinGradRecord.flags: *status_word & status_mask was non-zero */

/* rows per launch: the rows travel to the kernels by value; 128 x 16 B + the 129-entry chunk table + the scalars stay well under
 * the 4 KB kernel-argument limit.  A longer table takes several launches, which the library issues itself. */
#define BINGRAD_MAX_TENSORS 128

BINGRAD_API int bingrad_version(void);

/* One gradient: a contiguous run of `numel` >= 1 floats at any 4-byte offset (the gradients of a flat all-reduce buffer are
 * views).  A row whose pointer is 16-byte aligned moves 16 B per lane in its whole chunks, any other row and every last partial
 * chunk 4 B per lane.  Nothing outside [g, g + numel) is read or written. */
typedef struct BinGradTensor {
    float* g;
    int64_t numel;
} BinGradTensor;

/* What bingrad_norm leaves on the device, 32 bytes.  `flags` is 4-byte aligned at byte 16, so a data-parallel caller can
 * all-reduce (MAX) an int32 view of it before reading the record. */
typedef struct BinGradRecord {
    double sumsq;          /* sum of g * g over all rows; every product and the sum in double */
    float norm;            /* (float)sqrt(sumsq) */
    float coef;            /* 1.0f when max_norm == 0 or NONFINITE is set, else (float)min(1.0, max_norm / (sqrt(sumsq) + 1e-6)) */
    int32_t flags;         /* BINGRAD_FLAG_* */
    uint32_t status;       /* *status_word & status_mask as read; 0 when status_word is NULL */
    int32_t reserved[2];   /* written as 0 */
} BinGradRecord;

/* ---- the global gradient norm ------------------------------------------------------------------------------------------
 * `items`: HOST array of n rows.  bingrad_norm_workspace_bytes: the size of `workspace` for these rows (one double per
 * workgroup, at least 8), or a negative error code.
 * bingrad_norm: pass 1, one streaming kernel per BINGRAD_MAX_TENSORS rows: a workgroup owns one chunk of one row, converts each
 * element to double, squares and accumulates in double, reduces in a fixed order and stores its sum to its own slot of
 * `workspace`.  Pass 2, one workgroup: sums the slots in a fixed order and writes `record`.  There are no atomics: the record
 * is bit-reproducible from run to run.  Finite floats cannot overflow a double sum of any length that fits in memory, so
 * NONFINITE is exactly "some element is inf or NaN".
 * `max_norm`: 0 = no clipping (coef = 1.0f); otherwise coef is torch.nn.utils.clip_grad_norm_'s clamp(max_norm / (norm + 1e-6),
 * max = 1), evaluated in double and rounded once.  `status_word`: NULL, or a device uint32 (binhip.h's status word) that is
 * READ, never written: STATUS is set when *status_word & status_mask is non-zero.
 * n == 0 writes the record of an empty sum (sumsq 0, norm 0).  Errors, all before anything is launched: BINGRAD_E_ARG for n < 0,
 * a null `items` with n > 0, a null g or numel < 1 in any row, a negative or NaN max_norm, a null workspace or record;
 * BINGRAD_E_SHAPE for a row of more than 2^24 - 1 chunks of 4096 elements (6.9e10 elements): a launch holds at most that many
 * workgroups, so that its grid stays below 2^32 threads; a table whose rows add up to more is split into further launches.
 * The final pass is ONE workgroup that reads 8 B per slot (per 4096 gradient elements): its time grows linearly with the model. */
BINGRAD_API int64_t bingrad_norm_workspace_bytes(const BinGradTensor* items /* host array */, int n);
BINGRAD_API int bingrad_norm(const BinGradTensor* items /* host array */, int n, float max_norm, const uint32_t* status_word,
                 uint32_t status_mask, void* workspace, BinGradRecord* record, void* stream);

/* ---- the clip: g *= record->coef in place, in fp32 ---------------------------------------------------------------------
 * One kernel with the work split of pass 1.  Every workgroup reads `coef` from the record ON THE DEVICE and returns without a
 * store when it is exactly 1.0f: an unclipped step writes nothing, and so does a step whose norm is not finite.
 * NOTE the difference from torch.nn.utils.clip_grad_norm_: with an inf / NaN norm torch multiplies every gradient by 0 or NaN
 * and so turns the whole set into zeros and NaNs; here a non-finite gradient set is left exactly as it is, for the caller to
 * skip the step (flags) or to fail on.
 * Errors, before anything is launched: BINGRAD_E_ARG for n < 0, a null `items` with n > 0, a null g or numel < 1 in any row,
 * a null record.  n == 0 returns 0 without a launch. */
BINGRAD_API int bingrad_scale(const BinGradTensor* items /* host array */, int n, const BinGradRecord* record, void* stream);

#ifdef __cplusplus
}
#endif
