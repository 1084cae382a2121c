/*
 * binopt.h — flat C ABI of libbinopt.so: the optimizer side of the MI355X (gfx950) training step, the companion of
 * libbinhip.so (binhip.h).  It is a library of its own so that the interface of libbinhip.so (its version, its entry-point
 * count) is untouched by it: a binder that does not train with `train.optimizer: hip` never loads it.
 *
 * Conventions are binhip.h's: every pointer inside a row is a DEVICE pointer owned by the caller; the library never allocates,
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

/* The library is built with -fvisibility=hidden: the entry points declared here (BINOPT_API) are its ONLY dynamic symbols. */
#define BINOPT_API __attribute__((visibility("default")))

#define BINOPT_VERSION 100        /* what binopt_version() of a matching library returns */

#define BINOPT_E_ARG   (-1)       /* null pointer / bad value   (= BINHIP_E_ARG)   */
#define BINOPT_E_SHAPE (-2)       /* unsupported shape          (= BINHIP_E_SHAPE) */

BINOPT_API int binopt_version(void);

/* ---- the Adam update of a parameter group (torch.optim.Adam's single-tensor path, torch/optim/adam.py) ---------------
 * `items`: HOST array of n rows, one per tensor; the rows travel to the kernel by value (no device table, no copy), so the
 * library splits n into launches of at most BINOPT_ADAM_MAX_TENSORS rows.  Per element of a row, in fp32, IEEE sqrt and divide:
 *     g' = g + weight_decay * p                 (skipped when weight_decay == 0)
 *     m' = m + (1 - beta1) * (g' - m)
 *     v' = beta2 * v + (1 - beta2) * g' * g'
 *     p' = p - step_size * m' / (sqrtf(v') * inv_sqrt_bc2 + eps)
 * p, m, v are updated in place, g is only read.  step_size = lr / (1 - beta1^t) and inv_sqrt_bc2 = 1 / sqrt(1 - beta2^t) are the
 * caller's, computed in double and rounded once; they are per row because t may differ between parameters.  Every buffer is a
 * contiguous run of `numel` floats at any 4-byte offset (a row whose four pointers are 16-byte aligned moves 16 B per lane in
 * its whole chunks, any other row and every last partial chunk 4 B per lane); the buffers of one call must not overlap.  Nothing
 * outside [ptr, ptr + numel) is read or written.
 * beta1, beta2 are the fp32 roundings of the caller's hyper-parameters.  1 - beta is needed to full fp32 precision, which the
 * float no longer carries (1 - 0.999f is off from 0.001 by 1.3e-5), so the library forms it in double from the shortest decimal
 * that rounds to the float (0.999f -> 0.999) and rounds once; `beta2 * v` uses the float as passed.
 * n == 0 returns 0 without a launch.  Errors, all before anything is launched: BINOPT_E_ARG for n < 0, a null `items` with
 * n > 0, a null pointer or numel < 1 in any row, beta1 or beta2 outside [0, 1) (NaN included).  Neither allocates nor syncs;
 * re-entrant.                                                                                                             */
#define BINOPT_ADAM_MAX_TENSORS 64   /* rows per launch: 64 x 48 B + the chunk table stay under the 4 KB kernel-argument limit */
typedef struct BinAdamTensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t numel;
    float step_size;
    float inv_sqrt_bc2;
} BinAdamTensor;
BINOPT_API int binopt_adam_step(const BinAdamTensor* items /* host array */, int n, float beta1, float beta2, float eps,
                     float weight_decay, void* stream);

#ifdef __cplusplus
}
#endif
