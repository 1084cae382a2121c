/*
 * binscore.h — flat C ABI of libbinscore.so: the quality scores of one 8-bit planar YUV payload against another, per plane, measured
 * on the MI355X (gfx950) from planes that are on the device already (bin_amd/score.py, `python -m bin_amd.test --gt_video`).  The
 * companion of libbinhip.so, libbinopt.so, libbingrad.so, libbinema.so, libbinens.so, libbinyuv.so, libbinscene.so, libbinchain.so and
 * libbinrate.so, and a library of its own for the same reason as each of those: their interfaces are untouched by it, and a binder
 * that never scores a video never loads it.
 *
 * Conventions are binscene.h's: every pointer is a DEVICE pointer owned by the caller; the library never allocates, frees or retains
 * device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host synchronisation inside;
 * return value 0 = ok, negative = argument / shape / workspace error (returned before any HIP call), positive = hipError_t.  No
 * mutable process-global state; entry points are re-entrant.
 *
 * Plane shapes are binyuv.h's: Y is [H][W]; U and V are [ch][cw] with ch = ceil(H/2), cw = ceil(W/2) at 4:2:0 and ch = H, cw = W at
 * 4:4:4.  Odd sizes are legal and so is any base address: the planes are read byte by byte, so the U and V planes of one contiguous
 * payload may start at odd offsets.  a == b is legal.  Nothing outside the planes is read; nothing outside the workspace and the
 * record is written.
 *
 * The tile walk is libbinhip.so's (binhip_image_score / binhip_frame_score: one definition, shared as source): exact integer sums,
 * fp64 SSIM formulas, partial sums in fixed workspace slots added in a fixed order, so two calls give the same bits.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINSCORE_API) are its ONLY dynamic symbols. */
#define BINSCORE_API __attribute__((visibility("default")))

#define BINSCORE_VERSION 100        /* what binscore_version() of a matching library returns */

#define BINSCORE_E_ARG       (-1)   /* null pointer / bad value   (= BINHIP_E_ARG)       */
#define BINSCORE_E_SHAPE     (-2)   /* unsupported shape          (= BINHIP_E_SHAPE)     */
#define BINSCORE_E_WORKSPACE (-3)   /* workspace too small        (= BINHIP_E_WORKSPACE) */

#define BINSCORE_CHROMA_420 420     /* (= BINYUV_CHROMA_420) */
#define BINSCORE_CHROMA_444 444     /* (= BINYUV_CHROMA_444) */

#define BINSCORE_SSIM_G11 1         /* `flags`: the Gaussian 11x11 SSIM of the Y plane (= BINHIP_SCORE_SSIM_G11) */
#define BINSCORE_SSIM_U7  2         /* `flags`: the uniform 7x7 SSIM of the Y plane    (= BINHIP_SCORE_SSIM_U7)  */

typedef struct BinPlaneScores {
    uint64_t sse[3];                /* Y, U, V: sum over the plane of (a - b)^2, exact */
    uint64_t sad[3];                /* Y, U, V: sum over the plane of |a - b|, exact   */
    double ssim_g11;                /* of the Y plane as a one-channel image: 'valid' 11x11 Gaussian, sigma 1.5; NaN without its flag */
    double ssim_u7;                 /* of the Y plane: 7x7 uniform window, sample covariance; NaN without its flag                    */
} BinPlaneScores;                   /* 64 bytes */

BINSCORE_API int binscore_version(void);

/* Bytes of workspace binscore_planes needs for this shape; 0 = a bad shape, chroma or flag (what binscore_planes refuses). */
BINSCORE_API size_t binscore_workspace_bytes(int H, int W, int chroma, int flags);

/* (ay, au, av) against (by, bu, bv): the planes of two H x W payloads of one chroma family -> *out.  At most two tile launches (Y; U
 * and V together where their shape differs from Y's, else all three in one) and one final launch; every field of *out is written,
 * so two calls into one record leave the second call's values.  g11_taps: 11 doubles on the HOST, the 1-D Gaussian (read during
 * the call; needed with BINSCORE_SSIM_G11 only).
 * BINSCORE_E_ARG: a null plane, ws or out; a null g11_taps with its flag; an unknown flag or chroma; out or ws not 8-byte aligned;
 *   out or ws overlapping a plane or each other.
 * BINSCORE_E_SHAPE: H or W outside 1 .. 65535; below 11 with BINSCORE_SSIM_G11; below 7 with BINSCORE_SSIM_U7.
 * BINSCORE_E_WORKSPACE: ws_bytes below binscore_workspace_bytes(H, W, chroma, flags).                                             */
BINSCORE_API int binscore_planes(const uint8_t* ay, const uint8_t* au, const uint8_t* av,
                                 const uint8_t* by, const uint8_t* bu, const uint8_t* bv,
                                 int H, int W, int chroma, int flags, const double* g11_taps,
                                 void* ws, size_t ws_bytes, BinPlaneScores* out, void* stream);

#ifdef __cplusplus
}
#endif
