/*
 * binexpose.h — flat C ABI of libbinexpose.so: training crops cut out of a device-resident uint8 frame arena on the MI355X
 * (gfx950), with the blurry slots synthesised as a camera exposure: the mean of the sharp frames in LINEAR light, sensor noise
 * added there, re-encoded to an 8-bit code (dataset options `blur_gamma` and `blur_noise`, bin_amd/data/exposure.py).  The
 * companion of binhip_gather_windows_blur (libbinhip.so), which averages the 8-bit codes as the reference's script does and stays
 * the default; a library of its own, so that libbinhip.so's interface is untouched by it and a binder that never sets the options
 * never loads it.
 *
 * Conventions: every pointer but binexpose_check_curve's is a DEVICE pointer owned by the caller; the library never allocates,
 * frees or retains device memory; `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously, no host
 * synchronisation inside; return value 0 = ok, negative = argument / shape error (returned before any HIP call), positive =
 * hipError_t.  No mutable process-global state; entry points are re-entrant.
 *
 * THE SPECIFICATION.  Everything is exact integer arithmetic; ONE = 2^24 - 1 is full scale in linear light.
 *
 * A curve is three tables of 256 uint32_t, built by the caller on the host (the kernel takes tables and knows no curve); with
 * `dec` the decoding function of the transfer curve (e -> e^g, or the sRGB one), evaluated in float64:
 *   LIN[v] = rint(dec(v / 255) * ONE), v = 0 .. 255: the linear value of code v;
 *   MID[0] = 0, MID[c] = ceil(dec((c - 0.5) / 255) * ONE), c = 1 .. 255: the smallest linear value that encodes to c;
 *   decode(m) = the largest c with MID[c] <= m: rounding to the nearest code in the encoded domain;
 *   SIG[k] = rint(sqrt(read^2 + shot * (k + 0.5) / 256) * ONE * 65536 / 53509.92), k = 0 .. 255: the noise scale of the k-th of
 *     256 linear bins, sigma^2 = read^2 + shot * lin with full scale = 1; 53509.92 is the standard deviation of Z below.
 *     All-zero SIG means no noise, and the kernel then skips the generator.
 * A curve is VALID (binexpose_check_curve) when LIN[0] = 0, LIN is non-decreasing and LIN[255] <= ONE; MID[0] = 0 and MID is
 * strictly increasing; MID[c] <= LIN[c] < MID[c + 1] for every c (MID[256] = infinity), which gives decode(LIN[v]) = v: a
 * one-frame exposure without noise is the identity; every SIG[k] < 2^23.
 *
 * Per element of a blurry slot — output position (x, y) after crop and flip, channel c in output RGB order — with the sample's
 * half range h and key (k0, k1):
 *   1. S = the sum of LIN[code] over the 2h + 1 frames id - h .. id + h;
 *   2. m = S / (2h + 1), the integer quotient;
 *   3. (w0, w1, w2, w3) = Philox4x32-10(counter = (x, y, 4 * slot + c, 0), key = (k0, k1)): multipliers 0xD2511F53 and
 *      0xCD9E8D57, key increments 0x9E3779B9 and 0xBB67AE85, ten rounds (Random123's; counter and key all zero give
 *      6627e8d5 e169c58d bc57ac4c 9b00dbd8);
 *   4. Z = the sum of the eight 16-bit halves of those four words;
 *   5. n = ((Z - 262140) * SIG[m >> 16]) >> 16, in 64 bits, the shift arithmetic (a floor);
 *   6. m' = min(max(m + n, 0), ONE);
 *   7. code = decode(m');
 *   8. out = (float)code / 255.f, as binhip_gather_windows writes a code.
 * Z is an Irwin-Hall sum of eight uniform 16-bit values: symmetric around 262140, kurtosis 2.85 (a normal variable has 3), tails
 * cut at +-4.9 sigma.  The noise field is tied to OUTPUT coordinates: a flipped sample is not the mirror of the unflipped one's
 * noise.  A slot s >= n_blur is written exactly as binhip_gather_windows writes it: (float)byte / 255.f.
 *
 * Data path.  One lane owns 4 consecutive output pixels of a row (12 source bytes per frame, read as the aligned dwords that
 * overlap them); a block stages the three tables in LDS once; decode is an 8-step binary search there.  Inside the kernel every
 * table index and every frame id is clamped (h to [0, 16] and to the arena, id to [h, n_frames - 1 - h], y0 and x0 to the frame,
 * m >> 16 to 255), so a bad table or curve can never read outside the arena or the 768 words; what a clamped row computes is
 * unspecified.  Nothing outside `out` is written.
 */
#pragma once

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the entry points declared here (BINEXPOSE_API) are its ONLY dynamic symbols. */
#define BINEXPOSE_API __attribute__((visibility("default")))

#define BINEXPOSE_VERSION 100        /* what binexpose_version() of a matching library returns */

#define BINEXPOSE_E_ARG   (-1)       /* null pointer / bad value */
#define BINEXPOSE_E_SHAPE (-2)       /* unsupported shape        */

#define BINEXPOSE_ONE        16777215   /* 2^24 - 1: full scale in linear light                      */
#define BINEXPOSE_TABLE      256        /* entries of LIN, of MID and of SIG                         */
#define BINEXPOSE_MAX_SLOTS  32         /* n_slots limit (that of binhip_gather_windows)             */
#define BINEXPOSE_MAX_HALF   16         /* h limit: exposures of 2h + 1 <= 33 sharp frames           */
#define BINEXPOSE_SIG_LIMIT  8388608    /* 2^23: every SIG[k] is below it                            */

BINEXPOSE_API int binexpose_version(void);

/* HOST arrays of BINEXPOSE_TABLE uint32_t each; pure host code, no HIP call.  0 when the curve is valid (the rules above),
 * BINEXPOSE_E_ARG for a null pointer or a broken rule. */
BINEXPOSE_API int binexpose_check_curve(const uint32_t* lin, const uint32_t* mid, const uint32_t* sig);

/* frames: uint8 [n_frames][H][W][3] BGR, the sharp frames of a clip consecutive in time; table: int32 [n][n_slots + 6], rows
 * [n_slots ids][y0][x0][flip][h][k0][k1] (k0, k1: the 32 bits of the key words); curve_dev: 768 uint32_t, LIN then MID then SIG,
 * uploaded by the caller after binexpose_check_curve accepted them; out: fp32 [n_slots][n][3][ch][cw], RGB planes.  The first
 * n_blur slots are exposures, the others plain crops.
 * BINEXPOSE_E_ARG: a null pointer.  BINEXPOSE_E_SHAPE: n_frames, H, W, n, ch or cw < 1, n_slots outside [1, 32], ch > H, cw > W,
 *   n_blur outside [0, n_slots], n_slots * n * ch * ceil(cw / 4) beyond 2^31 - 1.                                              */
BINEXPOSE_API int binexpose_gather(const uint8_t* frames, int n_frames, int H, int W, const int32_t* table, int n, int n_slots,
                                   int n_blur, int ch, int cw, const uint32_t* curve_dev, float* out, void* stream);

#ifdef __cplusplus
}
#endif
