// The 12-byte window load of the gather kernels (binhip_data.hip: gather_windows_blur_kernel; extra/binexpose.hip:
// gather_exposed_kernel), shared by the two libraries as source, not as a symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// the 12 bytes at p (pixels va .. vb - 1 of them are needed), as in gather_windows_kernel: only dwords the window touches
__device__ __forceinline__ static void gw_load12(const uint8_t* __restrict__ p, int va, int vb, uint32_t& a0, uint32_t& a1,
                                                 uint32_t& a2) {
    const unsigned off = (unsigned)((uintptr_t)p & 3u);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(p - off);
    const int jlo = ((int)off + 3 * va) >> 2, jhi = ((int)off + 3 * vb - 1) >> 2;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = d[min(max(j, jlo), jhi)];
    a0 = __builtin_amdgcn_alignbyte(w[1], w[0], off);
    a1 = __builtin_amdgcn_alignbyte(w[2], w[1], off);
    a2 = __builtin_amdgcn_alignbyte(w[3], w[2], off);
}
