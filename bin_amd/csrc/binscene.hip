// binscene.hip (libbinscene.so, include/binscene.h) — the one kernel of the scene-cut detector (bin_amd/scene.py):
//   luma_stats_kernel : an 8-bit luma plane (and the plane before it) -> the 64-bin histogram of value >> 2 and the sum of absolute
//                       differences, added into one 264-byte record.
// The plane is n = H*W bytes.  The 16-byte aligned middle of `cur` moves as 16-byte vectors, grid-strided with 64-bit indices; the up
// to 15 bytes before and after it are taken one per lane by block 0.  Both paths hand dwords to add_word below: ONE accumulation.
// Histogram: every wave owns SC_SUBS sub-histograms in LDS (lane & 15 picks one; word = bin * SC_SUBS + sub, so the sixteen
// sub-histograms of a bin lie in sixteen banks), and a lane counts the run of equal bins among its consecutive pixels in a register
// and adds the run, not the pixel: on a flat plane that is one LDS add per 16 bytes, four lanes per word.  SAD: v_sad_u8, four
// bytes per instruction, summed per lane in 32 bits (the bound is asserted below), then across the wave by shuffles.  The block
// reduces in LDS and issues one global atomicAdd per non-empty bin and one 64-bit one for the SAD.  Integer sums: exact in any order.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binscene.h"

namespace {
constexpr int SC_THREADS = 256, SC_WAVE = 64, SC_WAVES = SC_THREADS / SC_WAVE, SC_SUBS = 16;
constexpr int SC_BINS = BINSCENE_BINS;
constexpr int64_t SC_MAX_BLOCKS = 512;                           // 2 workgroups per CU; beyond that blocks stride
constexpr int64_t SC_MAX_BYTES = INT32_MAX;

static_assert(sizeof(BinSceneRecord) == 264 && offsetof(BinSceneRecord, hist) == 8, "BinSceneRecord layout");
// a block's SAD fits 32 bits: at the grid cap a lane takes at most ceil(2^27 / lanes) vectors, below it one; plus one edge byte
static_assert(((SC_MAX_BYTES / 16) / (SC_MAX_BLOCKS * SC_THREADS) + 1) * 16 * 255 * SC_THREADS + 255 * 32 < UINT32_MAX, "32-bit block SAD");

struct Lane {                                                    // a lane's running state: its SAD and the open run of equal bins
    uint32_t sad, bin, run;
};

// ---- the accumulation: ONE definition for both data paths.  NB valid bytes in the low end of cw / pw (the rest zero).
template <int NB, bool PREV>
__device__ __forceinline__ void add_word(uint32_t cw, uint32_t pw, Lane& s, uint32_t* __restrict__ sub) {
    if (PREV) s.sad = __builtin_amdgcn_sad_u8(cw, pw, s.sad);
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const uint32_t bin = (cw >> (8 * i + 2)) & (SC_BINS - 1);
        if (bin != s.bin) {
            if (s.run) atomicAdd(sub + s.bin * SC_SUBS, s.run);
            s.bin = bin;
            s.run = 0;
        }
        ++s.run;
    }
}

struct __attribute__((packed, aligned(1))) Bytes16 {             // 16 bytes at any address
    uint32_t w[4];
};
}  // namespace

// PREV: 0 = no previous plane, 1 = prev shares cur's offset within 16 bytes (vector loads), 2 = it does not (unaligned loads)
template <int PREV>
__global__ void __launch_bounds__(SC_THREADS)
luma_stats_kernel(const uint8_t* __restrict__ cur, const uint8_t* __restrict__ prev, const int64_t n, const int head, const int64_t nvec,
                  const int tail, BinSceneRecord* __restrict__ rec) {
    __shared__ uint32_t hist[SC_WAVES][SC_BINS * SC_SUBS];
    __shared__ uint32_t total[SC_BINS];
    __shared__ uint32_t block_sad;
    const int tid = threadIdx.x, wave = tid / SC_WAVE, lane = tid % SC_WAVE;
    for (int i = tid; i < SC_WAVES * SC_BINS * SC_SUBS; i += SC_THREADS) (&hist[0][0])[i] = 0;
    if (tid < SC_BINS) total[tid] = 0;
    if (tid == 0) block_sad = 0;
    __syncthreads();

    uint32_t* sub = &hist[wave][lane % SC_SUBS];
    Lane s = {0u, 0u, 0u};
    const int64_t stride = (int64_t)gridDim.x * SC_THREADS;
    for (int64_t v = (int64_t)blockIdx.x * SC_THREADS + tid; v < nvec; v += stride) {
        const int64_t at = head + 16 * v;
        const uint4 c = *reinterpret_cast<const uint4*>(cur + at);
        uint4 p = make_uint4(0, 0, 0, 0);
        if (PREV == 1) {
            p = *reinterpret_cast<const uint4*>(prev + at);
        } else if (PREV == 2) {
            const Bytes16 b = *reinterpret_cast<const Bytes16*>(prev + at);
            p = make_uint4(b.w[0], b.w[1], b.w[2], b.w[3]);
        }
        add_word<4, PREV != 0>(c.x, p.x, s, sub);
        add_word<4, PREV != 0>(c.y, p.y, s, sub);
        add_word<4, PREV != 0>(c.z, p.z, s, sub);
        add_word<4, PREV != 0>(c.w, p.w, s, sub);
    }
    if (blockIdx.x == 0) {                                       // the edges: lanes 0 .. 15 the head, lanes 16 .. 31 the tail
        int64_t at = -1;
        if (tid < head) at = tid;
        else if (tid >= 16 && tid - 16 < tail) at = n - tail + (tid - 16);
        if (at >= 0) add_word<1, PREV != 0>(cur[at], PREV ? prev[at] : 0u, s, sub);
    }
    if (s.run) atomicAdd(sub + s.bin * SC_SUBS, s.run);

    uint32_t sad = s.sad;
    if (PREV) {
#pragma unroll
        for (int d = SC_WAVE / 2; d > 0; d >>= 1) sad += __shfl_down(sad, d, SC_WAVE);
        if (lane == 0 && sad) atomicAdd(&block_sad, sad);
    }
    __syncthreads();
    // thread (wave, bin = lane) sums its wave's sixteen sub-histograms of the bin (rotated: neighbours start in different banks)
    uint32_t part = 0;
#pragma unroll
    for (int k = 0; k < SC_SUBS; ++k) part += hist[wave][lane * SC_SUBS + ((k + lane) % SC_SUBS)];
    if (part) atomicAdd(&total[lane], part);
    __syncthreads();
    if (tid < SC_BINS && total[tid]) atomicAdd(&rec->hist[tid], total[tid]);
    if (PREV && tid == SC_BINS && block_sad) atomicAdd(reinterpret_cast<unsigned long long*>(&rec->sad), (unsigned long long)block_sad);
}

namespace {
bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}
}  // namespace

int binscene_version(void) { return BINSCENE_VERSION; }

int binscene_luma_stats(const uint8_t* cur, const uint8_t* prev, int H, int W, BinSceneRecord* rec, void* stream) {
    if (!cur || !rec || H < 1 || W < 1 || ((uintptr_t)rec & 7)) return BINSCENE_E_ARG;
    const int64_t n = (int64_t)H * W;
    if (n > SC_MAX_BYTES) return BINSCENE_E_SHAPE;
    if (overlap(rec, sizeof(BinSceneRecord), cur, (uint64_t)n) || (prev && overlap(rec, sizeof(BinSceneRecord), prev, (uint64_t)n)))
        return BINSCENE_E_ARG;
    const int64_t to_aligned = (16 - (int64_t)((uintptr_t)cur & 15)) & 15;
    const int head = (int)(to_aligned < n ? to_aligned : n);
    const int64_t nvec = (n - head) / 16;
    const int tail = (int)(n - head - 16 * nvec);
    const int64_t blocks = (nvec + SC_THREADS - 1) / SC_THREADS;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks < SC_MAX_BLOCKS ? blocks : SC_MAX_BLOCKS))), block(SC_THREADS);
    hipStream_t s = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(rec, 0, sizeof(BinSceneRecord), s)) return (int)e;
    const auto kernel = !prev ? luma_stats_kernel<0> : ((((uintptr_t)cur ^ (uintptr_t)prev) & 15) == 0 ? luma_stats_kernel<1> : luma_stats_kernel<2>);
    hipLaunchKernelGGL(kernel, grid, block, 0, s, cur, prev, n, head, nvec, tail, rec);
    return (int)hipGetLastError();
}
