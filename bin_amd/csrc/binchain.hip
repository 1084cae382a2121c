// binchain.hip (libbinchain.so, include/binchain.h) — the hand-off kernel of chained interpolation passes (bin_amd/chain.py):
//   chain_reframe_kernel : crop of a padded generator output, clamped to [0, 1], replicate-padded again: the next pass's input.
// An HBM-bound element-wise kernel with an index map: no LDS, no reuse.  Items (two pointers each) travel BY VALUE in the
// kernel-argument segment; blockIdx.y picks the item, blockIdx.x grid-strides over the units of its DESTINATION with 64-bit
// indices (a unit is a float on the 4 B path, a float4 on the 16 B path).  A lane clamps its source coordinate to the crop, so a
// pad lane reads the edge pixel it replicates; its one load comes before its one store.
// Data paths: at Ws, W, Wd, left and pad_left all multiples of 4 a destination float4 lies wholly inside the crop or wholly inside
// a pad, and its source float4 is aligned; an item whose two pointers are 16-byte aligned then moves float4s, a pad lane
// broadcasting the edge component of the float4 at its clamped column.  Any other item moves single floats.  Both paths apply the
// same clamp to the same source element, so they agree bit for bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/binchain.h"

namespace {
constexpr int CHAIN_THREADS = 256;
constexpr int64_t CHAIN_MAX_BLOCKS = 2048;                       // per launch, over all items (8 workgroups per CU); beyond that blocks stride
constexpr int64_t CHAIN_MAX_ELEMS = (int64_t)1 << 40;
constexpr int64_t CHAIN_MAX_SIDE = 2147483647;

struct ChainTable {
    BinChainItem item[BINCHAIN_MAX_ITEMS];
    uint32_t vec_mask;                                           // bit i: item i takes the 16 B path
};
struct ChainGeom {
    int32_t Hs, Ws, top, left, H, W, pad_left, pad_top, Hd, Wd;
};
static_assert(sizeof(BinChainItem) == 16, "BinChainItem layout");
static_assert(sizeof(ChainTable) + sizeof(ChainGeom) + 16 <= 3840, "the table must fit the by-value argument limit");

// binhip_frame_to_u8's clamp: NaN -> 0, -inf -> 0, +inf -> 1
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// Unit `u` of the destination (Wu units per row) -> its column unit, and the source row (in floats from src) it replicates.
// Tensors below 2^31 units (all but the largest) divide in 32 bits.
struct Where {
    int xu;
    int64_t src_row;
    __device__ __forceinline__ Where(int64_t u, int Wu, const ChainGeom& g, bool small) {
        int64_t p;
        int y;
        if (small) {
            const uint32_t row = (uint32_t)u / (uint32_t)Wu;
            xu = (int)((uint32_t)u - row * (uint32_t)Wu);
            const uint32_t plane = row / (uint32_t)g.Hd;
            y = (int)(row - plane * (uint32_t)g.Hd);
            p = plane;
        } else {
            const int64_t row = u / Wu;
            xu = (int)(u - row * Wu);
            p = row / g.Hd;
            y = (int)(row - p * g.Hd);
        }
        const int sy = g.top + clampi(y - g.pad_top, 0, g.H - 1);
        src_row = (p * g.Hs + sy) * (int64_t)g.Ws + g.left;
    }
};
}  // namespace

__global__ void __launch_bounds__(CHAIN_THREADS)
chain_reframe_kernel(const ChainTable tab, const ChainGeom g, const int64_t rows) {
    const BinChainItem& it = tab.item[blockIdx.y];
    const int64_t stride = (int64_t)gridDim.x * CHAIN_THREADS;
    if ((tab.vec_mask >> blockIdx.y) & 1u) {
        const int W4 = g.Wd >> 2;
        const int64_t units = rows * W4;
        const bool small = units < ((int64_t)1 << 31);
        float4* __restrict__ dst = reinterpret_cast<float4*>(it.dst);
        for (int64_t u = (int64_t)blockIdx.x * CHAIN_THREADS + threadIdx.x; u < units; u += stride) {
            const Where at(u, W4, g, small);
            const int x = (at.xu << 2) - g.pad_left;             // the crop column of the float4's first component
            const float4 v = *reinterpret_cast<const float4*>(it.src + at.src_row + clampi(x, 0, g.W - 4));
            const float a = x < 0 ? v.x : (x >= g.W ? v.w : v.x);
            const float b = x < 0 ? v.x : (x >= g.W ? v.w : v.y);
            const float c = x < 0 ? v.x : (x >= g.W ? v.w : v.z);
            const float d = x < 0 ? v.x : v.w;
            dst[u] = make_float4(clamp01(a), clamp01(b), clamp01(c), clamp01(d));
        }
    } else {
        const int64_t units = rows * g.Wd;
        const bool small = units < ((int64_t)1 << 31);
        for (int64_t e = (int64_t)blockIdx.x * CHAIN_THREADS + threadIdx.x; e < units; e += stride) {
            const Where at(e, g.Wd, g, small);
            it.dst[e] = clamp01(it.src[at.src_row + clampi(at.xu - g.pad_left, 0, g.W - 1)]);
        }
    }
}

namespace {
bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

bool overlaps(uintptr_t a, uintptr_t a_bytes, uintptr_t b, uintptr_t b_bytes) { return a < b + b_bytes && b < a + a_bytes; }

// 0 and the element count, E_ARG for a side < 1, E_SHAPE beyond 2^40 elements
int check_elems(int planes, int64_t h, int64_t w, int64_t* total) {
    if (planes < 1 || h < 1 || w < 1) return BINCHAIN_E_ARG;
    if (h > CHAIN_MAX_SIDE || w > CHAIN_MAX_SIDE) return BINCHAIN_E_SHAPE;
    const int64_t rows = (int64_t)planes * h;                    // < 2^62
    if (rows > CHAIN_MAX_ELEMS / w) return BINCHAIN_E_SHAPE;     // rows * w would pass 2^40
    *total = rows * w;
    return 0;
}
}  // namespace

int binchain_version(void) { return BINCHAIN_VERSION; }

int binchain_reframe(const BinChainItem* items, int n, int planes, int Hs, int Ws, int top, int left, int H, int W,
                     int pad_left, int pad_right, int pad_top, int pad_bottom, void* stream) {
    if (n < 0 || n > BINCHAIN_MAX_ITEMS || (n > 0 && !items)) return BINCHAIN_E_ARG;
    if (planes < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1) return BINCHAIN_E_ARG;
    if (pad_left < 0 || pad_right < 0 || pad_top < 0 || pad_bottom < 0 || top < 0 || left < 0) return BINCHAIN_E_ARG;
    if ((int64_t)top + H > Hs || (int64_t)left + W > Ws) return BINCHAIN_E_ARG;
    const int64_t Hd = (int64_t)H + pad_top + pad_bottom, Wd = (int64_t)W + pad_left + pad_right;
    int64_t src_total = 0, dst_total = 0;
    if (int rc = check_elems(planes, Hs, Ws, &src_total)) return rc;
    if (int rc = check_elems(planes, Hd, Wd, &dst_total)) return rc;
    if (n == 0) return 0;
    const uintptr_t src_bytes = (uintptr_t)src_total * 4, dst_bytes = (uintptr_t)dst_total * 4;
    const bool vec_shape = Ws % 4 == 0 && W % 4 == 0 && Wd % 4 == 0 && left % 4 == 0 && pad_left % 4 == 0;
    ChainTable tab = {};
    int n_vec = 0;
    for (int i = 0; i < n; ++i) {
        const BinChainItem& it = items[i];
        if (!it.src || !it.dst || !aligned(it.src, 4) || !aligned(it.dst, 4)) return BINCHAIN_E_ARG;
        if (overlaps((uintptr_t)it.dst, dst_bytes, (uintptr_t)it.src, src_bytes)) return BINCHAIN_E_ARG;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            if (overlaps((uintptr_t)it.dst, dst_bytes, (uintptr_t)items[j].src, src_bytes)) return BINCHAIN_E_ARG;
            if (overlaps((uintptr_t)it.dst, dst_bytes, (uintptr_t)items[j].dst, dst_bytes)) return BINCHAIN_E_ARG;
        }
        tab.item[i] = it;
        if (vec_shape && aligned(it.src, 16) && aligned(it.dst, 16)) { tab.vec_mask |= 1u << i; ++n_vec; }
    }
    const ChainGeom g = {Hs, Ws, top, left, H, W, pad_left, pad_top, (int32_t)Hd, (int32_t)Wd};
    const int64_t rows = (int64_t)planes * Hd;
    // one lane per float4 when every item takes the 16 B path, one per float otherwise (a 16 B item in such a mixed launch simply
    // leaves its later blocks idle), capped where a block starts to stride
    const int64_t units = n_vec == n ? dst_total / 4 : dst_total;
    const int64_t blocks = (units + CHAIN_THREADS - 1) / CHAIN_THREADS;
    const int64_t cap = CHAIN_MAX_BLOCKS / n > 0 ? CHAIN_MAX_BLOCKS / n : 1;
    hipLaunchKernelGGL(chain_reframe_kernel, dim3((unsigned)(blocks < cap ? blocks : cap), (unsigned)n), dim3(CHAIN_THREADS), 0,
                       (hipStream_t)stream, tab, g, rows);
    return (int)hipGetLastError();
}
