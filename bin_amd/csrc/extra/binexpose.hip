// binexpose.hip (libbinexpose.so, include/binexpose.h) — binhip_gather_windows_blur's launch shape (binhip_data.hip) with the
// blurry slots synthesised as a camera exposure: the mean of the sharp frames in linear light, sensor noise added there, and the
// result re-encoded.  The arithmetic is the header's specification, exact integers throughout; the kernel takes three tables and
// knows no curve.
// One lane = 4 consecutive output pixels of one output row: per frame of the exposure 12 source bytes (gw_load12), each looked up
// in LIN (LDS) and added to its own 32-bit sum (33 * (2^24 - 1) < 2^30).  Per element then: the quotient S / L as a multiply and
// shift, one Philox4x32-10 block when the curve has noise, the 64-bit product with SIG, the clamp, and the 8-step binary search
// through MID (LDS).  Lanes of sharp slots take the bytes as they are.  A block stages the 768 table words once; whether any SIG
// is non-zero is the block-wide OR taken with the same barrier.
#include "../binhip_gather_load.h"
#include "../../../include/binexpose.h"

namespace {
constexpr int GE_THREADS = 256;
static_assert(GE_THREADS == BINEXPOSE_TABLE, "lane i of a block stages entry i of each table");
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // one 16-byte store at dword alignment (binhip_data.hip)

// S / L = (S * GE_DIV[h]) >> 36 with GE_DIV[h] = ceil(2^36 / L), L = 2h + 1: with e = GE_DIV[h] * L - 2^36 < L the product
// overshoots S / L by S e / (2^36 L) < 1 / L whenever S e < 2^36, and S <= 33 * 2^24, e <= 32 give S e < 2^35.  S * GE_DIV[h] is
// about 2^36 S / L <= 2^60: no overflow.
constexpr int GE_DIV_SHIFT = 36;
struct GeDiv { uint64_t m[BINEXPOSE_MAX_HALF + 1]; };
constexpr GeDiv ge_div_table() {
    GeDiv t{};
    for (int h = 0; h <= BINEXPOSE_MAX_HALF; ++h) {
        const uint64_t L = 2 * h + 1, one = 1ull << GE_DIV_SHIFT;
        t.m[h] = (one + L - 1) / L;
    }
    return t;
}
constexpr bool ge_div_exact() {
    for (int h = 0; h <= BINEXPOSE_MAX_HALF; ++h) {
        const uint64_t L = 2 * h + 1, e = ge_div_table().m[h] * L - (1ull << GE_DIV_SHIFT);
        if (e >= L || L * BINEXPOSE_ONE * e >= (1ull << GE_DIV_SHIFT)) return false;
    }
    return true;
}
static_assert(ge_div_exact(), "the multiply-and-shift quotient is exact for every sum an exposure can reach");
__device__ const GeDiv GE_DIV = ge_div_table();

// Philox4x32-10 (Salmon et al., Random123): the sum of the eight 16-bit halves of the block of counter (c0, c1, c2, 0)
__device__ __forceinline__ uint32_t philox_halves_sum(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t k0, uint32_t k1) {
    uint32_t c3 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
        const uint32_t h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return (c0 & 0xffffu) + (c0 >> 16) + (c1 & 0xffffu) + (c1 >> 16) + (c2 & 0xffffu) + (c2 >> 16) + (c3 & 0xffffu) + (c3 >> 16);
}

// S += LIN[byte] for the 12 window bytes a[0..2] (little-endian), static indices: no scratch
__device__ __forceinline__ void add_linear(const uint32_t* __restrict__ lin, const uint32_t (&a)[3], uint32_t (&S)[12]) {
#pragma unroll
    for (int j = 0; j < 12; ++j) S[j] += lin[(a[j >> 2] >> (8 * (j & 3))) & 0xffu];
}
}  // namespace

// grid: ceil(n_slots * n * ch * ceil(cw / 4) / GE_THREADS); item t = (slot, sample, output row y, quad q), q fastest; table rows are
// [n_slots ids][y0][x0][flip][h][k0][k1]
__global__ void __launch_bounds__(GE_THREADS)
gather_exposed_kernel(const uint8_t* __restrict__ frames, int n_frames, int H, int W, const int32_t* __restrict__ table, int n,
                      int n_slots, int n_blur, int ch, int cw, int nq, unsigned items, const uint32_t* __restrict__ curve,
                      float* __restrict__ out) {
    __shared__ uint32_t lin[BINEXPOSE_TABLE], mid[BINEXPOSE_TABLE], sig[BINEXPOSE_TABLE];
    const uint32_t my_sig = curve[2 * BINEXPOSE_TABLE + threadIdx.x];
    lin[threadIdx.x] = curve[threadIdx.x];
    mid[threadIdx.x] = curve[BINEXPOSE_TABLE + threadIdx.x];
    sig[threadIdx.x] = my_sig;
    const bool noise = __syncthreads_or(my_sig != 0u) != 0;  // (the barrier behind the staging, too)

    const unsigned t = blockIdx.x * GE_THREADS + threadIdx.x;
    if (t >= items) return;
    const unsigned row = t / (unsigned)nq;
    const int q = (int)(t - row * (unsigned)nq);
    const unsigned sb = row / (unsigned)ch;                  // slot * n + sample
    const int y = (int)(row - sb * (unsigned)ch);
    const int s = (int)(sb / (unsigned)n), b = (int)(sb - (unsigned)s * (unsigned)n);
    const bool blurry = s < n_blur;

    // The host validates the table; the clamps only guarantee that a bad row can never read outside the arena.
    const int32_t* rec = table + (size_t)b * (n_slots + 6);
    const int h = blurry ? min(min(max(rec[n_slots + 3], 0), BINEXPOSE_MAX_HALF), (n_frames - 1) >> 1) : 0;
    const int id = min(max(rec[s], h), n_frames - 1 - h);    // id - h .. id + h inside [0, n_frames)
    const int y0 = min(max(rec[n_slots], 0), H - ch);
    const int x0 = min(max(rec[n_slots + 1], 0), W - cw);
    const bool flip = rec[n_slots + 2] != 0;
    const uint32_t k0 = (uint32_t)rec[n_slots + 4], k1 = (uint32_t)rec[n_slots + 5];

    const int k = min(4, cw - 4 * q);
    const int sx = flip ? x0 + cw - 4 - 4 * q : x0 + 4 * q;
    const int va = flip ? 4 - k : 0, vb = flip ? 4 : k;
    const long long stride = (long long)H * W * 3;           // bytes per frame
    const uint8_t* p = frames + (((long long)id * H + (y0 + y)) * W + sx) * 3;

    // code[j]: the 8-bit code of window byte j; pixel i = bytes 3i (B), 3i + 1 (G), 3i + 2 (R)
    uint32_t code[12];
    uint32_t a0[3];
    gw_load12(p, va, vb, a0[0], a0[1], a0[2]);
    if (!blurry) {
#pragma unroll
        for (int j = 0; j < 12; ++j) code[j] = (a0[j >> 2] >> (8 * (j & 3))) & 0xffu;
    } else {
        uint32_t S[12] = {};
        add_linear(lin, a0, S);
        int f = 1;
        for (; f + 1 <= h; f += 2) {                         // frames -f-1, -f, f, f+1: 16 loads in flight before the first lookup
            uint32_t a[4][3];
            gw_load12(p - (f + 1) * stride, va, vb, a[0][0], a[0][1], a[0][2]);
            gw_load12(p - f * stride, va, vb, a[1][0], a[1][1], a[1][2]);
            gw_load12(p + f * stride, va, vb, a[2][0], a[2][1], a[2][2]);
            gw_load12(p + (f + 1) * stride, va, vb, a[3][0], a[3][1], a[3][2]);
#pragma unroll
            for (int i = 0; i < 4; ++i) add_linear(lin, a[i], S);
        }
        if (f <= h) {                                        // odd h: the outermost pair
            uint32_t a[2][3];
            gw_load12(p - f * stride, va, vb, a[0][0], a[0][1], a[0][2]);
            gw_load12(p + f * stride, va, vb, a[1][0], a[1][1], a[1][2]);
#pragma unroll
            for (int i = 0; i < 2; ++i) add_linear(lin, a[i], S);
        }
        const uint64_t dm = GE_DIV.m[h];
#pragma unroll
        for (int j = 0; j < 12; ++j) {
            const int px = j / 3, cb = j % 3;                // source pixel of the window, BGR byte
            const int i = flip ? 3 - px : px;                // its output pixel
            long long m = (long long)(((uint64_t)S[j] * dm) >> GE_DIV_SHIFT);   // S / (2h + 1)
            if (noise) {
                const uint32_t z = philox_halves_sum((uint32_t)(4 * q + i), (uint32_t)y, (uint32_t)(4 * s + 2 - cb), k0, k1);
                const uint32_t sg = sig[min((uint32_t)(m >> 16), (uint32_t)(BINEXPOSE_TABLE - 1))];
                m += ((long long)((int)z - 262140) * (long long)sg) >> 16;
            }
            const uint32_t mc = (uint32_t)min(max(m, 0ll), (long long)BINEXPOSE_ONE);
            uint32_t c = 0;                                  // decode: the largest c with MID[c] <= mc (MID[0] = 0)
#pragma unroll
            for (int step = BINEXPOSE_TABLE / 2; step >= 1; step >>= 1)
                if (mid[c + step] <= mc) c += step;
            code[j] = c;
        }
    }

    const size_t plane = (size_t)ch * cw;
    float* op = out + ((size_t)sb * 3) * plane + (size_t)y * cw + 4 * q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                            // RGB plane c = BGR byte 2 - c; read_img's astype(float32) / 255.
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)(flip ? code[3 * (3 - i) + 2 - c] : code[3 * i + 2 - c]) / 255.f;
        float* oc = op + c * plane;
        if (k == 4) {
            *reinterpret_cast<f32x4_a4*>(oc) = f32x4_a4{v[0], v[1], v[2], v[3]};
        } else {                                             // the last quad of a row, cw % 4 != 0: k = 1 .. 3 pixels
            oc[0] = v[0];
            if (k > 1) oc[1] = v[1];
            if (k > 2) oc[2] = v[2];
        }
    }
}

int binexpose_version(void) { return BINEXPOSE_VERSION; }

int binexpose_check_curve(const uint32_t* lin, const uint32_t* mid, const uint32_t* sig) {
    if (!lin || !mid || !sig) return BINEXPOSE_E_ARG;
    if (lin[0] != 0u || mid[0] != 0u || lin[BINEXPOSE_TABLE - 1] > (uint32_t)BINEXPOSE_ONE) return BINEXPOSE_E_ARG;
    for (int c = 0; c < BINEXPOSE_TABLE; ++c) {
        if (c > 0 && (lin[c] < lin[c - 1] || mid[c] <= mid[c - 1])) return BINEXPOSE_E_ARG;
        if (mid[c] > lin[c] || (c + 1 < BINEXPOSE_TABLE && lin[c] >= mid[c + 1])) return BINEXPOSE_E_ARG;
        if (sig[c] >= (uint32_t)BINEXPOSE_SIG_LIMIT) return BINEXPOSE_E_ARG;
    }
    return 0;
}

int binexpose_gather(const uint8_t* frames, int n_frames, int H, int W, const int32_t* table, int n, int n_slots, int n_blur, int ch,
                     int cw, const uint32_t* curve_dev, float* out, void* stream) {
    if (!frames || !table || !curve_dev || !out) return BINEXPOSE_E_ARG;
    if (n_frames <= 0 || H <= 0 || W <= 0 || n <= 0 || ch <= 0 || cw <= 0 || n_slots < 1 || n_slots > BINEXPOSE_MAX_SLOTS)
        return BINEXPOSE_E_SHAPE;
    if (ch > H || cw > W || n_blur < 0 || n_blur > n_slots) return BINEXPOSE_E_SHAPE;
    const int nq = (int)(((long long)cw + 3) / 4);
    long long items = (long long)n_slots * n;                // factor by factor: the full product of four ints can pass 2^63
    if (items > 0x7fffffffLL || (items *= ch) > 0x7fffffffLL || (items *= nq) > 0x7fffffffLL) return BINEXPOSE_E_SHAPE;
    const unsigned blocks = (unsigned)((items + GE_THREADS - 1) / GE_THREADS);
    hipLaunchKernelGGL(gather_exposed_kernel, dim3(blocks), dim3(GE_THREADS), 0, (hipStream_t)stream, frames, n_frames, H, W, table, n,
                       n_slots, n_blur, ch, cw, nq, (unsigned)items, curve_dev, out);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : (int)e;
}
