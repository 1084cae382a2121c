// binhip_data.hip — training batches cut out of a device-resident uint8 frame arena (data/BIN_dataset.py:30-54, 63-183 and
// models/bin_model.py:147-202): per window, the reference's loader reads 17 frames, crops one (y0, x0) window of ch x cw from
// each, maybe flips it horizontally, and the model stages them as fp32 RGB CHW /255.  Here one launch does all of it for a
// batch: crop, flip, BGR -> RGB, /255 and the slot-major output layout.  The temporal reverse is the order of the frame ids in
// the table row, so the kernel does nothing for it.
// One lane = 4 consecutive output pixels of one output row: 12 source bytes, read as the aligned dwords that overlap them
// (neighbouring lanes cover one contiguous run of the source row, backwards when the row is flipped), and one 16-byte store
// per colour plane.  The last quad of a row with cw % 4 != 0 is predicated: it loads only the dwords its pixels touch and
// stores only its pixels.
#include "binhip_internal.h"
#include "binhip_gather_load.h"   // gw_load12

namespace {
constexpr int GW_THREADS = 256;
constexpr int GW_MAX_SLOTS = 32;
// one 16-byte store at the 4-byte alignment of an output row whose width is not a multiple of 4 (global_store_dwordx4 needs
// only dword alignment on gfx950, which runs with unaligned access enabled)
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
}  // namespace

// grid: ceil(n_slots * n * ch * ceil(cw / 4) / GW_THREADS); item t = (slot, sample, output row y, quad q), q fastest
__global__ void __launch_bounds__(GW_THREADS)
gather_windows_kernel(const uint8_t* __restrict__ frames, int n_frames, int H, int W, const int32_t* __restrict__ table, int n,
                      int n_slots, int ch, int cw, int nq, unsigned items, float* __restrict__ out) {
    const unsigned t = blockIdx.x * GW_THREADS + threadIdx.x;
    if (t >= items) return;
    const unsigned row = t / (unsigned)nq;
    const int q = (int)(t - row * (unsigned)nq);
    const unsigned sb = row / (unsigned)ch;                  // slot * n + sample
    const int y = (int)(row - sb * (unsigned)ch);
    const int s = (int)(sb / (unsigned)n), b = (int)(sb - (unsigned)s * (unsigned)n);

    // The host validates the table; the clamps only guarantee that a bad row can never read outside the arena.
    const int32_t* rec = table + (size_t)b * (n_slots + 3);
    const int id = min(max(rec[s], 0), n_frames - 1);
    const int y0 = min(max(rec[n_slots], 0), H - ch);
    const int x0 = min(max(rec[n_slots + 1], 0), W - cw);
    const bool flip = rec[n_slots + 2] != 0;

    // output pixel 4q + i (i < k) comes from source pixel x0 + 4q + i, or x0 + cw - 1 - 4q - i when flipped; both are
    // pixels va .. vb - 1 of the 4-pixel source window that starts at sx
    const int k = min(4, cw - 4 * q);
    const int sx = flip ? x0 + cw - 4 - 4 * q : x0 + 4 * q;  // left of x0 (even of the row) only for a flipped last quad
    const int va = flip ? 4 - k : 0, vb = flip ? 4 : k;
    const long long boff = (((long long)id * H + (y0 + y)) * W + sx) * 3;   // negative only for that flipped last quad
    const unsigned off = (unsigned)(((uintptr_t)frames + boff) & 3u);
    const uint32_t* d = reinterpret_cast<const uint32_t*>(frames + (boff - off));
    // needed bytes [off + 3 va, off + 3 vb) of d: dwords jlo .. jhi.  A dword outside that range is not needed; it loads a
    // needed one instead (no branch, and never an address the window does not touch)
    const int jlo = ((int)off + 3 * va) >> 2, jhi = ((int)off + 3 * vb - 1) >> 2;
    uint32_t w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = d[min(max(j, jlo), jhi)];
    // the 12 window bytes, little-endian: pixel p = bytes 3p (B), 3p + 1 (G), 3p + 2 (R)
    const uint32_t a0 = __builtin_amdgcn_alignbyte(w[1], w[0], off);
    const uint32_t a1 = __builtin_amdgcn_alignbyte(w[2], w[1], off);
    const uint32_t a2 = __builtin_amdgcn_alignbyte(w[3], w[2], off);
    const uint32_t px[4][3] = {{a0 & 0xffu, (a0 >> 8) & 0xffu, (a0 >> 16) & 0xffu},
                               {a0 >> 24, a1 & 0xffu, (a1 >> 8) & 0xffu},
                               {(a1 >> 16) & 0xffu, a1 >> 24, a2 & 0xffu},
                               {(a2 >> 8) & 0xffu, (a2 >> 16) & 0xffu, a2 >> 24}};

    const size_t plane = (size_t)ch * cw;
    float* o = out + ((size_t)sb * 3) * plane + (size_t)y * cw + 4 * q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                            // RGB plane c = BGR byte 2 - c; read_img's astype(float32) / 255.
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)(flip ? px[3 - i][2 - c] : px[i][2 - c]) / 255.f;   // static indices: no scratch
        float* oc = o + c * plane;
        if (k == 4) {
            *reinterpret_cast<f32x4_a4*>(oc) = f32x4_a4{v[0], v[1], v[2], v[3]};
        } else {                                             // the last quad of a row, cw % 4 != 0: k = 1 .. 3 pixels
            oc[0] = v[0];
            if (k > 1) oc[1] = v[1];
            if (k > 2) oc[2] = v[2];
        }
    }
}

int binhip_gather_windows(const uint8_t* frames, int n_frames, int H, int W, const int32_t* table, int n, int n_slots, int ch,
                          int cw, float* out, void* stream) {
    if (!frames || !table || !out) return BINHIP_E_ARG;
    if (n_frames <= 0 || H <= 0 || W <= 0 || n <= 0 || ch <= 0 || cw <= 0 || n_slots < 1 || n_slots > GW_MAX_SLOTS)
        return BINHIP_E_SHAPE;
    if (ch > H || cw > W) return BINHIP_E_SHAPE;
    const int nq = (cw + 3) / 4;
    const long long items = (long long)n_slots * n * ch * nq;
    if (items > 0x7fffffffLL) return BINHIP_E_SHAPE;
    const unsigned blocks = (unsigned)((items + GW_THREADS - 1) / GW_THREADS);
    hipLaunchKernelGGL(gather_windows_kernel, dim3(blocks), dim3(GW_THREADS), 0, (hipStream_t)stream, frames, n_frames, H, W, table,
                       n, n_slots, ch, cw, nq, (unsigned)items, out);
    BH_CHECK_LAUNCH();
    return 0;
}

// ---- the same gather with the blurry slots synthesised from the sharp frames of the arena (the reference's
// data_scripts/adobe240fps/create_dataset_blur_N_frames_average.py:116-134): a blurry frame is the truncated mean of the
// L = 2h + 1 consecutive sharp frames around its centre.  The lane of a blurry slot repeats the 12-byte load for the L frames
// (H W 3 bytes apart) and sums the bytes, two 16-bit sums per dword (L <= 33: a sum is at most 8415).  The script's float32
// sum / float(L) truncated equals the integer quotient S / L for every S <= 255 L (tests/test_cpu_blur_synth.py proves it),
// and S / L = (S * GW_DIV[h]) >> 23 with GW_DIV[h] = ceil(2^23 / L): the product overshoots S / L by less than
// 8415 / 2^23 < 1 / 33 <= 1 / L, which cannot reach the next integer, and both factors fit 24 bits.
namespace {
constexpr int GW_MAX_HALF = 16;
struct GwDiv { uint32_t m[GW_MAX_HALF + 1]; };
constexpr GwDiv gw_div_table() {
    GwDiv t{};
    for (int h = 0; h <= GW_MAX_HALF; ++h) t.m[h] = 0x7fffffu / (uint32_t)(2 * h + 1) + 1u;
    return t;
}
__device__ const GwDiv GW_DIV = gw_div_table();

}  // namespace

// grid and items as gather_windows_kernel; table rows are [n_slots ids][y0][x0][flip][h]
__global__ void __launch_bounds__(GW_THREADS)
gather_windows_blur_kernel(const uint8_t* __restrict__ frames, int n_frames, int H, int W, const int32_t* __restrict__ table,
                           int n, int n_slots, int n_blur, int ch, int cw, int nq, unsigned items, float* __restrict__ out) {
    const unsigned t = blockIdx.x * GW_THREADS + threadIdx.x;
    if (t >= items) return;
    const unsigned row = t / (unsigned)nq;
    const int q = (int)(t - row * (unsigned)nq);
    const unsigned sb = row / (unsigned)ch;                  // slot * n + sample
    const int y = (int)(row - sb * (unsigned)ch);
    const int s = (int)(sb / (unsigned)n), b = (int)(sb - (unsigned)s * (unsigned)n);

    // The host validates the table; the clamps only guarantee that a bad row can never read outside the arena.
    const int32_t* rec = table + (size_t)b * (n_slots + 4);
    const int h = s < n_blur ? min(min(max(rec[n_slots + 3], 0), GW_MAX_HALF), (n_frames - 1) >> 1) : 0;
    const int id = min(max(rec[s], h), n_frames - 1 - h);    // id - h .. id + h inside [0, n_frames)
    const int y0 = min(max(rec[n_slots], 0), H - ch);
    const int x0 = min(max(rec[n_slots + 1], 0), W - cw);
    const bool flip = rec[n_slots + 2] != 0;

    const int k = min(4, cw - 4 * q);
    const int sx = flip ? x0 + cw - 4 - 4 * q : x0 + 4 * q;
    const int va = flip ? 4 - k : 0, vb = flip ? 4 : k;
    const long long stride = (long long)H * W * 3;           // bytes per frame
    const uint8_t* p = frames + (((long long)id * H + (y0 + y)) * W + sx) * 3;

    // e[j] / o[j]: the sums of bytes 0 and 2 / 1 and 3 of window dword j, 16 bits each
    uint32_t e[3], o[3];
    {
        uint32_t a[3];
        gw_load12(p, va, vb, a[0], a[1], a[2]);
#pragma unroll
        for (int j = 0; j < 3; ++j) e[j] = a[j] & 0x00ff00ffu, o[j] = (a[j] >> 8) & 0x00ff00ffu;
    }
    int f = 1;
    for (; f + 1 <= h; f += 2) {                             // frames -f-1, -f, f, f+1: 16 loads in flight before the first add
        uint32_t a[4][3];
        gw_load12(p - (f + 1) * stride, va, vb, a[0][0], a[0][1], a[0][2]);
        gw_load12(p - f * stride, va, vb, a[1][0], a[1][1], a[1][2]);
        gw_load12(p + f * stride, va, vb, a[2][0], a[2][1], a[2][2]);
        gw_load12(p + (f + 1) * stride, va, vb, a[3][0], a[3][1], a[3][2]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) e[j] += a[i][j] & 0x00ff00ffu, o[j] += (a[i][j] >> 8) & 0x00ff00ffu;
    }
    if (f <= h) {                                            // odd h: the outermost pair
        uint32_t a[2][3];
        gw_load12(p - f * stride, va, vb, a[0][0], a[0][1], a[0][2]);
        gw_load12(p + f * stride, va, vb, a[1][0], a[1][1], a[1][2]);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) e[j] += a[i][j] & 0x00ff00ffu, o[j] += (a[i][j] >> 8) & 0x00ff00ffu;
    }
    // window byte 4j + i: i = 0, 2 in e[j] (low, high half), i = 1, 3 in o[j]; pixel p = bytes 3p (B), 3p + 1 (G), 3p + 2 (R)
    const uint32_t m = GW_DIV.m[h];
    uint32_t px[4][3];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const uint32_t pair = (i & 1) ? o[i >> 2] : e[i >> 2];
        const uint32_t sum = (i & 2) ? pair >> 16 : pair & 0xffffu;
        px[i / 3][i % 3] = __umul24(sum, m) >> 23;           // sum / (2h + 1)
    }

    const size_t plane = (size_t)ch * cw;
    float* op = out + ((size_t)sb * 3) * plane + (size_t)y * cw + 4 * q;
#pragma unroll
    for (int c = 0; c < 3; ++c) {                            // RGB plane c = BGR byte 2 - c; read_img's astype(float32) / 255.
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)(flip ? px[3 - i][2 - c] : px[i][2 - c]) / 255.f;
        float* oc = op + c * plane;
        if (k == 4) {
            *reinterpret_cast<f32x4_a4*>(oc) = f32x4_a4{v[0], v[1], v[2], v[3]};
        } else {
            oc[0] = v[0];
            if (k > 1) oc[1] = v[1];
            if (k > 2) oc[2] = v[2];
        }
    }
}

int binhip_gather_windows_blur(const uint8_t* frames, int n_frames, int H, int W, const int32_t* table, int n, int n_slots,
                               int n_blur, int ch, int cw, float* out, void* stream) {
    if (!frames || !table || !out) return BINHIP_E_ARG;
    if (n_frames <= 0 || H <= 0 || W <= 0 || n <= 0 || ch <= 0 || cw <= 0 || n_slots < 1 || n_slots > GW_MAX_SLOTS)
        return BINHIP_E_SHAPE;
    if (ch > H || cw > W || n_blur < 0 || n_blur > n_slots) return BINHIP_E_SHAPE;
    const int nq = (cw + 3) / 4;
    const long long items = (long long)n_slots * n * ch * nq;
    if (items > 0x7fffffffLL) return BINHIP_E_SHAPE;
    const unsigned blocks = (unsigned)((items + GW_THREADS - 1) / GW_THREADS);
    hipLaunchKernelGGL(gather_windows_blur_kernel, dim3(blocks), dim3(GW_THREADS), 0, (hipStream_t)stream, frames, n_frames, H, W,
                       table, n, n_slots, n_blur, ch, cw, nq, (unsigned)items, out);
    BH_CHECK_LAUNCH();
    return 0;
}
