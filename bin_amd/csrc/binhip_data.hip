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
