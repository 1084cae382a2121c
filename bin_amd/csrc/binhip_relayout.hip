// binhip_relayout.hip — weight relayout: OIHW fp32 -> the convolution kernels' layout, fp16 hi (+ lo) planes
// [rows_pad / cb][cin_chunks][k * k][cb][16], 16-byte half slots XOR-swizzled by (row >> 3) & 1 for conflict-free ds_read_b128
// (binhip_conv_common.h: weight_lane_off).  Three kinds of forward-shaped operator Wp[row r][K entry j][dy][dx] (include/binhip.h):
//   FWD         the layer's own weights, rows optionally in PixelShuffle's order, with its bias;
//   DGRAD       backward-data: in / out channels swapped, taps flipped;
//   RDB_GATHER  backward-data of one concat group of a residual dense block, the later convs stacked along K.
// One kernel, one validator: the per-op entry points are batches of one item.
#include "binhip_internal.h"
#include <vector>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// PixelShuffle(2) as an order of n channels: position i = sub * (n / 4) + c holds channel c * 4 + sub (UPNet.0's rows)
__device__ __forceinline__ int shuffled(int i, int n) { const int q = n / 4; return (i % q) * 4 + i / q; }

// ---- what differs between the kinds: the value of the operator at (row r, K entry j, tap dy, dx) ------------------------------
__device__ __forceinline__ int fwd_src_row(const BinRelayoutItem& L, int r) { return L.shuffle_or_group ? shuffled(r, L.cout) : r; }
__device__ __forceinline__ float fetch_fwd(const BinRelayoutItem& L, int r, int j, int dy, int dx) {
    const int src = fwd_src_row(L, r);
    if (src >= L.cout || j >= L.cin) return 0.f;
    return L.w[0][(((long long)src * L.cin + j) * L.ksize + dy) * L.ksize + dx];
}
// The dgrad of a stride-1 "same" conv is the same conv with in/out channels swapped and the taps flipped:
// W'[r = ci][j = co][dy][dx] = W[co][ci][k-1-dy][k-1-dx].  shuffle: the dgrad's input channels j are UPNet.0's permuted rows.
__device__ __forceinline__ float fetch_dgrad(const BinRelayoutItem& L, int r, int j, int dy, int dx) {
    const int k = L.ksize, co = L.shuffle_or_group ? shuffled(j, L.cout) : j;
    if (r >= L.cin || j >= L.cout) return 0.f;
    return L.w[0][(((long long)co * L.cin + r) * k + (k - 1 - dy)) * k + (k - 1 - dx)];
}
// Backward-data of a residual dense block (G0, C, G) in GATHER form.  Group g of the block's concat buffer (g = 0: the G0 input
// channels, g >= 1: the G outputs of conv g-1) receives dgrad contributions from every later conv c = g .. C-1.  Stacking those
// convs' masked output gradients (G channels each, contiguous in the gradient buffer) along K turns the sum into ONE
// forward-shaped conv per group:  Wg[r][G (c - g) + co][dy][dx] = W_c[co][base_g + r][2-dy][2-dx],  base_0 = 0,
// base_g = G0 + G (g - 1);  rows = G0 (group 0) or G, K = (C - g) G.
__device__ __forceinline__ float fetch_gather(const BinRelayoutItem& L, int r, int j, int dy, int dx) {
    const int G0 = L.shape.G0, G = L.shape.G, g = L.shuffle_or_group;
    const int conv = g + j / G, co = j % G;
    const int ci = (g == 0 ? 0 : G0 + G * (g - 1)) + r;
    return L.w[conv][(((long long)co * (G0 + G * conv) + ci) * 3 + (2 - dy)) * 3 + (2 - dx)];
}

// ---- what they share: thread t owns the 16-byte half slot t of the plane and, for t < rows_pad, bias_out[t] ---------------------
template <float (*FETCH)(const BinRelayoutItem&, int, int, int, int)>
__device__ __forceinline__ void relayout_slot(const BinRelayoutItem& L, long long t) {
    const int ks = L.ksize, cb = L.cout_block, nchunks = L.cin_chunks;
    if (t < L.rows_pad) {
        float b = 0.f;
        if (L.kind == BINHIP_RELAYOUT_FWD && L.bias) {
            const int src = fwd_src_row(L, (int)t);
            if (src < L.cout) b = L.bias[src];
        }
        L.bias_out[t] = b;
    }
    if (t >= (long long)L.rows_pad * nchunks * ks * ks * 2) return;
    const int s = (int)(t & 1);                        // half slot
    long long u = t >> 1;
    const int row = (int)(u % cb); u /= cb;            // row in its block
    const int tap = (int)(u % (ks * ks)); u /= (ks * ks);
    const int c = (int)(u % nchunks); u /= nchunks;    // 16-channel chunk of K
    const int zb = (int)u;                             // row block
    const int cg = s ^ ((row >> 3) & 1);               // the chunk's half this slot holds
    const int r = zb * cb + row, j0 = c * 16 + cg * 8, dy = tap / ks, dx = tap % ks;
    half8 hv, lv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float v = FETCH(L, r, j0 + e, dy, dx);
        hv[e] = (_Float16)v;
        lv[e] = (_Float16)(v - (float)hv[e]);
    }
    *reinterpret_cast<half8*>((_Float16*)L.w_hi + t * 8) = hv;
    if (L.w_lo) *reinterpret_cast<half8*>((_Float16*)L.w_lo + t * 8) = lv;
}

// A training step re-lays-out every weight of a set after each optimizer update (66 forward + 66 backward layouts per set): one
// launch per <= RELAYOUT_BATCH items instead of one per layer (528 -> 24 launches per step of ~4.5 us each).  Block b of the
// grid belongs to the item whose block range contains it.
#define RELAYOUT_BATCH 22
struct RelayoutBatch {
    BinRelayoutItem it[RELAYOUT_BATCH];
    unsigned start[RELAYOUT_BATCH + 1];
    int n;
};
static_assert(sizeof(RelayoutBatch) <= 4096, "kernel argument block");

__global__ void __launch_bounds__(256)
relayout_batch_kernel(const RelayoutBatch rb) {
    const unsigned b = blockIdx.x;
    int li = 0;
#pragma unroll
    for (int i = 1; i < RELAYOUT_BATCH; ++i)
        if (i < rb.n && b >= rb.start[i]) li = i;
    const BinRelayoutItem& L = rb.it[li];
    const long long t = (long long)(b - rb.start[li]) * 256 + threadIdx.x;
    if (L.kind == BINHIP_RELAYOUT_FWD) relayout_slot<fetch_fwd>(L, t);
    else if (L.kind == BINHIP_RELAYOUT_DGRAD) relayout_slot<fetch_dgrad>(L, t);
    else relayout_slot<fetch_gather>(L, t);
}

// Every rule an item must meet, each written once.  RDB_GATHER: the zeros of `shape` are resolved to bin_stage4's block here,
// so the kernel sees concrete (G0, C, G).
static int relayout_check(BinRelayoutItem& L) {
    if (!L.w[0] || !L.w_hi || !L.bias_out) return BINHIP_E_ARG;
    const bool blocks_ok = L.cout_block > 0 && L.rows_pad % L.cout_block == 0 && L.cout_block % 32 == 0;
    if (L.kind == BINHIP_RELAYOUT_FWD || L.kind == BINHIP_RELAYOUT_DGRAD) {
        if (L.rows_pad % 32 || !blocks_ok) return BINHIP_E_SHAPE;
        if ((L.ksize != 1 && L.ksize != 3 && L.ksize != 5) || L.cout <= 0 || L.cin <= 0) return BINHIP_E_SHAPE;
        // rows and K entries of the operator: (cout, cin) of a forward layer, swapped for its backward-data
        const bool fwd = L.kind == BINHIP_RELAYOUT_FWD;
        const int rows = fwd ? L.cout : L.cin, kdim = fwd ? L.cin : L.cout;
        if (kdim > L.cin_chunks * 16 || rows > L.rows_pad) return BINHIP_E_SHAPE;
        if (L.shuffle_or_group && (L.cout % 4 || (fwd && L.cout != L.rows_pad))) return BINHIP_E_SHAPE;
    } else if (L.kind == BINHIP_RELAYOUT_RDB_GATHER) {
        BinRdnShape& S = L.shape;
        if (S.G0 <= 0) S.G0 = 96;
        if (S.C <= 0) S.C = 4;
        if (S.G <= 0) S.G = 32;
        const int g = L.shuffle_or_group;
        if (S.C > BINHIP_RDN_MAX_CONVS || S.G0 % 32 || S.G % 32) return BINHIP_E_SHAPE;
        if (g < 0 || g >= S.C) return BINHIP_E_ARG;
        if (L.rows_pad != (g == 0 ? S.G0 : S.G) || L.cin_chunks != (S.C - g) * S.G / 16 || L.ksize != 3) return BINHIP_E_SHAPE;
        if (!blocks_ok) return BINHIP_E_SHAPE;
        for (int k = g; k < S.C; ++k) if (!L.w[k]) return BINHIP_E_ARG;
    } else {
        return BINHIP_E_ARG;
    }
    return 0;
}

extern "C" {

size_t binhip_weights_bytes(int cout_pad, int cin_chunks, int ksize) {
    if (cout_pad <= 0 || cin_chunks <= 0 || ksize <= 0) return 0;      // no such layout (a negative product would wrap to a huge size)
    return (size_t)cout_pad * cin_chunks * ksize * ksize * 32;
}

int binhip_dgrad_rows_pad(int ksize, int cin) {
    // rows of the backward-data conv = original input channels, padded to the kernel's cout granularity (the LFF
    // dgrad's 224 rows form ONE 224-row workgroup column, so its input — the 96-channel output gradient — is read once)
    if (cin <= 0) return 0;
    return ((cin + 31) / 32) * 32;
}

int binhip_weights_relayout_batch(const BinRelayoutItem* items, int n, void* stream) {
    if (!items || n <= 0) return BINHIP_E_ARG;
    std::vector<BinRelayoutItem> its(items, items + n);
    for (BinRelayoutItem& L : its)                     // validate everything before the first launch
        if (int rc = relayout_check(L)) return rc;
    for (int i0 = 0; i0 < n; i0 += RELAYOUT_BATCH) {
        RelayoutBatch rb;
        const int m = (n - i0 < RELAYOUT_BATCH) ? n - i0 : RELAYOUT_BATCH;
        unsigned blocks = 0;
        for (int i = 0; i < m; ++i) {
            const BinRelayoutItem& L = rb.it[i] = its[i0 + i];
            rb.start[i] = blocks;
            const long long total = (long long)L.rows_pad * L.cin_chunks * L.ksize * L.ksize * 2;
            blocks += (unsigned)((total + 255) / 256);
        }
        for (int i = m; i < RELAYOUT_BATCH; ++i) rb.it[i] = rb.it[0];
        for (int i = m; i <= RELAYOUT_BATCH; ++i) rb.start[i] = blocks;
        rb.n = m;
        hipLaunchKernelGGL(relayout_batch_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, rb);
        BH_CHECK_LAUNCH();
    }
    return 0;
}

int binhip_weights_relayout(const float* w_oihw, const float* bias, int cout, int cin, int ksize,
                            int cout_pad, int cin_chunks, int cout_block, int shuffle_perm,
                            void* w_hi, void* w_lo, float* bias_out, void* stream) {
    BinRelayoutItem it = {};
    it.w[0] = w_oihw; it.bias = bias; it.w_hi = w_hi; it.w_lo = w_lo; it.bias_out = bias_out;
    it.kind = BINHIP_RELAYOUT_FWD; it.cout = cout; it.cin = cin; it.ksize = ksize; it.rows_pad = cout_pad;
    it.cin_chunks = cin_chunks; it.cout_block = cout_block; it.shuffle_or_group = shuffle_perm;
    return binhip_weights_relayout_batch(&it, 1, stream);
}

int binhip_weights_relayout_dgrad(const float* w_oihw, int cout, int cin, int ksize, int rows_pad, int cin_chunks,
                                  int cout_block, int shuffle_perm, void* w_hi, void* w_lo, float* bias_out,
                                  void* stream) {
    BinRelayoutItem it = {};
    it.w[0] = w_oihw; it.w_hi = w_hi; it.w_lo = w_lo; it.bias_out = bias_out;
    it.kind = BINHIP_RELAYOUT_DGRAD; it.cout = cout; it.cin = cin; it.ksize = ksize; it.rows_pad = rows_pad;
    it.cin_chunks = cin_chunks; it.cout_block = cout_block; it.shuffle_or_group = shuffle_perm;
    return binhip_weights_relayout_batch(&it, 1, stream);
}

int binhip_weights_relayout_rdb_gather(const float* const* w_oihw4, int group, int cout_block, void* w_hi, void* w_lo,
                                       float* bias_out, void* stream) {
    if (!w_oihw4) return BINHIP_E_ARG;
    BinRelayoutItem it = {};                           // shape all zero: bin_stage4's block (96, -, 4, 32)
    // entries below `group` may be NULL here and are never read, but an item names w[0] whatever its group: w_hi stands in for them
    for (int i = 0; i < 4; ++i) it.w[i] = i < group ? (const float*)w_hi : w_oihw4[i];
    it.w_hi = w_hi; it.w_lo = w_lo; it.bias_out = bias_out;
    it.kind = BINHIP_RELAYOUT_RDB_GATHER; it.ksize = 3; it.cout_block = cout_block; it.shuffle_or_group = group;
    it.rows_pad = group == 0 ? 96 : 32;
    it.cin_chunks = 2 * (4 - group);
    return binhip_weights_relayout_batch(&it, 1, stream);
}

}  // extern "C"
