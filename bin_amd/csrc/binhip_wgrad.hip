// binhip_wgrad.hip — weight/bias gradients of the bin_stage4 convolutions on the matrix cores.
//
// Stands in for autograd's conv2d weight/bias backward of every F.conv2d on the path (reference
// models/archs/RDN.py:141,162,187-207, triggered by bin_model.py:140 `l_pix.backward()`):
//     dW[co][ci][dy][dx] = sum_{n,y,x} gY[co][n,y,x] * X[ci][n,y+dy-p,x+dx-p],   db[co] = sum gY[co]
// as a GEMM whose contraction dimension is the PIXEL index: per tap, D[ci 32][co 32] += X^T[ci][px16] * gY[px16][co]
// with v_mfma_f32_32x32x16_f16.  Both operands live in chunk planes ([pixel][16 ch], pixel-major), i.e. with the
// contraction index on the slow axis, so fragments are fetched with the LDS transpose read ds_read_b64_tr_b16
// (lane t of a 16-lane group addresses pixel t/4, 8-byte piece t%4 and receives channel t of pixels 0..3 — mapping
// verified on hardware by tools/probe_tr16.hip).
//
// Work split: block (pb, cp, z) owns input-channel pair cp (32 ci), output tile z (32 co, and for 5x5 one tap
// row), and walks pixel tiles pb, pb+PB, ... (8x32 pixels, halo patch + gY tile DMA'd to LDS, double buffered),
// keeping all its taps' 32x32 accumulators in registers (K-split over the 4 waves by pixel row).  At the end the
// 4 waves are reduced through LDS and ONE partial per block is written; a second kernel sums the PB partials in a
// fixed order (deterministic), un-scales and scatters to OIHW fp32.
// Tests: tests/wgrad_cases.py restates wg_geom() / w1_plan() and holds one case per kernel, variant and work-split property.
//
// Three main kernels with three schedules (one-burst DMA and a K-split over 4 waves in wgrad_mfma_kernel, DMA spread over the multiply
// steps and 8 waves in wgrad3x3_xrow_kernel, a streaming strip walk without K-split in wgrad1x1_kernel) over one core:
//     helper                                   generic 5x5 / wide 1x1    3x3 X-row                     streaming 1x1
//     tile_origin                              wg_issue                  wg3x_offsets                  issue
//     x_chunk_rsrc / g_chunk_rsrc              wg_issue                  wg3x_issue_part               issue
//     dma_lane / dma_offset                    wg_issue                  prologue / wg3x_offsets       prologue / issue
//     tr_addr                                  tr_issue_at               xa, xb2, g_off                tr_off
//     tr_issue (one address | two + immediate) tr_issue_at               load                          load
//     tr_tie, tr_value                         K-step loop               step loop                     K-step loop
//     acc_row                                  reduce_waves_to_partial   reduce_waves_to_partial       direct store
//     reduce_waves_to_partial<NW>, pairwise    NW = 4                    NW = 8                        (no K-split: none)
//     wg_block                                 workgroup id              workgroup id                  (2-D grid)
#include "binhip_internal.h"
#include <utility>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef short short4_ __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void_t;

struct WgradKArgs {
    const _Float16* x_hi;
    const _Float16* x_lo;
    const _Float16* g_hi;
    const _Float16* g_lo;
    float* partial;
    float* partial_b;
    long long x_group_stride;
    int x_cpg;
    int N, H, W;
    int cin_chunks, cout_chunks;
    int tiles_x, tiles_y, ntiles;
    int PB, ncp, ncot;
    int ppg;      // 1x1 kernel: input-channel pairs per workgroup column (blockIdx.y)
    int nz;       // generic / lean kernels: ncot * ndyg (1-D grid of PB * ncp * nz workgroups, see wg_block())
};

template <int KS, int TR, int NT>
struct WgCfg {
    static constexpr int THREADS = 256;
    static constexpr int PAD = KS / 2;
    static constexpr int TH = 8;
    static constexpr int PH = TH + TR - 1;
    static constexpr int PW = 32 + KS - 1;
    static constexpr int NTAP = TR * KS;
    static constexpr int XP = (PH * PW * 2 + 63) / 64;   // 1-KiB pieces per X chunk patch
    static constexpr int GP = TH * 32 * 2 / 64;          // 1-KiB pieces per gY chunk tile (= 8)
    static constexpr int XBYTES = XP * 1024, GBYTES = GP * 1024;
    static constexpr int PLANE_BYTES = 2 * XBYTES + 2 * GBYTES;
    static constexpr int NPL = (NT == 3) ? 2 : 1;
    static constexpr int BUF_BYTES = NPL * PLANE_BYTES;
    static constexpr int LDS_BYTES = (2 * BUF_BYTES > 16384) ? 2 * BUF_BYTES : 16384;
    static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
};

// ---- the core the three kernels share --------------------------------------------------------------------------------------------
// pixel tile -> image and the tile's first row / column (tiles are TH rows x 32 columns, row-major within an image)
struct TileOrigin { int img, ty0, tx0; };
__device__ __forceinline__ TileOrigin tile_origin(const WgradKArgs& a, int tile, int TH) {
    const int tx = tile % a.tiles_x, b = tile / a.tiles_x;
    return {b / a.tiles_y, (b % a.tiles_y) * TH, tx * 32};
}
// byte offset of pixel (y, x) of image img in a chunk plane; y / x may be one halo step outside the image (the range check of
// dma_offset() then decides), so this is a signed int (the entry point holds N * H * W below 2^26)
__device__ __forceinline__ int pixel_byte(const WgradKArgs& a, int img, int y, int x) {
    return (int)((((long long)img * a.H + y) * a.W + x) * 32);
}

// Buffer resource of one operand chunk plane (16 channels x all pixels) of precision plane pl (0 hi, 1 lo).  A chunk that does not
// exist (odd chunk count, ragged cout) gets a resource of size 0: every load from it returns zeros.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t chunk_rsrc(const _Float16* plane0, long long elem_off, bool have, unsigned plane_bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)(have ? plane0 + elem_off : plane0), 0, have ? plane_bytes : 0u, 0x00020000);
}
// X chunks may come in groups of x_cpg planes, x_group_stride elements apart (GFF.0 reads the first planes of each block buffer)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t x_chunk_rsrc(const WgradKArgs& a, int pl, int c, long long plane_elems, unsigned plane_bytes) {
    const long long off = (a.x_cpg > 0) ? (long long)(c / a.x_cpg) * a.x_group_stride + (long long)(c % a.x_cpg) * plane_elems
                                        : (long long)c * plane_elems;
    return chunk_rsrc(pl ? a.x_lo : a.x_hi, off, c < a.cin_chunks, plane_bytes);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t g_chunk_rsrc(const WgradKArgs& a, int pl, int c, long long plane_elems, unsigned plane_bytes) {
    return chunk_rsrc(pl ? a.g_lo : a.g_hi, (long long)c * plane_elems, c < a.cout_chunks, plane_bytes);
}

// Per-lane buffer offset of a 1-KiB DMA piece (64 lanes x 16 B = 32 pixels of one chunk).  Lane l of piece i carries 16-byte half
// (q & 1) of pixel p = q >> 1, q = 64 i + l, of a patch PW pixels wide and npix pixels large, and fetches the half swizzled by bit 3
// of p (so that the transpose reads below are conflict free).  dma_lane() is the tile-invariant part; dma_offset() adds the tile:
// base = pixel_byte() of the patch's pixel (0, 0), which is image pixel (y0, x0); a pixel outside the image or the patch gets an
// offset that fails the resource's range check and arrives as zeros.
struct DmaLane { int py, px, src; };
__device__ __forceinline__ DmaLane dma_lane(int piece, int lane, int PW, int npix, int W) {
    const int q = piece * 64 + lane, p = q >> 1, py = p / PW, px = p - py * PW;
    return {p < npix ? py : -(1 << 20), px, (py * W + px) * 32 + (((q & 1) ^ ((p >> 3) & 1)) << 4)};
}
__device__ __forceinline__ unsigned dma_offset(const DmaLane& d, int base, int y0, int x0, int H, int W) {
    const bool ok = (unsigned)(y0 + d.py) < (unsigned)H && (unsigned)(x0 + d.px) < (unsigned)W;
    return ok ? (unsigned)(base + d.src) : 0x80000000u;
}

// Fragments come from LDS by transpose reads issued from inline asm.  The compiler knows nothing about the alias classes of the
// transpose-read builtin, so after an LDS-DMA (buffer_load ... lds) it protects every builtin read with s_waitcnt vmcnt(0) — which
// serialises "prefetch the next stage" and "compute this one".  Asm reads are invisible to that pass; the price is that the lgkmcnt
// wait is ours: tr_issue() ... s_waitcnt lgkmcnt ... tr_tie() on the SAME registers before their first use.
typedef __attribute__((address_space(3))) const char lds_cchar_t;
__device__ __forceinline__ unsigned lds_addr(const char* p) { return (unsigned)(size_t)(lds_cchar_t*)p; }
// Byte offset, within a pair of chunk strips chunk_bytes apart, of the lane's 4-pixel read of the fragment that starts at pixel p0:
// lane -> channel column lane & 15 of chunk (lane >> 4) & 1, pixels p0 + 8 (lane >> 5) + 0..3; lane t of a 16-lane group addresses
// pixel t / 4, 8-byte piece t % 4, the 16-byte half un-swizzled by bit 3 of the pixel.  The read of pixels +4..7 is tr_addr(p0 + 4);
// where p0 is a multiple of 8 that is the same address + 128.
__device__ __forceinline__ unsigned tr_addr(int chunk_bytes, int p0, int lane) {
    const int t = lane & 15, ch = (lane >> 4) & 1, p = p0 + (lane >> 5) * 8 + (t >> 2);
    return (unsigned)(ch * chunk_bytes + p * 32 + ((((t & 3) >> 1) ^ ((p >> 3) & 1)) << 4) + ((t & 1) << 3));
}
struct TrFrag { short4_ a, b; };     // pixels +0..3 and +4..7 of the lane's channel
// (ordinary ds_read_b64 in place of the transpose read, timing-only build: 209.8 vs 204.9 us — the transpose unit is free)
template <int OFF>
__device__ __forceinline__ void tr_read(short4_& dst, unsigned addr) {
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
// the two issue forms: one address for a fragment at a pixel offset that is a multiple of 8, or both reads' addresses + an immediate
__device__ __forceinline__ void tr_issue(TrFrag& f, unsigned addr) { tr_read<0>(f.a, addr); tr_read<128>(f.b, addr); }
template <int OFF>
__device__ __forceinline__ void tr_issue(TrFrag& f, unsigned oa, unsigned ob) { tr_read<OFF>(f.a, oa); tr_read<OFF>(f.b, ob); }
// general pixel offset (tap-shifted patches): both 4-pixel reads get their own swizzled address
__device__ __forceinline__ void tr_issue_at(TrFrag& f, const char* img, int chunk_bytes, int p0, int lane) {
    tr_issue<0>(f, lds_addr(img) + tr_addr(chunk_bytes, p0, lane), lds_addr(img) + tr_addr(chunk_bytes, p0 + 4, lane));
}
// after an `s_waitcnt lgkmcnt` asm: re-defines the fragment's registers so that no use can be scheduled above the wait
__device__ __forceinline__ void tr_tie(TrFrag& f) { asm volatile("" : "+v"(f.a), "+v"(f.b)); }
__device__ __forceinline__ half8 tr_value(const TrFrag& f) {
    union { struct { short4_ a, b; } s; half8 h; } u;
    u.s.a = f.a; u.s.b = f.b;
    return u.h;
}
template <class F, int... S>
__device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, S...>) {
    (f(std::integral_constant<int, S>{}), ...);
}

// element e of a lane's 32x32 accumulator -> row m of the tile (the column is lane & 31, hi = lane >> 5)
__device__ __forceinline__ int acc_row(int e, int hi) { return (e & 3) + 8 * (e >> 2) + 4 * hi; }
// p[0] + p[STRIDE] + ... (N terms) as a balanced tree: ((0 + 1) + (2 + 3)), (((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)))
template <int N, int STRIDE>
__device__ __forceinline__ float pairwise(const float* p) {
    if constexpr (N == 1) return p[0];
    else return pairwise<N / 2, STRIDE>(p) + pairwise<N / 2, STRIDE>(p + (N / 2) * STRIDE);
}
// K-split kernels: the NW waves' accumulators of one tap are summed through LDS (red: [NW][32 m][32 n]) in that fixed order and
// the 32x32 partial tile goes to dst
template <int NW>
__device__ __forceinline__ void reduce_waves_to_partial(float* red, const floatx16& acc, int wave, int lane, float* dst) {
    const int n = lane & 31, hi = lane >> 5, tid = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) red[wave * 1024 + acc_row(e, hi) * 32 + n] = acc[e];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16 / NW; ++i) dst[tid + 64 * NW * i] = pairwise<NW, 1024>(red + tid + 64 * NW * i);
}

// generic kernel: DMA of one tile's X halo patches and gY tiles (both chunks of the pair, every plane) into stage buf, in one burst
template <int KS, int TR, int NT, int NW = 4>
__device__ __forceinline__ void wg_issue(const WgradKArgs& a, char* smem, int buf, int tile, int cp, int cot, int dy0,
                                         int wave, int lane, long long plane_elems, unsigned plane_bytes) {
    using C = WgCfg<KS, TR, NT>;
    const TileOrigin o = tile_origin(a, tile, C::TH);
    const int H = a.H, W = a.W;
    const int xy0 = o.ty0 + dy0 - C::PAD, xx0 = o.tx0 - C::PAD;
    const int xbase = pixel_byte(a, o.img, xy0, xx0), gbase = pixel_byte(a, o.img, o.ty0, o.tx0);
#pragma unroll
    for (int pl = 0; pl < C::NPL; ++pl) {
        char* pbase = smem + buf * C::BUF_BYTES + pl * C::PLANE_BYTES;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // ---- X patch of input chunk 2*cp + h
            const __amdgpu_buffer_rsrc_t rs = x_chunk_rsrc(a, pl, 2 * cp + h, plane_elems, plane_bytes);
            char* lds = pbase + h * C::XBYTES;
#pragma unroll
            for (int j = 0; j < (C::XP + NW - 1) / NW; ++j) {
                const int i = wave + NW * j;
                if (i >= C::XP) break;
                const unsigned vo = dma_offset(dma_lane(i, lane, C::PW, C::PH * C::PW, W), xbase, xy0, xx0, H, W);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(lds + i * 1024), 16, vo, 0, 0, 0);
            }
            // ---- gY tile of output chunk 2*cot + h
            const __amdgpu_buffer_rsrc_t gs = g_chunk_rsrc(a, pl, 2 * cot + h, plane_elems, plane_bytes);
            char* gl = pbase + 2 * C::XBYTES + h * C::GBYTES;
#pragma unroll
            for (int j = 0; j < (C::GP + NW - 1) / NW; ++j) {
                const int i = wave + NW * j;
                if (C::GP % NW != 0 && i >= C::GP) break;
                const unsigned vo = dma_offset(dma_lane(i, lane, 32, C::TH * 32, W), gbase, o.ty0, o.tx0, H, W);
                __builtin_amdgcn_raw_ptr_buffer_load_lds(gs, (lds_void_t*)(gl + i * 1024), 16, vo, 0, 0, 0);
            }
        }
    }
}

// Workgroup -> (pixel-block pb, channel pair cp, z = output tile / tap-row group) for the generic and lean kernels.  The
// ncp * nz workgroups of one pb walk the SAME pixel tiles (each re-reading the gY tile its siblings read, and for nz > 1 the X
// patch): the hardware deals consecutive workgroup ids round-robin to the 8 XCDs, so the plain (pb, cp, z) grid put the
// siblings on different XCDs = different L2s and every one of them fetched its gY from HBM (PMC: 811 MB per launch for
// 392 MB of operands in the dense-block layers).  With PB a multiple of 8 the id is unpacked as
//     xcd = id % 8, slot = id / 8, pb = (slot / G) * 8 + xcd, (cp, z) = slot % G        (G = ncp * nz)
// which keeps all siblings of a pb on ONE XCD, dispatched back to back.
__device__ __forceinline__ void wg_block(const WgradKArgs& a, int& pb, int& cp, int& z) {
    const int id = blockIdx.x, G = a.ncp * a.nz;
    int r;
    if ((a.PB & 7) == 0) {
        const int slot = id >> 3;
        pb = (slot / G) * 8 + (id & 7);
        r = slot % G;
    } else {
        pb = id / G;
        r = id % G;
    }
    cp = r % a.ncp;
    z = r / a.ncp;
}

template <int KS, int TR, int NT>
__global__ void __launch_bounds__((WgCfg<KS, TR, NT>::THREADS))
wgrad_mfma_kernel(const WgradKArgs a) {
    using C = WgCfg<KS, TR, NT>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int pb, cp, bz;
    wg_block(a, pb, cp, bz);
    const int cot = bz % a.ncot;
    const int dyg = bz / a.ncot;
    const int dy0 = dyg * TR;
    const long long plane_elems = (long long)a.N * a.H * a.W * 16;
    const unsigned plane_bytes = (unsigned)(plane_elems * 2);
    const bool do_bias = (cp == 0) && (dyg == 0);

    floatx16 acc[C::NTAP];
    floatx16 accb;
#pragma unroll
    for (int e = 0; e < 16; ++e) accb[e] = 0.f;
#pragma unroll
    for (int t = 0; t < C::NTAP; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
    half8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = (_Float16)1.0f;

    int tile = pb;
    if (tile < a.ntiles) wg_issue<KS, TR, NT>(a, smem, 0, tile, cp, cot, dy0, wave, lane, plane_elems, plane_bytes);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (; tile < a.ntiles; tile += a.PB) {
        const int nxt = tile + a.PB;
        if (nxt < a.ntiles) wg_issue<KS, TR, NT>(a, smem, cur ^ 1, nxt, cp, cot, dy0, wave, lane, plane_elems, plane_bytes);
        const char* xb = smem + cur * C::BUF_BYTES;
        const char* gb = xb + 2 * C::XBYTES;
        // 4 K-steps per wave and tile (2 rows x 2 half-rows of 16 pixels), software-pipelined: the transpose reads of
        // K-step s+1 are issued before the MFMAs of K-step s (a workgroup is alone on its CU, one wave per SIMD, so
        // nothing else hides the LDS latency); sched_barriers keep the scheduler from sinking the reads again.
        // The reads are issued from asm (tr_issue_at): the builtin would be fenced with vmcnt(0) against the prefetch above.
        TrFrag Bh[2], Bl[2], Ah[2][C::NTAP], Al[2][C::NTAP];
        auto load = [&](int s4, int q) {
            const int row = wave * 2 + (s4 >> 1), x0 = (s4 & 1) * 16;
            tr_issue_at(Bh[q], gb, C::GBYTES, row * 32 + x0, lane);
            if constexpr (NT == 3) tr_issue_at(Bl[q], gb + C::PLANE_BYTES, C::GBYTES, row * 32 + x0, lane);
#pragma unroll
            for (int t = 0; t < C::NTAP; ++t) {
                const int p0 = (row + t / KS) * C::PW + x0 + t % KS;
                tr_issue_at(Ah[q][t], xb, C::XBYTES, p0, lane);
                if constexpr (NT == 3) tr_issue_at(Al[q][t], xb + C::PLANE_BYTES, C::XBYTES, p0, lane);
            }
        };
        load(0, 0);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const int q = s4 & 1;
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            tr_tie(Bh[q]);
            if constexpr (NT == 3) tr_tie(Bl[q]);
#pragma unroll
            for (int t = 0; t < C::NTAP; ++t) {
                tr_tie(Ah[q][t]);
                if constexpr (NT == 3) tr_tie(Al[q][t]);
            }
            if (s4 + 1 < 4) load(s4 + 1, q ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            const half8 bh = tr_value(Bh[q]);
            half8 bl;
            if constexpr (NT == 3) bl = tr_value(Bl[q]);
            if (do_bias) {
                accb = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, bh, accb, 0, 0, 0);
                if constexpr (NT == 3) accb = __builtin_amdgcn_mfma_f32_32x32x16_f16(ones, bl, accb, 0, 0, 0);
            }
#pragma unroll
            for (int t = 0; t < C::NTAP; ++t) {
                const half8 ah = tr_value(Ah[q][t]);
                if constexpr (NT == 3) {
                    const half8 al = tr_value(Al[q][t]);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
                }
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }

    // ---- reduce the 4 waves through LDS, one partial per block ----------------------------------
    float* red = reinterpret_cast<float*>(smem);          // [4 waves][32 m][32 n]
    const int n = lane & 31, hi = lane >> 5;
    const long long blk = ((long long)bz * a.ncp + cp) * a.PB + pb;
#pragma unroll
    for (int t = 0; t < C::NTAP; ++t) reduce_waves_to_partial<4>(red, acc[t], wave, lane, a.partial + (blk * C::NTAP + t) * 1024);
    if (do_bias) {
        __syncthreads();
        // bias: every row m of accb holds sum_k gY[k][n]; keep row 0 (e = 0 of the lanes with hi == 0)
        if (hi == 0) red[wave * 32 + n] = accb[0];
        __syncthreads();
        if (tid < 32)
            a.partial_b[((long long)cot * a.PB + pb) * 32 + tid] = pairwise<4, 32>(red + tid);
    }
}


// 3x3 layers: eight waves, X-ROW form (the tile is 8 X rows and the halo sits on the operand that needs no column shifts;
// against a wave per gY row: -40 % LDS fragment reads for the same MFMAs, profiles/r03_experiments.md):
//     dW[dy][dx] = sum_r sum_x X[r][x + dx - 1] * gY[r - dy + 1][x]
// wave w owns X row r0 + w: three column-shifted X fragments per K-step, each used against the THREE gY rows r - dy + 1
// (a 10-row gY patch, rows r0 - 1 .. r0 + 8, zero outside the image): 6 X + 6 gY = 12 fragments for the same 27 MFMAs
// (-40 % LDS reads), identical for every wave, and the X halo rows are no longer fetched twice (X 8 x 34, gY 10 x 32 pixels per
// tile and pair: the same 75 KB).  Every (X row, dy) product is counted in exactly one tile because the X rows are
// partitioned; rows outside the image arrive as zeros from the DMA range check.  Step s = (ks, dy, dx): the reads of step
// s + 2 are issued while step s multiplies, counted lgkmcnt as above; X fragments live in one buffer per dx (A[1][dx] is
// fetched two steps after the last use of A[0][dx]), gY fragments alternate between two.
template <int NT>
struct Wg3xCfg {
    static constexpr int THREADS = 512;
    static constexpr int NPL = (NT == 3) ? 2 : 1;
    static constexpr int XR = 8, GR = 10, PW = 34;
    static constexpr int XP = (XR * PW * 2 + 63) / 64;                   // 1-KiB DMA pieces of an X chunk patch (9)
    static constexpr int GP = GR;                                        // one piece = one 32-pixel gY row
    static constexpr int XS = XP * 1024 + 128, GS = GP * 1024 + 128;     // chunk strides (+128 B: the pair's chunks on other banks)
    static constexpr int G0 = 2 * XS;
    static constexpr int PLANE = 2 * XS + 2 * GS;
    static constexpr int STAGE = NPL * PLANE;
    static constexpr int LDS_BYTES = 2 * STAGE;
    static constexpr int NXJ = (XP + 7) / 8, NGJ = (GP + 7) / 8;
    static_assert(PLANE + 512 + 2 * 1024 + 128 < 65536, "lo plane / K-step / gY row reachable with the 16-bit DS offset");
    static_assert(LDS_BYTES <= 160 * 1024 && LDS_BYTES >= 8 * 4096, "LDS budget; the final reduction needs 32 KB");
};

// DMA of one tile, in two halves so that the caller can spread the instructions over the multiply steps of the tile before
// (see the kernel): wg3x_offsets() = the per-lane buffer offsets of the tile (VALU only), wg3x_issue_part(PL, H) = the
// buffer_load ... lds instructions of plane PL, chunk H of the pair (X pieces, then gY pieces).
template <int NT>
struct Wg3xLanes {                       // tile-invariant dma_lane() of the wave's X and gY pieces (wave, wave + 8)
    DmaLane x[Wg3xCfg<NT>::NXJ], g[Wg3xCfg<NT>::NGJ];
};
template <int NT>
struct Wg3xTile {
    unsigned xvo[Wg3xCfg<NT>::NXJ], gvo[Wg3xCfg<NT>::NGJ];
};
template <int NT>
__device__ __forceinline__ void wg3x_offsets(const WgradKArgs& a, int tile, const Wg3xLanes<NT>& l, Wg3xTile<NT>& o) {
    using G = Wg3xCfg<NT>;
    const TileOrigin t = tile_origin(a, tile, G::XR);
    const int xbase = pixel_byte(a, t.img, t.ty0, t.tx0 - 1), gbase = pixel_byte(a, t.img, t.ty0 - 1, t.tx0);
#pragma unroll
    for (int j = 0; j < G::NXJ; ++j) o.xvo[j] = dma_offset(l.x[j], xbase, t.ty0, t.tx0 - 1, a.H, a.W);
#pragma unroll
    for (int j = 0; j < G::NGJ; ++j) o.gvo[j] = dma_offset(l.g[j], gbase, t.ty0 - 1, t.tx0, a.H, a.W);
}
template <int NT>
__device__ __forceinline__ void wg3x_issue_part(const WgradKArgs& a, char* stage, const int PL, const int HH, int cp, int cot,
                                                int wave, const Wg3xTile<NT>& o, long long plane_elems, unsigned plane_bytes) {
    using G = Wg3xCfg<NT>;
    const __amdgpu_buffer_rsrc_t rs = x_chunk_rsrc(a, PL, 2 * cp + HH, plane_elems, plane_bytes);
    char* lds = stage + PL * G::PLANE + HH * G::XS;
#pragma unroll
    for (int j = 0; j < G::NXJ; ++j)
        if (wave + 8 * j < G::XP)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(lds + (wave + 8 * j) * 1024), 16, o.xvo[j], 0, 0, 0);
    const __amdgpu_buffer_rsrc_t gs = g_chunk_rsrc(a, PL, 2 * cot + HH, plane_elems, plane_bytes);
    char* ldg = stage + PL * G::PLANE + G::G0 + HH * G::GS;
#pragma unroll
    for (int j = 0; j < G::NGJ; ++j)
        if (wave + 8 * j < G::GP)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(gs, (lds_void_t*)(ldg + (wave + 8 * j) * 1024), 16, o.gvo[j], 0, 0, 0);
}
template <int NT>
__device__ __forceinline__ void wg3x_issue_all(const WgradKArgs& a, char* stage, int cp, int cot, int wave,
                                               const Wg3xTile<NT>& o, long long plane_elems, unsigned plane_bytes) {
    wg3x_issue_part<NT>(a, stage, 0, 0, cp, cot, wave, o, plane_elems, plane_bytes);
    wg3x_issue_part<NT>(a, stage, 0, 1, cp, cot, wave, o, plane_elems, plane_bytes);
    if constexpr (NT == 3) {
        wg3x_issue_part<NT>(a, stage, 1, 0, cp, cot, wave, o, plane_elems, plane_bytes);
        wg3x_issue_part<NT>(a, stage, 1, 1, cp, cot, wave, o, plane_elems, plane_bytes);
    }
}

constexpr int WG3_DMA_FIRST = 1, WG3_DMA_STRIDE = 4;
template <int NT>
__global__ void __launch_bounds__(Wg3xCfg<NT>::THREADS)
wgrad3x3_xrow_kernel(const WgradKArgs a) {
    using G = Wg3xCfg<NT>;
    constexpr int NTAP = 9, NSTEP = 2 * NTAP;
    constexpr int NA = (NT == 3) ? 4 : 2;                                // read instructions of one fragment (pair x planes)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // = X row of the 8-row tile
    int pb, cp, bz;
    wg_block(a, pb, cp, bz);
    const int cot = bz % a.ncot;
    const int W = a.W;
    const long long plane_elems = (long long)a.N * a.H * W * 16;
    const unsigned plane_bytes = (unsigned)(plane_elems * 2);
    const bool do_bias = (cp == 0);

    floatx16 acc[NTAP];
    float bsum = 0.f;
#pragma unroll
    for (int t = 0; t < NTAP; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;

    // ---- tile-invariant per-lane state: the two 4-pixel reads of the X fragment of column shift dx (K-step 0, hi plane)
    unsigned xa[3], xb2[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        xa[dx] = tr_addr(G::XS, wave * G::PW + dx, lane);
        xb2[dx] = tr_addr(G::XS, wave * G::PW + dx + 4, lane);
    }
    // gY patch row `wave` (= image row r - 2); tap dy multiplies patch row wave + 2 - dy (an immediate)
    const unsigned g_off = (unsigned)G::G0 + tr_addr(G::GS, wave * 32, lane);
    Wg3xLanes<NT> dl;
#pragma unroll
    for (int j = 0; j < G::NXJ; ++j) dl.x[j] = dma_lane(wave + 8 * j, lane, G::PW, G::XR * G::PW, W);
#pragma unroll
    for (int j = 0; j < G::NGJ; ++j) dl.g[j] = dma_lane(wave + 8 * j, lane, 32, G::GP * 32, W);

    // row-major tiles at stride PB (a walk down 32-pixel columns saved HBM bytes and no time, profiles/r03_experiments.md)
    int tile = pb;
    const int tend = a.ntiles, tstep = a.PB;
    Wg3xTile<NT> to;
    if (tile < tend) {
        wg3x_offsets<NT>(a, tile, dl, to);
        wg3x_issue_all<NT>(a, smem, cp, cot, wave, to, plane_elems, plane_bytes);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int cur = 0;
    for (; tile < tend; tile += tstep) {
        const int nxt = tile + tstep;
        // The next tile's DMA is NOT issued in one burst here: a wave executes in order, and a burst of buffer_load ... lds
        // sits at the head of its instruction stream until the memory pipeline has accepted all of it, with nobody else on the
        // CU to multiply meanwhile.  One (plane, chunk) group goes out behind the MFMAs of steps 1, 5, 9 and 13 instead
        // (WG3_DMA_FIRST + k * WG3_DMA_STRIDE; a later step leaves its round trip less cover): 128-134 vs 136-138 us at 96
        // channels, profiles/r03_experiments.md.
        const bool pre = nxt < tend;
        if (pre) wg3x_offsets<NT>(a, nxt, dl, to);
        char* const stage_nxt = smem + (cur ^ 1) * G::STAGE;
        const unsigned st = lds_addr(smem + cur * G::STAGE);
        TrFrag Bh[2], Bl[2], Ah[3], Al[3];
        auto load = [&](auto SC) {
            constexpr int s = decltype(SC)::value, ks = s / NTAP, dy = (s % NTAP) / 3, dx = s % 3;
            if constexpr (dx == 0) {
                constexpr int bb = (ks * 3 + dy) & 1, off = ks * 512 + (2 - dy) * 1024;
                tr_issue<off>(Bh[bb], st + g_off, st + g_off + 128);
                if constexpr (NT == 3) tr_issue<off + G::PLANE>(Bl[bb], st + g_off, st + g_off + 128);
            }
            if constexpr (dy == 0) {
                tr_issue<ks * 512>(Ah[dx], st + xa[dx], st + xb2[dx]);
                if constexpr (NT == 3) tr_issue<ks * 512 + G::PLANE>(Al[dx], st + xa[dx], st + xb2[dx]);
            }
        };
        load(std::integral_constant<int, 0>{});
        load(std::integral_constant<int, 1>{});
        static_for([&](auto SC) {
            constexpr int s = decltype(SC)::value, ks = s / NTAP, dy = (s % NTAP) / 3, dx = s % 3, t = dy * 3 + dx;
            constexpr int bb = (ks * 3 + dy) & 1;
            // outstanding: the reads of steps s and s + 1, in issue order -> leave step s + 1's in flight
            constexpr int s1 = s + 1;
            constexpr int later = (s1 < NSTEP) ? NA * ((s1 % 3 == 0 ? 1 : 0) + ((s1 % NTAP) / 3 == 0 ? 1 : 0)) : 0;
            asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(later) : "memory");
            if constexpr (dy == 0) {
                tr_tie(Ah[dx]);
                if constexpr (NT == 3) tr_tie(Al[dx]);
            }
            if constexpr (dx == 0) {
                tr_tie(Bh[bb]);
                if constexpr (NT == 3) tr_tie(Bl[bb]);
            }
            if constexpr (s + 2 < NSTEP) load(std::integral_constant<int, s + 2>{});
            __builtin_amdgcn_sched_barrier(0);
            const half8 bh = tr_value(Bh[bb]);
            half8 bl;
            if constexpr (NT == 3) bl = tr_value(Bl[bb]);
            if (dy == 1 && dx == 0 && do_bias) {           // patch row wave + 1 = the wave's own image row: once per gY row
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    bsum += (float)bh[e];
                    if constexpr (NT == 3) bsum += (float)bl[e];
                }
            }
            const half8 ah = tr_value(Ah[dx]);
            if constexpr (NT == 3) {
                const half8 al = tr_value(Al[dx]);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc[t], 0, 0, 0);
            }
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc[t], 0, 0, 0);
            if constexpr (s >= WG3_DMA_FIRST && (s - WG3_DMA_FIRST) % WG3_DMA_STRIDE == 0 &&
                          (s - WG3_DMA_FIRST) / WG3_DMA_STRIDE < (NT == 3 ? 4 : 2)) {
                constexpr int grp = (s - WG3_DMA_FIRST) / WG3_DMA_STRIDE;           // (plane, chunk) = (0,0) (0,1) (1,0) (1,1)
                if (pre) wg3x_issue_part<NT>(a, stage_nxt, grp / 2, grp % 2, cp, cot, wave, to, plane_elems, plane_bytes);
            }
            __builtin_amdgcn_sched_barrier(0);
        }, std::make_integer_sequence<int, NSTEP>{});
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cur ^= 1;
    }

    // ---- the eight rows are summed through LDS in a fixed order: one partial per workgroup and tap
    float* red = reinterpret_cast<float*>(smem);          // [8 waves][32 m][32 n]
    const long long blk = ((long long)bz * a.ncp + cp) * a.PB + pb;
#pragma unroll
    for (int t = 0; t < NTAP; ++t) reduce_waves_to_partial<8>(red, acc[t], wave, lane, a.partial + (blk * NTAP + t) * 1024);
    if (do_bias) {
        __syncthreads();
        red[tid] = bsum;                              // [wave][kg][co]
        __syncthreads();
        if (tid < 32) {
            float tsum = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) tsum += red[k * 32 + tid];
            a.partial_b[((long long)cot * a.PB + pb) * 32 + tid] = tsum;
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------
// 1x1 convolutions (LFF 224->96, GFF.0 1152->96).  A 1x1 weight gradient does 2*Cin*Cout flops per pixel for
// (Cin + Cout) * 2 B of operands per plane: 77 flop/B in f16x3 — four times below the machine balance, so this is a
// STREAMING kernel and its design goal is bytes: every X and gY plane byte crosses HBM once per channel-pair group and
// enough of them are in flight per CU to cover the HBM latency.
//   * One workgroup (8 waves, one per CU: the LDS is all staging buffer) walks strips of TR x 32 pixels; a stage holds the
//     strip of ALL its operands — 6 gY chunks and `ppg` input-channel pairs, hi and lo planes — and is double buffered
//     (LFF, f16x3: 2 x 80 KB, so ~80 KB per CU are always in flight).
//   * Wave w owns input-channel pair(s) w*PPW .. of the group and all three 32-wide output tiles: its 3*PPW accumulator tiles
//     see every pixel of the strip, so there is no K-split across waves, no end-of-kernel cross-wave reduction, and the
//     accumulators are 48*PPW registers instead of the 192 a "one wave = one pixel row of all tiles" split needs (the round-1
//     kernel: 1 wave per SIMD, a barrier per 16 KB, gY read once per group of FOUR pairs — 1.09 GB for 0.84 GB of
//     operands on LFF at 40 x 128 x 128 — and 2.8 TB/s).
//   * ncp > 8 (GFF.0: 36 pairs): PPW = 2 and ceil(ncp / 16) balanced groups (3 x 12), gY re-read once per group.
// The last wave of group 0 also accumulates the bias gradient from the gY fragments it loads anyway.
constexpr int W1_NW = 8, W1_NCOT = 3;
struct W1Cfg {
    static constexpr int THREADS = 64 * W1_NW;
    static constexpr int LDS_BYTES = 160 * 1024;         // the opt-in limit; a launch asks for W1Plan::lds of it
};

struct W1Plan { int ppw, tr, cgroups, ppg; unsigned lds; };
static inline W1Plan w1_plan(int ncp) {
    W1Plan p;
    p.ppw = ncp <= W1_NW ? 1 : 2;
    const int cap = W1_NW * p.ppw;
    p.cgroups = (ncp + cap - 1) / cap;
    p.ppg = (ncp + p.cgroups - 1) / p.cgroups;
    const int slots = 2 * (2 * W1_NCOT + 2 * p.ppg);     // sized for two planes (f16x3); f16 uses half of it
    p.tr = (p.ppw == 1 && 2 * slots * 2 * 1024 <= 160 * 1024) ? 2 : 1;
    p.lds = 2u * slots * p.tr * 1024;
    return p;
}

template <int NT, int PPW, int TR>
__global__ void __launch_bounds__(W1Cfg::THREADS)
wgrad1x1_kernel(const WgradKArgs a) {
    constexpr int NPL = (NT == 3) ? 2 : 1;
    constexpr int CH = TR * 1024;                         // one chunk strip: TR rows x 32 px x 32 B
    constexpr int GSLOTS = NPL * 2 * W1_NCOT;
    constexpr int PAIR_BYTES = NPL * 2 * CH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pb = blockIdx.x;
    const int cpg = blockIdx.y;
    const int ppg = a.ppg;
    const int cp0 = cpg * ppg;
    const long long plane_elems = (long long)a.N * a.H * a.W * 16;
    const unsigned plane_bytes = (unsigned)(plane_elems * 2);
    const int nslots = GSLOTS + ppg * NPL * 2;
    const int stage_bytes = nslots * CH;
    const bool bias_wave = (cpg == 0) && (wave == W1_NW - 1);

    bool valid[PPW];
#pragma unroll
    for (int i = 0; i < PPW; ++i) valid[i] = (wave * PPW + i < ppg) && (cp0 + wave * PPW + i < a.ncp);

    floatx16 acc[PPW][W1_NCOT];
    float bsum[W1_NCOT] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < PPW; ++i)
#pragma unroll
        for (int j = 0; j < W1_NCOT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const DmaLane dl = dma_lane(0, lane, 32, 32, a.W);     // a DMA piece = one 32-pixel row of one chunk
    const unsigned tr_off = tr_addr(CH, 0, lane);

    auto issue = [&](int tile, int buf) {
        const TileOrigin o = tile_origin(a, tile, TR);
        char* stage = smem + buf * stage_bytes;
        for (int k = wave; k < nslots * TR; k += W1_NW) {
            const int slot = k / TR, r = k % TR;
            __amdgpu_buffer_rsrc_t rs;
            if (slot < GSLOTS) {
                rs = g_chunk_rsrc(a, slot / (2 * W1_NCOT), slot % (2 * W1_NCOT), plane_elems, plane_bytes);
            } else {
                const int xs = slot - GSLOTS;
                const int pr = xs / (NPL * 2), rem = xs % (NPL * 2);
                rs = x_chunk_rsrc(a, rem >> 1, 2 * (cp0 + pr) + (rem & 1), plane_elems, plane_bytes);
            }
            const unsigned vo = dma_offset(dl, pixel_byte(a, o.img, o.ty0 + r, o.tx0), o.ty0 + r, o.tx0, a.H, a.W);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, (lds_void_t*)(stage + slot * CH + r * 1024), 16, vo, 0, 0, 0);
        }
    };

    int tile = pb;
    int buf = 0;
    if (tile < a.ntiles) issue(tile, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (; tile < a.ntiles; tile += a.PB) {
        if (tile + a.PB < a.ntiles) issue(tile + a.PB, buf ^ 1);
        const unsigned gst = lds_addr(smem + buf * stage_bytes) + tr_off;
        const unsigned xst = gst + GSLOTS * CH + wave * PPW * PAIR_BYTES;
        // fragments of pixel step ks + 1 are in flight while step ks multiplies
        TrFrag Bh[2][W1_NCOT], Bl[2][W1_NCOT], Ah[2][PPW], Al[2][PPW];
        auto load = [&](int ks, int q) {
#pragma unroll
            for (int j = 0; j < W1_NCOT; ++j) {
                tr_issue(Bh[q][j], gst + 2 * j * CH + ks * 512);
                if constexpr (NT == 3) tr_issue(Bl[q][j], gst + (2 * W1_NCOT + 2 * j) * CH + ks * 512);
            }
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                tr_issue(Ah[q][i], xst + i * PAIR_BYTES + ks * 512);
                if constexpr (NT == 3) tr_issue(Al[q][i], xst + i * PAIR_BYTES + 2 * CH + ks * 512);
            }
        };
        load(0, 0);
#pragma unroll
        for (int ks = 0; ks < 2 * TR; ++ks) {
            const int q = ks & 1;
            // everything outstanding belongs to step ks; tie its registers to the wait so no use moves above it
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
            for (int j = 0; j < W1_NCOT; ++j) {
                tr_tie(Bh[q][j]);
                if constexpr (NT == 3) tr_tie(Bl[q][j]);
            }
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                tr_tie(Ah[q][i]);
                if constexpr (NT == 3) tr_tie(Al[q][i]);
            }
            if (ks + 1 < 2 * TR) load(ks + 1, q ^ 1);
            __builtin_amdgcn_sched_barrier(0);
            half8 bh[W1_NCOT], bl[W1_NCOT];
#pragma unroll
            for (int j = 0; j < W1_NCOT; ++j) {
                bh[j] = tr_value(Bh[q][j]);
                if constexpr (NT == 3) bl[j] = tr_value(Bl[q][j]);
            }
            if (bias_wave) {
#pragma unroll
                for (int j = 0; j < W1_NCOT; ++j)
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        bsum[j] += (float)bh[j][e];
                        if constexpr (NT == 3) bsum[j] += (float)bl[j][e];
                    }
            }
#pragma unroll
            for (int i = 0; i < PPW; ++i) {
                if (!valid[i]) continue;
                const half8 ah = tr_value(Ah[q][i]);
                half8 al;
                if constexpr (NT == 3) al = tr_value(Al[q][i]);
#pragma unroll
                for (int j = 0; j < W1_NCOT; ++j) {
                    if constexpr (NT == 3) {
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh[j], acc[i][j], 0, 0, 0);
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl[j], acc[i][j], 0, 0, 0);
                    }
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh[j], acc[i][j], 0, 0, 0);
                }
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        buf ^= 1;
    }

    // ---- every accumulator tile is complete in its wave: straight to the partial buffer (layout of the generic kernel,
    // ntap = 1, z = co tile; 32 lanes = 32 consecutive floats)
    const int n = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int i = 0; i < PPW; ++i) {
        if (!valid[i]) continue;
        const int cp = cp0 + wave * PPW + i;
#pragma unroll
        for (int j = 0; j < W1_NCOT; ++j) {
            if (j >= a.ncot) continue;
            float* dst = a.partial + (((long long)j * a.ncp + cp) * a.PB + pb) * 1024 + n;
#pragma unroll
            for (int e = 0; e < 16; ++e) dst[acc_row(e, hi) * 32] = acc[i][j][e];
        }
    }
    if (bias_wave) {
        // a gY fragment lane holds 8 pixels of output channel lane & 31; lanes l and l + 32 hold the two pixel halves
#pragma unroll
        for (int j = 0; j < W1_NCOT; ++j) {
            const float t = bsum[j] + __shfl_xor(bsum[j], 32);
            if (lane < 32 && j < a.ncot) a.partial_b[((long long)j * a.PB + pb) * 32 + lane] = t;
        }
    }
}

// final deterministic reduction over the PB partials + un-scale + scatter to OIHW, for a BATCH of layers in one launch
// (the backward plan reduces the five layers of a dense block together: 1 122 -> 306 reduce launches per training step).
// One 256-thread block per (z, cp, tap, m) row of 32 outputs of a layer: thread (nn, ps) sums every 8th partial
// (coalesced 128-B reads), the 8 slices are combined through LDS in a fixed order.  Rows >= nrows of a layer handle
// its bias (one per co tile).  Summation order per output is independent of the batching.
struct ReduceBatch {
    BhWgradReduce it[BH_WGRAD_BATCH];
    long long row_start[BH_WGRAD_BATCH + 1];
    int n;
};

__global__ void __launch_bounds__(256)
wgrad_reduce_kernel(const ReduceBatch rb, const float* __restrict__ inv_scale, int accumulate) {
    __shared__ float sm[8][32];
    long long row = blockIdx.x;
    int li = 0;
#pragma unroll
    for (int i = 1; i < BH_WGRAD_BATCH; ++i)
        if (i < rb.n && row >= rb.row_start[i]) li = i;
    const BhWgradReduce& L = rb.it[li];
    row -= rb.row_start[li];
    const float* __restrict__ partial = L.partial;
    const float* __restrict__ partial_b = L.partial_b;
    const int PB = L.PB, ncp = L.ncp, ncot = L.ncot, ks = L.ks, tr = L.tr, cout = L.cout, cin = L.cin;
    const long long nrows = L.nrows;
    const int ntap_blk = tr * ks;
    const int nn = threadIdx.x & 31, ps = threadIdx.x >> 5;
    const float is = inv_scale ? inv_scale[0] : 1.f;
    float s = 0.f;
    int co, ci = 0, dy = 0, dx = 0;
    bool is_bias = row >= nrows;
    if (!is_bias) {
        const int m = (int)(row & 31);
        long long u = row >> 5;
        const int tap = (int)(u % ntap_blk); u /= ntap_blk;
        const int cp = (int)(u % ncp); u /= ncp;
        const int z = (int)u;                       // = dyg * ncot + cot
        const int cot = z % ncot, dyg = z / ncot;
        co = cot * 32 + nn; ci = cp * 32 + m;
        dy = dyg * tr + tap / ks; dx = tap % ks;
        const long long base = (((long long)z * ncp + cp) * PB) * ntap_blk + tap;
        for (int p = ps; p < PB; p += 8) s += partial[(base + (long long)p * ntap_blk) * 1024 + m * 32 + nn];
    } else {
        const int cot = (int)(row - nrows);
        co = cot * 32 + nn;
        for (int p = ps; p < PB; p += 8) s += partial_b[((long long)cot * PB + p) * 32 + nn];
    }
    sm[ps][nn] = s;
    __syncthreads();
    if (ps != 0) return;
    const float tot = ((sm[0][nn] + sm[1][nn]) + (sm[2][nn] + sm[3][nn])) + ((sm[4][nn] + sm[5][nn]) + (sm[6][nn] + sm[7][nn]));
    if (co >= cout) return;
    int cr = co;
    if (L.shuffle) { const int cq = cout / 4; cr = (co % cq) * 4 + co / cq; }
    if (is_bias) {
        if (L.db) L.db[cr] = accumulate ? L.db[cr] + tot * is : tot * is;
        return;
    }
    if (ci >= cin) return;
    float* o = L.dw + (((long long)cr * cin + ci) * ks + dy) * ks + dx;
    *o = accumulate ? *o + tot * is : tot * is;
}

namespace {

struct WgGeom { int ncp, ncot, ndyg, tr, ntap, tiles_x, tiles_y, ntiles, PB; size_t partial_floats, bias_floats; };

bool use_w1(int ksize, int cout) { return ksize == 1 && cout <= 32 * W1_NCOT; }

WgGeom wg_geom(int ksize, int N, int H, int W, int cin_chunks, int cout, int cus) {
    WgGeom g;
    const bool w1 = use_w1(ksize, cout);
    g.tr = (ksize == 5) ? 1 : ksize;                    // tap rows per workgroup: the 5x5 splits its rows over ndyg workgroups
    g.ndyg = ksize / g.tr;
    g.ntap = g.tr * ksize;
    g.ncp = (cin_chunks + 1) / 2;
    g.ncot = (cout + 31) / 32;
    const W1Plan wp = w1_plan(g.ncp);
    const int th = w1 ? wp.tr : 8;                      // tile rows
    g.tiles_x = (W + 31) / 32;
    g.tiles_y = (H + th - 1) / th;
    g.ntiles = g.tiles_x * g.tiles_y * N;
    // One workgroup per CU in every kernel (3x3: two LDS stages of eight waves; streaming 1x1: the LDS is all staging buffer), so
    // the pixel blocks are the CUs over the workgroups that walk the same tiles: the streaming kernel's columns, else every
    // (cp, cot, dyg).  Floor: no straggler in an extra round.
    const int blocks = g.ncp * g.ncot * g.ndyg;         // partial tiles (x ntap) per pixel block
    int pb = (cus > 0 ? cus : 256) / (w1 ? wp.cgroups : blocks);
    if (pb < 1) pb = 1;
    if (pb > g.ntiles) pb = g.ntiles;
    if (!w1 && pb >= 8) pb &= ~7;                       // wg_block(): siblings of a pixel block share an XCD
    g.PB = pb;
    g.partial_floats = (size_t)blocks * pb * g.ntap * 1024;
    g.bias_floats = (size_t)g.ncot * pb * 32;
    return g;
}

size_t wg_workspace_bytes(const WgGeom& g) { return (g.partial_floats + g.bias_floats) * sizeof(float) + 256; }

// the shape checks binhip_wgrad_workspace_bytes() and bh_wgrad_partials() share; wg_geom() divides by the tap rows
int check_shape(int ksize, int N, int H, int W, int cin_chunks, int cout) {
    if (ksize != 1 && ksize != 3 && ksize != 5) return BINHIP_E_SHAPE;
    if (N <= 0 || H <= 0 || W <= 0 || cin_chunks <= 0 || cout <= 0) return BINHIP_E_SHAPE;
    return 0;
}

// one launch of a main kernel: block size and opt-in LDS limit from its config struct, `lds` bytes of it asked for
template <class Cfg, void (*KERNEL)(WgradKArgs)>
int launch(const WgradKArgs& a, dim3 grid, hipStream_t s, unsigned lds = Cfg::LDS_BYTES) {
    static std::atomic<unsigned long long> lds_set{0};
    if (int rc = bh_set_max_lds(KERNEL, Cfg::LDS_BYTES, lds_set)) return rc;
    KERNEL<<<grid, dim3(Cfg::THREADS), lds, s>>>(a);
    BH_CHECK_LAUNCH();
    return 0;
}
template <int KS, int NT>
int launch_generic(const WgradKArgs& a, dim3 grid, hipStream_t s) {
    return launch<WgCfg<KS, 1, NT>, wgrad_mfma_kernel<KS, 1, NT>>(a, grid, s);
}
template <int NT>
int launch_w1(const WgradKArgs& a, const WgGeom& g, const W1Plan& wp, hipStream_t s) {
    const dim3 grid((unsigned)g.PB, (unsigned)wp.cgroups);
    const unsigned want = (NT == 3) ? wp.lds : wp.lds / 2, lds = want < 16384 ? 16384 : want;
    return wp.ppw == 2 ? launch<W1Cfg, wgrad1x1_kernel<NT, 2, 1>>(a, grid, s, lds)
         : wp.tr == 2  ? launch<W1Cfg, wgrad1x1_kernel<NT, 1, 2>>(a, grid, s, lds)
                       : launch<W1Cfg, wgrad1x1_kernel<NT, 1, 1>>(a, grid, s, lds);
}

// CU count of the current device (sizes the pixel-block split); looked up per call — no cached global
int cus() {
    const int n = binhip_device_cus();
    return n > 0 ? n : 256;
}

}  // namespace

extern "C" {

size_t binhip_wgrad_workspace_bytes(int ksize, int N, int H, int W, int cin_chunks, int cout) {
    if (check_shape(ksize, N, H, W, cin_chunks, cout)) return 0;
    return wg_workspace_bytes(wg_geom(ksize, N, H, W, cin_chunks, cout, cus()));
}

}  // extern "C"

// main kernel of one layer's weight gradient: writes the per-block partials into `workspace` and fills `out` for the
// (batched) reduction
int bh_wgrad_partials(const BinConvDesc* d, const void* x_hi, const void* x_lo, const void* gy_hi, const void* gy_lo,
                      void* workspace, size_t workspace_bytes, float* dw_oihw, float* dbias, int cin, int shuffle_perm,
                      BhWgradReduce* out, void* stream) {
    if (!d || !x_hi || !gy_hi || !workspace || !dw_oihw) return BINHIP_E_ARG;
    if (d->nterms != 1 && d->nterms != 3) return BINHIP_E_ARG;
    if (d->nterms == 3 && (!x_lo || !gy_lo)) return BINHIP_E_ARG;
    if (int rc = check_shape(d->ksize, d->N, d->H, d->W, d->cin_chunks, d->cout)) return rc;
    if ((long long)d->N * d->H * d->W >= (1ll << 26)) return BINHIP_E_SHAPE;
    if (cin <= 0 || cin > d->cin_chunks * 16) return BINHIP_E_SHAPE;
    if (shuffle_perm && d->cout % 4) return BINHIP_E_SHAPE;
    if (d->x_cpg > 0 && d->x_group_stride < 0) return BINHIP_E_SHAPE;      // groups step forward from x (x_cpg <= 0: one group)
    const WgGeom g = wg_geom(d->ksize, d->N, d->H, d->W, d->cin_chunks, d->cout, cus());
    if (workspace_bytes < wg_workspace_bytes(g)) return BINHIP_E_WORKSPACE;
    float* part = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    WgradKArgs a;
    a.x_hi = (const _Float16*)x_hi; a.x_lo = (const _Float16*)x_lo;
    a.g_hi = (const _Float16*)gy_hi; a.g_lo = (const _Float16*)gy_lo;
    a.partial = part; a.partial_b = part + g.partial_floats;
    a.x_group_stride = d->x_group_stride; a.x_cpg = d->x_cpg;
    a.N = d->N; a.H = d->H; a.W = d->W;
    a.cin_chunks = d->cin_chunks; a.cout_chunks = (d->cout + 15) / 16;
    a.tiles_x = g.tiles_x; a.tiles_y = g.tiles_y; a.ntiles = g.ntiles;
    a.PB = g.PB; a.ncp = g.ncp; a.ncot = g.ncot; a.nz = g.ncot * g.ndyg;
    hipStream_t s = (hipStream_t)stream;
    const bool x3 = d->nterms == 3;
    const dim3 grid((unsigned)(g.PB * g.ncp * g.ncot * g.ndyg));        // generic / 3x3: wg_block() unpacks the id
    const W1Plan wp = w1_plan(g.ncp);
    a.ppg = use_w1(d->ksize, d->cout) ? wp.ppg : 0;
    int rc;
    if (use_w1(d->ksize, d->cout)) {
        rc = x3 ? launch_w1<3>(a, g, wp, s) : launch_w1<1>(a, g, wp, s);
    } else if (d->ksize == 3) {                     // eight waves, two LDS stages, one workgroup per CU; wave = X row
        rc = x3 ? launch<Wg3xCfg<3>, wgrad3x3_xrow_kernel<3>>(a, grid, s) : launch<Wg3xCfg<1>, wgrad3x3_xrow_kernel<1>>(a, grid, s);
    } else if (d->ksize == 1) {                     // 1x1 with more than 96 outputs (not on the bin_stage4 path)
        rc = x3 ? launch_generic<1, 3>(a, grid, s) : launch_generic<1, 1>(a, grid, s);
    } else {                                        // 5x5 (SFENet1)
        rc = x3 ? launch_generic<5, 3>(a, grid, s) : launch_generic<5, 1>(a, grid, s);
    }
    if (rc) return rc;
    out->partial = a.partial; out->partial_b = a.partial_b;
    out->PB = g.PB; out->ncp = g.ncp; out->ncot = g.ncot; out->ks = d->ksize; out->tr = g.tr;
    out->cout = d->cout; out->cin = cin; out->shuffle = shuffle_perm;
    out->dw = dw_oihw; out->db = dbias;
    out->nrows = (long long)g.ndyg * g.ncot * g.ncp * g.ntap * 32;
    return 0;
}

int bh_wgrad_reduce_batch(const BhWgradReduce* items, int n, const float* inv_scale, int accumulate, void* stream) {
    if (n <= 0) return 0;
    if (n > BH_WGRAD_BATCH) return BINHIP_E_ARG;
    ReduceBatch rb;
    long long rows = 0;
    for (int i = 0; i < n; ++i) {
        rb.it[i] = items[i];
        rb.row_start[i] = rows;
        rows += items[i].nrows + items[i].ncot;
    }
    for (int i = n; i <= BH_WGRAD_BATCH; ++i) rb.row_start[i] = rows;
    for (int i = n; i < BH_WGRAD_BATCH; ++i) rb.it[i] = items[0];
    rb.n = n;
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, rb, inv_scale, accumulate);
    BH_CHECK_LAUNCH();
    return 0;
}

extern "C" {

int binhip_conv2d_bwd_weight(const BinConvDesc* d, const void* x_hi, const void* x_lo, const void* gy_hi,
                             const void* gy_lo, const float* inv_scale, void* workspace, size_t workspace_bytes,
                             float* dw_oihw, float* dbias, int cin, int shuffle_perm, int accumulate, void* stream) {
    BhWgradReduce r;
    if (int rc = bh_wgrad_partials(d, x_hi, x_lo, gy_hi, gy_lo, workspace, workspace_bytes, dw_oihw, dbias, cin,
                                   shuffle_perm, &r, stream)) return rc;
    return bh_wgrad_reduce_batch(&r, 1, inv_scale, accumulate, stream);
}

}  // extern "C"
