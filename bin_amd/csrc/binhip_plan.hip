// binhip_plan.hip — one whole RDN sub-network (reference RDN.py:210-222 / 268-280 / 322-334) as a
// fixed sequence of kernel launches (bin_stage4: the input packer + 66 layers) issued from C on the caller's stream: no Python,
// no allocation, no host sync between layers (so the sequence is hipGraph-capturable).  Host code only; its launch trace is
// pinned without a GPU by tests/test_cpu_plan_trace.py.
//
// Workspace (chunk planes, fp16; each tensor = hi planes followed by lo planes when nterms == 3):
//   X0   [kc0]      pixel-unshuffled input frames, half resolution (h = H/2, w = W/2)
//   F1   [6]        SFENet1 output (f__1)
//   BLK  [13][14]   dense-block buffers: BLK[d][0:6] = input of RDB d (= output of RDB d-1),
//                   BLK[d][6+2c : 8+2c] = output of conv c of RDB d  -> "cat" is free
//   G0,G1 [6]       GFF.0 / GFF.1(+f__1)
//   U    [4]        UPNet.0 output after PixelShuffle, full resolution
// (numbers for bin_stage4's shape G0 = 96, D = 12, C = 4, G = 32; in general c0 = G0/16 planes per feature map, cg = G/16
//  per conv output, BLK [D + 1][c0 + C cg], layer index 2 + d (C + 1) + c — include/binhip.h, BinRdnShape)
//
// How the code below names things:
//   Planes   a tensor of a workspace as ONE value (offset of the hi planes, distance to the lo planes); sub() steps chunks into it
//   Bind     a base pointer (forward workspace, saved state, gradient workspace): hi(t) / lo(t) of a Planes, null for "no tensor"
//   Conv, Wgrad, Dgrad   one layer call with named fields whose defaults are the common case (3x3, half resolution, no
//            residual / mask / grouping): a call site names only what is unusual about its layer
#include "binhip_conv_common.h"

namespace {

// resolved network shape (BinRdnShape with the defaults filled in)
struct Shp {
    int G0, D, C, G;
    int c0, cg, cb;       // planes per feature map / per conv output / per dense-block buffer
    int L;                // layers
    bool stage4;          // bin_stage4's shape: the fused tail / three-phase kernels exist for it
};
bool resolve_shape(const BinRdnShape* s, Shp* o) {
    Shp h;
    const bool dflt = !s || (s->G0 == 0 && s->D == 0 && s->C == 0 && s->G == 0);
    h.G0 = dflt ? 96 : s->G0; h.D = dflt ? 12 : s->D; h.C = dflt ? 4 : s->C; h.G = dflt ? 32 : s->G;
    if (h.G0 < 32 || h.G0 > 256 || h.G0 % 32 || h.G < 32 || h.G > 128 || h.G % 32) return false;
    if (h.C < 1 || h.C > BINHIP_RDN_MAX_CONVS || h.D < 1 || h.D > 20) return false;
    h.c0 = h.G0 / 16; h.cg = h.G / 16; h.cb = h.c0 + h.C * h.cg;
    h.L = 2 + h.D * (h.C + 1) + 4;
    if (h.L > BINHIP_RDN_MAX_LAYERS) return false;
    h.stage4 = (h.G0 == 96 && h.C == 4 && h.G == 32);
    *o = h;
    return true;
}
inline int layer_conv(const Shp& sh, int d, int c) { return 2 + d * (sh.C + 1) + c; }      // c == C: the block's LFF

// the frame arguments every entry point takes: N, H, W positive, H and W even, 2 / 3 / 5 input frames
bool frames_ok(int N, int H, int W, int n_inputs) {
    // (N H W < 2^26: the limit of the full-resolution convolutions, checked here so that a frame they would refuse in the middle of
    //  the launch sequence is refused before the first launch, and by the workspace queries)
    return N > 0 && H > 0 && W > 0 && !(H & 1) && !(W & 1) && (n_inputs == 2 || n_inputs == 3 || n_inputs == 5) &&
           (long long)N * H * W < (1ll << 26);
}

// A tensor of a workspace, in fp16 elements from the 256-byte aligned base: hi planes at `off`, lo planes (nterms == 3) at
// `off + size`.  The default value is "no tensor" (no residual, no mask, no plane output).
struct Planes {
    int64_t off = -1, size = 0;
    bool present() const { return off >= 0; }
    Planes sub(int64_t elems) const { return {off + elems, size}; }      // `elems` (chunks x plane) further in, same lo distance
};
// the tensors behind one base pointer (rounded up to 256 B here)
struct Bind {
    _Float16* base;
    bool has_lo;                             // nterms == 3
    Bind(const void* p, bool lo) : base((_Float16*)(((uintptr_t)p + 255) & ~(uintptr_t)255)), has_lo(lo) {}
    void* hi(Planes t) const { return t.present() ? base + t.off : nullptr; }
    void* lo(Planes t) const { return t.present() && has_lo ? base + t.off + t.size : nullptr; }
};
// lays tensors out one behind the other; mul = 2: every tensor is followed by its lo planes
struct Carve {
    int64_t next; int mul;
    Planes take(int64_t size) { const Planes t{next, size}; next += mul * size; return t; }
};

struct Ws {
    int64_t P, PF;        // plane elems at half / full res
    int kc0;              // chunks of the packed input
    Planes x0, f1, blk, g0, g1, u;
    int64_t sync, total;  // element offset of the dense-block sync words (32 reserved + 2 flags per tile, uint32); all of it
    int tiles;            // 16x32 tiles of one dense-block conv launch
};

Ws make_ws(int N, int H, int W, int nin, int nt, const Shp& sh) {
    Ws w;
    const int h = H / 2, ww = W / 2;
    w.P = (int64_t)N * h * ww * 16; w.PF = (int64_t)N * H * W * 16;
    w.kc0 = (12 * nin + 15) / 16;
    Carve o{0, nt == 3 ? 2 : 1};
    w.x0 = o.take(w.kc0 * w.P); w.f1 = o.take(sh.c0 * w.P);
    w.blk = o.take((int64_t)(sh.D + 1) * sh.cb * w.P);
    w.g0 = o.take(sh.c0 * w.P); w.g1 = o.take(sh.c0 * w.P);
    w.u = o.take(4 * w.PF);
    // sync words of the one-launch dense blocks (binhip_conv_x3.hip): 32 reserved words + two flag words per tile; 4-byte words
    // kept in the fp16-element address space (2 elements each), 256-B aligned
    w.tiles = N * ((h + 15) / 16) * ((ww + 31) / 32);
    w.sync = (o.next + 127) & ~(int64_t)127;
    w.total = w.sync + 2 * (32 + 2 * (int64_t)w.tiles);
    return w;
}

// one forward layer
struct Conv {
    int layer, ks = 3, cin_chunks, cout, cout_pad = 0;      // cout_pad 0: = cout
    int epi = BINHIP_EPI_PLANES, relu = 0, H = 0, W = 0;    // H, W 0: the half-resolution grid
    Planes x;
    int x_cpg = 0;                                          // input chunk grouping (BinConvDesc)
    int64_t x_group_stride = 0;
    Planes y, res;                                          // (the FINAL epilogues write `out` instead)
    int reserved = 0;                                       // BINHIP_CONV_* bits of the call (BinConvDesc.reserved)
};

}  // namespace

extern "C" {

size_t binhip_rdn_workspace_bytes(int N, int H, int W, int n_inputs, int nterms, const BinRdnShape* shape) {
    Shp sh;
    if (!frames_ok(N, H, W, n_inputs) || !resolve_shape(shape, &sh)) return 0;
    return (size_t)make_ws(N, H, W, n_inputs, nterms, sh).total * 2 + 256;
}

int binhip_rdn_workspace_layout(int N, int H, int W, int n_inputs, int nterms, const BinRdnShape* shape, int64_t* out, int n_out) {
    if (!out || n_out < BINHIP_RDN_LAYOUT_WORDS) return BINHIP_E_ARG;
    Shp sh;
    if (!frames_ok(N, H, W, n_inputs) || !resolve_shape(shape, &sh)) return BINHIP_E_SHAPE;
    const Ws w = make_ws(N, H, W, n_inputs, nterms, sh);
    const Planes t[6] = {w.x0, w.f1, w.blk, w.g0, w.g1, w.u};
    out[0] = w.P; out[1] = w.PF; out[2] = w.kc0; out[15] = nterms == 3 ? 1 : 0;
    for (int i = 0; i < 6; ++i) { out[3 + 2 * i] = t[i].off; out[4 + 2 * i] = t[i].size; }
    return 0;
}

int binhip_rdn_forward(const BinRdnPlan* p, const float* const* inputs, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p || !inputs || !out || !workspace) return BINHIP_E_ARG;
    const int N = p->N, H = p->H, W = p->W, nin = p->n_inputs, nt = p->nterms;
    if (!frames_ok(N, H, W, nin)) return BINHIP_E_SHAPE;
    if (nt != 1 && nt != 3) return BINHIP_E_ARG;
    if (p->reserved & ~(BINHIP_PLAN_KEEP_ACTS | BINHIP_PLAN_NO_FUSE | BINHIP_PLAN_RDB3 | BINHIP_PLAN_FUSED_UPNET | BINHIP_PLAN_FUSED_UPNET_TRAIN |
                        BINHIP_PLAN_UPNET_FOLD | BINHIP_PLAN_HOLD_WEIGHTS)) return BINHIP_E_ARG;      // an undefined flag bit
    if ((p->reserved & BINHIP_PLAN_UPNET_FOLD) && (nt != 3 || (p->reserved & BINHIP_PLAN_KEEP_ACTS) || !(p->reserved & BINHIP_PLAN_FUSED_UPNET)))
        return BINHIP_E_ARG;              // the folded slab exists for the fused UPNet of fp32-class inference only
    // held weight fragments: the per-conv launches of fp32-class inference (the three-phase launch has the reloading form only)
    const bool hold = (p->reserved & BINHIP_PLAN_HOLD_WEIGHTS) != 0;
    if (hold && (nt != 3 || (p->reserved & (BINHIP_PLAN_KEEP_ACTS | BINHIP_PLAN_RDB3)))) return BINHIP_E_ARG;
    Shp sh;
    if (!resolve_shape(&p->shape, &sh)) return BINHIP_E_SHAPE;
    const size_t need = binhip_rdn_workspace_bytes(N, H, W, nin, nt, &p->shape);
    if (workspace_bytes < need) return BINHIP_E_WORKSPACE;
    for (int i = 0; i < nin; ++i) if (!inputs[i]) return BINHIP_E_ARG;
    for (int i = 0; i < sh.L; ++i) if (!p->w_hi[i] || !p->bias[i] || (nt == 3 && !p->w_lo[i])) return BINHIP_E_ARG;

    hipStream_t s = (hipStream_t)stream;
    const Ws w = make_ws(N, H, W, nin, nt, sh);
    const int h = H / 2, ww = W / 2;
    const Bind A(workspace, nt == 3);

    int rc = binhip_pack_inputs(inputs, nin, N, H, W, A.hi(w.x0), A.lo(w.x0), p->status, stream);
    if (rc) return rc;

    auto mk = [&](const Conv& l) -> BhConvCall {
        BhConvCall c;
        c.d.N = N; c.d.H = l.H ? l.H : h; c.d.W = l.W ? l.W : ww; c.d.ksize = l.ks; c.d.cin_chunks = l.cin_chunks; c.d.cout = l.cout;
        c.d.cout_pad = l.cout_pad ? l.cout_pad : l.cout; c.d.nterms = nt; c.d.epilogue = l.epi; c.d.relu = l.relu;
        c.d.x_cpg = l.x_cpg; c.d.x_group_stride = l.x_group_stride; c.d.status = p->status; c.d.reserved = l.reserved;
        // a 1x1 convolution is pointwise: any reshape of the pixel grid computes the same values.  [H][W] -> [H * W / 32][32] makes a
        // workgroup's TH x 32 tile TH KiB of CONTIGUOUS bytes per plane instead of TH runs of 1 KiB at a row pitch of W * 32 B:
        // 720p window -0.3 %; the same reshape in the backward plan did not pay (profiles/r06_experiments.md)
        if (l.ks == 1 && l.epi == BINHIP_EPI_PLANES && c.d.W > 32 && c.d.W % 32 == 0) { c.d.H *= c.d.W / 32; c.d.W = 32; }
        // SFENet1 on 2 / 3 input frames: 24 / 36 channels = the last chunk's upper half is zero padding (packer and relayout)
        if (l.layer == 0 && l.ks == 5 && (12 * nin) % 16 >= 1 && (12 * nin) % 16 <= 8) c.d.reserved = BINHIP_CONV_HALF_LAST_CHUNK;
        if (hold && l.ks == 3 && l.epi == BINHIP_EPI_PLANES) c.d.reserved |= BINHIP_CONV_HOLD_WEIGHTS;
        c.x_hi = A.hi(l.x); c.x_lo = A.lo(l.x);
        c.w_hi = p->w_hi[l.layer]; c.w_lo = p->w_lo[l.layer]; c.bias = p->bias[l.layer];
        c.r_hi = A.hi(l.res); c.r_lo = A.lo(l.res);
        c.y_hi = A.hi(l.y); c.y_lo = A.lo(l.y);
        c.status = p->status; c.prof = p->profiler;
        if (l.epi == BINHIP_EPI_FINAL || l.epi == BINHIP_EPI_FINAL_SUBPIX) {
            c.y_f32 = out; c.d.n_images = nin;
            for (int i = 0; i < nin; ++i) c.images[i] = inputs[i];
        }
        return c;
    };
    auto conv = [&](const Conv& l) -> int { return bh_launch_conv(mk(l), s); };
    // one-launch dense blocks (BINHIP_PLAN_RDB3, opt-in, fp32-class path): one memset per call zeroes the per-tile flags (block d
    // publishes d + 1, so the blocks of one call never confuse each other's flags; the memset only removes what an earlier call left)
    const bool rdb3 = (p->reserved & BINHIP_PLAN_RDB3) && nt == 3 && sh.stage4;
    unsigned* sync_words = (unsigned*)(A.base + w.sync);
    const int cus = binhip_device_cus();
    if (rdb3) {
        hipError_t me = hipMemsetAsync(sync_words, 0, (size_t)(32 + 2 * (size_t)w.tiles) * 4, s);
        if (me != hipSuccess) return (int)me;
    }
    const int64_t P = w.P;
    const int G0 = sh.G0, G = sh.G, C = sh.C, D = sh.D, c0 = sh.c0, cg = sh.cg, cb = sh.cb;
    // SFENet1 5x5 (RDN.py:187/245/299) and SFENet2 3x3 (:188)
    if ((rc = conv({.layer = 0, .ks = 5, .cin_chunks = w.kc0, .cout = G0, .x = w.x0, .y = w.f1}))) return rc;
    if ((rc = conv({.layer = 1, .cin_chunks = c0, .cout = G0, .x = w.f1, .y = w.blk}))) return rc;
    // D residual dense blocks (RDN.py:149-165)
    for (int d = 0; d < D; ++d) {
        const Planes b = w.blk.sub((int64_t)d * cb * P), b_next = b.sub(cb * P);     // this block's buffer; its output = the next one's input
        auto dense = [&](int c) -> Conv {            // conv c reads the concat so far and appends its G channels
            return {.layer = layer_conv(sh, d, c), .cin_chunks = c0 + cg * c, .cout = G, .relu = 1, .x = b, .y = b.sub((c0 + cg * c) * P)};
        };
        const bool fuse = sh.stage4 && !(p->reserved & BINHIP_PLAN_NO_FUSE);
        bool done3 = false;
        if (rdb3 && fuse) {
            // convs 0-2 as three phases of one launch (static tile ownership + neighbour flags instead of two kernel boundaries)
            ConvKArgs ka[3];
            bool ok3 = true;
            for (int c = 0; c < 3 && ok3; ++c) {
                if ((rc = bh_prepare_conv(mk(dense(c)), &ka[c]))) return rc;
                ok3 = ok3 && ka[c].wt;
            }
            if (ok3) {
                rc = bh_launch_rdb3_x3(ka, sync_words + 32, (unsigned)(d + 1), cus, s);
                if (rc == 0) done3 = true;
                else if (rc != BINHIP_E_SHAPE) return rc;          // E_SHAPE: not co-resident on this device -> per-conv launches
            }
        }
        for (int c = 0; c < (fuse ? C - 1 : C) && !done3; ++c) if ((rc = conv(dense(c)))) return rc;
        if (fuse) {
            // conv #3 + LFF + residual in one kernel (binhip_fused.hip); o3 is only written out for training
            const int L3 = layer_conv(sh, d, 3), LF = layer_conv(sh, d, 4);
            if ((rc = binhip_rdb_tail_fwd(N, h, ww, nt, A.hi(b), A.lo(b), p->w_hi[L3], p->w_lo[L3], p->bias[L3], p->w_hi[LF], p->w_lo[LF], p->bias[LF],
                                          A.hi(b_next), A.lo(b_next),
                                          ((p->reserved & BINHIP_PLAN_KEEP_ACTS) ? BINHIP_TAIL_STORE_O3 : 0) | (hold ? BINHIP_TAIL_HOLD_WEIGHTS : 0),
                                          p->status, stream)))
                return rc;
        } else if ((rc = conv({.layer = layer_conv(sh, d, C), .ks = 1, .cin_chunks = cb, .cout = G0, .x = b, .y = b_next, .res = b})))
            return rc;
    }
    const int LG = sh.L - 4;
    // GFF.0 1x1 over cat(RDBs_out) (RDN.py:199, 218): D groups of c0 chunks, one per dense block
    if ((rc = conv({.layer = LG, .ks = 1, .cin_chunks = D * c0, .cout = G0, .x = w.blk.sub(cb * P), .x_cpg = c0, .x_group_stride = cb * P, .y = w.g0})))
        return rc;
    // GFF.1 3x3, x += f__1 (RDN.py:200, 219)
    if ((rc = conv({.layer = LG + 1, .cin_chunks = c0, .cout = G0, .x = w.g0, .y = w.g1, .res = w.f1}))) return rc;
    // UPNet as ONE 5x5 convolution G0 -> 12 sub-pixel channels (BINHIP_PLAN_FUSED_UPNET, include/binhip.h): inference, and a training
    // forward (KEEP_ACTS) that also sets BINHIP_PLAN_FUSED_UPNET_TRAIN (backward: BINHIP_BWD_FUSED_UPNET); KEEP_ACTS alone keeps the two layers
    const bool fused_up = (p->reserved & BINHIP_PLAN_FUSED_UPNET) &&
                          (!(p->reserved & BINHIP_PLAN_KEEP_ACTS) || (p->reserved & BINHIP_PLAN_FUSED_UPNET_TRAIN)) &&
                          sh.L + 1 < BINHIP_RDN_MAX_LAYERS && p->w_hi[sh.L] && (nt == 1 || p->w_lo[sh.L]) && p->bias[sh.L] &&
                          p->w_hi[sh.L + 1] && p->bias[sh.L + 1];
    // BINHIP_PLAN_UPNET_FOLD: slot L holds the folded slab, the main launch walks it (fp32-class inference only)
    const bool fold = (p->reserved & BINHIP_PLAN_UPNET_FOLD) != 0;
    if (fused_up) {
        if ((rc = conv({.layer = sh.L, .ks = 5, .cin_chunks = c0, .cout = 12, .cout_pad = 32, .epi = BINHIP_EPI_FINAL_SUBPIX, .x = w.g1,
                        .reserved = fold ? BINHIP_CONV_UPNET_FOLD : 0})))
            return rc;
        // ... and the one-pixel full-resolution border ring from its own operators (UPNet.2 pads the intermediate, not the input)
        return bh_launch_upnet_ring(A.hi(w.g1), A.lo(w.g1), (const float*)p->w_hi[sh.L + 1], p->bias[sh.L + 1], out, inputs, nin, N, h, ww,
                                    G0, s);
    }
    // UPNet.0 3x3 G0->256 + PixelShuffle(2) (RDN.py:205-206)
    if ((rc = conv({.layer = LG + 2, .cin_chunks = c0, .cout = 256, .epi = BINHIP_EPI_SHUFFLE, .x = w.g1, .y = w.u}))) return rc;
    // UPNet.2 3x3 64->3 + mean(inputs) (RDN.py:207, 221/279/333), at full resolution
    return conv({.layer = LG + 3, .cin_chunks = 4, .cout = 3, .cout_pad = 32, .epi = BINHIP_EPI_FINAL, .H = H, .W = W, .x = w.u});
}

}  // extern "C"

// ====================================================================================================
// Backward of one RDN sub-network (autograd of RDN.py:210-222 / 268-280 / 322-334), again as one fixed launch
// sequence from C.  Gradient activations are chunk planes like the forward ones, stored multiplied by a per-call
// power-of-two scale (fp16 range); weight gradients come out as fp32 OIHW.
//   gOut [1 @HxW] <- gout*scale        gU [4 @HxW]     gUu [16]  (un-shuffled)      gG1, gG0, gF1 [6]
//   GY [13][6]: GY[0] = grad of SFENet2's output, GY[d+1] = grad of RDB d's output (GFF.0 dgrad + chained RDBs)
//   gcat [14]: gradient of the current dense block's concat buffer        gX0 [<=4]
namespace {

struct Bws {
    int64_t P, PF;
    int kc0, gx0_chunks;
    Planes gout, gu, guu, gg1, gg0, gf1, gy, gcat, gcat2, gx0;
    size_t wg_bytes, sc_off_bytes, wg_off_bytes, total_bytes;
};

Bws make_bws(int N, int H, int W, int nin, int nt, const Shp& sh) {
    Bws b;
    const int h = H / 2, w = W / 2;
    b.P = (int64_t)N * h * w * 16; b.PF = (int64_t)N * H * W * 16;
    b.kc0 = (12 * nin + 15) / 16; b.gx0_chunks = ((12 * nin + 31) / 32) * 2;
    Carve o{0, nt == 3 ? 2 : 1};
    b.gout = o.take(b.PF);
    b.gu = o.take(4 * b.PF);        // (no longer written: UPNet.2's backward-data stores through the inverse PixelShuffle; the layout is ABI)
    b.guu = o.take(16 * b.P);
    b.gg1 = o.take(sh.c0 * b.P); b.gg0 = o.take(sh.c0 * b.P); b.gf1 = o.take(sh.c0 * b.P);
    b.gy = o.take((int64_t)(sh.D + 1) * sh.c0 * b.P); b.gcat = o.take((int64_t)sh.cb * b.P);
    // dense blocks alternate between two: block d's weight gradients (side stream) still read one while block d-1's backward-data fills the other
    b.gcat2 = o.take((int64_t)sh.cb * b.P); b.gx0 = o.take((int64_t)b.gx0_chunks * b.P);
    // weight-gradient partial workspace: max over the layer shapes
    size_t wg = 0;
    auto mx = [&](size_t v) { if (v > wg) wg = v; };
    mx(binhip_wgrad_workspace_bytes(3, N, H, W, 4, 3));                       // UPNet.2
    mx(binhip_wgrad_workspace_bytes(3, N, h, w, sh.c0, 256));                 // UPNet.0
    mx(binhip_wgrad_workspace_bytes(3, N, h, w, sh.c0, sh.G0));               // GFF.1 / SFENet2
    mx(binhip_wgrad_workspace_bytes(1, N, h, w, sh.D * sh.c0, sh.G0));        // GFF.0
    mx(binhip_wgrad_workspace_bytes(1, N, h, w, sh.cb, sh.G0));               // LFF
    for (int c = 0; c < sh.C; ++c) mx(binhip_wgrad_workspace_bytes(3, N, h, w, sh.c0 + sh.cg * c, sh.G));
    mx(binhip_wgrad_workspace_bytes(5, N, h, w, b.kc0, sh.G0));               // SFENet1
    b.wg_bytes = wg;
    size_t bytes = ((size_t)o.next * 2 + 255) & ~(size_t)255;
    b.sc_off_bytes = bytes; bytes += 8192;                       // scale[2] + 1024 amax partials (+pad)
    b.wg_off_bytes = bytes; bytes += (size_t)(sh.C + 1) * wg;    // one partial region per layer of a dense block (batched reduce)
    b.total_bytes = bytes + 256;
    return b;
}

// weight gradient of one forward layer: x = its saved input, gy = the gradient of its output
struct Wgrad {
    int layer, ks = 3, H = 0, W = 0;         // H, W 0: the half-resolution grid
    int cin_chunks, cin, cout;
    Planes x;
    int x_cpg = 0;                           // the forward layer's input chunk grouping
    int64_t x_group_stride = 0;
    Planes gy;
    int shuffle = 0;                         // gy's channels are in UPNet.0's PixelShuffle-permuted order
    int slot = -1;                           // < 0: reduce at once; 0..C: keep the partials in that region for the block's one reduce
};
// data gradient through one forward layer, a convolution of gy with the transposed / flipped weights:
// y = [mask](conv(gy) [+ res on chunks < res_chunks] [+ y])
struct Dgrad {
    int layer, ks = 3, H = 0, W = 0;         // H, W 0: the half-resolution grid
    int gy_chunks, cout;                     // chunks of gy read; output channels (the forward layer's inputs)
    Planes gy, y, res;
    int res_chunks = 0;                      // 0: the residual applies to every chunk
    bool acc_inplace = false;                // y += (it already holds another path's share)
    Planes mask;                             // SAVED activation: ReLU backward on the output chunks >= mask_from
    int mask_from = 0, y_cpg = 0;            // y_cpg / y_group_stride: output chunk grouping (GFF.0 scatters to the blocks' gradients)
    int64_t y_group_stride = 0;
    int y_unshuf = 0;                        // > 0: store through the inverse PixelShuffle, chunks per sub-position
};

}  // namespace

extern "C" {

size_t binhip_rdn_backward_workspace_bytes(int N, int H, int W, int n_inputs, int nterms, const BinRdnShape* shape) {
    Shp sh;
    if (!frames_ok(N, H, W, n_inputs) || !resolve_shape(shape, &sh)) return 0;
    return make_bws(N, H, W, n_inputs, nterms, sh).total_bytes;
}

int binhip_rdn_backward_workspace_layout(int N, int H, int W, int n_inputs, int nterms, const BinRdnShape* shape, int64_t* out, int n_out) {
    if (!out || n_out < BINHIP_RDN_BWD_LAYOUT_WORDS) return BINHIP_E_ARG;
    Shp sh;
    if (!frames_ok(N, H, W, n_inputs) || !resolve_shape(shape, &sh)) return BINHIP_E_SHAPE;
    const Bws b = make_bws(N, H, W, n_inputs, nterms, sh);
    const Planes t[10] = {b.gout, b.gu, b.guu, b.gg1, b.gg0, b.gf1, b.gy, b.gcat, b.gcat2, b.gx0};
    out[0] = b.P; out[1] = b.PF; out[2] = b.gx0_chunks; out[23] = (int64_t)b.sc_off_bytes;
    for (int i = 0; i < 10; ++i) { out[3 + 2 * i] = t[i].off; out[4 + 2 * i] = t[i].size; }
    return 0;
}

int binhip_rdn_backward(const BinRdnBwdPlan* p, const void* saved, size_t saved_bytes, const float* gout, void* workspace,
                        size_t workspace_bytes, void* stream) {
    if (!p || !saved || !gout || !workspace || !p->zero_bias) return BINHIP_E_ARG;
    const int N = p->N, H = p->H, W = p->W, nin = p->n_inputs, nt = p->nterms;
    if (!frames_ok(N, H, W, nin)) return BINHIP_E_SHAPE;
    if (nt != 1 && nt != 3) return BINHIP_E_ARG;
    // BINHIP_BWD_SAVED_X3: the forward ran in the hi/lo (nterms = 3) layout but this backward computes single-product
    // (nterms = 1): it reads the HI planes of the saved activations (an fp16 rounding of them; the ReLU masks are the
    // sign of hi, which is the sign of hi + lo) at the offsets of the 3-term layout
    const int nt_saved = (p->reserved & BINHIP_BWD_SAVED_X3) ? 3 : nt;
    if (nt == 3 && (p->reserved & BINHIP_BWD_SAVED_X3)) return BINHIP_E_ARG;
    if (p->reserved & ~(BINHIP_BWD_ACCUMULATE | BINHIP_BWD_SAVED_X3 | BINHIP_BWD_FUSED_UPNET)) return BINHIP_E_ARG;   // an undefined flag bit
    Shp sh;
    if (!resolve_shape(&p->shape, &sh)) return BINHIP_E_SHAPE;
    if (saved_bytes < binhip_rdn_workspace_bytes(N, H, W, nin, nt_saved, &p->shape)) return BINHIP_E_WORKSPACE;
    const Bws b = make_bws(N, H, W, nin, nt, sh);
    if (workspace_bytes < b.total_bytes) return BINHIP_E_WORKSPACE;
    for (int i = 0; i < sh.L; ++i) if (!p->wt_hi[i] || (nt == 3 && !p->wt_lo[i]) || !p->dw[i] || !p->db[i]) return BINHIP_E_ARG;
    // BINHIP_BWD_FUSED_UPNET: slots L and L + 1 (checked with the rest, before the first launch)
    if ((p->reserved & BINHIP_BWD_FUSED_UPNET) &&
        (sh.L + 1 >= BINHIP_RDN_MAX_LAYERS || !p->wt_hi[sh.L] || (nt == 3 && !p->wt_lo[sh.L]) || !p->wt_hi[sh.L + 1] || !p->dw[sh.L] ||
         !p->db[sh.L] || !p->dw[sh.L + 1] || !p->db[sh.L + 1])) return BINHIP_E_ARG;
    const int G0 = sh.G0, G = sh.G, C = sh.C, D = sh.D, c0 = sh.c0, cg = sh.cg, cb = sh.cb, LG = sh.L - 4;

    hipStream_t s = (hipStream_t)stream;
    // Optional second stream (plan->aux_stream): the weight-gradient kernels of a layer depend only on that layer's
    // output gradient and the saved activations, not on the backward-data chain that continues behind it, so they run
    // on the side stream and overlap the chain (both kernel families are latency-bound at training sizes and fit a CU
    // together).  Ordering is by events created, recorded, waited on and destroyed inside this call (no state is kept):
    //   fork  — side stream waits for everything the main stream has queued so far (the gradient a wgrad reads);
    //   b_done[d] — main stream waits, before it overwrites a gradient-concat buffer, for the side-stream weight
    //   gradients of the block that read it two blocks earlier; the main stream joins the side stream before returning.
    hipStream_t sb = p->aux_stream ? (hipStream_t)p->aux_stream : s;
    const bool two = (sb != s);
    auto order = [&](hipStream_t from, hipStream_t to) -> int {      // `to` waits for `from`'s queue up to here
        if (!two) return 0;
        hipEvent_t e;
        hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
        if (r != hipSuccess) return (int)r;
        r = hipEventRecord(e, from);
        if (r == hipSuccess) r = hipStreamWaitEvent(to, e, 0);
        (void)hipEventDestroy(e);                                    // released once the recorded work completes
        return r == hipSuccess ? 0 : (int)r;
    };
    const Ws w = make_ws(N, H, W, nin, nt_saved, sh);
    const int h = H / 2, ww = W / 2;
    const int64_t P = w.P;
    const Bind S(saved, nt == 3);            // saved forward state (BINHIP_BWD_SAVED_X3: its hi planes only)
    const Bind Gw(workspace, nt == 3);       // gradient planes
    char* wbytes = (char*)Gw.base;
    float* sc = (float*)(wbytes + b.sc_off_bytes);
    float* amax_part = sc + 16;
    void* wgws = wbytes + b.wg_off_bytes;
    const float* inv = sc + 1;

    const int accumulate = (p->reserved & BINHIP_BWD_ACCUMULATE) ? 1 : 0;   // dw/db += instead of =
    int rc;
    if ((rc = binhip_grad_scale(gout, (int64_t)N * 3 * H * W, 16.f, amax_part, sc, stream))) return rc;
    // BINHIP_BWD_FUSED_UPNET: the forward ran UPNet as one 5x5 convolution on 12 sub-pixel channels (+ the border ring)
    const bool fused_up = (p->reserved & BINHIP_BWD_FUSED_UPNET) != 0;
    // gsub: the pixel-unshuffled, scaled gradient with the ring zeroed — ONE half-resolution chunk where gout would be, lo one plane further
    const Planes gsub = {b.gout.off, P};
    if (fused_up) {
        if ((rc = bh_upnet_gsub(gout, N, h, ww, sc, Gw.hi(gsub), Gw.lo(gsub), p->status, s))) return rc;
    } else if ((rc = binhip_nchw_to_planes_scaled(gout, N, 3, H, W, sc, Gw.hi(b.gout), Gw.lo(b.gout), p->status, stream))) return rc;

    // weight gradients run on the side stream; a slot's reduction is queued for flush_reduces() (one launch per dense block)
    BhWgradReduce pending[BH_WGRAD_BATCH];
    int npending = 0;
    auto wgrad = [&](const Wgrad& g) -> int {
        BinConvDesc d = {};
        d.N = N; d.H = g.H ? g.H : h; d.W = g.W ? g.W : ww; d.ksize = g.ks; d.cin_chunks = g.cin_chunks; d.cout = g.cout;
        d.nterms = nt; d.x_cpg = g.x_cpg; d.x_group_stride = g.x_group_stride; d.status = p->status;
        if (int rf = order(s, sb)) return rf;                        // its gY (and the scale) are queued on the main stream
        BhWgradReduce r;
        char* region = (char*)wgws + (size_t)(g.slot < 0 ? 0 : g.slot) * b.wg_bytes;
        const bool timed = bh_prof_begin(p->profiler, g.ks, g.cout, BINHIP_PROF_WGRAD, sb);
        const int rw = bh_wgrad_partials(&d, S.hi(g.x), S.lo(g.x), Gw.hi(g.gy), Gw.lo(g.gy), region, b.wg_bytes, p->dw[g.layer],
                                         p->db[g.layer], g.cin, g.shuffle, &r, (void*)sb);
        if (timed) bh_prof_end(p->profiler, sb);
        if (rw) return rw;
        if (g.slot < 0) return bh_wgrad_reduce_batch(&r, 1, inv, g.layer >= sh.L ? 0 : accumulate, (void*)sb);   // (fused UPNet: written)
        pending[npending++] = r;
        return 0;
    };
    auto flush_reduces = [&]() -> int {
        const int rr = bh_wgrad_reduce_batch(pending, npending, inv, accumulate, (void*)sb);
        npending = 0;
        return rr;
    };
    auto dgrad = [&](const Dgrad& g) -> int {
        BhConvCall c;
        c.d.N = N; c.d.H = g.H ? g.H : h; c.d.W = g.W ? g.W : ww; c.d.ksize = g.ks; c.d.cin_chunks = g.gy_chunks; c.d.cout = g.cout;
        c.d.cout_pad = binhip_dgrad_rows_pad(g.ks, g.cout); c.d.nterms = nt; c.d.epilogue = BINHIP_EPI_PLANES; c.d.status = p->status;
        c.x_hi = Gw.hi(g.gy); c.x_lo = Gw.lo(g.gy);
        c.w_hi = p->wt_hi[g.layer]; c.w_lo = p->wt_lo[g.layer]; c.bias = p->zero_bias;
        c.r_hi = Gw.hi(g.res); c.r_lo = Gw.lo(g.res); c.res_chunks = g.res_chunks;
        c.y_hi = Gw.hi(g.y); c.y_lo = Gw.lo(g.y);
        if (g.acc_inplace) { c.r2_hi = c.y_hi; c.r2_lo = c.y_lo; }
        c.m_hi = S.hi(g.mask); c.mask_from = g.mask_from;
        c.y_cpg = g.y_cpg; c.y_group_stride = g.y_group_stride; c.y_unshuf = g.y_unshuf;
        c.status = p->status;
        return bh_launch_conv(c, s);
    };

    // Everything below may have work in flight on the side stream: every exit — error or not — goes through ONE epilogue
    // that destroys the pending per-block events and joins the side stream into the main stream (the caller reuses
    // `workspace` / frees `saved` in main-stream order, also after a failed call).
    hipEvent_t b_done[20] = {};
    auto chain = [&]() -> int {
        if (fused_up) {
            // ---- the fused UPNet (G0 -> 12 sub-pixel channels, 5x5): X = G1, gY = gsub; then the ring's share of both gradients
            if ((rc = wgrad({.layer = sh.L, .ks = 5, .cin_chunks = c0, .cin = G0, .cout = 12, .x = w.g1, .gy = gsub}))) return rc;
            if ((rc = order(s, sb))) return rc;
            if ((rc = bh_upnet_ring_wgrad(gout, S.hi(w.g1), S.lo(w.g1), p->dw[sh.L + 1], p->db[sh.L + 1], N, h, ww, G0, 0, sb))) return rc;
            if ((rc = dgrad({.layer = sh.L, .ks = 5, .gy_chunks = 1, .cout = G0, .gy = gsub, .y = b.gg1}))) return rc;
            if ((rc = bh_upnet_ring_dgrad(gout, (const float*)p->wt_hi[sh.L + 1], sc, Gw.hi(b.gg1), Gw.lo(b.gg1), p->status, N, h, ww, G0, s))) return rc;
        } else {
            // ---- UPNet.2 (64 -> 3 at full res): X = U
            if ((rc = wgrad({.layer = LG + 3, .H = H, .W = W, .cin_chunks = 4, .cin = 64, .cout = 3, .x = w.u, .gy = b.gout}))) return rc;
            // its backward-data writes straight through the inverse PixelShuffle (y_unshuf; before, a 64-channel
            // full-resolution gradient went to b.gu and a separate layout pass — 856 MB per launch at N = 40 — turned it
            // into the 256 half-resolution channels UPNet.0's backward reads)
            if ((rc = dgrad({.layer = LG + 3, .H = H, .W = W, .gy_chunks = 1, .cout = 64, .gy = b.gout, .y = b.guu, .y_unshuf = 4}))) return rc;
            // ---- UPNet.0 (G0 -> 256): X = G1
            if ((rc = wgrad({.layer = LG + 2, .cin_chunks = c0, .cin = G0, .cout = 256, .x = w.g1, .gy = b.guu, .shuffle = 1}))) return rc;
            if ((rc = dgrad({.layer = LG + 2, .gy_chunks = 16, .cout = G0, .gy = b.guu, .y = b.gg1}))) return rc;
        }
        // ---- GFF.1 (+ f__1 skip): X = G0
        if ((rc = wgrad({.layer = LG + 1, .cin_chunks = c0, .cin = G0, .cout = G0, .x = w.g0, .gy = b.gg1}))) return rc;
        if ((rc = dgrad({.layer = LG + 1, .gy_chunks = c0, .cout = G0, .gy = b.gg1, .y = b.gg0}))) return rc;
        // ---- GFF.0 over cat(RDB outputs): X = BLK[1..D][0:c0]; gradient scattered to GY[1..D]
        if ((rc = wgrad({.layer = LG, .ks = 1, .cin_chunks = D * c0, .cin = D * G0, .cout = G0, .x = w.blk.sub(cb * P), .x_cpg = c0,
                         .x_group_stride = cb * P, .gy = b.gg0}))) return rc;
        if ((rc = dgrad({.layer = LG, .ks = 1, .gy_chunks = c0, .cout = D * G0, .gy = b.gg0, .y = b.gy.sub(c0 * P), .y_cpg = c0,
                         .y_group_stride = c0 * P}))) return rc;
        // ---- the D residual dense blocks, last to first
        for (int d = D - 1; d >= 0; --d) {
            const Planes blk = w.blk.sub((int64_t)d * cb * P);        // saved forward buffer of RDB d
            const Planes gy = b.gy.sub((int64_t)(d + 1) * c0 * P);    // grad of RDB d's output
            const Planes gcat = (d & 1) ? b.gcat2 : b.gcat;           // this block's gradient-concat buffer
            const int L = layer_conv(sh, d, 0);
            // LFF 1x1 (G0 + C G) -> G0 (+x): gcat = W'^T gy (+ gy on the first c0 chunks); ReLU mask of the last conv's output
            if ((rc = wgrad({.layer = L + C, .ks = 1, .cin_chunks = cb, .cin = G0 + C * G, .cout = G0, .x = blk, .gy = gy, .slot = C}))) return rc;
            // Block d+2 used this gcat buffer: its weight gradients (side stream) must have read it before it is refilled.
            // A full join of the side stream here would also wait for block d+1's weight gradients, which read the OTHER
            // buffer, and over-serialise; the side stream is in order, so "block d+2 done" = an event recorded there right
            // after block d+2's last wgrad.
            if (two && d + 2 <= D - 1 && b_done[d + 2]) {
                hipError_t r = hipStreamWaitEvent(s, b_done[d + 2], 0);
                (void)hipEventDestroy(b_done[d + 2]);
                b_done[d + 2] = nullptr;
                if (r != hipSuccess) return (int)r;
            }
            if ((rc = dgrad({.layer = L + C, .ks = 1, .gy_chunks = c0, .cout = G0 + C * G, .gy = gy, .y = gcat, .res = gy, .res_chunks = c0,
                             .mask = blk, .mask_from = c0 + cg * (C - 1)}))) return rc;
            // The C 3x3 convs in gather form (binhip_weights_relayout_rdb_gather): every group of gcat is produced
            // ONCE as L_g + conv(stacked G_c of the later convs) instead of being read-modified-written by each of them.
            for (int c = C - 1; c >= 0; --c) {
                const Planes gyc = gcat.sub((c0 + cg * c) * P);           // G_c .. G_{C-1}, contiguous chunks
                if ((rc = wgrad({.layer = L + c, .cin_chunks = c0 + cg * c, .cin = G0 + G * c, .cout = G, .x = blk, .gy = gyc, .slot = c})))
                    return rc;
                if (c > 0) {
                    // group c = conv c-1's output slot: G_{c-1} = relu'( L_c + sum_{c' >= c} dgrad_c' )
                    const Planes slot = gcat.sub((c0 + cg * (c - 1)) * P);
                    if ((rc = dgrad({.layer = L + c, .gy_chunks = cg * (C - c), .cout = G, .gy = gyc, .y = slot, .res = slot,
                                     .mask = blk.sub((c0 + cg * (c - 1)) * P)}))) return rc;
                } else {
                    // group 0: L_0 + all C convs -> grad of the block input = GY[d] (already holds GFF.0's share when d >= 1)
                    if ((rc = dgrad({.layer = L, .gy_chunks = cg * C, .cout = G0, .gy = gyc, .y = b.gy.sub((int64_t)d * c0 * P), .res = gcat,
                                     .acc_inplace = d >= 1}))) return rc;
                }
            }
            if ((rc = flush_reduces())) return rc;                       // the block's C + 1 layers in one reduce launch
            if (two) {
                hipError_t r = hipEventCreateWithFlags(&b_done[d], hipEventDisableTiming);
                if (r == hipSuccess) r = hipEventRecord(b_done[d], sb);
                if (r != hipSuccess) return (int)r;
            }
        }
        // ---- SFENet2: X = F1; gF1 = dgrad + gG1 (the `x += f__1` skip)
        if ((rc = wgrad({.layer = 1, .cin_chunks = c0, .cin = G0, .cout = G0, .x = w.f1, .gy = b.gy}))) return rc;
        if ((rc = dgrad({.layer = 1, .gy_chunks = c0, .cout = G0, .gy = b.gy, .y = b.gf1, .res = b.gg1}))) return rc;
        // ---- SFENet1 5x5: X = X0
        if ((rc = wgrad({.layer = 0, .ks = 5, .cin_chunks = w.kc0, .cin = 12 * nin, .cout = G0, .x = w.x0, .gy = b.gf1}))) return rc;
        bool need_in = false;
        for (int i = 0; i < nin; ++i) need_in = need_in || (p->gin[i] != nullptr);
        if (need_in) {
            if ((rc = dgrad({.layer = 0, .ks = 5, .gy_chunks = c0, .cout = 12 * nin, .gy = b.gf1, .y = b.gx0}))) return rc;
            if ((rc = binhip_unpack_input_grads(Gw.hi(b.gx0), Gw.lo(b.gx0), gout, sc, nin, N, H, W, p->gin, stream))) return rc;
        }
        return 0;
    };
    rc = chain();
    for (int d = 0; d < 20; ++d) if (b_done[d]) (void)hipEventDestroy(b_done[d]);
    const int rj = order(sb, s);
    return rc ? rc : rj;
}

}  // extern "C"
