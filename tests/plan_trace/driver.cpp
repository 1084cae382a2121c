// Drives binhip_rdn_forward / binhip_rdn_backward (bin_amd/csrc/binhip_plan.hip, linked against stubs.hip) through the smallest
// cases that reach each branch of the plan, with fake, distinct pointers; the stand-ins print the launch trace
// (tests/test_cpu_plan_trace.py compares it with tests/golden/plan_trace.txt).
#include <cstdint>
#include <cstdio>
#include "binhip.h"

extern int g_rdb3_rc;
void trace_reset_events();

static void* fp(uintptr_t v) { return (void*)v; }

enum { FWD = 1, BWD = 2 };
struct Case {
    const char* name;
    BinRdnShape shape;
    int N, H, W, nin;
    int nt_fwd, nt_bwd;
    int fwd_flags, bwd_flags;
    int run = FWD | BWD;
    bool aux = false;
    int gin = 0;                    // bit i: frame i wants its gradient
    bool fused_slots = false;       // fill slots L and L + 1 (the fused UPNet's operators)
    bool profiler = false;
    int rdb3_rc = 0;
    // refusals
    bool null_fwd_plan = false, null_bwd_plan = false;
    int null_layer = -1;            // this layer's w_hi / wt_hi is null
    int ws_short = 0, bws_short = 0;
};

static int layers(const BinRdnShape& s) { return s.G0 ? 2 + s.D * (s.C + 1) + 4 : BINHIP_RDN_LAYERS; }

static void run(const Case& c) {
    printf("== %s: shape(%d,%d,%d,%d) N%d %dx%d nin%d nt%d/%d fwd_flags%x bwd_flags%x aux%d gin%x\n", c.name, c.shape.G0, c.shape.D,
           c.shape.C, c.shape.G, c.N, c.H, c.W, c.nin, c.nt_fwd, c.nt_bwd, c.fwd_flags, c.bwd_flags, (int)c.aux, c.gin);
    trace_reset_events();
    g_rdb3_rc = c.rdb3_rc;
    const int L = layers(c.shape), nslots = c.fused_slots ? L + 2 : L;
    void* const status = fp(0x5000);
    void* const stream = fp(0xA0);
    void* const saved = fp(0x100000040);           // not 256-byte aligned: the plan rounds it up
    int64_t lay[BINHIP_RDN_BWD_LAYOUT_WORDS];

    const size_t wb = binhip_rdn_workspace_bytes(c.N, c.H, c.W, c.nin, c.nt_fwd, &c.shape);
    const size_t bb = binhip_rdn_backward_workspace_bytes(c.N, c.H, c.W, c.nin, c.nt_bwd, &c.shape);
    printf("workspace_bytes %zu backward_workspace_bytes %zu\n", wb, bb);
    int rc = binhip_rdn_workspace_layout(c.N, c.H, c.W, c.nin, c.nt_fwd, &c.shape, lay, BINHIP_RDN_LAYOUT_WORDS);
    printf("workspace_layout rc%d", rc);
    for (int i = 0; i < BINHIP_RDN_LAYOUT_WORDS && rc == 0; ++i) printf(" %lld", (long long)lay[i]);
    rc = binhip_rdn_backward_workspace_layout(c.N, c.H, c.W, c.nin, c.nt_bwd, &c.shape, lay, BINHIP_RDN_BWD_LAYOUT_WORDS);
    printf("\nbackward_workspace_layout rc%d", rc);
    for (int i = 0; i < BINHIP_RDN_BWD_LAYOUT_WORDS && rc == 0; ++i) printf(" %lld", (long long)lay[i]);
    printf("\n");

    if (c.run & FWD) {
        static BinRdnPlan p;
        p = BinRdnPlan{};
        p.N = c.N; p.H = c.H; p.W = c.W; p.n_inputs = c.nin; p.nterms = c.nt_fwd; p.reserved = c.fwd_flags; p.shape = c.shape;
        for (int i = 0; i < nslots; ++i) {
            p.w_hi[i] = fp(0x1000000 + 0x100 * i);
            p.w_lo[i] = c.nt_fwd == 3 ? fp(0x2000000 + 0x100 * i) : nullptr;
            p.bias[i] = (const float*)fp(0x3000000 + 0x100 * i);
        }
        if (c.null_layer >= 0) p.w_hi[c.null_layer] = nullptr;
        p.status = status;
        p.profiler = c.profiler ? (BinhipProfiler*)fp(0xF000) : nullptr;
        const float* in[5];
        for (int i = 0; i < 5; ++i) in[i] = (const float*)fp(0x6000000 + 0x100000 * i);
        rc = binhip_rdn_forward(c.null_fwd_plan ? nullptr : &p, in, (float*)fp(0x7000000), saved, wb - c.ws_short, stream);
        printf("forward rc%d\n", rc);
    }
    if (c.run & BWD) {
        static BinRdnBwdPlan b;
        b = BinRdnBwdPlan{};
        b.N = c.N; b.H = c.H; b.W = c.W; b.n_inputs = c.nin; b.nterms = c.nt_bwd; b.reserved = c.bwd_flags; b.shape = c.shape;
        for (int i = 0; i < nslots; ++i) {
            b.wt_hi[i] = fp(0x1100000 + 0x100 * i);
            b.wt_lo[i] = c.nt_bwd == 3 ? fp(0x2100000 + 0x100 * i) : nullptr;
            b.dw[i] = (float*)fp(0x8000000 + 0x100 * i);
            b.db[i] = (float*)fp(0x9000000 + 0x100 * i);
        }
        if (c.null_layer >= 0) b.wt_hi[c.null_layer] = nullptr;
        b.zero_bias = (const float*)fp(0x4000);
        b.status = status;
        b.aux_stream = c.aux ? fp(0xB0) : nullptr;
        b.profiler = c.profiler ? (BinhipProfiler*)fp(0xF000) : nullptr;
        for (int i = 0; i < c.nin && i < 5; ++i) b.gin[i] = (c.gin >> i) & 1 ? (float*)fp(0xC000000 + 0x100000 * i) : nullptr;
        const int nt_saved = (c.bwd_flags & BINHIP_BWD_SAVED_X3) ? 3 : c.nt_bwd;
        const size_t sb = binhip_rdn_workspace_bytes(c.N, c.H, c.W, c.nin, nt_saved, &c.shape);
        rc = binhip_rdn_backward(c.null_bwd_plan ? nullptr : &b, saved, sb - c.ws_short, (const float*)fp(0xD000000), fp(0x200000080),
                                 bb - c.bws_short, stream);
        printf("backward rc%d\n", rc);
    }
}

int main() {
    const BinRdnShape dflt = {0, 0, 0, 0}, stage4 = {96, 12, 4, 32};
    const int KEEP = BINHIP_PLAN_KEEP_ACTS, FUSED = BINHIP_PLAN_FUSED_UPNET, TRAIN = BINHIP_PLAN_FUSED_UPNET_TRAIN;
    Case c;
    // a: the all-zero default shape; 64-pixel half-resolution rows -> the 1x1 pixel-grid reshape; every input gradient
    c = {"a default shape, 1x1 reshape", dflt, 1, 32, 128, 2, 3, 3, 0, 0};
    c.gin = 3;
    run(c);
    // b: stage4 given explicitly, fused UPNet forward and backward, side stream, 3 frames (half last chunk on SFENet1), ragged tiles
    c = {"b fused UPNet training, side stream", stage4, 2, 34, 66, 3, 1, 1, KEEP | FUSED | TRAIN, BINHIP_BWD_FUSED_UPNET};
    c.aux = true; c.gin = 5; c.fused_slots = true;
    run(c);
    // c: another shape, unfused dense-block tails, accumulate, side stream (b_done[d + 2] wait, both gcat buffers), no input gradient
    c = {"c (64,3,2,64) NO_FUSE, accumulate", {64, 3, 2, 64}, 1, 32, 64, 5, 3, 3, BINHIP_PLAN_NO_FUSE, BINHIP_BWD_ACCUMULATE};
    c.aux = true;
    run(c);
    // d: the three-phase dense-block launch, taken and refused (per-conv fallback)
    c = {"d RDB3 taken", stage4, 1, 32, 64, 2, 3, 3, BINHIP_PLAN_RDB3 | FUSED, 0, FWD};
    c.fused_slots = true;
    run(c);
    c.name = "d RDB3 refused: per-conv launches"; c.rdb3_rc = BINHIP_E_SHAPE;
    run(c);
    // e: KEEP_ACTS | FUSED_UPNET without _TRAIN keeps the two UPNet layers
    c = {"e KEEP_ACTS without FUSED_UPNET_TRAIN", stage4, 1, 32, 64, 2, 1, 1, KEEP | FUSED, 0, FWD};
    c.fused_slots = true;
    run(c);
    // f: single-product backward on 3-term saved state
    c = {"f BWD_SAVED_X3", stage4, 1, 32, 64, 3, 3, 1, KEEP, BINHIP_BWD_SAVED_X3};
    c.gin = 7;
    run(c);
    // g: a profiler handle
    c = {"g profiler", stage4, 1, 32, 64, 2, 1, 1, KEEP, 0};
    c.profiler = true; c.gin = 1;
    run(c);
    // h: the most dense blocks, the smallest of everything else: the whole b_done array
    c = {"h D = 20", {32, 20, 1, 32}, 1, 32, 64, 2, 1, 1, KEEP, 0};
    c.aux = true; c.gin = 2;
    run(c);

    // i: refusals: a return code each, and no launch
    const Case ok = {"", stage4, 1, 32, 64, 2, 3, 3, KEEP, 0};
    c = ok; c.name = "i odd H"; c.H = 33; run(c);
    c = ok; c.name = "i n_inputs 4"; c.nin = 4; run(c);
    c = ok; c.name = "i nterms 2"; c.nt_fwd = c.nt_bwd = 2; run(c);
    c = ok; c.name = "i G0 48"; c.shape.G0 = 48; run(c);
    c = ok; c.name = "i forward workspace / saved state one byte short"; c.ws_short = 1; run(c);
    c = ok; c.name = "i backward workspace one byte short"; c.run = BWD; c.bws_short = 1; run(c);
    c = ok; c.name = "i null w_hi / wt_hi in the last layer"; c.null_layer = BINHIP_RDN_LAYERS - 1; run(c);
    c = ok; c.name = "i null plan"; c.null_fwd_plan = c.null_bwd_plan = true; run(c);
    c = ok; c.name = "i BWD_SAVED_X3 with nterms 3"; c.run = BWD; c.bwd_flags = BINHIP_BWD_SAVED_X3; run(c);
    c = ok; c.name = "i BWD_FUSED_UPNET with slot L empty"; c.run = BWD; c.bwd_flags = BINHIP_BWD_FUSED_UPNET; run(c);
    return 0;
}
