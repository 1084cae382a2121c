// binssim_refusals.cpp — a stand-alone host program over libbinssim's entry points for a sanitizer build: it calls
// binssim_workspace_bytes and every refusal path of binssim_forward and binssim_backward (include/binssim.h).  All of them return
// before any HIP call, so it needs no device and dereferences none of the made-up plane addresses.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       bin_amd/csrc/extra/binssim.hip tools/binssim_refusals.cpp -o binssim_refusals && ./binssim_refusals
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/binssim.h"

static int failures = 0;
#define EXPECT(expr, want)                                                                          \
    do {                                                                                            \
        const long long got__ = (long long)(expr);                                                  \
        if (got__ != (long long)(want)) {                                                           \
            std::fprintf(stderr, "line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got__, (long long)(want)); \
            ++failures;                                                                             \
        }                                                                                           \
    } while (0)

static float* p(uintptr_t v) { return reinterpret_cast<float*>(v); }

// two terms with made-up, well separated addresses: a 3 x 24 x 40 fp32 stack is 11 520 bytes, the terms lie 16 KiB apart
static const uintptr_t X = 0x100000, Y = 0x200000, GX = 0x300000, GY = 0x400000, G = 0x600000, OUT = 0x700000, WS = 0x8000000;
static BinSsimTerms terms(int n = 2) {
    BinSsimTerms t{};
    t.n_terms = n;
    for (int i = 0; i < n && i < BINSSIM_MAX_TERMS; ++i) {
        t.x[i] = p(X + 0x4000 * i);
        t.y[i] = p(Y + 0x4000 * i);
        t.gx[i] = p(GX + 0x4000 * i);
        t.gy[i] = p(GY + 0x4000 * i);
    }
    return t;
}

int main() {
    EXPECT(binssim_version(), BINSSIM_VERSION);
    // one double per BINSSIM_FWD_TILE_H x BINSSIM_FWD_TILE_W tile of windows, per plane, per term
    const int FH = BINSSIM_FWD_TILE_H, FW = BINSSIM_FWD_TILE_W;
    EXPECT(binssim_workspace_bytes(1, 1, 11, 11), 8);
    EXPECT(binssim_workspace_bytes(24, 1, 11, 11), 8 * 24);
    EXPECT(binssim_workspace_bytes(2, 3, FH + 10, FW + 10), 8 * 2 * 3);
    EXPECT(binssim_workspace_bytes(2, 3, FH + 11, FW + 11), 8 * 2 * 3 * 4);
    EXPECT(binssim_workspace_bytes(17, 24, 256, 256), 8 * 17 * 24 * 16 * 3);
    EXPECT(binssim_workspace_bytes(1, 32767, 256, 256) > 0, 1);
    EXPECT(binssim_workspace_bytes(0, 1, 11, 11), 0);
    EXPECT(binssim_workspace_bytes(25, 1, 11, 11), 0);
    EXPECT(binssim_workspace_bytes(1, 0, 11, 11), 0);
    EXPECT(binssim_workspace_bytes(1, 1, 10, 11), 0);
    EXPECT(binssim_workspace_bytes(1, 1, 11, 10), 0);
    EXPECT(binssim_workspace_bytes(1, 32768, 256, 256), 0);
    EXPECT(binssim_workspace_bytes(1, INT32_MAX, INT32_MAX, INT32_MAX), 0);
    EXPECT(binssim_workspace_bytes(INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN), 0);

    const double taps[11] = {};
    const size_t nb = binssim_workspace_bytes(2, 3, 24, 40), stack = sizeof(float) * 3 * 24 * 40;
    BinSsimTerms t = terms();
    auto fwd = [&](const BinSsimTerms* tt, int planes, int h, int w, const double* g, void* ws, size_t bytes, float* out) {
        return binssim_forward(tt, planes, h, w, g, ws, bytes, out, nullptr);
    };
    // ---- forward: pointers and counts
    EXPECT(fwd(nullptr, 3, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, nullptr, p(WS), nb, p(OUT)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, nullptr, nb, p(OUT)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, nullptr), BINSSIM_E_ARG);
    for (int n : {0, -1, 25, INT32_MAX, INT32_MIN}) {
        BinSsimTerms b = terms(n);
        EXPECT(fwd(&b, 3, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG);
    }
    { BinSsimTerms b = terms(); b.x[1] = nullptr; EXPECT(fwd(&b, 3, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.y[0] = nullptr; EXPECT(fwd(&b, 3, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.x[0] = p(X + 2); EXPECT(fwd(&b, 3, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.y[1] = p(Y + 0x4001); EXPECT(fwd(&b, 3, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG); }
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, p(OUT + 2)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS + 4), nb, p(OUT)), BINSSIM_E_ARG);
    { BinSsimTerms b = terms(); b.x[0] = nullptr; EXPECT(fwd(&b, 0, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_ARG); }   // named before the shape
    // ---- forward: shapes
    EXPECT(fwd(&t, 0, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    EXPECT(fwd(&t, -1, 24, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    EXPECT(fwd(&t, 3, 10, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    EXPECT(fwd(&t, 3, 24, 10, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    EXPECT(fwd(&t, 3, INT32_MIN, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    EXPECT(fwd(&t, 32768, 256, 256, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    EXPECT(fwd(&t, INT32_MAX, INT32_MAX, INT32_MAX, taps, p(WS), nb, p(OUT)), BINSSIM_E_SHAPE);
    // ---- forward: an output that is also an input, the outputs on each other
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, p(X)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, p(X + stack - 4)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, p(X - 4)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, p(Y + 0x4000 + 8)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(Y), nb, p(OUT)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(X + 0x4000 - 8), nb, p(OUT)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(OUT), nb, p(OUT)), BINSSIM_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb, p(WS + 8)), BINSSIM_E_ARG);
    // ---- forward: the workspace
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), nb - 1, p(OUT)), BINSSIM_E_WORKSPACE);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), 0, p(OUT)), BINSSIM_E_WORKSPACE);
    EXPECT(fwd(&t, 3, 48, 40, taps, p(WS), nb, p(OUT)), BINSSIM_E_WORKSPACE);
    EXPECT(fwd(&t, 3, 24, 40, taps, p(WS), 0, p(X - 8)), BINSSIM_E_WORKSPACE);   // one element before an input touches nothing

    auto bwd = [&](const BinSsimTerms* tt, int planes, int h, int w, const double* g11, const float* g) {
        return binssim_backward(tt, planes, h, w, g11, g, nullptr);
    };
    // ---- backward: pointers and counts
    EXPECT(bwd(nullptr, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, nullptr, p(G)), BINSSIM_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, taps, nullptr), BINSSIM_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, taps, p(G + 2)), BINSSIM_E_ARG);
    for (int n : {0, -1, 25}) {
        BinSsimTerms b = terms(n);
        EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG);
    }
    { BinSsimTerms b = terms(); b.x[1] = nullptr; EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.y[0] = nullptr; EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gx[1] = b.gy[1] = nullptr; EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }   // neither gradient
    { BinSsimTerms b = terms(); b.gx[0] = p(GX + 2); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gy[1] = p(GY + 0x4003); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gx[0] = b.gy[0] = nullptr; EXPECT(bwd(&b, 3, 10, 40, taps, p(G)), BINSSIM_E_ARG); }   // named before the shape
    // ---- backward: shapes
    EXPECT(bwd(&t, 0, 24, 40, taps, p(G)), BINSSIM_E_SHAPE);
    EXPECT(bwd(&t, 3, 10, 40, taps, p(G)), BINSSIM_E_SHAPE);
    EXPECT(bwd(&t, 3, 24, 10, taps, p(G)), BINSSIM_E_SHAPE);
    EXPECT(bwd(&t, 32768, 256, 256, taps, p(G)), BINSSIM_E_SHAPE);
    // ---- backward: an output that is also an input (its own term's, another term's, by one element at either end, g)
    { BinSsimTerms b = terms(); b.gx[0] = p(X); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gy[0] = p(Y + 0x4000); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gx[1] = p(X + stack - 4); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gx[1] = p(X - stack + 4); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gy[1] = p(G); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gy[1] = p(G + 4); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gy[1] = p(G - stack + 4); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    // ---- backward: an output named twice
    { BinSsimTerms b = terms(); b.gy[0] = p(GX); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gx[1] = p(GX); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    { BinSsimTerms b = terms(); b.gy[1] = p(GX + stack - 4); EXPECT(bwd(&b, 3, 24, 40, taps, p(G)), BINSSIM_E_ARG); }
    if (failures) {
        std::fprintf(stderr, "%d refusal checks failed\n", failures);
        return 1;
    }
    std::puts("binssim refusals ok");
    return 0;
}
