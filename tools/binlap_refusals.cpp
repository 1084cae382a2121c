// binlap_refusals.cpp — a stand-alone host program over libbinlap's entry points for a sanitizer build: it calls both workspace
// queries and every refusal path of binlap_forward and binlap_backward (include/binlap.h).  All of them return before any HIP call,
// so it needs no device and dereferences none of the made-up plane addresses.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       bin_amd/csrc/extra/binlap.hip tools/binlap_refusals.cpp -o binlap_refusals && ./binlap_refusals
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/binlap.h"

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
static const double EPS = 1e-6;
static BinLapTerms terms(int n = 2) {
    BinLapTerms t{};
    t.n_terms = n;
    for (int i = 0; i < n && i < BINLAP_MAX_TERMS; ++i) {
        t.x[i] = p(X + 0x4000 * i);
        t.y[i] = p(Y + 0x4000 * i);
        t.gx[i] = p(GX + 0x4000 * i);
        t.gy[i] = p(GY + 0x4000 * i);
    }
    return t;
}

// what the header says the queries count, restated: levels >= 1 of the pyramid in double, and one double per band tile of every level
static void want_bytes(int T, int planes, int H, int W, int levels, size_t* fwd, size_t* bwd) {
    size_t coarse = 0, slots = 0;
    int h = H, w = W;
    for (int l = 0; l < levels; ++l) {
        if (l) {
            h = (h + 1) / 2;
            w = (w + 1) / 2;
            coarse += (size_t)T * planes * h * w;
        }
        slots += (size_t)T * planes * ((h + BINLAP_UP_TILE_H - 1) / BINLAP_UP_TILE_H) * ((w + BINLAP_UP_TILE_W - 1) / BINLAP_UP_TILE_W);
    }
    *fwd = 8 * (coarse + slots);
    *bwd = 8 * (coarse ? 2 * coarse : 1);
}

int main() {
    EXPECT(binlap_version(), BINLAP_VERSION);
    const int good[][5] = {{1, 1, 1, 1, 1}, {2, 3, 5, 7, 2}, {2, 2, 33, 47, 5}, {17, 24, 256, 256, 5}, {24, 1, 17, 129, 4}, {1, 1, 128, 128, 8},
                           {1, 32767, 256, 256, 1}, {1, 1, 32768, 65535, 8}};
    for (const auto& g : good) {
        size_t f, b;
        want_bytes(g[0], g[1], g[2], g[3], g[4], &f, &b);
        EXPECT(binlap_forward_workspace_bytes(g[0], g[1], g[2], g[3], g[4]), f);
        EXPECT(binlap_backward_workspace_bytes(g[0], g[1], g[2], g[3], g[4]), b);
    }
    const int bad[][5] = {{0, 1, 16, 16, 5}, {25, 1, 16, 16, 5}, {-1, 1, 16, 16, 5}, {1, 0, 16, 16, 5}, {1, -1, 16, 16, 5}, {1, 1, 15, 16, 5},
                          {1, 1, 16, 15, 5}, {1, 1, 16, 16, 0}, {1, 1, 16, 16, 9}, {1, 1, 16, 16, -1}, {1, 1, 127, 128, 8}, {1, 1, 0, 1, 1},
                          {1, 32768, 256, 256, 1}, {1, INT32_MAX, INT32_MAX, INT32_MAX, 1}, {1, 1, INT32_MIN, 16, 1},
                          {INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN}, {1, 1, 16, 16, INT32_MAX}};
    for (const auto& g : bad) {
        EXPECT(binlap_forward_workspace_bytes(g[0], g[1], g[2], g[3], g[4]), 0);
        EXPECT(binlap_backward_workspace_bytes(g[0], g[1], g[2], g[3], g[4]), 0);
    }

    const size_t nb = binlap_forward_workspace_bytes(2, 3, 24, 40, 4), stack = sizeof(float) * 3 * 24 * 40;
    BinLapTerms t = terms();
    auto fwd = [&](const BinLapTerms* tt, int planes, int h, int w, int levels, double eps, void* ws, size_t bytes, float* out) {
        return binlap_forward(tt, planes, h, w, levels, eps, ws, bytes, out, nullptr);
    };
    // ---- forward: pointers and counts
    EXPECT(fwd(nullptr, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, nullptr, nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, nullptr), BINLAP_E_ARG);
    for (int n : {0, -1, 25, INT32_MAX, INT32_MIN}) {
        BinLapTerms b = terms(n);
        EXPECT(fwd(&b, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG);
    }
    { BinLapTerms b = terms(); b.x[1] = nullptr; EXPECT(fwd(&b, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.y[0] = nullptr; EXPECT(fwd(&b, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.x[0] = p(X + 2); EXPECT(fwd(&b, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.y[1] = p(Y + 0x4001); EXPECT(fwd(&b, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG); }
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, p(OUT + 2)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS + 4), nb, p(OUT)), BINLAP_E_ARG);
    // ---- forward: levels and eps, named before the shape
    for (int levels : {0, -1, 9, INT32_MAX, INT32_MIN}) EXPECT(fwd(&t, 3, 24, 40, levels, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG);
    for (double eps : {0.0, -0.0, -1e-6, (double)INFINITY, (double)NAN}) EXPECT(fwd(&t, 3, 24, 40, 4, eps, p(WS), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 0, 24, 40, 9, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 0, 24, 40, 4, 0.0, p(WS), nb, p(OUT)), BINLAP_E_ARG);
    { BinLapTerms b = terms(); b.x[0] = nullptr; EXPECT(fwd(&b, 0, 24, 40, 0, EPS, p(WS), nb, p(OUT)), BINLAP_E_ARG); }
    // ---- forward: shapes
    EXPECT(fwd(&t, 0, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, -1, 24, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, 3, 7, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, 3, 24, 7, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, 3, 24, 40, 6, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, 3, INT32_MIN, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, 32768, 256, 256, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, INT32_MAX, INT32_MAX, INT32_MAX, 8, EPS, p(WS), nb, p(OUT)), BINLAP_E_SHAPE);
    EXPECT(fwd(&t, 0, 24, 40, 4, EPS, p(WS), nb, p(X)), BINLAP_E_SHAPE);                 // named before an overlap
    // ---- forward: an output that is also an input, the outputs on each other
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, p(X)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, p(X + stack - 4)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, p(X - 4)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, p(Y + 0x4000 + 8)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(Y), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(X + 0x4000 - 8), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(X - nb + 8), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(OUT), nb, p(OUT)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb, p(WS + nb - 4)), BINLAP_E_ARG);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), 0, p(X)), BINLAP_E_ARG);                    // named before the workspace
    // ---- forward: the workspace
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), nb - 1, p(OUT)), BINLAP_E_WORKSPACE);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), 0, p(OUT)), BINLAP_E_WORKSPACE);
    EXPECT(fwd(&t, 3, 48, 40, 4, EPS, p(WS), nb, p(OUT)), BINLAP_E_WORKSPACE);
    EXPECT(fwd(&t, 3, 24, 40, 4, EPS, p(WS), 0, p(X - 8)), BINLAP_E_WORKSPACE);          // one element before an input touches nothing
    EXPECT(fwd(&t, 3, 8, 8, 4, EPS, p(WS), 0, p(OUT)), BINLAP_E_WORKSPACE);              // the smallest plane four levels take

    const size_t nbb = binlap_backward_workspace_bytes(2, 3, 24, 40, 4);
    auto bwd = [&](const BinLapTerms* tt, int planes, int h, int w, int levels, double eps, const float* g, void* ws, size_t bytes) {
        return binlap_backward(tt, planes, h, w, levels, eps, g, ws, bytes, nullptr);
    };
    // ---- backward: pointers and counts
    EXPECT(bwd(nullptr, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, nullptr, p(WS), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G + 2), p(WS), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), nullptr, nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(WS + 4), nbb), BINLAP_E_ARG);
    for (int n : {0, -1, 25}) {
        BinLapTerms b = terms(n);
        EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG);
    }
    { BinLapTerms b = terms(); b.x[1] = nullptr; EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.y[0] = nullptr; EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gx[1] = b.gy[1] = nullptr; EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }   // neither gradient
    { BinLapTerms b = terms(); b.gx[1] = nullptr; EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), 0), BINLAP_E_WORKSPACE); }          // one is enough
    { BinLapTerms b = terms(); b.gx[0] = p(GX + 2); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gy[1] = p(GY + 0x4003); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gx[0] = b.gy[0] = nullptr; EXPECT(bwd(&b, 3, 7, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }    // named before the shape
    // ---- backward: levels and eps
    for (int levels : {0, -1, 9}) EXPECT(bwd(&t, 3, 24, 40, levels, EPS, p(G), p(WS), nbb), BINLAP_E_ARG);
    for (double eps : {0.0, -1e-6, (double)INFINITY, (double)NAN}) EXPECT(bwd(&t, 3, 24, 40, 4, eps, p(G), p(WS), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 0, 24, 40, 9, EPS, p(G), p(WS), nbb), BINLAP_E_ARG);
    // ---- backward: shapes
    EXPECT(bwd(&t, 0, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_SHAPE);
    EXPECT(bwd(&t, 3, 7, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_SHAPE);
    EXPECT(bwd(&t, 3, 24, 7, 4, EPS, p(G), p(WS), nbb), BINLAP_E_SHAPE);
    EXPECT(bwd(&t, 3, 24, 40, 6, EPS, p(G), p(WS), nbb), BINLAP_E_SHAPE);
    EXPECT(bwd(&t, 32768, 256, 256, 4, EPS, p(G), p(WS), nbb), BINLAP_E_SHAPE);
    EXPECT(bwd(&t, 0, 24, 40, 4, EPS, p(G), p(X), nbb), BINLAP_E_SHAPE);                 // named before an overlap
    // ---- backward: an output that is also an input (its own term's, another term's, by one element at either end, g)
    { BinLapTerms b = terms(); b.gx[0] = p(X); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gy[0] = p(Y + 0x4000); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gx[1] = p(X + stack - 4); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gx[1] = p(X - stack + 4); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gy[1] = p(G); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gy[1] = p(G + 4); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gy[1] = p(G - stack + 4); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    // ---- backward: an output named twice
    { BinLapTerms b = terms(); b.gy[0] = p(GX); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gx[1] = p(GX); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    { BinLapTerms b = terms(); b.gy[1] = p(GX + stack - 4); EXPECT(bwd(&b, 3, 24, 40, 4, EPS, p(G), p(WS), nbb), BINLAP_E_ARG); }
    // ---- backward: the used workspace on an output, an input or g
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(GX), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(GY + 0x4000 + stack - 8), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(X), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(Y - nbb + 8), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(G), nbb), BINLAP_E_ARG);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(X), 0), BINLAP_E_ARG);                     // named before the workspace
    // ---- backward: the workspace
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(WS), nbb - 1), BINLAP_E_WORKSPACE);
    EXPECT(bwd(&t, 3, 24, 40, 4, EPS, p(G), p(WS), 0), BINLAP_E_WORKSPACE);
    EXPECT(bwd(&t, 3, 24, 44, 4, EPS, p(G), p(WS), nbb), BINLAP_E_WORKSPACE);
    EXPECT(bwd(&t, 3, 24, 40, 1, EPS, p(G), p(WS), 7), BINLAP_E_WORKSPACE);              // one level still takes its pad double
    if (failures) {
        std::fprintf(stderr, "%d refusal checks failed\n", failures);
        return 1;
    }
    std::puts("binlap refusals ok");
    return 0;
}
