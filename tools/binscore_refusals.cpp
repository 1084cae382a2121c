// binscore_refusals.cpp — a stand-alone host program over libbinscore's entry points for a sanitizer build: it calls
// binscore_workspace_bytes and every refusal path of binscore_planes (include/binscore.h).  All of them return before any HIP call,
// so it needs no device and dereferences none of the made-up plane addresses.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       bin_amd/csrc/binscore.hip tools/binscore_refusals.cpp -o binscore_refusals && ./binscore_refusals
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/binscore.h"

static int failures = 0;
#define EXPECT(expr, want)                                                                          \
    do {                                                                                            \
        const long long got__ = (long long)(expr);                                                  \
        if (got__ != (long long)(want)) {                                                           \
            std::fprintf(stderr, "line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got__, (long long)(want)); \
            ++failures;                                                                             \
        }                                                                                           \
    } while (0)

int main() {
    const int G11 = BINSCORE_SSIM_G11, U7 = BINSCORE_SSIM_U7, BOTH = G11 | U7;
    EXPECT(binscore_version(), BINSCORE_VERSION);
    // one 64-byte slot per 16 x 246 tile of every plane
    EXPECT(binscore_workspace_bytes(24, 40, 420, BOTH), 64 * 4);
    EXPECT(binscore_workspace_bytes(17, 247, 420, BOTH), 64 * 6);
    EXPECT(binscore_workspace_bytes(17, 247, 444, BOTH), 64 * 12);
    EXPECT(binscore_workspace_bytes(1, 1, 420, 0), 64 * 3);
    EXPECT(binscore_workspace_bytes(65535, 65535, 444, 0), 64ll * 3 * 4096 * 267);
    EXPECT(binscore_workspace_bytes(0, 40, 420, 0), 0);
    EXPECT(binscore_workspace_bytes(24, 65536, 420, 0), 0);
    EXPECT(binscore_workspace_bytes(24, 40, 422, 0), 0);
    EXPECT(binscore_workspace_bytes(24, 40, 420, 4), 0);
    EXPECT(binscore_workspace_bytes(10, 40, 420, G11), 0);
    EXPECT(binscore_workspace_bytes(6, 40, 420, U7), 0);
    EXPECT(binscore_workspace_bytes(INT32_MAX, INT32_MAX, 444, 0), 0);
    EXPECT(binscore_workspace_bytes(INT32_MIN, -1, 444, -1), 0);

    auto p = [](uintptr_t v) { return reinterpret_cast<uint8_t*>(v); };
    uint8_t *AY = p(0x100000), *AU = p(0x200000), *AV = p(0x300000), *BY = p(0x400000), *BU = p(0x500000), *BV = p(0x600000);
    void* WS = p(0x8000000);
    BinPlaneScores* OUT = reinterpret_cast<BinPlaneScores*>(p(0x700000));
    const double taps[11] = {};
    const size_t nb = binscore_workspace_bytes(24, 40, 420, BOTH);
    auto call = [&](const uint8_t* ay, const uint8_t* au, const uint8_t* av, const uint8_t* by, const uint8_t* bu, const uint8_t* bv, int h,
                    int w, int chroma, int flags, const double* g, void* ws, size_t bytes, void* out) {
        return binscore_planes(ay, au, av, by, bu, bv, h, w, chroma, flags, g, ws, bytes, static_cast<BinPlaneScores*>(out), nullptr);
    };
    // null pointers
    EXPECT(call(nullptr, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, nullptr, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, nullptr, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, nullptr, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, nullptr, BV, 24, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, nullptr, 24, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, nullptr, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, nullptr), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, nullptr, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, G11, nullptr, WS, nb, OUT), BINSCORE_E_ARG);
    // flags, chroma, alignment
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, 4, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, -1, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 422, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 0, BOTH, taps, WS, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, p(0x700004)), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, p(0x8000001), nb, OUT), BINSCORE_E_ARG);
    // overlaps (the planes of a 24 x 40 4:2:0 payload are 960, 240 and 240 bytes)
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, AY), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, AY + 952), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, AU + 232), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, BY - 56), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb, BV + 8), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, AY + 8, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, BU - 8, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, reinterpret_cast<uint8_t*>(OUT) - 8, nb, OUT), BINSCORE_E_ARG);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 65535, 65535, 444, 0, taps, p(0x8), ~(size_t)0, p(0x7ffffffffff8)), BINSCORE_E_ARG);
    // shapes
    EXPECT(call(AY, AU, AV, BY, BU, BV, 0, 40, 420, 0, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, -7, 420, 0, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 65536, 40, 420, 0, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, INT32_MAX, INT32_MAX, 444, 0, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 10, 40, 420, BOTH, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 10, 420, G11, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 6, 40, 420, U7, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 6, 444, U7, taps, WS, nb, OUT), BINSCORE_E_SHAPE);
    // the workspace
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, nb - 1, OUT), BINSCORE_E_WORKSPACE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 24, 40, 420, BOTH, taps, WS, 0, OUT), BINSCORE_E_WORKSPACE);
    EXPECT(call(AY, AU, AV, BY, BU, BV, 65535, 65535, 444, 0, taps, WS, nb, OUT), BINSCORE_E_WORKSPACE);
    if (failures) {
        std::fprintf(stderr, "%d refusal checks failed\n", failures);
        return 1;
    }
    std::puts("binscore refusals ok");
    return 0;
}
