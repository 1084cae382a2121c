// bincrop_refusals.cpp — a stand-alone host program over libbincrop's entry points for a sanitizer build: it calls every refusal path
// of bincrop_yuv_crops_to_bgr (include/bincrop.h).  All of them return before any HIP call, so it needs no device and dereferences
// none of the made-up addresses.  Build and run:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       bin_amd/csrc/extra/bincrop.hip tools/bincrop_refusals.cpp -o bincrop_refusals && ./bincrop_refusals
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../include/bincrop.h"

static int failures = 0;
#define EXPECT(expr, want)                                                                          \
    do {                                                                                            \
        const long long got__ = (long long)(expr);                                                  \
        if (got__ != (long long)(want)) {                                                           \
            std::fprintf(stderr, "line %d: %s = %lld, expected %lld\n", __LINE__, #expr, got__, (long long)(want)); \
            ++failures;                                                                             \
        }                                                                                           \
    } while (0)

static uint8_t* p(uintptr_t v) { return reinterpret_cast<uint8_t*>(v); }
static const BinCropRow* rows(uintptr_t v) { return reinterpret_cast<const BinCropRow*>(v); }

// made-up, well separated addresses: an arena of 4096 bytes, a table of 3 rows (96 bytes), an output of 3 x 4 x 8 x 3 = 288 bytes
static const uintptr_t A = 0x100000, T = 0x200000, OUT = 0x300000;
static const int64_t AB = 4096;
static const int64_t TOP = (int64_t)1 << 40;

static int call(uintptr_t arena = A, int64_t arena_bytes = AB, uintptr_t table = T, int n = 3, int ch = 4, int cw = 8, int chroma = 420,
                uintptr_t out = OUT) {
    return bincrop_yuv_crops_to_bgr(p(arena), arena_bytes, rows(table), n, ch, cw, chroma, p(out), nullptr);
}

int main() {
    EXPECT(bincrop_version(), BINCROP_VERSION);
    EXPECT(sizeof(BinCropRow), 32);
    // ---- pointers
    EXPECT(call(0), BINCROP_E_ARG);
    EXPECT(call(A, AB, 0), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, 0), BINCROP_E_ARG);
    for (uintptr_t odd : {T + 1, T + 2, T + 4, T + 7}) EXPECT(call(A, AB, odd), BINCROP_E_ARG);
    // ---- counts
    for (int n : {0, -1, INT32_MIN}) EXPECT(call(A, AB, T, n), BINCROP_E_ARG);
    for (int ch : {0, -1, INT32_MIN}) EXPECT(call(A, AB, T, 3, ch), BINCROP_E_ARG);
    for (int cw : {0, -1, INT32_MIN}) EXPECT(call(A, AB, T, 3, 4, cw), BINCROP_E_ARG);
    // ---- chroma
    for (int chroma : {0, 422, 411, -420, 1, INT32_MAX}) EXPECT(call(A, AB, T, 3, 4, 8, chroma), BINCROP_E_ARG);
    // ---- the arena's size
    for (int64_t bytes : {(int64_t)0, (int64_t)-1, INT64_MIN}) EXPECT(call(A, bytes), BINCROP_E_ARG);
    // ---- beyond 2^40: the arena, the output; argument errors come first
    EXPECT(call(A, TOP + 1, T, 3, 4, 8, 420, 0x7000000000000000u), BINCROP_E_SHAPE);
    EXPECT(call(A, INT64_MAX, T, 3, 4, 8, 420, 0x7000000000000000u), BINCROP_E_SHAPE);
    EXPECT(call(A, AB, T, 1, 1 << 20, 1 << 20), BINCROP_E_SHAPE);                          // 3 * 2^40 bytes
    EXPECT(call(A, AB, T, 1 << 11, 1 << 14, 1 << 14), BINCROP_E_SHAPE);
    EXPECT(call(A, AB, T, INT32_MAX, INT32_MAX, INT32_MAX), BINCROP_E_SHAPE);
    EXPECT(call(A, AB, T, INT32_MAX, INT32_MAX, INT32_MAX, 444), BINCROP_E_SHAPE);
    EXPECT(call(A, TOP + 1, T, 3, 4, 8, 7), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, INT32_MAX, INT32_MAX, INT32_MAX, 420, 0), BINCROP_E_ARG);
    EXPECT(call(A, AB, 0, 1, 1 << 20, 1 << 20), BINCROP_E_ARG);
    // ---- the output on the arena: by one byte at either end, inside, around; and on the table
    EXPECT(call(A, AB, T, 3, 4, 8, 420, A), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, A + AB - 1), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, A - 287), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, A + 100), BINCROP_E_ARG);
    EXPECT(call(A + 10, 20, T, 3, 4, 8, 420, A), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, T), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, T + 95), BINCROP_E_ARG);
    EXPECT(call(A, AB, T, 3, 4, 8, 420, T - 287), BINCROP_E_ARG);
    if (failures) {
        std::fprintf(stderr, "%d refusal checks failed\n", failures);
        return 1;
    }
    std::puts("bincrop refusals ok");
    return 0;
}
