// binscore.hip (libbinscore.so, include/binscore.h) — the scores of one planar 8-bit YUV payload against another (bin_amd/score.py):
//   per plane the sums of squared and of absolute differences (exact), and of the Y plane as a one-channel image the Gaussian
//   11x11 SSIM (util.calculate_ssim) and the uniform 7x7 SSIM (util.compare_ssim).
// The tile walk is binhip_score_walk.h's, the one libbinhip.so's image and frame scores run: PlanePairs below is its third loader.
// A slice of the walk is a plane, a same-channel neighbour 1 byte away, a 5-column halo and 246 output columns per 256-thread row;
// slice 0 of a launch that begins with the Y plane takes the SSIM flags, every other slice only the sums.  A call is the Y launch,
// the launch of U and V together where their shape differs from Y's (4:2:0 above 1 x 1; otherwise all three planes are the slices
// of one launch) and plane_score_final_kernel, which adds the workspace slots of each plane in a fixed order and writes the record.
#include "binhip_score_walk.h"
#include "../../include/binscore.h"

namespace {
static_assert(BINSCORE_SSIM_G11 == SC_FLAG_G11 && BINSCORE_SSIM_U7 == SC_FLAG_U7, "the header's flags are the walk's");
static_assert(sizeof(BinPlaneScores) == 64 && offsetof(BinPlaneScores, sad) == 24 && offsetof(BinPlaneScores, ssim_g11) == 48,
              "BinPlaneScores layout");

struct PlanePairs {                                  // up to three [H][W] u8 planes of one shape per side; grid z = plane
    static constexpr int STRIDE = 1, HALO = 5 * STRIDE, TE = SC_THREADS - 2 * HALO;      // 246 output columns
    const uint8_t* a[3];
    const uint8_t* b[3];
    int ssim_slice;                                  // the slice that is a Y plane (it takes the SSIM flags), or -1
    __host__ __device__ static int row_elems(int W) { return W; }
    __device__ int slice_flags(int z, int flags) const { return z == ssim_slice ? flags : 0; }
    __device__ void load(int z, int gi, int e, int H, int W, uint8_t& xa, uint8_t& xb) const {
        const size_t o = (size_t)gi * (size_t)W + e;
        xa = a[z][o];
        xb = b[z][o];
    }
};

struct PlaneSlots { int first[3], count[3]; };       // the workspace slots of the Y, U and V planes

bool overlap(const void* a, uint64_t na, const void* b, uint64_t nb) {
    return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na;
}

void chroma_shape(int H, int W, int chroma, int& ch, int& cw) {
    ch = chroma == BINSCORE_CHROMA_444 ? H : (H + 1) / 2;
    cw = chroma == BINSCORE_CHROMA_444 ? W : (W + 1) / 2;
}

int score_shape(int H, int W, int chroma, int flags) {
    if (flags & ~(BINSCORE_SSIM_G11 | BINSCORE_SSIM_U7)) return BINSCORE_E_ARG;
    if (chroma != BINSCORE_CHROMA_420 && chroma != BINSCORE_CHROMA_444) return BINSCORE_E_ARG;
    if (H <= 0 || W <= 0 || H > 65535 || W > 65535) return BINSCORE_E_SHAPE;
    if ((flags & BINSCORE_SSIM_G11) && (H < 11 || W < 11)) return BINSCORE_E_SHAPE;
    if ((flags & BINSCORE_SSIM_U7) && (H < 7 || W < 7)) return BINSCORE_E_SHAPE;
    return 0;
}

size_t plane_slots(int H, int W) { return (size_t)sc_tiles_y(H) * sc_tiles_x<PlanePairs>(W); }
}  // namespace

// one workgroup: the slots of each plane in a fixed order, then the record
__global__ void __launch_bounds__(256)
plane_score_final_kernel(const ScorePartial* __restrict__ part, PlaneSlots slots, int H, int W, int flags, BinPlaneScores* __restrict__ out) {
    __shared__ long long sl[6][256];
    __shared__ double sd[2][256];
    const int t = threadIdx.x;
    long long acc[6] = {0, 0, 0, 0, 0, 0};
    double g = 0.0, u = 0.0;
    for (int p = 0; p < 3; ++p) {
        const ScorePartial* q = part + slots.first[p];
        for (int s = t; s < slots.count[p]; s += 256) {
            acc[p] += q[s].sse;
            acc[3 + p] += q[s].sad;
            if (p == 0) {                            // the Y plane's launch has it in slice 0: channel 0 of its slots
                g += q[s].g11[0];
                u += q[s].u7[0];
            }
        }
    }
    for (int c = 0; c < 6; ++c) sl[c][t] = acc[c];
    sd[0][t] = g;
    sd[1][t] = u;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            for (int c = 0; c < 6; ++c) sl[c][t] += sl[c][t + o];
            sd[0][t] += sd[0][t + o];
            sd[1][t] += sd[1][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        const double nan = __builtin_nan("");
        BinPlaneScores r;
        for (int p = 0; p < 3; ++p) {
            r.sse[p] = (uint64_t)sl[p][0];
            r.sad[p] = (uint64_t)sl[3 + p][0];
        }
        // the mean of the valid map (util.calculate_ssim, compare_ssim on a 2-D array)
        const double ng = (double)(H - 10) * (double)(W - 10), nu = (double)(H - 6) * (double)(W - 6);
        r.ssim_g11 = (flags & BINSCORE_SSIM_G11) ? sd[0][0] / ng : nan;
        r.ssim_u7 = (flags & BINSCORE_SSIM_U7) ? sd[1][0] / nu : nan;
        *out = r;
    }
}

int binscore_version(void) { return BINSCORE_VERSION; }

size_t binscore_workspace_bytes(int H, int W, int chroma, int flags) {
    if (score_shape(H, W, chroma, flags) != 0) return 0;
    int ch, cw;
    chroma_shape(H, W, chroma, ch, cw);
    return (plane_slots(H, W) + 2 * plane_slots(ch, cw)) * sizeof(ScorePartial);
}

int binscore_planes(const uint8_t* ay, const uint8_t* au, const uint8_t* av, const uint8_t* by, const uint8_t* bu, const uint8_t* bv,
                    int H, int W, int chroma, int flags, const double* g11_taps, void* ws, size_t ws_bytes, BinPlaneScores* out,
                    void* stream) {
    if (!ay || !au || !av || !by || !bu || !bv || !ws || !out) return BINSCORE_E_ARG;
    if (((uintptr_t)out & 7) || ((uintptr_t)ws & 7)) return BINSCORE_E_ARG;
    const int rc = score_shape(H, W, chroma, flags);
    if (rc != 0) return rc;
    if ((flags & BINSCORE_SSIM_G11) && !g11_taps) return BINSCORE_E_ARG;
    const size_t need = binscore_workspace_bytes(H, W, chroma, flags);
    if (ws_bytes < need) return BINSCORE_E_WORKSPACE;
    int ch, cw;
    chroma_shape(H, W, chroma, ch, cw);
    const uint64_t ny = (uint64_t)H * W, nc = (uint64_t)ch * cw;
    const void* planes[6] = {ay, au, av, by, bu, bv};
    const uint64_t bytes[6] = {ny, nc, nc, ny, nc, nc};
    for (int i = 0; i < 6; ++i)
        if (overlap(out, sizeof(BinPlaneScores), planes[i], bytes[i]) || overlap(ws, need, planes[i], bytes[i])) return BINSCORE_E_ARG;
    if (overlap(out, sizeof(BinPlaneScores), ws, need)) return BINSCORE_E_ARG;

    ScoreTaps taps{};
    if (flags & BINSCORE_SSIM_G11)
        for (int k = 0; k < 11; ++k) taps.w[k] = g11_taps[k];
    hipStream_t s = (hipStream_t)stream;
    ScorePartial* part = (ScorePartial*)ws;
    const int ty = sc_tiles_y(H), tx = sc_tiles_x<PlanePairs>(W), tcy = sc_tiles_y(ch), tcx = sc_tiles_x<PlanePairs>(cw);
    const PlaneSlots slots{{0, ty * tx, ty * tx + tcy * tcx}, {ty * tx, tcy * tcx, tcy * tcx}};
    if (ch == H && cw == W) {                        // one shape: the three planes are the slices of one launch
        const PlanePairs ld{{ay, au, av}, {by, bu, bv}, 0};
        hipLaunchKernelGGL(score_tile_kernel<PlanePairs>, dim3(tx, ty, 3), dim3(SC_THREADS), 0, s, ld, H, W, flags, taps, part);
    } else {
        const PlanePairs ly{{ay, nullptr, nullptr}, {by, nullptr, nullptr}, 0};
        hipLaunchKernelGGL(score_tile_kernel<PlanePairs>, dim3(tx, ty, 1), dim3(SC_THREADS), 0, s, ly, H, W, flags, taps, part);
        const PlanePairs lc{{au, av, nullptr}, {bu, bv, nullptr}, -1};
        hipLaunchKernelGGL(score_tile_kernel<PlanePairs>, dim3(tcx, tcy, 2), dim3(SC_THREADS), 0, s, lc, ch, cw, 0, taps,
                           part + slots.first[1]);
    }
    hipLaunchKernelGGL(plane_score_final_kernel, dim3(1), dim3(256), 0, s, part, slots, H, W, flags, out);
    return (int)hipGetLastError();
}
