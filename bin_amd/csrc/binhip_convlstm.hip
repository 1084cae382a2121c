// binhip_convlstm.hip — ConvLSTMCell (RDN.py:50-95), fp32 NCHW:
//   * the (3, 3) cell of the live path as ONE fused kernel (conv 6 -> 12 + gates) and its three-pass backward (gates, input, weights);
//     the gate path is one template over the pixels a thread owns (PIX = 4: rows of whole float4s on 16-byte aligned planes; PIX = 1: the rest)
//   * the elementwise gate kernels of cells of any other size, whose gates conv runs on the general convolution kernels
#include "binhip_internal.h"
#include "binhip_reduce.h"

// ---- ConvLSTM cell ------------------------------------------------------------------------------
__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }
// The per-pixel gate arithmetic of the cell (RDN.py:74-92) and of its backward, with the multiply-adds spelled out (fmaf /
// __fmul_rn) so that both widths of the gate path compile to the same roundings.
__device__ __forceinline__ void lstm_point_fwd(float gi, float gj, float gf, float go, float cprev, float fb, float& c1, float& h1) {
    c1 = fmaf(cprev, sigmoidf_(gf + fb), __fmul_rn(sigmoidf_(gi), tanhf(gj)));
    h1 = __fmul_rn(tanhf(c1), sigmoidf_(go));
}
__device__ __forceinline__ void lstm_point_bwd(float gi, float gj, float gf, float go, float cprev, float fb, float ghv, float gcv,
                                               float& di, float& dj, float& df, float& dob, float& dcp) {
    const float si = sigmoidf_(gi), tj = tanhf(gj), sf = sigmoidf_(gf + fb), so = sigmoidf_(go);
    const float c1 = fmaf(cprev, sf, __fmul_rn(si, tj));
    const float tc = tanhf(c1);
    const float gct = fmaf(__fmul_rn(ghv, so), fmaf(-tc, tc, 1.f), gcv);
    di = __fmul_rn(__fmul_rn(gct, tj), __fmul_rn(si, 1.f - si));
    dj = __fmul_rn(__fmul_rn(gct, si), fmaf(-tj, tj, 1.f));
    df = __fmul_rn(__fmul_rn(gct, cprev), __fmul_rn(sf, 1.f - sf));
    dob = __fmul_rn(__fmul_rn(ghv, tc), __fmul_rn(so, 1.f - so));
    dcp = __fmul_rn(gct, sf);
}

// ---- the gate path of the fused cell, forward and backward pass 1: ONE definition, PIX = pixels per thread --------------------------
// A thread owns PIX consecutive pixels of a row.  Per (channel, row) it loads the PIX pixels (PIX = 4: one 16-byte load; PIX = 1: one
// scalar) and the two edge scalars, which serve 3 taps x PIX pixels; the 12 gate weights of a tap are three ds_read_b128 (LDS layout
// [channel][tap][gate]) reused by every pixel; and EVERY load of the epilogue (c_prev; in the backward also g_h, g_c) is issued and
// pinned before the first store: loads and stores share vmcnt on gfx9, so a load issued between stores waits for the stores before it
// (the one-pixel kernel that did so ran at 36.9 us per 768x1344 cell = 1.0 TB/s of a 37 MB pass).  Only the row load and the vector
// width of the epilogue depend on PIX.
// Each pixel's fmaf chain runs in the order bias, then channel, dy, dx, and an out-of-image tap contributes fma(w, 0, g), so the two
// widths agree bit for bit.  fma(w, 0, g) = g for every finite w, which is what skipping the tap would give; the two rules differ only
// for a non-finite weight (w * 0 = NaN) and for a bias of -0.0 (-0.0 + 0 = +0.0).  A PIX = 1 kernel that skipped such taps (as the
// one-pixel kernels before this template did) disagrees there with the PIX = 4 kernel on the same data, so one rule serves both.
#define CL_NW (12 * 6 * 9)        // gate weights; the 12 biases follow them in LDS
__device__ __forceinline__ void convlstm_stage_weights(float* ws, const float* __restrict__ w, const float* __restrict__ b) {
    for (int i = threadIdx.x; i < CL_NW + 12; i += blockDim.x) {
        if (i < CL_NW) {
            const int o = i / 54, r = i % 54;              // w[(o * 6 + ci) * 9 + tap]  ->  ws[(ci * 9 + tap) * 12 + o]
            ws[r * 12 + o] = w[i];
        } else {
            ws[i] = b[i - CL_NW];
        }
    }
}
// PIX floats at p + o, one vector access for PIX = 4
template <int PIX>
__device__ __forceinline__ void ld_px(const float* p, long long o, float (&v)[PIX]) {
    if constexpr (PIX == 4) {
        const float4 q = *reinterpret_cast<const float4*>(p + o);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        v[0] = p[o];
    }
}
template <int PIX>
__device__ __forceinline__ void ld_px_or_zero(const float* p, long long o, float (&v)[PIX]) {
    if (p) {
        ld_px<PIX>(p, o, v);
    } else {
#pragma unroll
        for (int i = 0; i < PIX; ++i) v[i] = 0.f;
    }
}
template <int PIX>
__device__ __forceinline__ void st_px(float* p, long long o, const float (&v)[PIX]) {
    if constexpr (PIX == 4) *reinterpret_cast<float4*>(p + o) = float4{v[0], v[1], v[2], v[3]};
    else p[o] = v[0];
}
template <int PIX>
__device__ __forceinline__ void pin_px(float (&v)[PIX]) {
    if constexpr (PIX == 4) asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
    else asm volatile("" : "+v"(v[0]));
}
// thread -> image n, row y, first pixel x0; false past the end
template <int PIX>
__device__ __forceinline__ bool convlstm_decode(int N, int H, int W, int& n, int& y, int& x0) {
    const int WP = W / PIX;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * H * WP) return false;
    const int xq = (int)(t % WP);
    y = (int)((t / WP) % H);
    n = (int)(t / ((long long)WP * H));
    x0 = xq * PIX;
    return true;
}
template <int PIX>
__device__ __forceinline__ void convlstm_gates(const float* __restrict__ x, const float* __restrict__ hp, const float* ws,
                                               int n, int y, int x0, int H, int W, long long HW, float (&g)[12][PIX]) {
#pragma unroll
    for (int o = 0; o < 12; ++o)
#pragma unroll
        for (int p = 0; p < PIX; ++p) g[o][p] = ws[CL_NW + o];
    const int nin = hp ? 6 : 3;
#pragma unroll 1
    for (int ci = 0; ci < nin; ++ci) {
        const float* src = (ci < 3) ? (x + ((long long)n * 3 + ci) * HW) : (hp + ((long long)n * 3 + (ci - 3)) * HW);
        float v[3][PIX + 2];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {                   // the three rows' loads first, then their 9 x 12 x PIX fmas
            const int yy = y + dy - 1;
            const bool ok = yy >= 0 && yy < H;
            const float* r = src + (long long)(ok ? yy : y) * W + x0;          // (an out-of-image row reads row y: in bounds, unused)
            float c[PIX];
            ld_px<PIX>(r, 0, c);
            const float l = (x0 > 0) ? r[-1] : 0.f, rt = (x0 + PIX < W) ? r[PIX] : 0.f;
            v[dy][0] = ok ? l : 0.f;
#pragma unroll
            for (int p = 0; p < PIX; ++p) v[dy][1 + p] = ok ? c[p] : 0.f;
            v[dy][PIX + 1] = ok ? rt : 0.f;
        }
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const float4* wq = reinterpret_cast<const float4*>(ws + ((ci * 9) + dy * 3 + dx) * 12);
                const float4 w0 = wq[0], w1 = wq[1], w2 = wq[2];
                const float wv[12] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w, w2.x, w2.y, w2.z, w2.w};
#pragma unroll
                for (int o = 0; o < 12; ++o)
#pragma unroll
                    for (int p = 0; p < PIX; ++p) g[o][p] = fmaf(wv[o], v[dy][p + dx], g[o][p]);
            }
    }
}

template <int PIX>
__global__ void __launch_bounds__(256)
convlstm_kernel(const float* __restrict__ x, const float* __restrict__ cp, const float* __restrict__ hp,
                const float* __restrict__ w, const float* __restrict__ b, float fb, int N, int H, int W,
                float* __restrict__ cn, float* __restrict__ hn) {
    __shared__ __attribute__((aligned(16))) float ws[CL_NW + 12];
    convlstm_stage_weights(ws, w, b);
    __syncthreads();
    const long long HW = (long long)H * W;
    int n, y, x0;
    if (!convlstm_decode<PIX>(N, H, W, n, y, x0)) return;
    float g[12][PIX];
    convlstm_gates<PIX>(x, hp, ws, n, y, x0, H, W, HW, g);
    const long long o0 = ((long long)n * 3) * HW + (long long)y * W + x0;
    float cprev[3][PIX];
#pragma unroll
    for (int k = 0; k < 3; ++k) ld_px_or_zero<PIX>(cp, o0 + k * HW, cprev[k]);
#pragma unroll
    for (int k = 0; k < 3; ++k) pin_px<PIX>(cprev[k]);
    __builtin_amdgcn_sched_barrier(0);
    float c1[3][PIX], h1[3][PIX];
#pragma unroll
    for (int k = 0; k < 3; ++k)             // i = g[0:3], j = g[3:6], f = g[6:9], o = g[9:12]  (RDN.py:79)
#pragma unroll
        for (int p = 0; p < PIX; ++p) lstm_point_fwd(g[k][p], g[3 + k][p], g[6 + k][p], g[9 + k][p], cprev[k][p], fb, c1[k][p], h1[k][p]);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (cn) st_px<PIX>(cn, o0 + k * HW, c1[k]);
        st_px<PIX>(hn, o0 + k * HW, h1[k]);
    }
}

// ---- ConvLSTM backward -----------------------------------------------------------------------------
// pass 1: recompute the gates per pixel, emit dgates [N,12,H,W] (i,j,f,o order) and gc_prev
template <int PIX>
__global__ void __launch_bounds__(256)
convlstm_bwd_gates_kernel(const float* __restrict__ x, const float* __restrict__ cp, const float* __restrict__ hp,
                          const float* __restrict__ w, const float* __restrict__ b, float fb, int N, int H, int W,
                          const float* __restrict__ gh, const float* __restrict__ gc, float* __restrict__ dgates,
                          float* __restrict__ gcp) {
    __shared__ __attribute__((aligned(16))) float ws[CL_NW + 12];
    convlstm_stage_weights(ws, w, b);
    __syncthreads();
    const long long HW = (long long)H * W;
    int n, y, x0;
    if (!convlstm_decode<PIX>(N, H, W, n, y, x0)) return;
    float g[12][PIX];
    convlstm_gates<PIX>(x, hp, ws, n, y, x0, H, W, HW, g);
    const long long pix = (long long)y * W + x0;
    const long long o0 = ((long long)n * 3) * HW + pix;
    float cprev[3][PIX], ghv[3][PIX], gcv[3][PIX];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        ld_px_or_zero<PIX>(cp, o0 + k * HW, cprev[k]);
        ld_px_or_zero<PIX>(gh, o0 + k * HW, ghv[k]);
        ld_px_or_zero<PIX>(gc, o0 + k * HW, gcv[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) { pin_px<PIX>(cprev[k]); pin_px<PIX>(ghv[k]); pin_px<PIX>(gcv[k]); }
    __builtin_amdgcn_sched_barrier(0);
    const long long d0 = ((long long)n * 12) * HW + pix;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float di[PIX], dj[PIX], df[PIX], dob[PIX], dcp[PIX];
#pragma unroll
        for (int p = 0; p < PIX; ++p)
            lstm_point_bwd(g[k][p], g[3 + k][p], g[6 + k][p], g[9 + k][p], cprev[k][p], fb, ghv[k][p], gcv[k][p], di[p], dj[p], df[p], dob[p], dcp[p]);
        st_px<PIX>(dgates, d0 + (long long)(k) * HW, di);
        st_px<PIX>(dgates, d0 + (long long)(3 + k) * HW, dj);
        st_px<PIX>(dgates, d0 + (long long)(6 + k) * HW, df);
        st_px<PIX>(dgates, d0 + (long long)(9 + k) * HW, dob);
        if (gcp) st_px<PIX>(gcp, o0 + k * HW, dcp);
    }
}
// pass 2: dx / dh_prev = conv_transpose(dgates, w)
__global__ void __launch_bounds__(256)
convlstm_bwd_input_kernel(const float* __restrict__ dgates, const float* __restrict__ w, int N, int H, int W,
                          float* __restrict__ gx, float* __restrict__ ghp) {
    __shared__ float ws[648];
    for (int i = threadIdx.x; i < 648; i += blockDim.x) ws[i] = w[i];
    __syncthreads();
    const long long HW = (long long)H * W;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (long long)N * HW) return;
    const int n = (int)(t / HW);
    const long long pix = t - (long long)n * HW;
    const int y = (int)(pix / W), xx = (int)(pix - (long long)y * W);
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
        const int yy = y - (dy - 1);
        if (yy < 0 || yy >= H) continue;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) {
            const int xq = xx - (dx - 1);
            if (xq < 0 || xq >= W) continue;
            for (int o = 0; o < 12; ++o) {
                const float d = dgates[((long long)n * 12 + o) * HW + (long long)yy * W + xq];
#pragma unroll
                for (int ci = 0; ci < 6; ++ci) acc[ci] = fmaf(ws[(o * 6 + ci) * 9 + dy * 3 + dx], d, acc[ci]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const long long o = ((long long)n * 3 + k) * HW + pix;
        if (gx) gx[o] = acc[k];
        if (ghp) ghp[o] = acc[3 + k];
    }
}
// pass 3: dW / db partials per pixel strip (LDS tiles), then a fixed-order final sum
#define CL_TW 64
#define CL_TH 8
__global__ void __launch_bounds__(256)
convlstm_bwd_weight_kernel(const float* __restrict__ dgates, const float* __restrict__ x, const float* __restrict__ hp,
                           int N, int H, int W, int tiles_x, int tiles_y, float* __restrict__ partials) {
    __shared__ float sd[12][CL_TH][CL_TW];
    __shared__ float sx[6][CL_TH + 2][CL_TW + 2];
    int b = blockIdx.x;
    const int tx = b % tiles_x; b /= tiles_x;
    const int ty = b % tiles_y;
    const int n = b / tiles_y;
    const int x0 = tx * CL_TW, y0 = ty * CL_TH;
    const long long HW = (long long)H * W;
    for (int i = threadIdx.x; i < 12 * CL_TH * CL_TW; i += 256) {
        const int o = i / (CL_TH * CL_TW), r = (i / CL_TW) % CL_TH, c = i % CL_TW;
        const int yy = y0 + r, xx = x0 + c;
        sd[o][r][c] = (yy < H && xx < W) ? dgates[((long long)n * 12 + o) * HW + (long long)yy * W + xx] : 0.f;
    }
    // (no previous state — every cell of bin_stage4's two-window schedule, RDN.py:57-68 — means the recurrent half of the gates
    //  conv saw zeros: its 324 weight gradients are exactly zero and neither their inputs nor their sums are formed; round 5)
    const int nci = hp ? 6 : 3;
    for (int i = threadIdx.x; i < nci * (CL_TH + 2) * (CL_TW + 2); i += 256) {
        const int ci = i / ((CL_TH + 2) * (CL_TW + 2)), r = (i / (CL_TW + 2)) % (CL_TH + 2), c = i % (CL_TW + 2);
        const int yy = y0 + r - 1, xx = x0 + c - 1;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
            if (ci < 3) v = x[((long long)n * 3 + ci) * HW + (long long)yy * W + xx];
            else if (hp) v = hp[((long long)n * 3 + (ci - 3)) * HW + (long long)yy * W + xx];
        }
        sx[ci][r][c] = v;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 660; k += 256) {
        float acc = 0.f;
        if (k < 648) {
            const int o = k / 54, ci = (k / 9) % 6, dy = (k % 9) / 3, dx = k % 3;
            if (ci < nci)
                for (int r = 0; r < CL_TH; ++r)
                    for (int c = 0; c < CL_TW; ++c) acc = fmaf(sd[o][r][c], sx[ci][r + dy][c + dx], acc);
        } else {
            const int o = k - 648;
            for (int r = 0; r < CL_TH; ++r)
                for (int c = 0; c < CL_TW; ++c) acc += sd[o][r][c];
        }
        partials[(long long)blockIdx.x * 660 + k] = acc;
    }
}
// one 256-thread block per output k (648 weights + 12 biases): thread t adds the partials t, t + 256, ... in double, the
// 256 sums are combined by a fixed tree -> deterministic (a single thread per output walking all `nb` partials took 250 us)
__global__ void __launch_bounds__(256)
convlstm_bwd_weight_final_kernel(const float* __restrict__ partials, int nb, float* __restrict__ dw, float* __restrict__ db) {
    const int k = blockIdx.x;
    const double s = block_reduce_strided(nb, 0.0, [&](int i) { return (double)partials[(long long)i * 660 + k]; }, BhAdd());
    if (threadIdx.x == 0) {
        if (k < 648) dw[k] = (float)s; else db[k - 648] = (float)s;
    }
}

// ---- ConvLSTM gate arithmetic for cells OTHER than the (3, 3) cell of the live path (reference RDN.py:74-82, any
// input_size / hidden_size: RDN.py:14-24).  The gates conv of such a cell runs on the general convolution kernels; these two
// elementwise kernels are the rest: gates [N, 4h, H, W] (i, j, f, o) -> c', h' and its backward.
// (They associate their products differently from lstm_point_* above — dc * tj * si * (1 - si) against (gct * tj) * (si * (1 - si)) —
// so they stay separate: routing them through lstm_point_* would change their bits.)
__global__ void __launch_bounds__(256)
lstm_gates_fwd_kernel(const float* __restrict__ gates, const float* __restrict__ cp, float fb, int hid, long long HW,
                      long long total, float* __restrict__ cn, float* __restrict__ hn) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;          // over [N, hid, H, W]
    if (t >= total) return;
    const long long chw = (long long)hid * HW;
    const long long n = t / chw, r = t - n * chw;
    const float* g = gates + n * 4 * chw + r;
    const float cprev = cp ? cp[t] : 0.f;
    const float c1 = cprev * sigmoidf_(g[2 * chw] + fb) + sigmoidf_(g[0]) * tanhf(g[chw]);
    cn[t] = c1;
    hn[t] = tanhf(c1) * sigmoidf_(g[3 * chw]);
}
__global__ void __launch_bounds__(256)
lstm_gates_bwd_kernel(const float* __restrict__ gates, const float* __restrict__ cp, const float* __restrict__ gh,
                      const float* __restrict__ gc, float fb, int hid, long long HW, long long total,
                      float* __restrict__ dg, float* __restrict__ gcp) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long chw = (long long)hid * HW;
    const long long n = t / chw, r = t - n * chw;
    const float* g = gates + n * 4 * chw + r;
    float* d = dg + n * 4 * chw + r;
    const float cprev = cp ? cp[t] : 0.f;
    const float si = sigmoidf_(g[0]), tj = tanhf(g[chw]), sf = sigmoidf_(g[2 * chw] + fb), so = sigmoidf_(g[3 * chw]);
    const float c1 = cprev * sf + si * tj;
    const float tc = tanhf(c1);
    const float ghv = gh ? gh[t] : 0.f;
    const float dc = (gc ? gc[t] : 0.f) + ghv * so * (1.f - tc * tc);
    d[0] = dc * tj * si * (1.f - si);
    d[chw] = dc * si * (1.f - tj * tj);
    d[2 * chw] = dc * cprev * sf * (1.f - sf);
    d[3 * chw] = ghv * tc * so * (1.f - so);
    if (gcp) gcp[t] = dc * sf;
}


extern "C" {

// PIX = 4 needs rows of whole float4s and every plane pointer 16-byte aligned (null = absent = fine)
static inline bool convlstm_vec4_ok(int W, const void* a, const void* b, const void* c, const void* d, const void* e, const void* f,
                                    const void* g) {
    uintptr_t m = 0;
    for (const void* p : {a, b, c, d, e, f, g}) m |= (uintptr_t)p;
    return (W & 3) == 0 && (m & 15) == 0;
}

int binhip_convlstm_fwd(const float* x, const float* c_prev, const float* h_prev, const float* w, const float* b,
                        float forget_bias, int N, int H, int W, float* c_new, float* h_new, void* stream) {
    if (!x || !w || !b || !h_new) return BINHIP_E_ARG;
    if ((c_prev == nullptr) != (h_prev == nullptr)) return BINHIP_E_ARG;
    if (N <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    const long long total = (long long)N * H * W;
    if (convlstm_vec4_ok(W, x, c_prev, h_prev, c_new, h_new, nullptr, nullptr))
        hipLaunchKernelGGL(convlstm_kernel<4>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           x, c_prev, h_prev, w, b, forget_bias, N, H, W, c_new, h_new);
    else
        hipLaunchKernelGGL(convlstm_kernel<1>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           x, c_prev, h_prev, w, b, forget_bias, N, H, W, c_new, h_new);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_lstm_gates_fwd(const float* gates, const float* c_prev, float forget_bias, int N, int hidden, int H, int W,
                          float* c_new, float* h_new, void* stream) {
    if (!gates || !c_new || !h_new) return BINHIP_E_ARG;
    if (N <= 0 || hidden <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    const long long HW = (long long)H * W, total = (long long)N * hidden * HW;
    hipLaunchKernelGGL(lstm_gates_fwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gates,
                       c_prev, forget_bias, hidden, HW, total, c_new, h_new);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_lstm_gates_bwd(const float* gates, const float* c_prev, const float* g_h, const float* g_c, float forget_bias, int N,
                          int hidden, int H, int W, float* g_gates, float* g_cprev, void* stream) {
    if (!gates || !g_gates || (!g_h && !g_c)) return BINHIP_E_ARG;
    if (N <= 0 || hidden <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    const long long HW = (long long)H * W, total = (long long)N * hidden * HW;
    hipLaunchKernelGGL(lstm_gates_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, gates,
                       c_prev, g_h, g_c, forget_bias, hidden, HW, total, g_gates, g_cprev);
    BH_CHECK_LAUNCH();
    return 0;
}

size_t binhip_convlstm_bwd_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    const size_t tiles = (size_t)((W + CL_TW - 1) / CL_TW) * ((H + CL_TH - 1) / CL_TH) * N;
    return ((size_t)N * 12 * H * W + tiles * 660) * sizeof(float) + 256;
}

int binhip_convlstm_bwd(const float* x, const float* c_prev, const float* h_prev, const float* w, const float* b,
                        float forget_bias, int N, int H, int W, const float* g_h, const float* g_c, void* workspace,
                        size_t workspace_bytes, float* gx, float* g_hprev, float* g_cprev, float* dw, float* db,
                        void* stream) {
    if (!x || !w || !b || !workspace || (!g_h && !g_c)) return BINHIP_E_ARG;
    if ((c_prev == nullptr) != (h_prev == nullptr)) return BINHIP_E_ARG;
    if (N <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    if (workspace_bytes < binhip_convlstm_bwd_workspace_bytes(N, H, W)) return BINHIP_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    float* dg = (float*)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* part = dg + (size_t)N * 12 * H * W;
    const long long total = (long long)N * H * W;
    const unsigned nb = (unsigned)((total + 255) / 256);
    if (convlstm_vec4_ok(W, x, c_prev, h_prev, g_h, g_c, dg, g_cprev))
        hipLaunchKernelGGL(convlstm_bwd_gates_kernel<4>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, x, c_prev, h_prev,
                           w, b, forget_bias, N, H, W, g_h, g_c, dg, g_cprev);
    else
        hipLaunchKernelGGL(convlstm_bwd_gates_kernel<1>, dim3(nb), dim3(256), 0, s, x, c_prev, h_prev, w, b, forget_bias, N, H, W,
                           g_h, g_c, dg, g_cprev);
    if (gx || g_hprev)
        hipLaunchKernelGGL(convlstm_bwd_input_kernel, dim3(nb), dim3(256), 0, s, dg, w, N, H, W, gx, g_hprev);
    if (dw && db) {
        const int tiles_x = (W + CL_TW - 1) / CL_TW, tiles_y = (H + CL_TH - 1) / CL_TH;
        const int nblk = tiles_x * tiles_y * N;
        hipLaunchKernelGGL(convlstm_bwd_weight_kernel, dim3((unsigned)nblk), dim3(256), 0, s, dg, x, h_prev, N, H, W, tiles_x,
                           tiles_y, part);
        hipLaunchKernelGGL(convlstm_bwd_weight_final_kernel, dim3(660), dim3(256), 0, s, part, nblk, dw, db);
    }
    BH_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
