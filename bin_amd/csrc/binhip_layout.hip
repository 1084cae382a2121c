// binhip_layout.hip — the layout and frame glue of libbinhip.so, every kernel a one-pass copy (each input byte read once, each output
// byte written once):
//   * fp32 NCHW <-> fp16 chunk planes (nchw_to_planes, planes_to_nchw), the exact fp32 space-to-depth (pixel_unshuffle_f32)
//   * the RDN's input side: pixel_reshuffle(cat(frames), 2) straight into chunk planes (pack_inputs, RDN.py:107-132) and its inverse
//     with the mean skip path (unpack_input_grads); the inverse PixelShuffle on chunk planes (unshuffle_planes)
//   * the harness's u8 image <-> padded fp32 frame glue (u8_to_frame, frame_to_u8)
//   * binhip_version, binhip_device_cus
#include "binhip_internal.h"
#include <initializer_list>

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// ---- fp32 NCHW -> chunk planes -----------------------------------------------------------------
// one thread = one 16-byte slot (8 channels of one pixel)
__global__ void nchw_to_planes_kernel(const float* __restrict__ x, int N, int C, int H, int W,
                                      _Float16* __restrict__ y_hi, _Float16* __restrict__ y_lo,
                                      const float* __restrict__ scale, unsigned* __restrict__ flags) {
    const float sc = scale ? scale[0] : 1.f;
    const long long HW = (long long)H * W;
    const long long total = (long long)bh_chunks_dev(C) * N * HW * 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int s = (int)(t & 1);
    long long u = t >> 1;
    const long long pix = u % HW; u /= HW;
    const int n = (int)(u % N);
    const int ch = (int)(u / N);
    half8 hv, lv;
    unsigned sat = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * 16 + s * 8 + e;
        const float v = (c < C) ? x[((long long)n * C + c) * HW + pix] * sc : 0.f;
        hv[e] = split_hi(v, sat);
        lv[e] = split_lo(v, hv[e]);
    }
    *reinterpret_cast<half8*>(y_hi + t * 8) = hv;
    if (y_lo) *reinterpret_cast<half8*>(y_lo + t * 8) = lv;
    if (sat != 0 && flags) atomicOr(flags, BINHIP_FLAG_SATURATED);
}

// one thread = one (n, c, pixel) output element; reads are 2-byte gathers (test/boundary glue only)
__global__ void planes_to_nchw_kernel(const _Float16* __restrict__ x_hi, const _Float16* __restrict__ x_lo,
                                      int N, int C, int H, int W, float* __restrict__ y) {
    const long long HW = (long long)H * W;
    const long long total = (long long)N * C * HW;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long pix = t % HW;
    const int c = (int)((t / HW) % C);
    const int n = (int)(t / (HW * C));
    const long long o = (((long long)(c >> 4) * N + n) * HW + pix) * 16 + (c & 15);
    float v = (float)x_hi[o];
    if (x_lo) v += (float)x_lo[o];
    y[t] = v;
}

// ---- exact fp32 space-to-depth (the standalone pixel_reshuffle of the reference's API, RDN.py:107-132) --------------
__global__ void pixel_unshuffle_f32_kernel(const float* __restrict__ x, int N, int C, int H, int W, int r,
                                           float* __restrict__ y) {
    const int h = H / r, w = W / r;
    const long long total = (long long)N * C * H * W;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int ox = (int)(t % w);
    const int oy = (int)((t / w) % h);
    const int oc = (int)((t / ((long long)w * h)) % (C * r * r));
    const int n = (int)(t / ((long long)w * h * C * r * r));
    const int c = oc / (r * r), i = (oc / r) % r, j = oc % r;
    y[t] = x[(((long long)n * C + c) * H + (oy * r + i)) * W + (ox * r + j)];
}

// ---- K1: pixel_reshuffle(cat(images), 2) -> chunk planes at half resolution ---------------------
struct PackArgs {
    const float* img[5];
    int nimg, N, H, W;   // full-res H, W
};
__global__ void pack_inputs_kernel(PackArgs a, _Float16* __restrict__ y_hi, _Float16* __restrict__ y_lo,
                                   unsigned* __restrict__ flags) {
    const int h = a.H / 2, w = a.W / 2;
    const long long hw = (long long)h * w;
    const int C = 12 * a.nimg;
    const int nch = (C + 15) / 16;
    const long long total = (long long)nch * a.N * hw * 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int s = (int)(t & 1);
    long long u = t >> 1;
    const long long pix = u % hw; u /= hw;
    const int n = (int)(u % a.N);
    const int ch = (int)(u / a.N);
    const int y = (int)(pix / w), x = (int)(pix % w);
    half8 hv, lv;
    unsigned sat = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = ch * 16 + s * 8 + e;     // = 4*cc + 2*i + j   (RDN.py:128-132)
        float v = 0.f;
        if (c < C) {
            const int cc = c >> 2, i = (c >> 1) & 1, j = c & 1;
            const int im = cc / 3, rgb = cc - im * 3;
            v = a.img[im][(((long long)n * 3 + rgb) * a.H + (2 * y + i)) * a.W + (2 * x + j)];
        }
        hv[e] = split_hi(v, sat);
        lv[e] = split_lo(v, hv[e]);
    }
    *reinterpret_cast<half8*>(y_hi + t * 8) = hv;
    if (y_lo) *reinterpret_cast<half8*>(y_lo + t * 8) = lv;
    if (sat != 0 && flags) atomicOr(flags, BINHIP_FLAG_SATURATED);
}

// ---- harness glue: the per-frame host work of test.py moved onto the device -----------------
// u8 HWC BGR image -> fp32 CHW RGB in [0,1] (read_image, test.py:44-56) + ReplicationPad2d (test.py:348-371)
__global__ void u8_to_frame_kernel(const unsigned char* __restrict__ img, int H, int W, int pl, int pt, int Hp, int Wp,
                                   float* __restrict__ out) {
    const long long total = (long long)3 * Hp * Wp;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int x = (int)(t % Wp), y = (int)((t / Wp) % Hp), c = (int)(t / ((long long)Wp * Hp));
    int sy = y - pt, sx = x - pl;
    sy = sy < 0 ? 0 : (sy >= H ? H - 1 : sy);
    sx = sx < 0 ? 0 : (sx >= W ? W - 1 : sx);
    out[t] = (float)img[((long long)sy * W + sx) * 3 + (2 - c)] / 255.f;
}
// fp32 CHW RGB -> cropped u8 HWC BGR: clamp [0,1], x255, round-half-even (utils/util.py:113-137), crop (test.py:394-402)
__global__ void frame_to_u8_kernel(const float* __restrict__ x, int Hp, int Wp, int top, int left, int H, int W,
                                   unsigned char* __restrict__ out) {
    const long long total = (long long)H * W * 3;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int c = (int)(t % 3), xx = (int)((t / 3) % W), yy = (int)(t / (3LL * W));
    float v = x[((long long)(2 - c) * Hp + (yy + top)) * Wp + (xx + left)];
    v = fminf(fmaxf(v, 0.f), 1.f);
    out[t] = (unsigned char)rintf(v * 255.0f);
}

// ---- inverse PixelShuffle on chunk planes: [C/16] planes at 2H x 2W -> [4*C/16] planes at H x W, output chunk
// sub*(C/16) + c (the channel order UPNet.0's permuted rows use).  Pure 16-byte slot copy.
__global__ void unshuffle_planes_kernel(const _Float16* __restrict__ x, int N, int H, int W, int nch,
                                        _Float16* __restrict__ y) {
    const long long hw = (long long)H * W;
    const long long total = (long long)4 * nch * N * hw * 2;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const int s = (int)(t & 1);
    long long u = t >> 1;
    const long long pix = u % hw; u /= hw;
    const int n = (int)(u % N); u /= N;
    const int oc = (int)u;                       // output chunk = sub*nch + c
    const int sub = oc / nch, c = oc - sub * nch;
    const int yy = (int)(pix / W), xx = (int)(pix - (long long)yy * W);
    const long long src = ((((long long)c * N + n) * (2 * H) + (2 * yy + (sub >> 1))) * (2 * W) + (2 * xx + (sub & 1))) * 16 + s * 8;
    *reinterpret_cast<half8*>(y + t * 8) = *reinterpret_cast<const half8*>(x + src);
}

// ---- gradients w.r.t. the RDN's input frames: inverse of pack_inputs (pixel-shuffle of the SFENet1 input
// gradient) un-scaled, plus the mean skip path gout / k (RDN.py:221/279/333).
struct UnpackArgs {
    float* out[5];
    int nimg, N, H, W;
};
__global__ void unpack_input_grads_kernel(UnpackArgs a, const _Float16* __restrict__ g_hi, const _Float16* __restrict__ g_lo,
                                          const float* __restrict__ gout, const float* __restrict__ sc) {
    const long long HW = (long long)a.H * a.W;
    const long long total = (long long)a.N * 3 * HW;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const long long pix = t % HW;
    const int rgb = (int)((t / HW) % 3);
    const int n = (int)(t / (3 * HW));
    const int Y = (int)(pix / a.W), X = (int)(pix - (long long)Y * a.W);
    const int h = a.H / 2, w = a.W / 2;
    const float inv = sc ? sc[1] : 1.f;
    const float skip = gout[t] / (float)a.nimg;
    for (int im = 0; im < a.nimg; ++im) {
        if (!a.out[im]) continue;
        float v = skip;
        if (g_hi) {
            const int c = 4 * (im * 3 + rgb) + 2 * (Y & 1) + (X & 1);
            const long long o = ((((long long)(c >> 4) * a.N + n) * h + (Y >> 1)) * w + (X >> 1)) * 16 + (c & 15);
            float g = (float)g_hi[o];
            if (g_lo) g += (float)g_lo[o];
            v += g * inv;
        }
        a.out[im][t] = v;
    }
}


// Every launch below is one thread per 16-byte slot or per element, 256 to a block, and the runtime refuses a launch of 2^32 threads
// or more: `nb` = the blocks of f0 * f1 * .. threads (factors >= 1), or false when the launch would not fit (BINHIP_E_SHAPE; nothing
// a plan issues comes near it: include/binhip.h, "Launch limit of the layout entry points").
static bool bh_layout_blocks(unsigned* nb, std::initializer_list<long long> factors) {
    const long long limit = (1LL << 32) - 256;          // the largest thread count whose round-up to whole blocks stays below 2^32
    long long total = 1;
    for (long long f : factors) {
        if (f < 1 || total > limit / f) return false;   // (total * f > limit, without forming the product)
        total *= f;
    }
    *nb = (unsigned)((total + 255) / 256);
    return true;
}

extern "C" {

int binhip_version(void) { return BINHIP_VERSION; }

int binhip_device_cus(void) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1;
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return -1;
    return n;
}

int binhip_nchw_to_planes(const float* x, int N, int C, int H, int W, void* y_hi, void* y_lo, void* status, void* stream) {
    if (!x || !y_hi) return BINHIP_E_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {bh_chunks(C), N, H, W, 2})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(nchw_to_planes_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream,
                       x, N, C, H, W, (_Float16*)y_hi, (_Float16*)y_lo, (const float*)nullptr, (unsigned*)status);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_nchw_to_planes_scaled(const float* x, int N, int C, int H, int W, const float* scale, void* y_hi,
                                 void* y_lo, void* status, void* stream) {
    if (!x || !y_hi || !scale) return BINHIP_E_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {bh_chunks(C), N, H, W, 2})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(nchw_to_planes_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream,
                       x, N, C, H, W, (_Float16*)y_hi, (_Float16*)y_lo, scale, (unsigned*)status);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_planes_to_nchw(const void* x_hi, const void* x_lo, int N, int C, int H, int W, float* y, void* stream) {
    if (!x_hi || !y) return BINHIP_E_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return BINHIP_E_SHAPE;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {N, C, H, W})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(planes_to_nchw_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream,
                       (const _Float16*)x_hi, (const _Float16*)x_lo, N, C, H, W, y);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_pixel_unshuffle_f32(const float* x, int N, int C, int H, int W, int r, float* y, void* stream) {
    if (!x || !y) return BINHIP_E_ARG;
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || r < 1 || H % r || W % r) return BINHIP_E_SHAPE;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {N, C, H, W})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(pixel_unshuffle_f32_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, x,
                       N, C, H, W, r, y);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_pack_inputs(const float* const* images, int n_images, int N, int H, int W, void* y_hi, void* y_lo,
                       void* status, void* stream) {
    if (!images || !y_hi) return BINHIP_E_ARG;
    if (n_images < 1 || n_images > 5 || N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return BINHIP_E_SHAPE;
    PackArgs a;
    for (int i = 0; i < 5; ++i) a.img[i] = (i < n_images) ? images[i] : nullptr;
    for (int i = 0; i < n_images; ++i) if (!images[i]) return BINHIP_E_ARG;
    a.nimg = n_images; a.N = N; a.H = H; a.W = W;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {bh_chunks(12 * n_images), N, H / 2, W / 2, 2})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(pack_inputs_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream,
                       a, (_Float16*)y_hi, (_Float16*)y_lo, (unsigned*)status);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_u8_to_frame(const unsigned char* bgr_hwc, int H, int W, int pad_left, int pad_right, int pad_top,
                       int pad_bottom, float* out_chw, void* stream) {
    if (!bgr_hwc || !out_chw) return BINHIP_E_ARG;
    if (H <= 0 || W <= 0 || pad_left < 0 || pad_right < 0 || pad_top < 0 || pad_bottom < 0) return BINHIP_E_SHAPE;
    const int Hp = H + pad_top + pad_bottom, Wp = W + pad_left + pad_right;
    const long long total = (long long)3 * Hp * Wp;
    hipLaunchKernelGGL(u8_to_frame_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, bgr_hwc, H,
                       W, pad_left, pad_top, Hp, Wp, out_chw);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_frame_to_u8(const float* chw, int Hp, int Wp, int top, int left, int H, int W, unsigned char* bgr_hwc,
                       void* stream) {
    if (!chw || !bgr_hwc) return BINHIP_E_ARG;
    if (H <= 0 || W <= 0 || top < 0 || left < 0 || top + H > Hp || left + W > Wp) return BINHIP_E_SHAPE;
    const long long total = (long long)H * W * 3;
    hipLaunchKernelGGL(frame_to_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, chw, Hp, Wp,
                       top, left, H, W, bgr_hwc);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_unshuffle_planes(const void* x_hi, const void* x_lo, int N, int H, int W, int nchunks, void* y_hi, void* y_lo,
                            void* stream) {
    if (!x_hi || !y_hi || ((x_lo == nullptr) != (y_lo == nullptr))) return BINHIP_E_ARG;
    if (N <= 0 || H <= 0 || W <= 0 || nchunks <= 0) return BINHIP_E_SHAPE;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {4, nchunks, N, H, W, 2})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(unshuffle_planes_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x_hi, N, H, W,
                       nchunks, (_Float16*)y_hi);
    if (x_lo)
        hipLaunchKernelGGL(unshuffle_planes_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const _Float16*)x_lo, N, H,
                           W, nchunks, (_Float16*)y_lo);
    BH_CHECK_LAUNCH();
    return 0;
}

int binhip_unpack_input_grads(const void* gx0_hi, const void* gx0_lo, const float* gout, const float* scale,
                              int n_images, int N, int H, int W, float* const* outs, void* stream) {
    if (!gout || !outs) return BINHIP_E_ARG;
    if (n_images < 1 || n_images > 5 || N <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1)) return BINHIP_E_SHAPE;
    UnpackArgs a;
    for (int i = 0; i < 5; ++i) a.out[i] = (i < n_images) ? outs[i] : nullptr;
    a.nimg = n_images; a.N = N; a.H = H; a.W = W;
    unsigned nb;
    if (!bh_layout_blocks(&nb, {N, 3, H, W})) return BINHIP_E_SHAPE;
    hipLaunchKernelGGL(unpack_input_grads_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream,
                       a, (const _Float16*)gx0_hi, (const _Float16*)gx0_lo, gout, scale);
    BH_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
