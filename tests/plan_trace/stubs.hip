// Recording stand-ins for everything bin_amd/csrc/binhip_plan.hip calls (tests/test_cpu_plan_trace.py): the project's launchers
// and queries and the five HIP runtime entry points.  Each prints ONE line: its name, the stream, every scalar argument, every
// pointer as a hex number and every field of a BhConvCall / BinConvDesc / BhWgradReduce.  Nothing is dereferenced but those call
// structs and the host arrays of pointers (printed element by element: their own addresses differ from run to run).  No GPU, no
// HIP runtime.
#include "binhip_conv_common.h"
#include <cstdio>
#include <cstring>

#define X(p) ((unsigned long long)(uintptr_t)(p))

int g_rdb3_rc = 0;          // what bh_launch_rdb3_x3 answers (the driver sets BINHIP_E_SHAPE for the per-conv fallback)
static int n_events = 0;    // fake events are numbered in creation order

static void desc(const BinConvDesc& d) {
    printf(" d{N%d H%d W%d k%d cin%d cout%d pad%d nt%d epi%d relu%d cpg%d gs%lld nimg%d rsv%d st%llx}", d.N, d.H, d.W, d.ksize,
           d.cin_chunks, d.cout, d.cout_pad, d.nterms, d.epilogue, d.relu, d.x_cpg, (long long)d.x_group_stride, d.n_images,
           d.reserved, X(d.status));
}
static void call(const char* what, const BhConvCall& c) {
    printf("%s", what);
    desc(c.d);
    printf(" x%llx/%llx w%llx/%llx b%llx r%llx/%llx r2%llx/%llx m%llx rch%d mf%d ycpg%d ygs%lld yu%d y%llx/%llx f32%llx img", X(c.x_hi),
           X(c.x_lo), X(c.w_hi), X(c.w_lo), X(c.bias), X(c.r_hi), X(c.r_lo), X(c.r2_hi), X(c.r2_lo), X(c.m_hi), c.res_chunks,
           c.mask_from, c.y_cpg, (long long)c.y_group_stride, c.y_unshuf, X(c.y_hi), X(c.y_lo), X(c.y_f32));
    for (int i = 0; i < 5; ++i) printf(" %llx", X(c.images[i]));
    printf(" st%llx prof%llx\n", X(c.status), X(c.prof));
}
static void ptrs(const char* tag, const void* const* a, int n) {
    printf(" %s[", tag);
    for (int i = 0; a && i < n; ++i) printf(i ? " %llx" : "%llx", X(a[i]));
    printf("]");
}

int bh_launch_conv(const BhConvCall& c, hipStream_t s) {
    printf("[s%llx] ", X(s));
    call("conv", c);
    return 0;
}
// the three-phase launch gets kernel argument blocks: keep what identifies the call, so that its line shows which three it got
int bh_prepare_conv(const BhConvCall& c, ConvKArgs* out) {
    call("prepare_conv", c);
    memset(out, 0, sizeof(*out));
    out->x_hi = (const _Float16*)c.x_hi; out->w_hi = (const _Float16*)c.w_hi; out->y_hi = (_Float16*)c.y_hi;
    out->wt = 1;
    return 0;
}
int bh_launch_rdb3_x3(const ConvKArgs* k, unsigned* flags, unsigned epoch, int cus, hipStream_t s) {
    printf("[s%llx] rdb3_x3", X(s));
    for (int i = 0; i < 3; ++i) printf(" (x%llx w%llx y%llx)", X(k[i].x_hi), X(k[i].w_hi), X(k[i].y_hi));
    printf(" flags%llx epoch%u cus%d -> %d\n", X(flags), epoch, cus, g_rdb3_rc);
    return g_rdb3_rc;
}
int bh_launch_upnet_ring(const void* x_hi, const void* x_lo, const float* wvar, const float* bvar, float* out, const float* const* images,
                         int nimg, int N, int H, int W, int cin, hipStream_t s) {
    printf("[s%llx] upnet_ring x%llx/%llx w%llx b%llx out%llx", X(s), X(x_hi), X(x_lo), X(wvar), X(bvar), X(out));
    ptrs("img", (const void* const*)images, nimg);
    printf(" nimg%d N%d H%d W%d cin%d\n", nimg, N, H, W, cin);
    return 0;
}
bool bh_prof_begin(BinhipProfiler* pr, int ks, int cout_pad, int epi, hipStream_t s) {
    printf("[s%llx] prof_begin %llx k%d cout%d epi%d\n", X(s), X(pr), ks, cout_pad, epi);
    return pr != nullptr;
}
void bh_prof_end(BinhipProfiler* pr, hipStream_t s) { printf("[s%llx] prof_end %llx\n", X(s), X(pr)); }
int bh_upnet_gsub(const float* g, int N, int H, int W, const float* scale, void* y_hi, void* y_lo, void* status, hipStream_t s) {
    printf("[s%llx] upnet_gsub g%llx N%d H%d W%d sc%llx y%llx/%llx st%llx\n", X(s), X(g), N, H, W, X(scale), X(y_hi), X(y_lo), X(status));
    return 0;
}
int bh_upnet_ring_dgrad(const float* g, const float* wvar, const float* scale, void* gx_hi, void* gx_lo, void* status, int N, int H, int W,
                        int cin, hipStream_t s) {
    printf("[s%llx] upnet_ring_dgrad g%llx w%llx sc%llx gx%llx/%llx st%llx N%d H%d W%d cin%d\n", X(s), X(g), X(wvar), X(scale), X(gx_hi),
           X(gx_lo), X(status), N, H, W, cin);
    return 0;
}
int bh_upnet_ring_wgrad(const float* g, const void* x_hi, const void* x_lo, float* dwvar, float* dbvar, int N, int H, int W, int cin,
                        int accumulate, hipStream_t s) {
    printf("[s%llx] upnet_ring_wgrad g%llx x%llx/%llx dw%llx db%llx N%d H%d W%d cin%d acc%d\n", X(s), X(g), X(x_hi), X(x_lo), X(dwvar),
           X(dbvar), N, H, W, cin, accumulate);
    return 0;
}
static void reduce_item(const BhWgradReduce& r) {
    printf(" (p%llx pb%llx dw%llx db%llx rows%lld PB%d ncp%d ncot%d k%d tr%d cout%d cin%d sh%d)", X(r.partial), X(r.partial_b), X(r.dw),
           X(r.db), r.nrows, r.PB, r.ncp, r.ncot, r.ks, r.tr, r.cout, r.cin, r.shuffle);
}
int bh_wgrad_partials(const BinConvDesc* d, const void* x_hi, const void* x_lo, const void* gy_hi, const void* gy_lo, void* workspace,
                      size_t workspace_bytes, float* dw_oihw, float* dbias, int cin, int shuffle_perm, BhWgradReduce* out, void* stream) {
    printf("[s%llx] wgrad_partials", X(stream));
    desc(*d);
    printf(" x%llx/%llx gy%llx/%llx ws%llx+%zu dw%llx db%llx cin%d sh%d\n", X(x_hi), X(x_lo), X(gy_hi), X(gy_lo), X(workspace),
           workspace_bytes, X(dw_oihw), X(dbias), cin, shuffle_perm);
    // the reduction item, from the arguments alone
    out->partial = (const float*)workspace; out->partial_b = (const float*)((const char*)workspace + workspace_bytes / 2);
    out->dw = dw_oihw; out->db = dbias;
    out->nrows = (long long)d->N * d->H * d->W;
    out->PB = d->nterms; out->ncp = d->cin_chunks; out->ncot = (d->cout + 31) / 32; out->ks = d->ksize; out->tr = d->x_cpg;
    out->cout = d->cout; out->cin = cin; out->shuffle = shuffle_perm;
    return 0;
}
int bh_wgrad_reduce_batch(const BhWgradReduce* items, int n, const float* inv_scale, int accumulate, void* stream) {
    printf("[s%llx] wgrad_reduce n%d inv%llx acc%d", X(stream), n, X(inv_scale), accumulate);
    for (int i = 0; i < n; ++i) reduce_item(items[i]);
    printf("\n");
    return 0;
}

extern "C" {
int binhip_device_cus(void) {
    printf("device_cus\n");
    return 256;
}
// the two sizing queries: fixed arithmetic of the arguments (the real ones need their kernels' tile tables; all that matters is that
// every build of the recorder sees the same function), not printed: their results show in cout_pad and in the workspace sizes
int binhip_dgrad_rows_pad(int ksize, int cin) {
    return (cin + 31) / 32 * 32 + 32 * (ksize == 5);
}
size_t binhip_wgrad_workspace_bytes(int ksize, int N, int H, int W, int cin_chunks, int cout) {
    return ((size_t)ksize * ksize * cin_chunks * 16 * cout * 4 * (1 + (size_t)N * H * W / 1024) + 255) & ~(size_t)255;
}
int binhip_grad_scale(const float* g, int64_t numel, float target, float* partials, float* scale_out, void* stream) {
    printf("[s%llx] grad_scale g%llx n%lld target%g part%llx sc%llx\n", X(stream), X(g), (long long)numel, target, X(partials), X(scale_out));
    return 0;
}
int binhip_nchw_to_planes_scaled(const float* x, int N, int C, int H, int W, const float* scale, void* y_hi, void* y_lo, void* status,
                                 void* stream) {
    printf("[s%llx] nchw_to_planes_scaled x%llx N%d C%d H%d W%d sc%llx y%llx/%llx st%llx\n", X(stream), X(x), N, C, H, W, X(scale), X(y_hi),
           X(y_lo), X(status));
    return 0;
}
int binhip_pack_inputs(const float* const* images, int n_images, int N, int H, int W, void* y_hi, void* y_lo, void* status, void* stream) {
    printf("[s%llx] pack_inputs", X(stream));
    ptrs("img", (const void* const*)images, n_images);
    printf(" n%d N%d H%d W%d y%llx/%llx st%llx\n", n_images, N, H, W, X(y_hi), X(y_lo), X(status));
    return 0;
}
int binhip_rdb_tail_fwd(int N, int H, int W, int nterms, const void* blk_hi, const void* blk_lo, const void* wc_hi, const void* wc_lo,
                        const float* bias_c, const void* wl_hi, const void* wl_lo, const float* bias_l, void* y_hi, void* y_lo,
                        int store_o3, void* status, void* stream) {
    printf("[s%llx] rdb_tail_fwd N%d H%d W%d nt%d blk%llx/%llx wc%llx/%llx bc%llx wl%llx/%llx bl%llx y%llx/%llx o3%d st%llx\n", X(stream), N, H,
           W, nterms, X(blk_hi), X(blk_lo), X(wc_hi), X(wc_lo), X(bias_c), X(wl_hi), X(wl_lo), X(bias_l), X(y_hi), X(y_lo), store_o3,
           X(status));
    return 0;
}
int binhip_unpack_input_grads(const void* gx0_hi, const void* gx0_lo, const float* gout, const float* scale, int n_images, int N, int H,
                              int W, float* const* outs, void* stream) {
    printf("[s%llx] unpack_input_grads gx0%llx/%llx gout%llx sc%llx n%d N%d H%d W%d", X(stream), X(gx0_hi), X(gx0_lo), X(gout), X(scale),
           n_images, N, H, W);
    ptrs("out", (const void* const*)outs, n_images);
    printf("\n");
    return 0;
}
}  // extern "C"

// ---- the HIP runtime: numbered fake events, so that the two-stream ordering is part of the trace
void trace_reset_events() { n_events = 0; }
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned flags) {
    *event = (hipEvent_t)(uintptr_t)(0xE000 + ++n_events);
    printf("event_create e%llx flags%u\n", X(*event), flags);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) {
    printf("event_destroy e%llx\n", X(event));
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    printf("[s%llx] event_record e%llx\n", X(stream), X(event));
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned flags) {
    printf("[s%llx] wait_event e%llx flags%u\n", X(stream), X(event), flags);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream) {
    printf("[s%llx] memset %llx value%d bytes%zu\n", X(stream), X(dst), value, bytes);
    return hipSuccess;
}
