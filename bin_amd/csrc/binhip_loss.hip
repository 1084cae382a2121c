// binhip_loss.hip — the pixel criteria of bin_model.get_loss (bin_model.py:52-60: Charbonnier mean, loss.py:137-141; L1 sum; L2 sum)
// and the gradient-scale reduction.
//   * ONE loss path: up to BINHIP_LOSS_MAX_TERMS (x, y) pairs per launch (binhip_multi_loss_fwd / _bwd); binhip_pixel_loss_fwd / _bwd and
//     the first ABI's binhip_charbonnier_* are that path with one term.  Forward: deterministic two-pass sum (fp32 partials per block,
//     one block that sums them in double); backward: one streaming pass per output tensor.
//   * binhip_grad_scale: two-pass amax -> the power-of-two scale of the fp16 gradient planes.
#include "binhip_internal.h"
#include "binhip_reduce.h"

#define CHARB_BLOCKS 1024        // grid cap of the forward partial pass and of the amax pass = floats of `partials` per term
#define LOSS_BWD_BLOCKS 4096     // grid cap of the backward pass

template <int KIND>
__device__ __forceinline__ float crit_term(float d, float eps) {
    if constexpr (KIND == BINHIP_LOSS_CHARBONNIER) return sqrtf(d * d + eps);
    else if constexpr (KIND == BINHIP_LOSS_L1_SUM) return fabsf(d);
    else return d * d;
}
template <int KIND>
__device__ __forceinline__ float crit_grad(float d, float eps) {
    if constexpr (KIND == BINHIP_LOSS_CHARBONNIER) return d / sqrtf(d * d + eps);
    else if constexpr (KIND == BINHIP_LOSS_L1_SUM) return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);      // torch: sign(0) = 0
    else return 2.f * d;
}

// blockIdx.y = term; the partial sums of a term depend on its own grid row alone, so a term gives the same bits whatever launch it is in
template <int KIND>
__global__ void __launch_bounds__(256)
multi_loss_partial_kernel(const BinLossTerms t, long long n, float eps, float* __restrict__ partials) {
    const float* __restrict__ x = t.x[blockIdx.y];
    const float* __restrict__ y = t.y[blockIdx.y];
    float acc = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        acc += crit_term<KIND>(x[i] - y[i], eps);
    acc = block_reduce_waves(acc, BhAdd());
    if (threadIdx.x == 0) partials[(long long)blockIdx.y * gridDim.x + blockIdx.x] = acc;
}
// one block: every term's final reduction in double (`denom`: numel for the mean criterion, 1 for the sum criteria), then the
// left-to-right fp32 sum of the terms / T.  The term values stay in LDS for that sum, so `terms` may be null (the one-term entry points).
__global__ void __launch_bounds__(256)
multi_loss_final_kernel(const float* __restrict__ partials, int nb, int nterms, double denom, float* __restrict__ terms,
                        float* __restrict__ loss) {
    __shared__ float tv[BINHIP_LOSS_MAX_TERMS];          // written and read by thread 0 alone
    for (int t = 0; t < nterms; ++t) {
        const double s = block_reduce_strided(nb, 0.0, [&](int i) { return (double)partials[(long long)t * nb + i]; }, BhAdd());
        if (threadIdx.x == 0) {
            tv[t] = (float)(s / denom);
            if (terms) terms[t] = tv[t];
        }
    }
    if (threadIdx.x == 0) {
        float s = tv[0];
        for (int t = 1; t < nterms; ++t) s = s + tv[t];
        // (ATen divides a device tensor by a host scalar as a product with the fp32 reciprocal; the same here, so that the fused
        //  loss and the per-term path — torch ops over binhip_pixel_loss_fwd results — agree bit for bit; T = 1: the term itself)
        loss[0] = s * (1.0f / (float)nterms);
    }
}
// blockIdx.y = output tensor k: out[k] = s * (sign_a * crit'(x_a - y_a) [+ sign_b * crit'(x_b - y_b)])
template <int KIND>
__global__ void __launch_bounds__(256)
multi_loss_bwd_kernel(const BinLossTerms t, const BinLossGrads g, long long n, float eps, float scale, float inv_terms,
                      const float* __restrict__ gl) {
    const int k = blockIdx.y;
    const int ta = g.term_a[k], tb = g.term_b[k];
    const float s = (gl[0] * inv_terms) * scale;       // d loss / d term = gloss * (1 / T) (as autograd's division node), then / numel
    const float sa = g.sign_a[k], sb = g.sign_b[k];
    const float* __restrict__ xa = t.x[ta];
    const float* __restrict__ ya = t.y[ta];
    const float* __restrict__ xb = tb >= 0 ? t.x[tb] : nullptr;
    const float* __restrict__ yb = tb >= 0 ? t.y[tb] : nullptr;
    float* __restrict__ out = g.out[k];
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        // each term's gradient is rounded on its own (s * crit') and the two are then added: what autograd's accumulation of
        // the per-term gradients computes
        float v = sa * (s * crit_grad<KIND>(xa[i] - ya[i], eps));
        if (xb) v += sb * (s * crit_grad<KIND>(xb[i] - yb[i], eps));
        out[i] = v;
    }
}

// ---- gradient scaling: scale = 2^floor(log2(target / amax)) so fp16 gradient planes neither overflow nor
// underflow; sc[0] = scale, sc[1] = 1/scale.  Two-pass amax (deterministic).
__global__ void __launch_bounds__(256)
amax_partial_kernel(const float* __restrict__ x, long long n, float* __restrict__ partials) {
    float m = 0.f;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        m = fmaxf(m, fabsf(x[i]));
    m = block_reduce_waves(m, BhMax());
    if (threadIdx.x == 0) partials[blockIdx.x] = m;
}
__global__ void __launch_bounds__(256)
grad_scale_final_kernel(const float* __restrict__ partials, int nb, float target, float* __restrict__ sc) {
    // max is order-independent: a parallel sweep is exact
    const float m = block_reduce_strided(nb, 0.f, [&](int i) { return partials[i]; }, BhMax());
    if (threadIdx.x != 0) return;
    float s = 1.f;
    if (m > 0.f && isfinite(m)) {
        // e = floor(log2(target / m)), the largest e with m * 2^e <= target, exactly from the binary exponents (m = fm 2^em,
        // target = ft 2^et, fm, ft in [0.5, 1)), so that m * scale <= target does not hang on the last-ulp rounding of
        // log2f(target / m) when m sits a few ulps above a power of two.
        int em, et;
        const float fm = frexpf(m, &em), ft = frexpf(target, &et);
        int e = et - em - (fm > ft ? 1 : 0);
        e = e > 40 ? 40 : (e < -40 ? -40 : e);
        s = ldexpf(1.f, e);
    }
    sc[0] = s;
    sc[1] = 1.f / s;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
template <int KIND> struct LossKind { static constexpr int value = KIND; };
// f(LossKind<kind>()) for the three criteria; BINHIP_E_ARG for any other `kind`
template <class F>
static int with_kind(int kind, F&& f) {
    switch (kind) {
    case BINHIP_LOSS_CHARBONNIER: f(LossKind<BINHIP_LOSS_CHARBONNIER>()); return 0;
    case BINHIP_LOSS_L1_SUM: f(LossKind<BINHIP_LOSS_L1_SUM>()); return 0;
    case BINHIP_LOSS_L2_SUM: f(LossKind<BINHIP_LOSS_L2_SUM>()); return 0;
    default: return BINHIP_E_ARG;
    }
}
static unsigned capped_blocks(int64_t numel, int cap) {
    const long long nb = ((long long)numel + 255) / 256;
    return (unsigned)(nb > cap ? cap : nb);
}
static bool mean_criterion(int kind) { return kind == BINHIP_LOSS_CHARBONNIER; }

// `t` checked by the caller; `terms` may be null
static int loss_fwd(int kind, const BinLossTerms& t, int64_t numel, float eps, float* partials, float* terms, float* loss, hipStream_t s) {
    if (numel <= 0) return BINHIP_E_SHAPE;
    const unsigned nb = capped_blocks(numel, CHARB_BLOCKS);
    const int rc = with_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(multi_loss_partial_kernel<decltype(k)::value>, dim3(nb, (unsigned)t.n_terms), dim3(256), 0, s, t,
                           (long long)numel, eps, partials);
    });
    if (rc) return rc;
    hipLaunchKernelGGL(multi_loss_final_kernel, dim3(1), dim3(256), 0, s, partials, (int)nb, (int)t.n_terms,
                       mean_criterion(kind) ? (double)numel : 1.0, terms, loss);
    BH_CHECK_LAUNCH();
    return 0;
}
static int loss_bwd(int kind, const BinLossTerms& t, const BinLossGrads& g, int64_t numel, float eps, const float* gloss, hipStream_t s) {
    if (numel <= 0) return BINHIP_E_SHAPE;
    const unsigned nb = capped_blocks(numel, LOSS_BWD_BLOCKS);
    // gloss / T, and for the mean criterion / numel: the per-term rounding order of the per-term path (g / T first, then / numel)
    const float scale = mean_criterion(kind) ? 1.f / (float)numel : 1.f;
    const float inv_t = 1.0f / (float)t.n_terms;
    const int rc = with_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(multi_loss_bwd_kernel<decltype(k)::value>, dim3(nb, (unsigned)g.n_out), dim3(256), 0, s, t, g,
                           (long long)numel, eps, scale, inv_t, gloss);
    });
    if (rc) return rc;
    BH_CHECK_LAUNCH();
    return 0;
}
static bool kind_ok(int kind) { return kind >= BINHIP_LOSS_CHARBONNIER && kind <= BINHIP_LOSS_L2_SUM; }

extern "C" {

int binhip_charbonnier_partials(int64_t numel) { (void)numel; return CHARB_BLOCKS; }

int binhip_pixel_loss_fwd(int kind, const float* x, const float* y, int64_t numel, float eps, float* partials, float* loss,
                          void* stream) {
    if (!x || !y || !partials || !loss || !kind_ok(kind)) return BINHIP_E_ARG;
    BinLossTerms t = {};
    t.x[0] = x; t.y[0] = y; t.n_terms = 1;
    return loss_fwd(kind, t, numel, eps, partials, nullptr, loss, (hipStream_t)stream);
}

// one term, one output per requested gradient: d/dx = +crit', d/dy = -crit' (both asked for: x and y are read once per output)
int binhip_pixel_loss_bwd(int kind, const float* x, const float* y, int64_t numel, float eps, const float* gloss, float* gx,
                          float* gy, void* stream) {
    if (!x || !y || !gloss || (!gx && !gy) || !kind_ok(kind)) return BINHIP_E_ARG;
    BinLossTerms t = {};
    t.x[0] = x; t.y[0] = y; t.n_terms = 1;
    BinLossGrads g = {};
    for (float* out : {gx, gy}) {
        if (!out) continue;
        g.out[g.n_out] = out;
        g.term_a[g.n_out] = 0; g.sign_a[g.n_out] = out == gx ? 1.f : -1.f;
        g.term_b[g.n_out] = -1;
        ++g.n_out;
    }
    return loss_bwd(kind, t, g, numel, eps, gloss, (hipStream_t)stream);
}

int binhip_multi_loss_fwd(int kind, const BinLossTerms* t, int64_t numel, float eps, float* partials, float* terms, float* loss,
                          void* stream) {
    if (!t || !partials || !terms || !loss || !kind_ok(kind)) return BINHIP_E_ARG;
    if (t->n_terms <= 0 || t->n_terms > BINHIP_LOSS_MAX_TERMS) return BINHIP_E_ARG;
    for (int i = 0; i < t->n_terms; ++i)
        if (!t->x[i] || !t->y[i]) return BINHIP_E_ARG;
    return loss_fwd(kind, *t, numel, eps, partials, terms, loss, (hipStream_t)stream);
}

int binhip_multi_loss_bwd(int kind, const BinLossTerms* t, int64_t numel, float eps, const float* gloss, const BinLossGrads* g,
                          void* stream) {
    if (!t || !g || !gloss || !kind_ok(kind)) return BINHIP_E_ARG;
    if (t->n_terms <= 0 || t->n_terms > BINHIP_LOSS_MAX_TERMS || g->n_out <= 0 || g->n_out > BINHIP_LOSS_MAX_TERMS) return BINHIP_E_ARG;
    for (int i = 0; i < t->n_terms; ++i)                   // the kernel reads x[term] and y[term] of the terms the outputs name
        if (!t->x[i] || !t->y[i]) return BINHIP_E_ARG;
    for (int k = 0; k < g->n_out; ++k)
        if (!g->out[k] || g->term_a[k] < 0 || g->term_a[k] >= t->n_terms || g->term_b[k] >= t->n_terms) return BINHIP_E_ARG;
    return loss_bwd(kind, *t, *g, numel, eps, gloss, (hipStream_t)stream);
}

int binhip_charbonnier_fwd(const float* x, const float* y, int64_t numel, float eps, float* partials, float* loss,
                           void* stream) {
    return binhip_pixel_loss_fwd(BINHIP_LOSS_CHARBONNIER, x, y, numel, eps, partials, loss, stream);
}

int binhip_charbonnier_bwd(const float* x, const float* y, int64_t numel, float eps, const float* gloss, float* gx,
                           float* gy, void* stream) {
    return binhip_pixel_loss_bwd(BINHIP_LOSS_CHARBONNIER, x, y, numel, eps, gloss, gx, gy, stream);
}

int binhip_grad_scale(const float* g, int64_t numel, float target, float* partials, float* scale_out, void* stream) {
    if (!g || !partials || !scale_out) return BINHIP_E_ARG;
    if (numel <= 0 || !(target > 0.f)) return BINHIP_E_SHAPE;
    const unsigned nb = capped_blocks(numel, CHARB_BLOCKS);
    hipLaunchKernelGGL(amax_partial_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, g, (long long)numel, partials);
    hipLaunchKernelGGL(grad_scale_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, (int)nb, target, scale_out);
    BH_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
