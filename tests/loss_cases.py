"""Case tables, float64 references and comparison code for the pixel-loss reductions and the gradient-scale reduction
(tests/test_gpu_small_kernels.py; tests/test_cpu_small_kernels.py runs float32 torch through the same comparison).

References: Charbonnier mean (reference loss.py:137-141), nn.L1Loss / nn.MSELoss(reduction='sum') (bin_model.py:52-57) and
`sum(terms) / T` (bin_model.py:395-425) in float64 torch with float64 autograd; for the gradient scale exact integer arithmetic on
math.frexp.  Yardstick as in lstm_cases.py: e32 = float32 torch against float64 on the same inputs, bar = max(B, 4 * e32),
4 * e32 <= 8 * B asserted."""
import math

import numpy as np
import torch

KINDS = ("cb", "l1", "l2")                                  # bin_amd._lib.LOSS_CHARBONNIER, LOSS_L1_SUM, LOSS_L2_SUM = 0, 1, 2
KIND_ID = {"cb": 0, "l1": 1, "l2": 2}
FWD_CAP, BWD_CAP = 1024 * 256, 4096 * 256                   # threads of the capped forward / backward grids (binhip_loss.hip)
NUMELS = [1, 2, 255, 256, 257, 65535, FWD_CAP - 1, FWD_CAP, FWD_CAP + 1, BWD_CAP - 1, BWD_CAP, BWD_CAP + 1, 2 ** 24 + 3]
CAP_NUMELS = [FWD_CAP - 1, FWD_CAP, FWD_CAP + 1, BWD_CAP - 1, BWD_CAP, BWD_CAP + 1]
EPS_VALUES = (1e-6, 1e-3, 1e-12)
GLOSS = 0.37
LOSS_B = 1e-6                                               # |loss - ref| <= 1e-6 * max(1, |ref|)
GRAD_B_ABS, GRAD_B_REL = 1e-9, 1e-5                         # max|g - ref| <= 1e-9 + 1e-5 * max|ref|
FACTOR, CAP = 4.0, 8.0
MULTI_T = (1, 2, 17, 24)
# (kind, T, numel, eps): Charbonnier at every T and both grid caps +- 1; the two sum criteria at the wrapper's T = 17 there, and at
# the other T at a small size; and the wrapper's Charbonnier form with an eps other than the default, at a small size and past a cap
# (the multi-term kernels receive eps on a path of their own)
MULTI_CASES = [("cb", T, n, 1e-6) for T in MULTI_T for n in [257] + CAP_NUMELS] + \
              [(k, 17, n, 1e-6) for k in ("l1", "l2") for n in [257] + CAP_NUMELS] + \
              [(k, T, 257, 1e-6) for k in ("l1", "l2") for T in (1, 2, 24)] + \
              [("cb", 17, n, eps) for n in (257, FWD_CAP + 1) for eps in EPS_VALUES[1:]]


def make_xy(numel, seed=5):
    """float32 x, y in [0, 1) with a stretch of exact ties x == y (L1's sign(0) = 0, Charbonnier's 0 / sqrt(eps))."""
    g = torch.Generator().manual_seed(seed * 7919 + numel % 1000003)
    x, y = torch.rand(numel, generator=g), torch.rand(numel, generator=g)
    n_ties = max(numel // 8, 1 if numel > 1 else 0)
    y[numel // 2: numel // 2 + n_ties] = x[numel // 2: numel // 2 + n_ties]
    return x, y


def criterion(kind, x, y, eps):
    d = x - y
    if kind == "cb":
        return torch.mean(torch.sqrt(d * d + eps))
    if kind == "l1":
        return d.abs().sum()
    return (d * d).sum()


def reference(kind, x, y, eps, gloss, dtype):
    """loss, d(gloss * loss)/dx, d(gloss * loss)/dy in `dtype`."""
    xr, yr = x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)
    loss = criterion(kind, xr, yr, eps)
    (loss * gloss).backward()
    return {"loss": loss.detach(), "gx": xr.grad, "gy": yr.grad}


def multi_pairs(T, tensors):
    """The (x, y) index pairs of a T-term loss over `tensors` = 14 outputs o0..o13, 14 targets g0..g13 (indices 14..27) and three
    spare pairs (28..33).  T = 17 is the reference wrapper's own pairing (bin_model.py:395-425): 14 output / target terms and the
    three cycle terms that pair two outputs with each other, so o1, o5, o2 are `x` twice and o7, o9, o8 are `x` of one term and `y`
    of another.  No tensor sits in more than two terms (BinLossGrads holds two)."""
    o, g = list(range(14)), list(range(14, 28))
    p17 = [(o[i], g[i]) for i in range(14)] + [(o[1], o[7]), (o[5], o[9]), (o[2], o[8])]
    if T == 1:
        idx = [(o[0], g[0])]
    elif T == 2:
        idx = [(o[0], g[0]), (o[1], o[0])]                  # o0: x of term 0, y of term 1
    elif T == 17:
        idx = p17
    elif T == 24:
        idx = p17 + [(o[0], o[3]), (o[4], o[6]), (o[10], o[11]), (o[12], o[13]), (28, 29), (30, 31), (32, 33)]
    else:
        raise ValueError(T)
    assert len(idx) == T
    return [(tensors[a], tensors[b]) for a, b in idx], idx


def make_multi(numel, seed=9):
    g = torch.Generator().manual_seed(seed * 104729 + numel % 1000003)
    ts = [torch.rand(numel, generator=g) for _ in range(34)]
    n_ties = max(numel // 16, 1)
    ts[14][:n_ties] = ts[0][:n_ties]                        # exact ties in term 0
    ts[7][-n_ties:] = ts[1][-n_ties:]                       # and in a cycle term
    return ts


def multi_reference(kind, T, tensors, eps, gloss, dtype):
    """terms [T], loss = sum(terms) / T, and the gradient of gloss * loss w.r.t. every tensor that takes part ({index: grad})."""
    ts = [t.to(dtype).clone().requires_grad_(True) for t in tensors]
    pairs, idx = multi_pairs(T, ts)
    terms = [criterion(kind, x, y, eps) for x, y in pairs]
    loss = sum(terms) / len(terms)
    (loss * gloss).backward()
    used = sorted({i for p in idx for i in p})
    return {"terms": torch.stack([t.detach() for t in terms]), "loss": loss.detach(), "grads": {i: ts[i].grad for i in used}}


def loss_err(got, ref):
    return abs(float(got) - float(ref)) / max(1.0, abs(float(ref)))


def loss_bar(e32):
    assert FACTOR * e32 <= CAP * LOSS_B, f"yardstick cap broken: 4 * e32 = {FACTOR * e32:.3e}"
    return max(LOSS_B, FACTOR * e32)


def grad_err(got, ref):
    return float((got.double() - ref.double()).abs().max())


def grad_bar(e32, ref):
    B = GRAD_B_ABS + GRAD_B_REL * float(ref.double().abs().max())
    assert FACTOR * e32 <= CAP * B, f"yardstick cap broken: 4 * e32 = {FACTOR * e32:.3e} > 8 * {B:.3e}"
    return max(B, FACTOR * e32)


def check_loss(tag, got, ref64, ref32, label="kernel"):
    g = torch.as_tensor(got).detach().cpu()
    assert bool(torch.isfinite(g).all()), tag
    e32, e = loss_err(ref32, ref64), loss_err(g, ref64)
    b = loss_bar(e32)
    print(f"[small-kernels] loss {tag}: e32={e32:.3e} bar={b:.3e} {label}={e:.3e} ratio={e / b:.3f}")
    assert e <= b, (tag, e, b)
    return e / b


def check_terms(tag, got, ref64, ref32, label="kernel"):
    return max(check_loss(f"{tag} term{i}", got[i], ref64[i], ref32[i], label) for i in range(len(ref64)))


def check_grad(tag, got, ref64, ref32, label="kernel"):
    g = got.detach().cpu().reshape(ref64.shape)
    assert bool(torch.isfinite(g).all()), tag
    e32, e = grad_err(ref32, ref64), grad_err(g, ref64)
    b = grad_bar(e32, ref64)
    print(f"[small-kernels] lossgrad {tag}: e32={e32:.3e} bar={b:.3e} {label}={e:.3e} ratio={e / b:.3f}")
    assert e <= b, (tag, e, b)
    return e / b


# ---- binhip_grad_scale: scale = 2^e, e = the largest integer with amax * 2^e <= target, clamped to +-40; all zero -> 1 ----------
SCALE_NUMELS = [1, 255, 256, 257] + CAP_NUMELS
ONE = np.float32(1.0)
SCALE_AMAX = [ONE, np.nextafter(ONE, np.float32(2)), np.nextafter(ONE, np.float32(0)), np.float32(2.0 ** -9),
              np.nextafter(np.float32(2.0 ** -9), np.float32(1)), np.float32(0.75), np.float32(3.1e-5), np.float32(1e-20), np.float32(1234.5),
              np.nextafter(np.float32(16.0), np.float32(32)), np.nextafter(np.float32(10.0), np.float32(32)), np.float32(10.0)]
SCALE_TARGETS = (16.0, 10.0, 6.3)


def scale_reference(amax, target):
    """(scale, 1 / scale) by exact integer arithmetic on the binary exponents; amax, target float32 values."""
    amax, target = float(np.float32(amax)), float(np.float32(target))
    if amax == 0.0:
        return 1.0, 1.0
    fm, em = math.frexp(amax)
    ft, et = math.frexp(target)
    e = et - em - (1 if fm > ft else 0)
    assert amax * 2.0 ** e <= target < amax * 2.0 ** (e + 1)          # (exact: powers of two times float32 values in double)
    e = max(-40, min(40, e))
    return 2.0 ** e, 2.0 ** -e


def scale_input(numel, amax, seed=3, negative=False):
    """float32 vector whose largest magnitude `amax` sits in the LAST element (a grid-stride loop that stops early misses it)."""
    g = torch.Generator().manual_seed(seed + numel % 65521)
    v = (torch.rand(numel, generator=g) - 0.5) * float(amax) * 0.9          # |v| <= 0.45 amax
    v[-1] = -float(amax) if negative else float(amax)
    return v
