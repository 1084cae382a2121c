"""The SSIM term of `pixel_criterion: cb+ssim` (include/binssim.h) restated in float64, and the case table of
tests/test_cpu_ssim_loss.py and tests/test_gpu_ssim_loss.py (a plain helper module, imported by name).

Two restatements that share no arithmetic beyond the window sums: `ssim_ref` writes the definition with F.conv2d and leaves the
gradient to autograd; `closed_form` evaluates the header's closed-form gradient (coefficient maps a_x, a_y, b, c spread back with
F.conv_transpose2d).  The CPU suite holds them to each other; the GPU suite holds the kernels to `ssim_ref`.

The table.  The backward kernel's pixel tile is TH x TW (the binding's SSIM_BWD_TILE); H and W take 11, 12 and the tile's edges
TH - 1, TH, TH + 1, TH + 10, TH + 11 (the halo of 10 ends in the tile / one pixel past it), 2 TH + 5, paired as a covering set and
not as the product, and a few more shapes cross the forward kernel's window tile (SSIM_FWD_TILE).  planes cycles 1, 3, 7 and the
number of terms 1, 2, 17, 24.  Term t of a case takes content kind (case + t) mod 7 and asks for gx only / gy only / both by
t mod 3, so every kind meets every gradient request."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from bin_amd import _lib
from bin_amd.utils.util import _gauss_taps

C1, C2 = 0.01 ** 2, 0.03 ** 2
TH, TW = _lib.SSIM_BWD_TILE
FH, FW = _lib.SSIM_FWD_TILE
KINDS = ("noise", "smooth", "flat", "equal", "zeros", "wide", "mag8")
NEEDS = ((True, False), (False, True), (True, True))


def taps():
    return torch.from_numpy(np.asarray(_gauss_taps(), dtype=np.float64))


def _window():
    w = taps()
    return torch.outer(w, w)[None, None]


def _stats(x, y):
    """The five window means of float64 [planes, H, W] tensors, each [planes, 1, H - 10, W - 10]."""
    w = _window()
    x, y = x[:, None], y[:, None]
    return (F.conv2d(x, w), F.conv2d(y, w), F.conv2d(x * x, w), F.conv2d(y * y, w), F.conv2d(x * y, w))


def ssim_ref(x, y):
    """ssim(x, y) of include/binssim.h as a float64 scalar with a graph: tensors [..., H, W] of any floating type."""
    x = x.double().reshape((-1,) + tuple(x.shape[-2:]))
    y = y.double().reshape((-1,) + tuple(y.shape[-2:]))
    mx, my, exx, eyy, exy = _stats(x, y)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    s = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sxx + syy + C2))
    return s.mean()


def ssim_ref_grads(x, y):
    """(ssim, d ssim / dx, d ssim / dy) in float64 by autograd over ssim_ref; the gradients shaped like the inputs."""
    xd, yd = x.detach().double().requires_grad_(), y.detach().double().requires_grad_()
    s = ssim_ref(xd, yd)
    gx, gy = torch.autograd.grad(s, (xd, yd))
    return s.detach(), gx, gy


def closed_form(x, y):
    """The same three from the header's closed form, no autograd."""
    shape = x.shape
    x = x.detach().double().reshape((-1,) + tuple(shape[-2:]))
    y = y.detach().double().reshape((-1,) + tuple(shape[-2:]))
    mx, my, exx, eyy, exy = _stats(x, y)
    sxx, syy, sxy = exx - mx * mx, eyy - my * my, exy - mx * my
    A1, A2 = 2 * mx * my + C1, 2 * sxy + C2
    B1, B2 = mx * mx + my * my + C1, sxx + syy + C2
    S = A1 * A2 / (B1 * B2)
    b = -2 * S / B2
    c = 2 * A1 / (B1 * B2)
    ax = 2 * my * (A2 - A1) / (B1 * B2) + 2 * mx * S * (1 / B2 - 1 / B1)
    ay = 2 * mx * (A2 - A1) / (B1 * B2) + 2 * my * S * (1 / B2 - 1 / B1)
    w = _window()
    T = lambda m: F.conv_transpose2d(m, w)[:, 0]
    n = S.numel()
    gx = (T(ax) + x * T(b) + y * T(c)) / n
    gy = (T(ay) + y * T(b) + x * T(c)) / n
    return S.mean(), gx.reshape(shape), gy.reshape(shape)


# ------------------------------------------------------------------------------------------------ content
def content(kind, shape, seed):
    """(x, y) fp32 tensors of `shape` [planes, H, W]."""
    g = np.random.Generator(np.random.PCG64(seed))
    planes, h, w = shape
    if kind == "noise":
        x, y = g.random(shape), g.random(shape)
    elif kind == "smooth":                       # a sinusoid plus 1 % noise: ssim about 0.99
        ii, jj = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        base = 0.5 + 0.3 * np.sin(0.21 * ii + 0.1 * np.arange(planes)[:, None, None]) * np.cos(0.17 * jj)
        x, y = base + 0.01 * (g.random(shape) - 0.5), base + 0.01 * (g.random(shape) - 0.5)
    elif kind == "flat":                         # 0.5 +- 1e-3
        x, y = 0.5 + 1e-3 * (2 * g.random(shape) - 1), 0.5 + 1e-3 * (2 * g.random(shape) - 1)
    elif kind == "equal":
        x = g.random(shape)
        y = x.copy()
    elif kind == "zeros":
        x, y = np.zeros(shape), np.zeros(shape)
    elif kind == "wide":                         # values in [-0.2, 1.2]
        x, y = -0.2 + 1.4 * g.random(shape), -0.2 + 1.4 * g.random(shape)
    elif kind == "mag8":                         # values of magnitude 8
        x, y = 16 * g.random(shape) - 8, 16 * g.random(shape) - 8
    else:
        raise ValueError(kind)
    return torch.from_numpy(x.astype(np.float32)), torch.from_numpy(y.astype(np.float32))


# ------------------------------------------------------------------------------------------------ the table
HS = (11, 12, TH - 1, TH, TH + 1, TH + 10, TH + 11, 2 * TH + 5)
WS = (11, 12, TW - 1, TW, TW + 1, TW + 10, TW + 11, 2 * TW + 5)


def _shapes():
    out = []
    for shift in (0, 3, 6):                      # every H and every W three times (the last round twice), in different company
        for i, h in enumerate(HS):
            if shift == 6 and i % 2:
                continue
            out.append((h, WS[(i + shift) % len(WS)]))
    # the forward kernel's tile of FH x FW windows: exactly one tile, one window more, and a second tile row next to a narrow one
    out += [(FH + 10, FW + 10), (FH + 11, FW + 11), (2 * FH + 13, 12)]
    return out


SHAPES = _shapes()
PLANES = (1, 3, 7)
TERMS = (1, 2, 17, 24)
CASES = [(i, h, w, PLANES[i % 3], TERMS[(i + i // 4) % 4]) for i, (h, w) in enumerate(SHAPES)]


def case_id(case):
    i, h, w, planes, terms = case
    return f"c{i}-{planes}x{h}x{w}-T{terms}"


def term_kind(case, t):
    return KINDS[(case[0] + t) % len(KINDS)]


def term_need(t):
    return NEEDS[t % 3]


@functools.lru_cache(maxsize=None)
def case_terms(i):
    """The terms of case i, made once: [(kind, x, y, g, (want_gx, want_gy))], x and y fp32 [planes, H, W], g a Python float that is
    an fp32 value of magnitude 0.5 .. 2 and either sign."""
    case = CASES[i]
    _, h, w, planes, terms = case
    gs = np.random.Generator(np.random.PCG64(7000 + i))
    out = []
    for t in range(terms):
        kind = term_kind(case, t)
        x, y = content(kind, (planes, h, w), 100 * i + t)
        g = float(np.float32(gs.uniform(0.5, 2.0) * (1 if gs.random() < 0.5 else -1)))
        out.append((kind, x, y, g, term_need(t)))
    return out


@functools.lru_cache(maxsize=None)
def case_reference(i):
    """Per term of case i: (ssim, g * d ssim / dx, g * d ssim / dy) in float64 from ssim_ref, computed once and shared."""
    out = []
    for kind, x, y, g, need in case_terms(i):
        s, gx, gy = ssim_ref_grads(x, y)
        out.append((s, g * gx, g * gy))
    return out


# ------------------------------------------------------------------------------------------------ the bars
VALUE_BAR = 2.0 ** -24          # one fp32 rounding of a number of magnitude <= 1; the double sums add nothing visible


def grad_bar(ref, planes, h, w):
    """Per element: one fp32 rounding with a factor 2, plus the slack for the order of the double sums (amplified by at most
    2 / C2), relative to the largest gradient or, where the gradient vanishes, to one window's share."""
    floor = max(float(ref.abs().max()), 1.0 / (planes * (h - 10) * (w - 10)))
    return 2.0 ** -23 * ref.abs() + 1e-9 * floor


def worst_fraction(got, ref, planes, h, w):
    """max over the elements of |got - ref| / bar."""
    return float(((got.double() - ref).abs() / grad_bar(ref, planes, h, w)).max())
