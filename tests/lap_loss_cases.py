"""The Laplacian-pyramid term of `pixel_criterion: cb+lap` (include/binlap.h) restated in float64, and the case table of
tests/test_cpu_lap_loss.py and tests/test_gpu_lap_loss.py (a plain helper module, imported by name; it never loads the library).

The restatement is explicit index arithmetic: `reduce_matrix(n)` and `expand_matrix(n)` fill the 1-D operators R (ceil(n/2) x n)
and E (n x ceil(n/2)) tap by tap from the header's two formulas, clamp included, and a plane is walked as R_h g R_w^T and
E_h c E_w^T.  `lap_ref` is the value with a graph (autograd gives its gradient); `closed_form` is the header's recurrence
G_{L-1} = r_{L-1}, G_l = r_l + R^T (G_{l+1} - E^T r_l) with the transposed matrices, no autograd.  The CPU suite holds the two to
each other; the GPU suite holds the kernels to `closed_form`.

The table: (planes, H, W, levels) as the issue lists them, then one and one past a tile of either kernel geometry (the binding's
LAP_UP_TILE in fine pixels, LAP_DOWN_TILE in coarse pixels) with two levels, more planes than a grid row, and one
workload-shaped case.  Term t of case i takes content kind (i + t) mod 5 and asks for gx only / gy only / both by t mod 3."""
import functools

import numpy as np
import torch

from bin_amd import _lib

EPS = 1e-6
K = (1.0 / 16, 4.0 / 16, 6.0 / 16, 4.0 / 16, 1.0 / 16)
UH, UW = _lib.LAP_UP_TILE
DH, DW = _lib.LAP_DOWN_TILE
KINDS = ("noise", "near", "equal", "offset", "edge")
NEEDS = ((True, False), (False, True), (True, True))
OFFSET = 0.25


def _clamp(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


@functools.lru_cache(maxsize=None)
def reduce_matrix(n):
    """R of one dimension: [ceil(n / 2), n] float64, R[i, clamp(2 i + a - 2, 0, n - 1)] += K[a]."""
    m = (n + 1) // 2
    r = torch.zeros(m, n, dtype=torch.float64)
    for i in range(m):
        for a in range(5):
            r[i, _clamp(2 * i + a - 2, 0, n - 1)] += K[a]
    return r


@functools.lru_cache(maxsize=None)
def expand_matrix(n):
    """E of one dimension: [n, ceil(n / 2)] float64, E[p, clamp((p + a - 2) / 2, 0, m - 1)] += 2 K[a] for the a with p + a - 2 even."""
    m = (n + 1) // 2
    e = torch.zeros(n, m, dtype=torch.float64)
    for p in range(n):
        for a in range(5):
            s = p + a - 2
            if s % 2 == 0:
                e[p, _clamp(s // 2, 0, m - 1)] += 2 * K[a]
    return e


def _planes(t):
    return t.double().reshape((-1,) + tuple(t.shape[-2:]))


def reduce(g):
    return reduce_matrix(g.shape[-2]) @ g @ reduce_matrix(g.shape[-1]).T


def expand(c, h, w):
    return expand_matrix(h) @ c @ expand_matrix(w).T


def bands(d, levels):
    """[b_0 .. b_{L-1}] of float64 planes d [planes, H, W]."""
    gs = [d]
    for _ in range(levels - 1):
        gs.append(reduce(gs[-1]))
    return [g - expand(gs[l + 1], g.shape[-2], g.shape[-1]) if l < levels - 1 else g for l, g in enumerate(gs)]


def lap_ref(x, y, levels, eps=EPS):
    """lap(x, y) of include/binlap.h as a float64 scalar with a graph: tensors [..., H, W] of any floating type."""
    return sum((b * b + eps).sqrt().mean() for b in bands(_planes(x) - _planes(y), levels))


def closed_form(x, y, levels, eps=EPS):
    """(lap, d lap / dx, d lap / dy) in float64 from the header's recurrence, no autograd; the gradients shaped like the inputs."""
    bs = bands(_planes(x.detach()) - _planes(y.detach()), levels)
    value = sum((b * b + eps).sqrt().mean() for b in bs)
    rs = [b / (b * b + eps).sqrt() / b.numel() for b in bs]
    G = rs[-1]
    for l in range(levels - 2, -1, -1):
        h, w = rs[l].shape[-2:]
        q = G - expand_matrix(h).T @ rs[l] @ expand_matrix(w)
        G = rs[l] + reduce_matrix(h).T @ q @ reduce_matrix(w)
    G = G.reshape(x.shape)
    return value, G, -G


# ------------------------------------------------------------------------------------------------ content
def content(kind, shape, seed):
    """(x, y) fp32 tensors of `shape` [planes, H, W]."""
    g = np.random.Generator(np.random.PCG64(seed))
    planes, h, w = shape
    if kind == "noise":                          # uniform noise
        x, y = g.random(shape), g.random(shape)
    elif kind == "near":                         # bands near the kink scale sqrt(eps)
        x = g.random(shape).astype(np.float32)
        y = x + np.float32(1e-4) * g.random(shape).astype(np.float32)
    elif kind == "equal":
        x = g.random(shape)
        y = x.copy()
    elif kind == "offset":                       # x on a 2^-12 grid, so that y = x + 1/4 is exact in fp32: d is one constant
        x = np.floor(g.random(shape) * 4096) / 4096
        y = x + OFFSET
    elif kind == "edge":                         # a step edge, in y three pixels further right
        jj = np.broadcast_to(np.arange(w), shape)
        at = w // 2 + (np.arange(planes) % 2)[:, None, None]
        x = 0.2 + 0.6 * (jj >= at)
        y = 0.2 + 0.6 * (jj >= at + 3)
    else:
        raise ValueError(kind)
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)), torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32))


# ------------------------------------------------------------------------------------------------ the table
SHAPES = [
    (1, 1, 1, 1), (2, 4, 4, 2), (3, 5, 7, 2), (2, 33, 47, 5), (1, 32, 32, 5), (1, 17, 129, 4),
    (1, UH, UW, 2), (1, UH + 1, UW + 1, 2),                    # one band tile, one pixel past it in both dimensions
    (1, 2 * DH, 2 * DW, 2), (1, 2 * DH + 1, 2 * DW + 1, 2),    # one reduce tile of coarse pixels, one coarse pixel past it
    (1, 2 * DH + 2, 2 * DW + 2, 2),                            #   (the same coarse size from an even fine size)
    (24, 16, 16, 3),                                           # more planes than a grid row of workgroups
    (8 * 3, 64, 64, 5),                                        # the workload's planes at a quarter of its crop
]
TERMS = (17, 1, 3, 24, 5)
CASES = [(i, p, h, w, L, TERMS[i % len(TERMS)]) for i, (p, h, w, L) in enumerate(dict.fromkeys(SHAPES))]


def case_id(case):
    i, planes, h, w, levels, terms = case
    return f"c{i}-{planes}x{h}x{w}-L{levels}-T{terms}"


def term_kind(case, t):
    return KINDS[(case[0] + t) % len(KINDS)]


def term_need(t):
    return NEEDS[t % 3]


@functools.lru_cache(maxsize=None)
def case_terms(i):
    """The terms of case i, made once: [(kind, x, y, g, (want_gx, want_gy))], x and y fp32 [planes, H, W], g a Python float that is
    an fp32 value of magnitude 0.5 .. 2 and either sign."""
    case = CASES[i]
    _, planes, h, w, _, terms = case
    gs = np.random.Generator(np.random.PCG64(9000 + i))
    out = []
    for t in range(terms):
        kind = term_kind(case, t)
        x, y = content(kind, (planes, h, w), 100 * i + t)
        g = float(np.float32(gs.uniform(0.5, 2.0) * (1 if gs.random() < 0.5 else -1)))
        out.append((kind, x, y, g, term_need(t)))
    return out


@functools.lru_cache(maxsize=None)
def case_reference(i):
    """Per term of case i: (lap, g * d lap / dx, g * d lap / dy) in float64 from closed_form, computed once and shared."""
    levels = CASES[i][4]
    out = []
    for kind, x, y, g, need in case_terms(i):
        v, gx, gy = closed_form(x, y, levels)
        out.append((v, g * gx, g * gy))
    return out


# ------------------------------------------------------------------------------------------------ the bar
def bar(ref):
    """Per element of a result `ref` (float64): 2^-23 |ref| + 2^-40 max|ref| — one fp32 rounding with a factor 2 of slack, plus the
    round-off of the double arithmetic on either side."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return 2.0 ** -23 * ref.abs() + 2.0 ** -40 * ref.abs().max()


def worst_fraction(got, ref):
    """max over the elements of |got - ref| / bar; 0 where both the difference and the bar vanish (x = y: an exactly zero gradient
    is asked for, and anything else is infinitely far out)."""
    ref = torch.as_tensor(ref, dtype=torch.float64)
    d, b = (torch.as_tensor(got).double().reshape(ref.shape) - ref).abs(), bar(ref)
    frac = torch.where(d == 0, torch.zeros_like(d), d / b)
    return float(frac.max())
