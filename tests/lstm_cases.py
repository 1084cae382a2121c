"""Case table, float64 reference and comparison code of the ConvLSTM part of tests/test_gpu_small_kernels.py (and of its CPU
twin tests/test_cpu_small_kernels.py, which runs plain float32 torch through the same comparison).

Reference: oracle.rdn_oracle.convlstm_cell (reference RDN.py:74-92) in float64 with torch autograd.  Yardstick: the same oracle in
float32 on the CPU: for every case and output e32 = error(float32 oracle, float64 oracle); the kernel's bar is max(B, 4 * e32) with
B the bar the suite already applies to that quantity, and 4 * e32 <= 8 * B is asserted so that a broken yardstick cannot widen a bar
(a case that breaks the cap is re-drawn, not exempted).  Factor 4: the kernels sum in another order and use the hardware exp; they
have no reason to be further from float64 than a small multiple of another float32 evaluation, while a wrong tap, gate, bias or
tile is orders of magnitude outside.  Every element of every case is compared: there are no ReLU ties here, so nothing is masked.

Inputs are drawn in float32 and promoted, so the float32 oracle, the float64 oracle and the kernels see the same numbers."""
from collections import namedtuple

import torch

from oracle import rdn_oracle as O

TILE_W, TILE_H = 64, 8                 # convlstm_bwd_weight_kernel's tile (binhip_convlstm.hip CL_TW x CL_TH)
FINAL_STRIDE = 256                     # convlstm_bwd_weight_final_kernel's strided loop: tiles i, i + 256, ...

# B: forward c', h' max-abs; gradients max-abs over max-abs of the reference tensor (`rel`)
BARS = {"c": 2e-6, "h": 2e-6, "gx": 2e-5, "gcp": 2e-5, "ghp": 2e-5, "dw": 2e-4, "db": 2e-4}
FACTOR, CAP = 4.0, 8.0
MIN_REF_MAX = 1e-3                     # every compared gradient tensor has a maximum that is not itself an underflow

Case = namedtuple("Case", "tag n h w state fb regime variant seed")

SMALL_SHAPES = [(1, 1, 1), (1, 1, 4), (1, 4, 1), (3, 3, 5), (1, 8, 64), (1, 7, 63), (2, 9, 65), (1, 16, 128), (2, 18, 70),
                (5, 8, 12), (3, 40, 132)]
TILE_SHAPES = [(1, 264, 512)]                          # 264 tiles: just past the final reduction's first stride
LARGE_SHAPES = [(8, 256, 256), (1, 720, 1280)]         # 1024 and 1800 tiles
EXPECTED_TILES = {(1, 8, 64): 1, (1, 7, 63): 1, (2, 9, 65): 8, (1, 16, 128): 4, (2, 18, 70): 12, (1, 264, 512): 264,
                  (8, 256, 256): 1024, (1, 720, 1280): 1800}
REGIME_SCALE = {"moderate": 0.2, "saturated": 3.0, "overflow": 0.2}
# re-drawn: at 3x40x132 WITH state (forget_bias 1 and -2.5) and s = 3 float32 torch itself is 4.6e-6 from float64 in c' (47 520
# pixels of gates up to 34, 4 * e32 = 9.2 B), past the cap; s = 2 still saturates (max |gate| 22.9, 10 % of gates beyond +-8) and
# keeps the yardstick inside it.  The case without state keeps s = 3.  Key: (regime, n, h, w, state)
SCALE_OVERRIDE = {("saturated", 3, 40, 132, True): 2.0}
# pointer variants of the C entry points: which arguments are NULL
VARIANTS = ("full", "gh_only", "gc_only", "no_gx", "no_dw", "no_state_grads", "no_cnew")
OVERFLOW_SHAPES = [(2, 9, 20), (3, 7, 13)]
# hidden channel 0 keeps its four gates moderate; channels 1 and 2 sit at +-30, +-90 and +-200 by bias alone (|200| is past the
# overflow of exp in float32); gate order i, j, f, o, three channels each (RDN.py:79)
OVERFLOW_BIAS = {1: 30.0, 4: -90.0, 7: 200.0, 10: -30.0, 2: -200.0, 5: 30.0, 8: -90.0, 11: 90.0}


def tiles(n, h, w):
    return -(-w // TILE_W) * -(-h // TILE_H) * n


def _tag(n, h, w, state, fb, regime, variant):
    t = f"{n}x{h}x{w}_{'state' if state else 'nostate'}_{regime}"
    if fb != 1.0:
        t += f"_fb{fb:g}"
    if variant != "full":
        t += "_" + variant
    return t


def _cases():
    out = []

    def add(shape, state, fb=1.0, regime="moderate", variant="full", seed=7):
        n, h, w = shape
        out.append(Case(_tag(n, h, w, state, fb, regime, variant), n, h, w, state, fb, regime, variant, seed))

    for shape in SMALL_SHAPES + TILE_SHAPES + LARGE_SHAPES:
        for state in (False, True):
            add(shape, state)
    for shape in SMALL_SHAPES:
        for fb in (0.0, -2.5):                       # WITH state only: without one c_prev = 0 and the forget gate has no effect
            add(shape, True, fb)
        add(shape, False, 1.0, "saturated")
        add(shape, True, 1.0, "saturated")
        add(shape, True, -2.5, "saturated")
    for shape in OVERFLOW_SHAPES:
        for fb in (1.0, 0.0):
            add(shape, True, fb, "overflow")
    for shape in ((2, 9, 65), (1, 16, 128)):         # one ragged, one aligned
        for variant in VARIANTS[1:]:
            add(shape, True, 0.0, "moderate", variant)
        add(shape, False, 1.0, "moderate", "gh_only")
        add(shape, False, 1.0, "moderate", "gc_only")
        add(shape, True, 1.0, "saturated", "gh_only")
    return out


CASES = _cases()
CASE_BY_TAG = {c.tag: c for c in CASES}
assert len(CASE_BY_TAG) == len(CASES)


def make_inputs(case):
    """float32 CPU tensors: x, c0, h0 (None without state), w, b, gh, gc."""
    g = torch.Generator().manual_seed(case.seed * 100003 + case.n * 10007 + case.h * 101 + case.w)
    shp = (case.n, 3, case.h, case.w)
    s = SCALE_OVERRIDE.get((case.regime, case.n, case.h, case.w, case.state), REGIME_SCALE[case.regime])
    x = torch.rand(shp, generator=g)
    c0 = (torch.rand(shp, generator=g) - 0.5) * (8.0 if case.regime == "overflow" else 2.0)
    h0 = (torch.rand(shp, generator=g) - 0.5) * 2.0
    w = (torch.rand(12, 6, 3, 3, generator=g) - 0.5) * 2 * s
    b = (torch.rand(12, generator=g) - 0.5) * 2 * s
    if case.regime == "overflow":
        for k, v in OVERFLOW_BIAS.items():
            b[k] = v
    gh = torch.rand(shp, generator=g) - 0.5
    gc = torch.rand(shp, generator=g) - 0.5
    if not case.state:
        c0 = h0 = None
    return {"x": x, "c0": c0, "h0": h0, "w": w, "b": b, "gh": gh, "gc": gc}


def wanted(case):
    """Names of the outputs the variant produces."""
    v = case.variant
    names = ["c", "h", "gx", "dw", "db"] + (["gcp", "ghp"] if case.state else [])
    if v == "no_gx":
        names.remove("gx")
    if v == "no_dw":
        names.remove("dw"), names.remove("db")
    if v == "no_state_grads":
        names.remove("gcp"), names.remove("ghp")
    if v == "no_cnew":
        names.remove("c")
    return names


def reference(case, inp, dtype):
    """The oracle cell and its autograd gradients in `dtype`; all outputs, whatever the variant leaves out."""
    T = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    x, c0, h0, w, b = (T(inp[k]) for k in ("x", "c0", "h0", "w", "b"))
    h, (c, _) = O.convlstm_cell(x, [c0, h0] if case.state else None, w, b, forget_bias=case.fb)
    loss = 0
    if case.variant != "gc_only":
        loss = loss + (h * inp["gh"].to(dtype)).sum()
    if case.variant != "gh_only":
        loss = loss + (c * inp["gc"].to(dtype)).sum()
    loss.backward()
    out = {"c": c.detach(), "h": h.detach(), "gx": x.grad, "dw": w.grad, "db": b.grad}
    if case.state:
        out["gcp"], out["ghp"] = c0.grad, h0.grad
    return out


def gates_reference(gates, c_prev, fb, gh, gc, dtype):
    """The gate arithmetic alone (RDN.py:79-82) for a cell of any hidden size: gates [N, 4 hid, H, W] in i, j, f, o order ->
    c', h' and the gradients w.r.t. gates and c_prev.  gh or gc None = that upstream gradient absent."""
    g = gates.to(dtype).clone().requires_grad_(True)
    cp = None if c_prev is None else c_prev.to(dtype).clone().requires_grad_(True)
    i, j, f, o = g.chunk(4, 1)
    c = (cp if cp is not None else 0) * torch.sigmoid(f + fb) + torch.sigmoid(i) * torch.tanh(j)
    h = torch.tanh(c) * torch.sigmoid(o)
    loss = 0
    if gh is not None:
        loss = loss + (h * gh.to(dtype)).sum()
    if gc is not None:
        loss = loss + (c * gc.to(dtype)).sum()
    loss.backward()
    out = {"c": c.detach(), "h": h.detach(), "dgates": g.grad}
    if cp is not None:
        out["gcp"] = cp.grad
    return out


GATES_BARS = {"c": 2e-6, "h": 2e-6, "dgates": 2e-5, "gcp": 2e-5}
GATES_HIDDEN = (1, 3, 16, 33)
GATES_REGIMES = ("moderate", "saturated", "overflow")
GATES_FB = (1.0, 0.0, -2.5)
GATES_SHAPE = (2, 5, 7)                      # N, H, W


def make_gates(hidden, regime, seed=11):
    """float32 gates [N, 4 hid, H, W], c_prev, gh, gc for the elementwise kernels of the general cell."""
    n, h, w = GATES_SHAPE
    g = torch.Generator().manual_seed(seed * 1009 + hidden * 17 + GATES_REGIMES.index(regime))
    gates = (torch.rand(n, 4 * hidden, h, w, generator=g) - 0.5) * {"moderate": 4.0, "saturated": 60.0, "overflow": 4.0}[regime]
    cp = (torch.rand(n, hidden, h, w, generator=g) - 0.5) * (8.0 if regime == "overflow" else 2.0)
    if regime == "overflow":                 # half of the gate values at +-30, +-90, +-200, the rest moderate
        levels = torch.tensor([30.0, -30.0, 90.0, -90.0, 200.0, -200.0])
        pick = torch.randint(0, 12, gates.shape, generator=g)
        gates = torch.where(pick < 6, levels[pick.clamp_max(5)], gates)
    gh = torch.rand(n, hidden, h, w, generator=g) - 0.5
    gc = torch.rand(n, hidden, h, w, generator=g) - 0.5
    return gates, cp, gh, gc


def err(name, got, ref):
    """The project's metrics: forward max-abs; gradients max-abs over max-abs of the reference (test_gpu_convlstm._rel)."""
    d = float((got.double() - ref.double()).abs().max())
    if name in ("c", "h"):
        return d
    return d / max(float(ref.double().abs().max()), 1e-12)


def bar(name, e32, bars=BARS):
    B = bars[name]
    assert FACTOR * e32 <= CAP * B, f"yardstick cap broken for {name}: 4 * e32 = {FACTOR * e32:.3e} > 8 * B = {CAP * B:.3e}"
    return max(B, FACTOR * e32)


def compare(tag, names, got, ref64, ref32, bars=BARS, label="kernel"):
    """Assert every output in `names` finite and within max(B, 4 e32) of float64; prints e32, bar and error per output and
    returns {name: (e32, bar, error)}.  The same code judges the kernels (GPU module) and float32 torch (CPU module)."""
    res, bad = {}, []
    for nm in names:
        e32 = err(nm, ref32[nm], ref64[nm])
        bb = bar(nm, e32, bars)
        g = got[nm].detach().cpu()
        assert g.shape == ref64[nm].shape, (tag, nm, tuple(g.shape))
        assert bool(torch.isfinite(g).all()), f"{tag}: {nm} is not finite"
        e = err(nm, g, ref64[nm])
        res[nm] = (e32, bb, e)
        print(f"[small-kernels] lstm {tag} {nm}: e32={e32:.3e} bar={bb:.3e} {label}={e:.3e} ratio={e / bb:.3f}")
        if not e <= bb:
            bad.append((nm, e, bb))
    assert not bad, (tag, bad)
    return res


def off1(t):
    """A copy of `t` whose data pointer is 4 bytes past a 16-byte boundary (forces the one-pixel-per-thread ConvLSTM kernels)."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v
