"""The top of the N H W < 2^26 domain: case table, periodic exact operands, band references and the every-pixel comparison shared by
tests/test_gpu_domain_top.py (the kernels, at the top) and tests/test_cpu_domain_top.py (the table's conditions, and float32 torch as
a stand-in kernel at a scaled-down geometry, with deliberately wrong restatements that must be reported).

Every convolution-class kernel addresses a 16-channel chunk plane with a 32-bit byte offset whose out-of-range sentinel 0x80000000
makes the zero padding, so a plane has to stay below 2 GiB: every entry point refuses N H W >= 2^26 (include/binhip.h).  This module
runs the ACCEPTING side, the largest planes the library takes, and holds every pixel of the result to float64.

Method.  A float64 reference of 2^26 pixels is out of reach and not needed:
  * operands are the exact families of tests/conv_ref_cases.py (A: small integers, both precisions; B: a + b 2^-11 with a live lo
    plane, nterms 3), under whose conditions a kernel equals float64 with NO tolerance, in any summation order;
  * one PERIOD of P = 37 rows is drawn on the CPU ([1, C, P, W]); row r of image n of the device tensor is period row (r + PHASES[n])
    mod P, gathered on the device straight into plane layout (the big tensor never exists on the host);
  * a float64 reference (torch, on the test's device) is computed for the top band of image 0, one output period plus two halos (and
    two rows) long, which holds the image's top edge AND one whole period of interior rows, and for a short band at every other image edge (the bottom of the
    last image among them);
  * every other output row y of image n must equal the verified interior period row (y + PHASES[n]) mod P: one elementwise compare on
    the device of the output against the period, broadcast over whole periods.
Equality is required throughout (fp16 / fp32 VALUES: +0 and -0 are one value, a NaN is a mismatch).

Why a wrong offset shows.  One period of one chunk plane is P W 32 bytes, which has the odd factor 37: no power of two (2^28 .. 2^32, the
wraps a dropped cast or a 32-bit overflow would produce) is a whole number of periods, so a wrapped offset lands on a different period
row; the rows within a period are independent draws.  PHASES are pairwise different, so image m read for image n shows; they are even,
so that the half-resolution rows of the inverse-PixelShuffle store are again periodic with period P (half row y' holds full rows 2 y',
2 y' + 1; with the phase 2 q these are period rows 2 (y' + q) mod P, and j -> 2 j mod P is a bijection for odd P).

Exactness at this size.  conv_ref_cases.conditions() evaluates the operation on absolute values, which costs a reference per band.  The
table is thinned against a SUFFICIENT analytic form of the same conditions instead, which holds for every pixel of every shape at
once: with xm = max(|hi| + |lo|) of an activation and S = the largest absolute row sum of the weights (|hi| + |lo|), every partial sum
of the product form Whi Xhi + Wlo Xhi + Whi Xlo is at most xm S (+ bias, residual, acc, mean of the images).  Required: that bound
times the family's scale (1, or 2^11 for B) stays below 2^24, and every plane-stored value stays within +-2048: an integer there is an
fp16 number, and a multiple of 2^-11 there survives its hi / lo split (hi has an ulp of at most 1, the remainder at most 1024 steps of
2^-11).  tests/test_cpu_domain_top.py also runs conv_ref_cases.conditions() itself on the bands of the tall shape, the GPU module on
the top band of every case it runs.

Weight gradient.  A sum over 2^26 pixels cannot stay exact on dense data; two sparse forms replace the periodic one:
  bands   x and g are zero except in full-width bands of 8 rows (family A / B values, thinned): at the top of image 0, at the bottom of
          the last image, straddling the plane byte offsets 2^28, 2^29 and 2^30, and ending on the plane's last row below 2^31.  The
          float64 dW, db come from the bands alone (a band's zero surroundings are its padding); equality is required.
  census  g = 1 on channel 0 everywhere, x = 1 on channel 0 at every fourth pixel of the flattened plane.  dW[0, 0, tap] is then the
          number of in-image pixel pairs, below 2^24 and so exact in fp32 in any order; it is wrong if a pixel is counted twice or not
          at all.  census_counts() is integer arithmetic.  (db[0] = N H W is above 2^24: not part of the claim.)
"""
import functools
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch
import torch.nn.functional as F

import conv_cases as cc
import conv_ref_cases as rc
import wgrad_cases as wg

P = 37                                   # rows of a period: odd, no multiple of any tile height (1, 2, 8, 16)
PHASES = (0, 12, 26)                     # even, pairwise different mod P
NHW_LIMIT = 1 << 26
MAX_LIVE_BYTES = 96 << 30

WIDE, TALL = (3, 2731, 8191), (1, 958697, 70)                    # 2^26 - 1 pixels; 67 108 790 pixels in three tile columns
EVEN_WIDE, EVEN_TALL = (2, 4096, 8190), (1, 958696, 70)          # where H and W must be even
SHUFFLE_IN = ((1, 4096, 4094), (1, 479348, 35))                  # the OUTPUT plane (4x) is the one just under 2^26
SCALED_DOWN = {WIDE: (3, 120, 45), TALL: (1, 300, 6), EVEN_WIDE: (2, 130, 46), EVEN_TALL: (1, 300, 6),
               SHUFFLE_IN[0]: (1, 130, 23), SHUFFLE_IN[1]: (1, 150, 3)}       # the CPU module's geometry per shape


def _c(tag, kind, ks, cin, cout, rows, **opts):
    return cc.Case(tag, kind, ks, cin, cout, opts, rows)


# One case per addressing path; channels the smallest the dispatcher row admits (pixels are what is under test).  rows: as in conv_cases
CASES = (
    _c("p3", "fwd", 3, 16, 32, {1: "launch_cfg<3,1,1,2,8,1,1,2,P>: patch_offsets, plain plane store, residual", 3: "conv_x3_kernel<3,P,WIDE=0>"},
       relu=True, res=True),
    _c("p5", "fwd", 5, 16, 32, {1: "launch_cfg<5,1,1,2,8,1,1,2,P>", 3: "conv_x3_kernel<5,P>"}),
    _c("p1", "fwd", 1, 16, 32, {1: "launch_cfg<1,1,1,4,4,4,1,2,P>: the 1x1 path", 3: "launch_cfg<1,1,1,4,4,2,3,2,P>"}),
    _c("p3_grouped", "fwd", 3, 32, 32, {1: "launch_cfg<3,1,1,2,8,1,1,2,P>, x_cpg = 1", 3: "conv_x3_kernel<3,P,WIDE=0>, x_cpg = 1"},
       relu=True, x_cpg=1),
    _c("s3", "fwd", 3, 16, 256, {1: "launch_cfg<3,2,2,4,4,1,1,2,S>: the PixelShuffle 4x plane", 3: "conv_x3_kernel<3,S,WIDE=1>"}, epilogue="shuffle"),
    _c("f3_c3", "fwd", 3, 64, 3, {1: "final_dot2_kernel: fp32 images, fp32 NCHW store", 3: "final_m16_kernel"}, epilogue="final", nimg=2),
    _c("f3_c4", "fwd", 3, 16, 4, {1: "launch_cfg<3,1,1,2,8,1,1,2,F>: conv_epilogue FINAL", 3: "conv_x3_kernel<3,F>"}, epilogue="final", nimg=3),
    _c("f5_subpix", "fwd", 5, 16, 12, {1: "launch_cfg<5,1,1,2,8,1,1,2,FINAL_SUBPIX>: the fused UPNet's main launch", 3: "conv_x3_kernel<5,FINAL_SUBPIX>"},
       epilogue="subpix", nimg=3),
    _c("b3_mask", "bwd", 3, 32, 16, {1: "launch_cfg<3,1,1,2,8,1,1,2,P> XTRA", 3: "conv_x3_kernel<3,P,WIDE=0> XTRA"}, res=True, mask_from=1),
    _c("b1_acc", "bwd", 1, 32, 16, {1: "launch_cfg<1,1,1,4,4,4,1,2,P> XTRA", 3: "launch_cfg<1,1,1,4,4,2,3,2,P> XTRA"}, acc=True),
    _c("b1_ycpg", "bwd", 1, 32, 16, {1: "launch_cfg<1,1,1,4,4,4,1,2,P>: grouped y (y_cpg = 1, a guarded gap plane after each group)",
                                      3: "launch_cfg<1,1,1,4,4,2,3,2,P>: grouped y"}, y_cpg=1),
    _c("b3_unshuf", "bwd", 3, 16, 16, {1: "launch_cfg<3,1,1,2,8,1,1,2,P> XTRA: the unshuffle store", 3: "conv_x3_kernel<3,P,WIDE=0> XTRA"}, y_unshuf=1),
    # the gather-form dense-block dgrad (binhip_weights_relayout_rdb_gather), group 3 of bin_stage4's block: the gradient of conv 2's 32
    # outputs from conv 3's output gradient, = conv_transpose with conv 3's weight columns 160 .. 191 (+ the slot, masked)
    _c("b3_gather", "bwd", 3, 32, 32, {1: "launch_cfg<3,1,1,2,8,1,1,2,P> XTRA, gather-form weights", 3: "conv_x3_kernel<3,P,WIDE=0> XTRA, gather-form weights"},
       res=True, mask_from=0, gather=3),
    _c("tail_o3", "tail", 3, 192, 32, {1: "rdb_tail_kernel<1,2>: its own offset loop, store_o3", 3: "rdb_tail_x3_kernel, store_o3"}, store_o3=True),
)
BY_TAG = {c.tag: c for c in CASES}
TAGS = tuple(c.tag for c in CASES)
NTERMS = (1, 3)


def shapes(case):
    if case.opts.get("epilogue") == "shuffle":
        return SHUFFLE_IN
    return (EVEN_WIDE, EVEN_TALL) if case.opts.get("y_unshuf") else (WIDE, TALL)


def halo(case):
    return case.ks // 2


def row_scale(case):
    """Output rows per input row."""
    if case.opts.get("epilogue") in ("shuffle", "subpix"):
        return Fraction(2)
    return Fraction(1, 2) if case.opts.get("y_unshuf") else Fraction(1)


def out_period(case):
    """(rows of the output's period, output phase of image n as a function) — module docstring."""
    s = row_scale(case)
    if s == 2:
        return 2 * P, lambda n: 2 * PHASES[n]
    if s == 1:
        return P, lambda n: PHASES[n]
    return P, lambda n: PHASES[n] // 2


# ------------------------------------------------------------------------------------------------ table conditions (no GPU)
def plane_period_bytes(w):
    return P * w * 32


def wrap_is_visible(w):
    """Condition 1: no shift by 2^28 .. 2^32 bytes is a whole number of periods of a plane of width w."""
    return all((1 << k) % plane_period_bytes(w) != 0 for k in range(28, 33)) and P % 2 == 1 and P > 1


def phases_differ(n):
    ph = [p % P for p in PHASES[:n]]
    return len(set(ph)) == n and all(p % 2 == 0 for p in PHASES[:n])


def chunks_of(case, nterms, shape):
    """{buffer: (chunk planes or fp32 channels, pixels per plane, bytes per pixel-and-plane)} of one call: operands and outputs."""
    n, h, w = shape
    px = n * h * w
    o = case.opts
    pl = 32 * (2 if nterms == 3 else 1)
    if case.kind == "tail":
        return {"blk": (14, px, pl), "y": (6, px, pl)}
    if case.kind == "bwd":
        nch = cc.chunks(case.cin)
        d = {"gy": (cc.chunks(case.cout), px, pl)}
        for k in ("res", "acc"):
            if o.get(k):
                d[k] = (nch, px, pl)
        if "mask_from" in o:
            d["mask"] = (nch, px, pl)
        d["y"] = (4 * o["y_unshuf"], px // 4, pl) if o.get("y_unshuf") else (nch, px, pl)
        if o.get("y_cpg"):                                 # the gap planes, and the gathered copy the comparison reads
            d["y"] = (nch // o["y_cpg"] * (o["y_cpg"] + 1) + nch, px, pl)
        return d
    d = {"x": (cc.x_buffer_channels(case) // 16 if o.get("x_cpg") else cc.chunks(case.cin), px, pl)}
    epi = o.get("epilogue", "planes")
    if epi == "planes":
        d["y"] = (cc.chunks(case.cout), px, pl)
        if o.get("res"):
            d["res"] = (cc.chunks(case.cout), px, pl)
    elif epi == "shuffle":
        d["y"] = (cc.chunks(case.cout // 4), 4 * px, pl)
    else:
        up = 4 if epi == "subpix" else 1
        c = case.cout // up
        d["imgs"] = (o["nimg"] * c, up * px, 4)
        d["f32"] = (c, up * px, 4)
        if epi == "subpix":
            d["f32"] = (case.cout, px, 4)                  # ops.conv2d allocates [N, cout, H, W]: the same bytes
    return d


def live_bytes(case, nterms, shape):
    """Device bytes live during the call: operands + outputs (the convolution entry points take no workspace)."""
    return sum(a * b * c for a, b, c in chunks_of(case, nterms, shape).values())


# ------------------------------------------------------------------------------------------------ period operands
def _gen(case, width, family, attempt):
    return torch.Generator().manual_seed(7919 * TAGS.index(case.tag) + 31 * width + (1 if family == "A" else 2) + 1000003 * attempt)


def _draw(case, width, family, density, attempt, what):
    """One period of the case's operands ([1, C, P, width] activations; images [1, c, up P, up width]) at a weight density; keys as
    conv_cases.white_noise_operands.  `what`: "weights" (and biases; redrawn per thinning attempt) or "activations" (drawn once)."""
    gen = _gen(case, width, family, attempt)
    if what == "weights":
        keep = lambda d: {k: v for k, v in d.items() if k in ("w", "b", "w3", "b3", "wl", "bl")}
    else:
        keep = lambda d: {k: v for k, v in d.items() if k not in ("w", "b", "w3", "b3", "wl", "bl")}
    return keep(_draw_all(case, width, family, density, gen, what == "weights"))


def _draw_all(case, width, family, density, gen, weights_only):
    o = case.opts
    if weights_only:
        act = lambda c, s=1: None
    else:
        act = (lambda c, s=1: rc._ints((1, c, s * P, s * width), gen)) if family == "A" else \
            (lambda c, s=1: rc._split_values((1, c, s * P, s * width), gen))

    def weight(*s):
        if not weights_only:
            return None
        v = torch.randint(-2, 3, s, generator=gen).float() if family == "A" else rc._split_values(s, gen)
        return v * (torch.rand(s, generator=gen) < density).float()

    bias = lambda c: torch.randint(-3, 4, (c,), generator=gen).float()
    if case.kind == "tail":
        wl = weight(96, 224, 1, 1)
        if family == "B" and wl is not None:
            wl[:, 192:] = wl[:, 192:].round()
        return {"blk": act(224), "w3": weight(32, 192, 3, 3), "b3": bias(32), "wl": wl, "bl": bias(96)}
    wt = weight(case.cout, case.cin, case.ks, case.ks)
    if case.kind == "bwd":
        nch16 = cc.chunks(case.cin) * 16
        return {"w": wt, "gy": act(case.cout), "res": act(nch16) if o.get("res") else None, "acc": act(nch16) if o.get("acc") else None,
                "mask": rc._ints((1, nch16, P, width), gen) if "mask_from" in o and not weights_only else None}
    epi = o.get("epilogue", "planes")
    imgs, res = [], None
    if epi in ("final", "subpix") and not weights_only:
        up, nimg = (2 if epi == "subpix" else 1), o.get("nimg", 0)
        imgs = [rc._ints((1, case.cout // (up * up), up * P, up * width), gen, False) * nimg for _ in range(nimg)]
    elif o.get("res"):
        res = act(case.cout)
    return {"w": wt, "b": bias(case.cout), "x": act(cc.x_buffer_channels(case)), "imgs": imgs, "res": res}


def _mag(t, nterms=3):
    """max(|hi| + |lo|) of an activation as stored."""
    hi, lo = rc.split16(t, nterms)
    return float((hi.abs() + lo.abs()).max())


def _wsum(w, dims):
    hi, lo = rc.split16(w, 3)
    return (hi.abs() + lo.abs()).sum(dims)


def _on_grid(t, family):
    grid = 1.0 if family == "A" else 2.0 ** 11
    return bool((t * grid == (t * grid).round()).all())          # (exact in fp32: a power-of-two scale)


def _act_facts(family, opnd):
    """{name: (on the family's grid, max(|hi| + |lo|))} of the activations and images of a period: what the analytic conditions need of
    them (computed once per period; the weights are redrawn)."""
    f = {}
    for k, v in opnd.items():
        if k == "imgs":
            f[k] = (all(_on_grid(t, family) for t in v), max([float(t.abs().max()) for t in v] or [0.0]))
        elif k in ACTIVATIONS and v is not None:
            f[k] = (_on_grid(v, family), _mag(v))
    return f


def sufficient_conditions(case, family, opnd, facts=None):
    """The analytic, shape-independent form of conv_ref_cases.conditions() (module docstring): a list of the broken ones."""
    scale = 1.0 if family == "A" else 2.0 ** 11
    facts = facts if facts is not None else _act_facts(family, opnd)
    bad = [f"operand {k} is off the grid" for k, (ok, _) in facts.items() if not ok]
    bad += [f"operand {k} is off the grid" for k, v in opnd.items() if k not in facts and v is not None and not isinstance(v, list)
            and not _on_grid(v, family)]
    mag = lambda name: facts[name][1]
    o = case.opts
    stored = {}
    if case.kind == "tail":
        xm = mag("blk")
        o3 = xm * float(_wsum(opnd["w3"], (1, 2, 3)).max()) + float(opnd["b3"].abs().max())
        wl = _wsum(opnd["wl"], (2, 3))
        y = float((wl[:, :192].sum(1) * xm + wl[:, 192:].sum(1) * o3).max()) + float(opnd["bl"].abs().max()) + xm
        stored = {"o3": o3, "y": y}
        bounds = dict(stored)
        if family == "B" and bool(rc.split16(opnd["wl"], 3)[1][:, 192:].any()):
            bad.append("LFF lo weights on the o3 columns")
    elif case.kind == "bwd":
        b = mag("gy") * float(_wsum(opnd["w"], (0, 2, 3)).max())
        b += sum(mag(k) for k in ("res", "acc") if opnd[k] is not None)
        stored = bounds = {"y": b}
    else:
        b = mag("x") * float(_wsum(opnd["w"], (1, 2, 3)).max()) + float(opnd["b"].abs().max())
        if opnd["res"] is not None:
            b += mag("res")
        if opnd["imgs"]:
            b += facts["imgs"][1]
        bounds = {"y": b}
        stored = {} if o.get("epilogue") in ("final", "subpix") else bounds
    for nm, b in bounds.items():
        if not b * scale < rc.EXACT_LIMIT:
            bad.append(f"{nm}: bound {b * scale:.4g} >= 2^24")
    for nm, b in stored.items():
        if not b <= rc.F16_EXACT_INT:
            bad.append(f"{nm}: stored bound {b:.6g} > 2048")
    return bad


@functools.lru_cache(maxsize=None)
def period_operands(tag, family, width):
    """One period of operands (fp32 CPU tensors, cached, never modified): the weights are thinned until sufficient_conditions holds."""
    case = BY_TAG[tag]
    density = 1.0 if family == "A" else 0.1
    acts = _draw(case, width, family, 0.0, 0, "activations")
    facts = _act_facts(family, acts)
    for attempt in range(14):
        opnd = dict(acts, **_draw(case, width, family, density, 1 + attempt, "weights"))
        if not sufficient_conditions(case, family, opnd, facts):
            assert float(opnd["w3" if case.kind == "tail" else "w"].abs().sum()) > 0, (tag, family, "the weights were thinned to nothing")
            return opnd
        density *= 0.5
    raise AssertionError(f"{tag} {family}: no weight density down to {density} meets the conditions")


ACTIVATIONS = ("x", "res", "gy", "acc", "mask", "blk")


def band_operands(case, opnd, n, r0, r1, dev):
    """The operands of input rows r0 .. r1 - 1 of image n, as conv_ref_cases.reference() takes them, on `dev`."""
    idx = (torch.arange(r0, r1) + PHASES[n]) % P
    out = {}
    for k, v in opnd.items():
        if k in ACTIVATIONS and v is not None:
            out[k] = v[:, :, idx].to(dev)
        elif k == "imgs":
            up = 2 if case.opts.get("epilogue") == "subpix" else 1
            iidx = (torch.arange(up * r0, up * r1) + up * PHASES[n]) % (up * P)
            out[k] = [t[:, :, iidx].to(dev) for t in v]
        else:
            out[k] = None if v is None else v.to(dev)
    return out


# ------------------------------------------------------------------------------------------------ plane layout, device expansion
def to_planes(x):
    """NCHW -> [chunks, N, H, W, 16], channels zero-padded (any dtype, any device)."""
    n, c, h, w = x.shape
    nch = (c + 15) // 16
    if c % 16:
        x = F.pad(x, (0, 0, 0, 0, 0, nch * 16 - c))
    return x.reshape(n, nch, 16, h, w).permute(1, 0, 3, 4, 2).contiguous()


def split_planes(v, nterms):
    """(hi, lo or None) fp16 planes of an fp32 / fp64 NCHW tensor whose values are fp32 numbers: the stored split."""
    v = v.float()
    hi = v.half()
    lo = (v - hi.float()).half() if nterms == 3 else None
    return to_planes(hi), (to_planes(lo) if nterms == 3 else None)


Planes = namedtuple("Planes", "hi lo")          # what the library wrappers read: .hi, .lo (bin_amd.ops.CP has the same two)


def expand_rows(per, n_images, h, period, phase):
    """per [A, 1 or absent.., period, B...] -> [A, N, H, ...]: row r of image n is per row (r + phase(n)) mod period; gathered on per's
    device, one index_select per (a, n) straight into the result."""
    a = per.shape[0]
    rest = tuple(per.shape[2:])
    out = torch.empty((a, n_images, h) + rest, dtype=per.dtype, device=per.device)
    for n in range(n_images):
        idx = ((torch.arange(h, device=per.device) + phase(n)) % period)
        for i in range(a):
            torch.index_select(per[i], 0, idx, out=out[i, n])
    return out


def expand_operands(case, nterms, shape, opnd, dev):
    """{name: Planes} of the activations at `shape`, {"imgs": [fp32 NCHW]}: the periodic device tensors."""
    n, h, w = shape
    out = {}
    for k in ACTIVATIONS:
        v = opnd.get(k)
        if v is None:
            out[k] = None
            continue
        hi, lo = split_planes(v.to(dev), nterms)                       # [chunks, 1, P, W, 16]
        ph = lambda i: PHASES[i]
        out[k] = Planes(expand_rows(hi[:, 0], n, h, P, ph), expand_rows(lo[:, 0], n, h, P, ph) if lo is not None else None)
    if opnd.get("imgs"):
        up = 2 if case.opts.get("epilogue") == "subpix" else 1
        imgs = []
        for t in opnd["imgs"]:
            e = expand_rows(t[0].to(dev), n, up * h, up * P, lambda i: up * PHASES[i])       # [c, N, upH, upW]
            imgs.append(e.permute(1, 0, 2, 3).contiguous())
        out["imgs"] = imgs
    return out


# ------------------------------------------------------------------------------------------------ the every-pixel comparison
def out_views(case, nterms, outs):
    """[(name, tensor viewed as [A, N, rows, B])] of the outputs a call returned ({"y": .hi/.lo planes, "o3": .., "f32": NCHW})."""
    v = []
    for nm in rc.output_names(case):
        t = outs[nm]
        if nm == "f32":
            v.append(("f32", t.permute(1, 0, 2, 3)))
        else:
            c, n, h, w, _ = t.hi.shape
            v.append((nm + ".hi", t.hi.reshape(c, n, h, w * 16)))
            if nterms == 3:
                v.append((nm + ".lo", t.lo.reshape(c, n, h, w * 16)))
    return v


def ref_views(case, nterms, ref):
    """The float64 reference {name: [1, C, rows, W]} in the same views: [(name, [A, rows, B])], stored as the kernel stores it."""
    v = []
    for nm in rc.output_names(case):
        r = ref[nm]
        if nm == "f32":
            v.append(("f32", r[0].float()))
            assert torch.equal(v[-1][1].double(), r[0]), "the reference is not an fp32 number"
        else:
            hi, lo = split_planes(r, nterms)
            a, _, rows, w, _ = hi.shape
            v.append((nm + ".hi", hi.reshape(a, rows, w * 16)))
            if nterms == 3:
                v.append((nm + ".lo", lo.reshape(a, rows, w * 16)))
    return v


def _mismatch(got, exp, where, bad, limit=6):
    ne = got != exp
    k = int(ne.sum())
    if k and len(bad) < limit:
        at = tuple(int(i) for i in ne.nonzero()[0])
        bad.append(f"{where}: {k} elements differ, first at {at}: got {float(got[at])!r} expected {float(exp.expand_as(got)[at])!r}")
    return k


def compare_periodic(name, view, per, period, phase, n_images, lo_row, hi_row, bad):
    """Rows lo_row .. hi_row - 1 of every image of view [A, N, H, B] against per [A, period, B]: row y of image n must equal per row
    (y + phase(n)) mod period.  Whole periods are compared by broadcasting; returns the number of rows compared."""
    a = view.shape[0]
    rows = 0
    for n in range(n_images):
        first = lo_row + (-(lo_row + phase(n))) % period               # the first row that starts a period
        m = max((hi_row - first) // period, 0)
        rest = ((lo_row, first), (first + m * period, hi_row)) if m else ((lo_row, hi_row),)
        for i in range(a):
            if m:
                blk = view[i, n, first:first + m * period].unflatten(0, (m, period))
                _mismatch(blk, per[i][None], f"{name} image {n} plane {i} rows {first}.. (period, row in period, element)", bad)
            for r0, r1 in rest:
                if r1 > r0:
                    idx = (torch.arange(r0, r1, device=view.device) + phase(n)) % period
                    _mismatch(view[i, n, r0:r1], per[i][idx], f"{name} image {n} plane {i} rows {r0}..{r1 - 1}", bad)
        rows += max(hi_row - lo_row, 0)
    return rows


def bands_of(case, shape):
    """[(image, first input row, one past the last, first and one-past-last VALID output row)] of the float64 bands: the long top band
    of image 0 and a short band at every other image edge.  Output rows are in output units."""
    n, h, w = shape
    hl, s = halo(case), row_scale(case)
    long_rows = int(out_period(case)[0] / s) + 2 * hl + 2              # one whole output period between the edge and the cut
    long_rows += long_rows % 2                                         # whole output rows of the unshuffle store
    short = 2 * hl + 2
    out = []
    for i in range(n):
        top = min(long_rows if i == 0 else short, h)
        out.append((i, 0, top, 0, int((top - (hl if top < h else 0)) * s)))
        bot = min(short, h)
        out.append((i, h - bot, h, -((-(h - bot + hl) * s.numerator) // s.denominator), int(h * s)))
    return out


def check_outputs(case, nterms, family, shape, opnd, outs, dev, label="kernel", ref_dev=None):
    """Hold EVERY row of the outputs of one call at `shape` to float64: the bands by their own reference, every other row by the
    verified period; the family's conditions are evaluated on the top band and must hold.  Returns {"views": the names of the output
    views compared, "rows": output rows per view, all of them compared}; raises AssertionError naming view, image, plane, row and element."""
    n, h, w = shape
    hl, s = halo(case), row_scale(case)
    hl_out = -(-hl * s.numerator // s.denominator)
    period, phase = out_period(case)
    views = out_views(case, nterms, outs)
    h_out = int(h * s)
    bad, cond, covered = [], None, {}
    pers = None
    lo_row, hi_row = {}, {}
    for (img, r0, r1, v0, v1) in bands_of(case, shape):
        bo = band_operands(case, opnd, img, r0, r1, ref_dev if ref_dev is not None else dev)
        if cond is None:
            cond = [rc.conditions(case, nt, family, bo) for nt in ((3, 1) if family == "A" else (3,))]
        ref = rc.reference(case, nterms, rc.as_read(bo, nterms))
        o0 = int(r0 * s)                                               # output row of the band's first row
        rv = [(nm, t.to(dev)) for nm, t in ref_views(case, nterms, ref)]
        for (nm, view), (nm2, exp) in zip(views, rv):
            assert nm == nm2 and view.shape[0] == exp.shape[0] and view.shape[3] == exp.shape[2], (nm, nm2, tuple(view.shape), tuple(exp.shape))
            _mismatch(view[:, img, v0:v1], exp[:, v0 - o0:v1 - o0], f"{nm} image {img} band rows {v0}..{v1 - 1} (plane, row - {v0}, element)", bad)
            covered.setdefault(nm, torch.zeros(n, h_out, dtype=torch.bool))[img, v0:v1] = True
        if img == 0 and r0 == 0:                                       # the interior period, out of the verified long band
            assert v1 - hl_out >= period, "the long band holds no whole interior period"
            rows = torch.arange(hl_out, hl_out + period)
            order = torch.empty(period, dtype=torch.long)
            order[(rows + phase(0)) % period] = rows
            pers = [(nm, exp[:, order.to(exp.device)]) for nm, exp in rv]
    for (nm, view), (_, per) in zip(views, pers):
        compare_periodic(nm, view, per, period, phase, n, hl_out, h_out - hl_out, bad)
        covered[nm][:, hl_out:h_out - hl_out] = True
        assert bool(covered[nm].all()), f"{nm}: rows left unchecked"
    assert not any(cond), (case.tag, family, shape, "the family's conditions fail on the top band", cond)
    assert not bad, (case.tag, nterms, family, shape, label, bad)
    return {"views": [nm for nm, _ in views], "rows": n * h_out}


# ------------------------------------------------------------------------------------------------ the library call, and a stand-in
def call_library(case, nterms, shape, opnd, dev_in):
    """One call of the library at `shape` on the expanded device operands `dev_in`; weights and bias from `opnd`.  Returns the outputs
    as conv_cases.call_library does.  Output buffers come from the wrappers' own torch.empty (guarded under poison.poisoned)."""
    from bin_amd import _lib as L, ops
    n, h, w = shape
    o = case.opts
    cp = lambda p, ch=None: None if p is None else ops.CP(p.hi, p.lo, ch if ch is not None else p.hi.shape[0] * 16)
    if case.kind == "tail":
        blk = cp(dev_in["blk"], 224)
        cw3 = ops.ConvWeights(opnd["w3"].cuda(), opnd["b3"].cuda(), nterms=nterms)
        cwl = ops.ConvWeights(opnd["wl"].cuda(), opnd["bl"].cuda(), nterms=nterms)
        y = ops.rdb_tail(blk, cw3, cwl, store_o3=bool(o.get("store_o3")))
        return {"y": y, "o3": blk.sub(12, 2)} if o.get("store_o3") else {"y": y}
    if case.kind == "bwd":
        if o.get("gather"):                                            # bin_stage4's block (96, 4, 32): conv c is [32, 96 + 32 c, 3, 3]
            g = o["gather"]
            block = [torch.zeros(32, 96 + 32 * c, 3, 3) for c in range(4)]
            block[g][:, 96 + 32 * (g - 1):96 + 32 * g] = opnd["w"]
            dw = ops.RdbGatherWeights([t.cuda() for t in block], g, nterms)
        else:
            dw = ops.DgradWeights(opnd["w"].cuda(), nterms=nterms)
        kw = {}
        if o.get("y_cpg"):                                             # as test_gff0_backward_data_scatters_into_groups: guarded gap planes
            cpg, nch = o["y_cpg"], cc.chunks(case.cin)
            out = ops.CP.empty(nch // cpg * (cpg + 1), n, h, w, nterms, torch.device("cuda"))
            out.hi.fill_(rc.GUARD_HI)
            if out.lo is not None:
                out.lo.fill_(rc.GUARD_LO)
            kw = dict(out=out, y_cpg=cpg, y_group_stride=(cpg + 1) * n * h * w * 16)
        y = ops.conv2d_bwd_data(cp(dev_in["gy"]), dw, res=cp(dev_in["res"]), res_chunks=o.get("res_chunks", 0), acc=cp(dev_in["acc"]),
                                mask=cp(dev_in["mask"]), mask_from=o.get("mask_from", 0), y_unshuf=o.get("y_unshuf", 0), **kw)
        if o.get("y_cpg"):
            data = [g * (cpg + 1) + i for g in range(nch // cpg) for i in range(cpg)]
            gaps = [g * (cpg + 1) + cpg for g in range(nch // cpg)]
            assert bool((y.hi[gaps] == rc.GUARD_HI).all()), "a gap plane was written (hi)"
            assert y.lo is None or bool((y.lo[gaps] == rc.GUARD_LO).all()), "a gap plane was written (lo)"
            y = ops.CP(y.hi[data], None if y.lo is None else y.lo[data], nch * 16)
        return {"y": y}
    epi = o.get("epilogue", "planes")
    cw = ops.ConvWeights(opnd["w"].cuda(), opnd["b"].cuda(), nterms=nterms, shuffle=epi == "shuffle")
    kw = {}
    if o.get("x_cpg"):
        kw = dict(x_cpg=o["x_cpg"], x_group_stride=(o["x_cpg"] + 1) * n * h * w * 16)
    x = cp(dev_in["x"])
    if epi in ("final", "subpix"):
        y = ops.conv2d(x, cw, epilogue=L.EPI_FINAL if epi == "final" else L.EPI_FINAL_SUBPIX, images=dev_in["imgs"], **kw)
        return {"f32": y.view(n, case.cout // 4, 2 * h, 2 * w) if epi == "subpix" else y}
    if epi == "shuffle":
        return {"y": ops.conv2d(x, cw, epilogue=L.EPI_SHUFFLE, **kw)}
    return {"y": ops.conv2d(x, cw, relu=bool(o.get("relu")), residual=cp(dev_in["res"]), **kw)}


WRONG = ("row_wrapped_mod_64", "image_1_reads_image_0", "last_row_dropped", "one_row_fetched_as_zeros", "store_one_row_late")


def _nchw(p, nterms):
    """Planes -> (hi, lo) float64 NCHW, as conv_ref_cases.reference() reads an activation."""
    f = lambda t: t.permute(1, 0, 4, 2, 3).reshape(t.shape[1], t.shape[0] * 16, t.shape[2], t.shape[3]).double()
    hi = f(p.hi)
    return hi, (f(p.lo) if nterms == 3 else torch.zeros_like(hi))


def stand_in(case, nterms, shape, opnd, dev_in, wrong=None):
    """float32 torch as the kernel, on the expanded operands at a (small) shape, with the kernels' stores applied; `wrong`: one of
    WRONG, a deliberately wrong restatement."""
    n, h, w = shape
    R = {}
    for k, v in opnd.items():
        if k in ACTIVATIONS:
            R[k] = None if v is None else _nchw(dev_in[k], nterms)
        elif k == "imgs":
            R[k] = [t.double() for t in dev_in.get("imgs", [])]
        else:
            R[k] = None if v is None else (v.double() if k in ("b", "b3", "bl") else rc.split16(v, nterms))
    main = "blk" if case.kind == "tail" else "gy" if case.kind == "bwd" else "x"

    def rows_from(src_rows):
        R[main] = tuple(t[:, :, src_rows] for t in R[main])
    if wrong == "row_wrapped_mod_64":
        rows_from(torch.arange(h) % 64)
    elif wrong == "image_1_reads_image_0":
        R[main] = tuple(t[[0] + list(range(0, n - 1))] if n > 1 else t for t in R[main])
        if n == 1:
            return None
    elif wrong == "one_row_fetched_as_zeros":
        R[main] = tuple(t.clone() for t in R[main])
        for t in R[main]:
            t[:, :, h // 2] = 0
    out = rc.reference(case, nterms, R, dt=torch.float32)
    res = {}
    for nm in rc.output_names(case):
        v = out[nm].float()
        if wrong == "last_row_dropped":
            v = v.clone()
            v[:, :, -1] = 0
        elif wrong == "store_one_row_late":
            v = torch.cat((torch.zeros_like(v[:, :, :1]), v[:, :, :-1]), 2)
        if nm == "f32":
            res[nm] = v
        else:
            res[nm] = Planes(*split_planes(v, nterms))
    return res


# ------------------------------------------------------------------------------------------------ weight gradient: census and bands
WGRAD_KS = (3, 5, 1)                     # wgrad3x3_xrow_kernel, wgrad_mfma_kernel<5,..>, wgrad1x1_kernel
WGRAD_CIN, WGRAD_COUT = 16, 32
BAND_ROWS = 8


def census_counts(shape, ks):
    """dW[0, 0, dy, dx] of the census, in integer arithmetic: the number of x pixels (flat index divisible by 4) at (y', x') whose
    output pixel (y' - dy + c, x' - dx + c) lies in the same image."""
    n, h, w = shape
    c = ks // 2
    out = np.zeros((ks, ks), np.int64)
    img = np.arange(n, dtype=np.int64)[:, None]
    for dy in range(ks):
        oy = dy - c
        ys = np.arange(max(0, oy), min(h, h + oy), dtype=np.int64)[None, :]
        base = (img * h + ys) * w                                     # flat index of the row's first pixel
        for dx in range(ks):
            ox = dx - c
            xa, xb = max(0, ox), min(w, w + ox)
            if xb <= xa or ys.size == 0:
                continue
            out[dy, dx] = int(((base + xb - 1) // 4 - (base + xa - 1) // 4).sum())
    return out


def census_brute(shape, ks):
    n, h, w = shape
    x = (torch.arange(n * h * w) % 4 == 0).double().view(n, 1, h, w)
    dw, _ = wg.reference(x, torch.ones(n, 1, h, w), ks)
    return dw[0, 0].round().long().numpy()


def census_planes(shape, nterms, dev):
    """(x, g) Planes of the census at `shape`: x one chunk, g two (cout 32)."""
    n, h, w = shape

    def zeros(ch):
        t = torch.empty((ch, n, h, w, 16), dtype=torch.float16, device=dev)
        t.zero_()
        return t
    x, g = zeros(1), zeros(2)
    x.view(-1, 16)[::4, 0] = 1
    g[0].view(-1, 16)[:, 0] = 1
    return Planes(x, zeros(1) if nterms == 3 else None), Planes(g, zeros(2) if nterms == 3 else None)


def band_starts(shape):
    """First rows (global row index n H + r) of the 8-row bands: the top of image 0, the bottom of the last image, straddling the plane
    byte offsets 2^28, 2^29, 2^30, and ending on the last row below 2^31 — merged into runs that stay inside one image."""
    n, h, w = shape
    total = n * h
    want = [0, total - BAND_ROWS]
    for k in (28, 29, 30):
        want.append(((1 << k) // 32) // w - BAND_ROWS // 2)            # the row that holds that byte, four rows above it
    want.append(min(((1 << 31) // 32 - 1) // w, total - 1) - BAND_ROWS + 1)
    rows = sorted({r for s in want for r in range(max(s, 0), min(s + BAND_ROWS, total))})
    runs, start = [], rows[0]
    for a, b in zip(rows, rows[1:] + [None]):
        if b is None or b != a + 1 or b % h == 0:                      # a gap, or the next image begins
            runs.append((start, a + 1))
            start = b
    return runs


def band_values(shape, ks, family, run_index, rows):
    """(x [1, cin, rows, W], g [1, cout, rows, W]) fp32 of one band, thinned so that the sum over ALL bands keeps the 2^24 condition."""
    n, h, w = shape
    gen = torch.Generator().manual_seed(104729 * run_index + 31 * w + ks + (0 if family == "A" else 7))
    npix = 6 * BAND_ROWS * w
    if family == "A":
        x = torch.randint(-3, 4, (1, WGRAD_CIN, rows, w), generator=gen).float()
        g = torch.randint(-3, 4, (1, WGRAD_COUT, rows, w), generator=gen).float() * wg.channel_mults(WGRAD_COUT).view(1, -1, 1, 1)
        keep = min(1.0, (1 << 23) / (npix * 45.0))                     # |x| <= 3, |g| <= 15: sum|x||g| <= 45 per pixel pair
    else:
        xa, xb = wg._split_values((1, WGRAD_CIN, rows, w), gen)
        ga, gb = wg._split_values((1, WGRAD_COUT, rows, w), gen)
        x, g = xa + xb * 2.0 ** -11, ga + gb * 2.0 ** -11
        keep = min(0.10, 1400.0 / npix)
    g = g * (torch.rand(g.shape, generator=gen) < keep).float()
    return x, g


def wgrad_ref(x, g, ks):
    """(dW, db) float64 of one image stack by the definition dW[co][ci][dy][dx] = sum_px g[co][px] x[ci][px + tap], one matrix product
    per tap (tests/test_cpu_domain_top.py holds it to wgrad_cases.reference)."""
    x, g = x.double(), g.double()
    c = ks // 2
    n, _, h, w = x.shape
    xp = F.pad(x, (c, c, c, c))
    dw = torch.stack([torch.stack([torch.einsum("nohw,nihw->oi", g, xp[:, :, dy:dy + h, dx:dx + w]) for dx in range(ks)], -1)
                      for dy in range(ks)], -2)
    return dw, g.sum((0, 2, 3))


def wgrad_split_ref(x, g, ks, nterms):
    """The kernels' definition on the stored planes (wgrad_cases.split_reference): xh gh + xl gh + xh gl; nterms 1: the hi planes."""
    xh, xl = wg.split16(x)
    gh, gl = wg.split16(g)
    if nterms == 1:
        return wgrad_ref(xh, gh, ks)
    d1, b1 = wgrad_ref(xh.double() + xl.double(), gh, ks)
    d2, b2 = wgrad_ref(xh, gl, ks)
    return d1 + d2, b1 + b2


def band_reference(shape, ks, family, nterms, dev="cpu"):
    """(runs, [(x, g)], dW, db, bound): the float64 result of the bands alone, and the same sum on absolute values (the condition)."""
    runs = band_starts(shape)
    data, dw, db, bw, bb = [], 0, 0, 0.0, 0.0
    for i, (a, b) in enumerate(runs):
        x, g = band_values(shape, ks, family, i, b - a)
        data.append((x, g))
        x, g = x.to(dev), g.to(dev)
        d, e = wgrad_split_ref(x, g, ks, nterms)
        dw, db = dw + d, db + e
        hi_lo = lambda t: sum(p.abs() for p in wg.split16(t))           # |hi| + |lo| (an fp32 number: the split of the sum is the pair again)
        d, e = wgrad_ref(hi_lo(x), hi_lo(g), ks)
        bw, bb = bw + float(d.max()), bb + float(e.max())
    return runs, data, dw.cpu(), db.cpu(), max(bw, bb)


def band_planes(shape, nterms, runs, data, dev):
    n, h, w = shape

    def zeros(ch):
        t = torch.empty((ch, n, h, w, 16), dtype=torch.float16, device=dev)
        t.zero_()
        return t
    x = Planes(zeros(1), zeros(1) if nterms == 3 else None)
    g = Planes(zeros(2), zeros(2) if nterms == 3 else None)
    for (a, b), (xv, gv) in zip(runs, data):
        img, r0 = a // h, a % h
        for dst, v in ((x, xv), (g, gv)):
            hi, lo = split_planes(v.to(dev), nterms)
            dst.hi[:, img, r0:r0 + b - a] = hi[:, 0]
            if nterms == 3:
                dst.lo[:, img, r0:r0 + b - a] = lo[:, 0]
    return x, g


def wgrad_live_bytes(shape, ks, nterms):
    from bin_amd import _lib as L
    n, h, w = shape
    ws = L.lib().binhip_wgrad_workspace_bytes(ks, n, h, w, 1, WGRAD_COUT)
    return 3 * n * h * w * 32 * (2 if nterms == 3 else 1) + ws, ws


# ------------------------------------------------------------------------------------------------ layout glue
LAYOUT_C = 16                            # channels of the nchw <-> planes round trip: one chunk


# ------------------------------------------------------------------------------------------------ ConvLSTM (fp32 NCHW, hidden 3)
# The cell runs at quarter resolution of a plan frame, so N H W just under 2^24 is its top.  Not exact: the bars of lstm_cases.py,
# max(B, 4 e32), unchanged, on the bands AND on the periodicity compare.  Per-pixel outputs (c, h, gx, gcp, ghp; gx and ghp see the
# gates of a 3 x 3 neighbourhood, themselves 3 x 3 of the inputs: halo 2) go by the periodic method.  dw and db are sums over all
# pixels; a row's contribution depends on that row and its two neighbours alone, and is linear in (gh, gc), so the float64 total is
# ONE backward through a batch of three-row images, the middle row's upstream gradients weighted by how often that row occurs:
# the P interior rows of the period (weight: the number of interior rows of all images in that phase), and per image its first row
# under a zero row and its last row over one (weight 1).
LSTM_SHAPES = ((2, 2048, 4095), (1, 239674, 70))
LSTM_HALO = 2
LSTM_FB = 1.0
LSTM_PIXEL_OUTPUTS = ("c", "h", "gx", "gcp", "ghp")
LSTM_PLANES = ("x", "c0", "h0", "gh", "gc")


def lstm_period(width, seed=7):
    """One period of the cell's fp32 inputs ([3, P, width] each, drawn as lstm_cases.make_inputs draws its moderate regime) and w, b."""
    g = torch.Generator().manual_seed(seed * 100003 + 31 * width)
    shp = (3, P, width)
    d = {"x": torch.rand(shp, generator=g), "c0": (torch.rand(shp, generator=g) - 0.5) * 2.0, "h0": (torch.rand(shp, generator=g) - 0.5) * 2.0}
    d["w"] = (torch.rand(12, 6, 3, 3, generator=g) - 0.5) * 2 * 0.2
    d["b"] = (torch.rand(12, generator=g) - 0.5) * 2 * 0.2
    d["gh"], d["gc"] = torch.rand(shp, generator=g) - 0.5, torch.rand(shp, generator=g) - 0.5
    return d


def lstm_eval(inp, dtype, row_weight=None):
    """The oracle cell and its autograd gradients in `dtype` on inp (x, c0, h0, gh, gc [B, 3, rows, W]; w, b); `row_weight`
    [B, 1, rows, 1] multiplies the upstream gradients."""
    from oracle import rdn_oracle as O
    T = lambda t: t.to(dtype).clone().requires_grad_(True)
    x, c0, h0, w, b = (T(inp[k]) for k in ("x", "c0", "h0", "w", "b"))
    h, (c, _) = O.convlstm_cell(x, [c0, h0], w, b, forget_bias=LSTM_FB)
    gh, gc = inp["gh"].to(dtype), inp["gc"].to(dtype)
    if row_weight is not None:
        gh, gc = gh * row_weight.to(dtype), gc * row_weight.to(dtype)
    ((h * gh).sum() + (c * gc).sum()).backward()
    return {"c": c.detach(), "h": h.detach(), "gx": x.grad, "gcp": c0.grad, "ghp": h0.grad, "dw": w.grad, "db": b.grad}


def lstm_band(per, n, r0, r1, dev):
    idx = (torch.arange(r0, r1) + PHASES[n]) % P
    d = {k: per[k][:, idx][None].to(dev) for k in LSTM_PLANES}
    d["w"], d["b"] = per["w"].to(dev), per["b"].to(dev)
    return d


def lstm_sum_batch(per, shape, dev):
    """(inputs [P + 2 N, 3, 3, W], row_weight): the three-row images whose weighted backward is the whole tensor's dw, db."""
    n, h, w = shape
    assert h >= 3
    rows, weights = [], []
    counts = np.zeros(P, np.int64)
    for i in range(n):
        counts += np.bincount((np.arange(1, h - 1) + PHASES[i]) % P, minlength=P)
    for j in range(P):
        rows.append(((j - 1) % P, j, (j + 1) % P))
        weights.append(float(counts[j]))
    for i in range(n):
        rows.append((None, PHASES[i] % P, (1 + PHASES[i]) % P))
        rows.append(((h - 2 + PHASES[i]) % P, (h - 1 + PHASES[i]) % P, None))
        weights += [1.0, 1.0]
    zero = torch.zeros(3, w)
    d = {k: torch.stack([torch.stack([zero if r is None else per[k][:, r] for r in tri], 1) for tri in rows]).to(dev) for k in LSTM_PLANES}
    d["w"], d["b"] = per["w"].to(dev), per["b"].to(dev)
    rw = torch.zeros(len(rows), 1, 3, 1)
    rw[:, 0, 1, 0] = torch.tensor(weights)
    return d, rw.to(dev)


def max_diff_periodic(view, per, period, phase, n_images, lo_row, hi_row):
    """max |view - expanded period| over rows lo_row .. hi_row - 1 of every image (NaN if any element is NaN)."""
    worst = torch.zeros((), dtype=torch.float64, device=view.device)
    for n in range(n_images):
        first = lo_row + (-(lo_row + phase(n))) % period
        m = max((hi_row - first) // period, 0)
        rest = ((lo_row, first), (first + m * period, hi_row)) if m else ((lo_row, hi_row),)
        for i in range(view.shape[0]):
            if m:
                d = (view[i, n, first:first + m * period].unflatten(0, (m, period)) - per[i][None]).abs()
                worst = torch.maximum(worst, torch.where(torch.isnan(d).any(), torch.full_like(worst, float("nan")), d.max().double()))
            for r0, r1 in rest:
                if r1 > r0:
                    idx = (torch.arange(r0, r1, device=view.device) + phase(n)) % period
                    d = (view[i, n, r0:r1] - per[i][idx]).abs()
                    worst = torch.maximum(worst, torch.where(torch.isnan(d).any(), torch.full_like(worst, float("nan")), d.max().double()))
    return float(worst)


def lstm_check(shape, per, got, dev, ref_dev, label="kernel"):
    """Every pixel of c, h, gx, gcp, ghp ([N, 3, H, W] on dev) and dw, db against float64 under lstm_cases' bars; returns
    {name: (e32, bar, error)}."""
    import lstm_cases as lc
    n, h, w = shape
    hl = LSTM_HALO
    long_rows = min(P + 2 * hl + 2, h)
    short = min(2 * hl + 2, h)
    bands = [(0, 0, long_rows, 0, long_rows - hl)]
    for i in range(n):
        if i:
            bands.append((i, 0, short, 0, short - hl))
        bands.append((i, h - short, h, h - short + hl, h))
    res, worst, scale, e32 = {}, {}, {}, {}
    pers = None
    phase = lambda i: PHASES[i]
    for (img, r0, r1, v0, v1) in bands:
        inp = lstm_band(per, img, r0, r1, ref_dev)
        r64 = lstm_eval(inp, torch.float64)
        if pers is None:
            r32 = lstm_eval(inp, torch.float32)
            order = torch.empty(P, dtype=torch.long)
            rows = torch.arange(hl, hl + P)
            order[rows % P] = rows
            pers = {nm: r64[nm][0][:, order.to(ref_dev)].float().to(dev) for nm in LSTM_PIXEL_OUTPUTS}
            for nm in LSTM_PIXEL_OUTPUTS:
                scale[nm] = 1.0 if nm in ("c", "h") else max(float(r64[nm][0, :, hl:hl + P].abs().max()), 1e-12)
                e32[nm] = float((r32[nm].double() - r64[nm])[0, :, :v1].abs().max()) / scale[nm]
        for nm in LSTM_PIXEL_OUTPUTS:
            d = (got[nm][img, :, v0:v1].double() - r64[nm][0, :, v0 - r0:v1 - r0].to(dev)).abs()
            worst[nm] = max(worst.get(nm, 0.0), float("nan") if bool(torch.isnan(d).any()) else float(d.max()))
    bad = []
    for nm in LSTM_PIXEL_OUTPUTS:
        e = max_diff_periodic(got[nm].permute(1, 0, 2, 3), pers[nm], P, phase, n, hl, h - hl)
        e = (float("nan") if e != e or worst[nm] != worst[nm] else max(e, worst[nm])) / scale[nm]
        bb = lc.bar(nm, e32[nm])
        res[nm] = (e32[nm], bb, e)
        if not e <= bb:
            bad.append((nm, e, bb))
    batch, rw = lstm_sum_batch(per, shape, ref_dev)
    s64, s32 = lstm_eval(batch, torch.float64, rw), lstm_eval(batch, torch.float32, rw)
    for nm in ("dw", "db"):
        ee = lc.err(nm, s32[nm].cpu(), s64[nm].cpu())
        bb = lc.bar(nm, ee)
        e = lc.err(nm, got[nm].detach().cpu(), s64[nm].cpu())
        res[nm] = (ee, bb, e)
        if not e <= bb:
            bad.append((nm, e, bb))
    for nm, (a, bb, e) in res.items():
        print(f"[domain-top] lstm shape={rc.shape_str(shape)} {nm}: e32={a:.3e} bar={bb:.3e} {label}={e:.3e} ratio={e / bb:.3f}")
    assert not bad, (shape, bad)
    return res


def lstm_expand(per, shape, dev):
    """{x, c0, h0, gh, gc: fp32 [N, 3, H, W]} periodic on dev."""
    n, h, w = shape
    return {k: expand_rows(per[k].to(dev), n, h, P, lambda i: PHASES[i]).permute(1, 0, 2, 3).contiguous() for k in LSTM_PLANES}


# ------------------------------------------------------------------------------------------------ one plan call
# binhip_rdn_forward at the largest even frame with the smallest supported configuration, 5 inputs: white-noise periodic frames (full
# resolution: period 2 P rows, the even PHASES, so that the half-resolution planes have period P), the float64 oracle on the bands
# and one interior period, rows at least the receptive field away from a cut edge: SFENet1 5x5 (2) + SFENet2 (1) + D C dense convs
# (1) + GFF.1 (1) + UPNet.0 (1) = 6 half-resolution rows, doubled, + UPNet.2 (1) = 13 full-resolution rows; PLAN_HALO = 16 keeps
# the bands on even rows.  Bars: rdn_config_cases.FWD_BARS (max-abs), unchanged, on the bands and on the periodicity compare.
PLAN_SHAPE, PLAN_CFG, PLAN_K, PLAN_HALO = EVEN_WIDE, (32, 1, 1, 32), 5, 16


def plan_periods(width, k=PLAN_K, seed=23):
    g = torch.Generator().manual_seed(seed + 31 * width)
    return [torch.rand(3, 2 * P, width, generator=g) for _ in range(k)]


def plan_frames(pers, shape, dev):
    n, h, w = shape
    return [expand_rows(p.to(dev), n, h, 2 * P, lambda i: PHASES[i]).permute(1, 0, 2, 3).contiguous() for p in pers]


def plan_check(shape, pers, weights, y, dev, ref_dev, bar, label="kernel"):
    """Every pixel of y [N, 3, H, W] against the float64 oracle (weights: name -> numpy, as bin_amd.weights.general_rdn_weights gives
    them): max |y - ref| <= bar over the bands and, against the verified period, over every other row.  Returns (error, max|ref - mean|)."""
    from oracle import rdn_oracle as O
    n, h, w = shape
    hl, period = PLAN_HALO, 2 * P
    assert h % 2 == 0 and h >= period + 2 * hl + 2
    Wd = {f"m.{nm}": torch.from_numpy(v).double().to(ref_dev) for nm, v in weights.items()}
    long_rows, short = period + 2 * hl + 2, 2 * hl + 2
    bands = [(0, 0, long_rows, 0, long_rows - hl)]
    for i in range(n):
        if i:
            bands.append((i, 0, short, 0, short - hl))
        bands.append((i, h - short, h, h - short + hl, h))
    worst, size, per = 0.0, 0.0, None
    for (img, r0, r1, v0, v1) in bands:
        idx = (torch.arange(r0, r1) + PHASES[img]) % period
        xs = [p[:, idx][None].double().to(ref_dev) for p in pers]
        with torch.no_grad():
            ref = O.rdn(xs, Wd, "m")
        size = max(size, float((ref - sum(xs) / len(xs))[0, :, v0 - r0:v1 - r0].abs().max()))
        d = (y[img, :, v0:v1].double() - ref[0, :, v0 - r0:v1 - r0].to(dev)).abs()
        worst = float("nan") if bool(torch.isnan(d).any()) else max(worst, float(d.max()))
        if per is None:
            rows = torch.arange(hl, hl + period)
            order = torch.empty(period, dtype=torch.long)
            order[rows % period] = rows
            per = ref[0][:, order.to(ref_dev)].to(dev)                 # float64 [3, 2 P, W]
    e = max_diff_periodic(y.permute(1, 0, 2, 3), per, period, lambda i: PHASES[i], n, hl, h - hl)
    e = float("nan") if e != e or worst != worst else max(e, worst)
    print(f"[domain-top] plan shape={rc.shape_str(shape)} {label}: max|y - ref| = {e:.3e} (bar {bar:.0e}; max|ref - mean| {size:.3e})")
    assert size >= 100 * bar, f"y - mean(frames) = {size:.2e} is below 100x the bar"
    assert e <= bar, (label, e, bar)
    return e, size


# ------------------------------------------------------------------------------------------------ upnet_gsub (plan backward)
# upnet_gsub_kernel packs dL/dO (fp32 [N, 3, H, W], read at 64-bit indices) into ONE half-resolution chunk plane: channel 4 c + 2 i + j
# of pixel (y, x) = g[c][2 y + i][2 x + j] * scale, the outermost full-resolution pixel ring zeroed, channels 12 .. 15 zero.  It is
# reachable only through binhip_rdn_backward (BINHIP_BWD_FUSED_UPNET), which leaves the plane at the start of the "g out" region of its
# workspace.  Pure layout: with a periodic gout (period 2 P full-resolution rows, the even PHASES) the plane is periodic in its half-
# resolution rows 1 .. H/2 - 2 (period P, phase PHASES / 2); rows 0 and H/2 - 1 of every image lose a full-resolution row to the
# ring and are compared on their own.  scale is a power of two, so g * scale is exact and the split is the kernel's bit for bit.
def gsub_period(width, seed=41):
    g = torch.Generator().manual_seed(seed + 31 * width)
    return torch.randn(3, 2 * P, width, generator=g) * 1e-3


def gsub_rows(per, full_rows, scale, zero_rows=()):
    """(hi, lo) fp16 [len(full_rows) / 2, W / 2 * 16] of the plane rows made of the full-resolution period rows `full_rows` (an even
    number, pairs in order); `zero_rows`: positions in full_rows that belong to the ring."""
    g = per[:, full_rows].float() * scale                         # [3, 2 r, W]
    g[:, :, 0] = 0
    g[:, :, -1] = 0
    for z in zero_rows:
        g[:, z] = 0
    sub = F.pixel_unshuffle(g[None], 2)                            # [1, 12, r, W / 2], channel 4 c + 2 i + j
    hi, lo = split_planes(sub, 3)                                  # [1, 1, r, W / 2, 16]
    return hi[0, 0].flatten(1), lo[0, 0].flatten(1)


def gsub_check(shape, per, scale, hi, lo, label="kernel"):
    """Every element of the gsub plane(s) hi, lo (or None) [1, N, H / 2, W / 2, 16] of a backward at full-resolution `shape`."""
    n, h, w = shape
    hh = h // 2
    dev = hi.device
    per = per.to(dev)
    idx = torch.arange(2 * P, device=dev)
    ph, pl = gsub_rows(per, idx, scale)                            # period of the plane: row j = full rows 2 j, 2 j + 1
    half = lambda i: PHASES[i] // 2
    bad = []
    for nm, t, exp in (("hi", hi, ph), ("lo", lo, pl)):
        if t is None:
            continue
        view = t.reshape(1, n, hh, (w // 2) * 16)
        compare_periodic(f"gsub {nm}", view, exp[None], P, half, n, 1, hh - 1, bad)
        for i in range(n):
            for row, full, zero in ((0, (0, 1), 0), (hh - 1, (h - 2, h - 1), 1)):
                rows = torch.tensor([(r + PHASES[i]) % (2 * P) for r in full], device=dev)
                e = gsub_rows(per, rows, scale, zero_rows=(zero,))[0 if nm == "hi" else 1]
                _mismatch(view[0, i, row:row + 1], e, f"gsub {nm} image {i} ring row {row}", bad)
    assert not bad, (shape, label, bad)
