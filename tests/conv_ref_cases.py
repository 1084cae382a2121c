"""Operand families, float64 references, exactness conditions and bars that hold every case of tests/conv_cases.py (one per reachable
row of bh_dispatch_conv, plus the fused dense-block tail) to float64: shared by tests/test_gpu_conv_float64.py (the kernels) and
tests/test_cpu_conv_ref_cases.py (float32 torch as a stand-in kernel, and deliberately wrong restatements that must be caught).

The reference reads the operands AS THE KERNEL READS THEM.  Activation, residual, acc and mask planes: hi = fp16(v), lo = fp16(v - hi)
(nterms 3; binhip_internal.h split_hi / split_lo, what binhip_nchw_to_planes stores) or hi alone (nterms 1); the GPU module checks
the uploaded planes against this split bit for bit.  Weights: the same split of the fp32 OIHW weight, which is what the relayout
stores.  Bias and the FINAL images: fp32.  The product form is the kernels' definition (header of binhip_conv_x3.hip; the same three
products in final_m16_kernel — Wlo*Xhi and Whi*Xhi on the hi sub-stage, Whi*Xlo on the lo one — in conv_x3_kernel<5, ..>'s tap pairs
and in rdb_tail_x3_kernel, `hi: conv += Wlo*Xhi, Whi*Xhi / lo: conv += Whi*Xlo`):
        nterms 3:  Whi*Xhi + Wlo*Xhi + Whi*Xlo            nterms 1:  Whi*Xhi
evaluated in float64.  (The folded UPNet slab, BINHIP_CONV_UPNET_FOLD, is not reachable through bin_amd.ops and not in the table.)

Contracts read out of the code (asserted here, listed in DESIGN.md):
  * channels past cout in the last output chunk.  Only b5_sfe1 has any (24 of 32 lanes): weight rows and bias past cout are zero
    (include/binhip.h, binhip_weights_relayout*) and conv_epilogue adds acc on every lane of a live chunk, so those lanes hold
    [mask](0 + res + acc) = acc passed through: PAD_LANES.  Every other case ends on a whole chunk, or stores fp32 NCHW of exactly
    cout channels (FINAL; FINAL_SUBPIX stores colours c < cout / 4 only).
  * mean(images): every FINAL epilogue (conv_epilogue, final_dot2_kernel, final_m16_kernel, x3 FINAL / FINAL_SUBPIX) computes
    `sj / (float)nimg`, an IEEE division (the build has no fast-math flag), never a multiplication by a rounded 1 / nimg: with images
    that are integer multiples of nimg the integer cases are exact for nimg 3 and 5 too.  MEAN_FORM.
  * o3 of the fused tail: both kernels apply bias and ReLU, round o3 to its fp16 planes (split_pair) and feed the LFF's last two
    K-steps from those STORED values (rdb_tail_kernel: registers -> LDS tile -> MFMA; rdb_tail_x3_kernel: the swapped store slots are
    the B fragments), with or without store_o3.  The residual blk[0:96] enters as stored (hi [+ lo]).  So in the f16 mode y sees two
    roundings, o3's and its own: tail_second_rounding() adds the first to y's bound.
  * every other f16 kernel rounds once: conv_epilogue adds bias, residual and acc in fp32, applies mask / ReLU (on split_pair's
    clamp) and converts to fp16 once; the PixelShuffle store likewise.

Operand families (per case and shape, seeded like conv_cases._gen)
  A  integers, both precisions: activations uniform in -3 .. 3 with some zeros stored as -0.0, weights in -2 .. 2 thinned until the
     conditions hold, integer bias, images integer multiples of nimg.  Conditions: the same operation on absolute values < 2^24 (fp32
     accumulation is then exact in any order) and every plane-stored value (outputs, o3) exactly representable (an integer with
     |v| <= 2048 for nterms 1, decode(split(v)) == v for nterms 3).  Expectation: equal to float64, no tolerance.
  B  split-exact, nterms 3: a + b * 2^-11 as in wgrad_cases (hi = a, lo = b * 2^-11; |a| = 1 with b of the other sign left out), most
     weights zero, so all three products are live and multiples of 2^-11.  Conditions: 2^11 * (the operation on absolute values) <
     2^24 and the result survives its own split.  The tail's LFF weights get lo = 0 on the o3 columns: o3's hi plane is a multiple of
     2^-11 but not an integer, so Llo * o3hi would leave the 2^-11 grid.  Expectation: equal to float64.
  C  white noise: exactly the operands conv_cases.white_noise_bits draws.  e32 = float32 torch against float64 on the operands as read;
     the fp32-class term is max(B_F32, 4 e32) of max|ref| per tensor, 4 e32 <= 8 B_F32 asserted (yardstick as in lstm_cases.py).
     nterms 3 and the fp32 outputs of nterms 1: that term alone.  nterms 1 into fp16 planes, per element:
         |got - ref| <= 2^-11 |ref| + 2^-25 + (1 + 2^-11) * term
     = one rounding of the kernel's fp32 value v to fp16 (half an ulp <= 2^-11 |v|, half a subnormal step 2^-25), with |v - ref| <=
     term.  Derived, not measured.
"""
import functools

import torch
import torch.nn.functional as F

import conv_cases as cc
import wgrad_cases as wg

B_F32 = 2e-5                 # = TOL_OPS[3] of tests/test_gpu_conv.py (the GPU module asserts it is not weaker)
FACTOR, CAP = 4.0, 8.0
EXACT_LIMIT = float(1 << 24)
F16_EXACT_INT = 2048.0
Q = 2.0 ** -11
PAD_LANES = {"b5_sfe1": "acc"}          # tag -> what the lanes past cout of the last chunk hold; every other case has none
MEAN_FORM = "division"                  # sum / (float)nimg in every FINAL epilogue: integer cases exact for nimg 3 and 5

WRONG = ("right_pad", "corner_tap_row16", "drop_wlo_xhi", "mask_from_plus_1", "mask_lt", "res_extra_chunk", "subpixel_swapped",
         "gap_as_data", "mean_count", "second_image_from_first")


def families(nterms):
    return ("A", "B", "C") if nterms == 3 else ("A", "C")


def shape_str(shape):
    return "%dx%dx%d" % tuple(shape)


# ------------------------------------------------------------------------------------------------ operands
def _gen(case, shape, salt):
    n, h, w = shape
    return torch.Generator().manual_seed(1000003 * cc.TAGS.index(case.tag) + 7919 * h + 31 * w + n + 104729 * salt)


def _ints(shape, gen, with_neg_zero=True):
    t = torch.randint(-3, 4, shape, generator=gen).float()
    if with_neg_zero:                      # half of the zeros as -0.0: the mask's `<= 0` at exactly 0, both signs
        t = torch.where((t == 0) & (torch.rand(shape, generator=gen) < 0.5), torch.tensor(-0.0), t)
    return t


def _split_values(shape, gen):
    a, b = wg._split_values(shape, gen)          # a + b * 2^-11, without the pairs whose hi would not be a
    return a + b * Q


def _draw(case, shape, family, density, attempt):
    """One draw of family A or B at a weight density; same keys as conv_cases.white_noise_operands."""
    n, h, w = shape
    o = case.opts
    gen = _gen(case, shape, (1 if family == "A" else 2) + 10 * attempt)
    act = (lambda *s: _ints(s, gen)) if family == "A" else (lambda *s: _split_values(s, gen))

    def weight(*s):
        v = torch.randint(-2, 3, s, generator=gen).float() if family == "A" else _split_values(s, gen)
        return v * (torch.rand(s, generator=gen) < density).float()

    bias = lambda c: torch.randint(-3, 4, (c,), generator=gen).float()
    if case.kind == "tail":
        wl = weight(96, 224, 1, 1)
        if family == "B":
            wl[:, 192:] = wl[:, 192:].round()      # lo = 0 on the o3 columns (module docstring)
        return {"blk": act(n, 224, h, w), "w3": weight(32, 192, 3, 3), "b3": bias(32), "wl": wl, "bl": bias(96)}
    wt = weight(case.cout, case.cin, case.ks, case.ks)
    if case.kind == "bwd":
        nch16 = cc.chunks(case.cin) * 16
        return {"w": wt, "gy": act(n, case.cout, h, w), "res": act(n, nch16, h, w) if o.get("res") else None,
                "acc": act(n, nch16, h, w) if o.get("acc") else None,
                "mask": _ints((n, nch16, h, w), gen) if "mask_from" in o else None}
    epi = o.get("epilogue", "planes")
    imgs, res = [], None
    if epi in ("final", "subpix"):
        up, nimg = (2 if epi == "subpix" else 1), o.get("nimg", 0)
        imgs = [_ints((n, case.cout // (up * up), up * h, up * w), gen, False) * nimg for _ in range(nimg)]
    elif o.get("res"):
        res = act(n, case.cout, h, w)
    return {"w": wt, "b": bias(case.cout), "x": act(n, cc.x_buffer_channels(case), h, w), "imgs": imgs, "res": res}


@functools.lru_cache(maxsize=None)
def operands(tag, family, shape):
    """The operands of (case, family, shape) as fp32 CPU tensors; cached and never modified.  A and B: the weights are thinned (density
    halved, redrawn) until conditions() holds, for both precisions where the family serves both."""
    case = cc.BY_TAG[tag]
    if family == "C":
        return cc.white_noise_operands(case, shape)
    density = 1.0 if family == "A" else 0.1
    for attempt in range(12):
        opnd = _draw(case, shape, family, density, attempt)
        if all(not conditions(case, nt, family, opnd) for nt in ((3, 1) if family == "A" else (3,))):
            return opnd
        density *= 0.5
    raise AssertionError(f"{tag} {family} {shape}: no weight density down to {density} meets the conditions")


# ------------------------------------------------------------------------------------------------ operands as read
def split16(t, nterms):
    """(hi, lo) as float64: the stored split of an fp32 tensor (wgrad_cases.split16); lo is zero for nterms 1."""
    hi, lo = wg.split16(t.float())
    return hi.double(), (lo if nterms == 3 else torch.zeros_like(lo)).double()


def store(v, nterms):
    """What a plane store makes of the fp32 value v: fp16(v), or decode(split(v)), as float64."""
    hi, lo = split16(v, nterms)
    return hi + lo


def as_read(opnd, nterms):
    """Every operand as the kernel reads it: activations and weights as (hi, lo) float64 pairs, bias and images float64."""
    R = {}
    for k, v in opnd.items():
        if v is None:
            R[k] = None
        elif k == "imgs":
            R[k] = [t.double() for t in v]
        elif k in ("b", "b3", "bl"):
            R[k] = v.double()
        else:
            R[k] = split16(v, nterms)
    return R


def _abs(R):
    f = lambda v: None if v is None else [t.abs() for t in v] if isinstance(v, list) else \
        (v[0].abs(), v[1].abs()) if isinstance(v, tuple) else v.abs()
    return {k: f(v) for k, v in R.items()}


# ------------------------------------------------------------------------------------------------ references
def _conv_one(x, w, ks, wrong, transpose=False):
    """conv2d(x, w, padding = ks // 2) — or, transpose, conv_transpose2d(x, w, padding = ks // 2), which the wrong restatements
    evaluate as the forward-shaped convolution the kernel runs: W'[ci][co][dy][dx] = W[co][ci][k-1-dy][k-1-dx] (include/binhip.h)."""
    p = ks // 2
    if wrong is None:
        return F.conv_transpose2d(x, w, padding=p) if transpose else F.conv2d(x, w, padding=p)
    if transpose:
        w = w.transpose(0, 1).flip(2, 3)
    n, _, h, wd = x.shape
    if wrong == "second_image_from_first" and n > 1:
        x = x[:1].expand(n, -1, -1, -1)
    xp = F.pad(x, (p, p, p, p))
    if wrong == "right_pad" and p > 0 and h > 1:          # the first pad column holds what follows in memory: the next row's start
        xp = xp.clone()
        xp[:, :, p:p + h - 1, p + wd] = x[:, :, 1:, 0]
    y = F.conv2d(xp, w)
    if wrong == "corner_tap_row16" and ks > 1 and h > 16:
        w2 = w.clone()
        w2[:, :, 0, 0] = 0
        y = y.clone()
        y[:, :, 16] = F.conv2d(xp, w2)[:, :, 16]
    return y


def _conv3(x, w, ks, nterms, dt, wrong, transpose=False):
    """The kernels' product form on (hi, lo) pairs: Whi*Xhi + Wlo*Xhi + Whi*Xlo, or Whi*Xhi."""
    xh, xl, wh, wl = x[0].to(dt), x[1].to(dt), w[0].to(dt), w[1].to(dt)
    if nterms == 1:
        return _conv_one(xh, wh, ks, wrong, transpose)
    first = wh if wrong == "drop_wlo_xhi" else wh + wl
    return _conv_one(xh, first, ks, wrong, transpose) + _conv_one(xl, wh, ks, wrong, transpose)


def _shuffle(y, swapped):
    """PixelShuffle(2): channel c * 4 + i * 2 + j -> pixel (2 y + i, 2 x + j) of channel c."""
    n, c4, h, w = y.shape
    t = y.reshape(n, c4 // 4, 2, 2, h, w)                # [n, c, i, j, y, x]
    t = t.permute(0, 1, 4, 3, 5, 2) if swapped else t.permute(0, 1, 4, 2, 5, 3)
    return t.reshape(n, c4 // 4, 2 * h, 2 * w)


def _pair_sum(p, dt):
    return p[0].to(dt) + p[1].to(dt)


def reference(case, nterms, R, dt=torch.float64, wrong=None, plain=False, o3_from=None):
    """{output name: tensor of dtype dt} of the case on operands as read.  `plain`: no ReLU and no mask (the absolute-value bound).
    `o3_from` (tail): the o3 whose stored form the LFF consumes instead of this evaluation's own — the float32 yardstick takes the
    float64 reference's, so that e32 measures float32 arithmetic and not an fp16 rounding of o3 that fell the other way.
    Outputs: "y" NCHW planes content (bwd: all chunks(cin) * 16 lanes; y_unshuf: the 64 * yu half-resolution channels), "f32", and
    for the tail "o3" (before its store) and "y"."""
    o = case.opts
    if case.kind == "tail":
        blk = R["blk"]
        o3 = _conv3((blk[0][:, :192], blk[1][:, :192]), R["w3"], 3, nterms, dt, wrong) + R["b3"].to(dt).view(1, -1, 1, 1)
        if not plain:
            o3 = o3.relu()
        s_hi, s_lo = (o3, torch.zeros_like(o3)) if plain else split16(o3 if o3_from is None else o3_from, nterms)   # the STORED o3
        cat = (torch.cat((blk[0][:, :192].to(dt), s_hi.to(dt)), 1), torch.cat((blk[1][:, :192].to(dt), s_lo.to(dt)), 1))
        y = _conv3(cat, R["wl"], 1, nterms, dt, wrong) + R["bl"].to(dt).view(1, -1, 1, 1) + _pair_sum(blk, dt)[:, :96]
        return {"y": y, "o3": o3}
    if case.kind == "bwd":
        gx = _conv3(R["gy"], R["w"], case.ks, nterms, dt, wrong, transpose=True)
        nch16 = cc.chunks(case.cin) * 16
        gx = F.pad(gx, (0, 0, 0, 0, 0, nch16 - gx.shape[1]))      # weight rows past cin are zero
        if R["res"] is not None:
            rc = o.get("res_chunks", 0) + (1 if wrong == "res_extra_chunk" else 0)
            upto = 16 * rc if o.get("res_chunks", 0) > 0 else nch16
            gx[:, :upto] = gx[:, :upto] + _pair_sum(R["res"], dt)[:, :upto]
        if R["acc"] is not None:
            gx = gx + _pair_sum(R["acc"], dt)
        if R["mask"] is not None and not plain:
            m0 = 16 * (o.get("mask_from", 0) + (1 if wrong == "mask_from_plus_1" else 0))
            act = R["mask"][0][:, m0:]                            # the hi plane of the saved activation
            gx[:, m0:] = gx[:, m0:] * ((act >= 0) if wrong == "mask_lt" else (act > 0)).to(dt)
        yu = o.get("y_unshuf", 0)
        if yu:                                                    # plane (2 (Y & 1) + (X & 1)) * yu + c at (Y / 2, X / 2)
            n, c, h, w = gx.shape
            gx = F.pixel_unshuffle(gx, 2).reshape(n, c, 4, h // 2, w // 2).transpose(1, 2).reshape(n, 4 * c, h // 2, w // 2)
        return {"y": gx}
    x = R["x"]
    cpg = o.get("x_cpg")
    if cpg:
        nchunk = cc.chunks(case.cin)
        if wrong == "gap_as_data":
            planes = list(range(nchunk))
        else:
            planes = [(i // cpg) * (cpg + 1) + i % cpg for i in range(nchunk)]
        idx = torch.tensor([16 * p + l for p in planes for l in range(16)])
        x = (x[0][:, idx], x[1][:, idx])
    y = _conv3(x, R["w"], case.ks, nterms, dt, wrong) + R["b"].to(dt).view(1, -1, 1, 1)
    epi = o.get("epilogue", "planes")
    if epi == "planes":
        if R["res"] is not None:
            y = y + _pair_sum(R["res"], dt)
        if o.get("relu") and not plain:
            y = y.relu()
        return {"y": y}
    if epi == "shuffle":
        return {"y": _shuffle(y, wrong == "subpixel_swapped")}
    if epi == "subpix":
        y = _shuffle(y, wrong == "subpixel_swapped")
    if R["imgs"]:
        nimg = len(R["imgs"])
        y = y + sum(t.to(dt) for t in R["imgs"]) / (nimg + 1 if wrong == "mean_count" else nimg)
    return {"f32": y}


def plane_outputs(case):
    """Names of the outputs that go through an fp16 plane store."""
    if case.kind == "tail":
        return ("y", "o3")
    return () if case.opts.get("epilogue") in ("final", "subpix") else ("y",)


def output_names(case):
    if case.kind == "tail":
        return ("y", "o3") if case.opts.get("store_o3") else ("y",)
    return ("f32",) if case.opts.get("epilogue") in ("final", "subpix") else ("y",)


# ------------------------------------------------------------------------------------------------ conditions of the exact families
def _integral(t, scale=1.0):
    return bool((t * scale == (t * scale).round()).all())


def conditions(case, nterms, family, opnd):
    """The family's conditions on the reference alone: a list of the broken ones (empty = they hold)."""
    R = as_read(opnd, nterms)
    bad = []
    scale = 1.0 if family == "A" else 2.0 ** 11
    for k, v in R.items():                    # every operand on the family's grid, so every product and partial sum is as well
        if v is None or k == "imgs":
            continue
        if isinstance(v, tuple):
            ok = _integral(v[0]) and (_integral(v[1], 2.0 ** 11) if family == "B" else not bool(v[1].any()))
        else:
            ok = _integral(v)
        if not ok:
            bad.append(f"operand {k} is off the grid")
    if family == "B" and case.kind == "tail" and bool(R["wl"][1][:, 192:].any()):
        bad.append("LFF lo weights on the o3 columns")
    bound = reference(case, nterms, _abs(R), plain=True)
    for nm, t in bound.items():
        if not float(t.max()) * scale < EXACT_LIMIT:
            bad.append(f"{nm}: the operation on absolute values reaches {float(t.max()) * scale:.4g} >= 2^24")
    ref = reference(case, nterms, R)
    for nm in plane_outputs(case):
        v = ref[nm]
        if family == "A" and nterms == 1 and not (_integral(v) and float(v.abs().max()) <= F16_EXACT_INT):
            bad.append(f"{nm}: max |v| = {float(v.abs().max()):.6g} is not an exact fp16 integer")
        if not torch.equal(store(v, nterms), v):
            bad.append(f"{nm} does not survive its store")
        if family == "B" and nm == "o3":      # Lhi * o3hi and Lhi * o3lo stay on the 2^-11 grid
            hi, lo = split16(v, 3)
            if not (_integral(hi, 2.0 ** 11) and _integral(lo, 2.0 ** 11)):
                bad.append("o3's planes leave the 2^-11 grid")
    return bad


# ------------------------------------------------------------------------------------------------ comparison
@functools.lru_cache(maxsize=None)
def references(tag, nterms, family, shape):
    """(float64 reference, float32 torch on the same operands as read) per output; cached, never modified."""
    case = cc.BY_TAG[tag]
    R = as_read(operands(tag, family, shape), nterms)
    ref = reference(case, nterms, R)
    ref32 = reference(case, nterms, R, dt=torch.float32, o3_from=ref.get("o3")) if family == "C" else None
    return ref, ref32


def f32_term(name, ref, ref32):
    """(e32, bar): float32 torch's own error relative to max|ref| and the fp32-class bar max(B, 4 e32), with the cap asserted."""
    scale = max(float(ref.abs().max()), 1e-30)
    e32 = float((ref32.double() - ref).abs().max()) / scale
    assert FACTOR * e32 <= CAP * B_F32, f"yardstick cap broken for {name}: 4 * e32 = {FACTOR * e32:.3e} > 8 * B = {CAP * B_F32:.3e}"
    return e32, max(B_F32, FACTOR * e32)


def tail_second_rounding(tag, shape, bar_o3):
    """f16 tail: what o3's own rounding may move y by, per element.  The stored o3 is within r = 2^-11 |o3| + 2^-25 + (1 + 2^-11) t of
    the unrounded reference o3 (t = the fp32-class term of o3) and the reference's stored o3 within 2^-11 |o3| + 2^-25 of it; the LFF
    multiplies the difference by |L| on the 32 o3 columns."""
    ref, _ = references(tag, 1, "C", shape)
    o3 = ref["o3"]
    t = bar_o3 * float(o3.abs().max())
    d = 2 * (Q * o3.abs() + 2.0 ** -25) + (1 + Q) * t
    wl = split16(operands(tag, "C", shape)["wl"], 1)[0][:, 192:].abs()
    return F.conv2d(d, wl)


def compare(case, nterms, family, shape, got, label="kernel"):
    """Hold the outputs `got` ({name: float64 CPU tensor}) of one call to the float64 reference by the family's rule; prints one
    [conv-f64] line per output and returns {name: (e32, bar, error, ratio)}.  Raises AssertionError naming row, shape and element."""
    ref, ref32 = references(case.tag, nterms, family, tuple(shape))
    res, bad = {}, []
    bars = {}
    for nm in output_names(case):
        g, r = got[nm].double(), ref[nm]
        assert g.shape == r.shape, (case.tag, nm, tuple(g.shape), tuple(r.shape))
        assert bool(torch.isfinite(g).all()), f"{case.tag} {nm}: not finite"
        scale = max(float(r.abs().max()), 1e-30)
        d = (g - r).abs()
        err = float(d.max()) / scale
        if family in ("A", "B"):
            e32 = bar = 0.0
            ratio = 0.0 if torch.equal(g, r) else float("inf")
        else:
            e32, bar = f32_term(f"{case.tag} {nm}", r, ref32[nm])
            bars[nm] = bar
            if nterms == 1 and nm in plane_outputs(case):
                tol = Q * r.abs() + 2.0 ** -25 + (1 + Q) * bar * scale
                if case.kind == "tail" and nm == "y":
                    if "o3" not in bars:
                        bars["o3"] = f32_term(f"{case.tag} o3", ref["o3"], ref32["o3"])[1]
                    tol = tol + tail_second_rounding(case.tag, tuple(shape), bars["o3"])
                ratio = float((d / tol).max())
            else:
                ratio = err / bar
        res[nm] = (e32, bar, err, ratio)
        print(f"[conv-f64] row={case.rows[nterms]!r} case={case.tag} nterms={nterms} family={family} shape={shape_str(shape)} out={nm} "
              f"e32={e32:.3e} bar={bar:.3e} {label}={err:.3e} ratio={ratio:.3f}")
        if not ratio <= 1.0:
            worst = d if family in ("A", "B") or not (nterms == 1 and nm in plane_outputs(case)) else d / tol
            at = tuple(int(i) for i in torch.unravel_index(worst.argmax(), worst.shape))
            bad.append(f"{nm}: row {case.rows[nterms]!r} shape {shape_str(shape)} family {family} element {at}: got {float(g[at])!r} "
                       f"reference {float(r[at])!r} (ratio {ratio:.3g})")
    assert not bad, (case.tag, nterms, bad)
    return res


# ------------------------------------------------------------------------------------------------ stand-in kernels for the CPU module
def restated(case, nterms, family, shape, dt=torch.float64, wrong=None):
    """The case restated in torch (dtype dt, optionally deliberately wrong) with the kernels' plane stores applied: what a kernel
    would hand to compare()."""
    R = as_read(operands(case.tag, family, tuple(shape)), nterms)
    out = reference(case, nterms, R, dt=dt, wrong=wrong)
    return {nm: store(v, nterms) if nm in plane_outputs(case) else v.float().double() for nm, v in out.items()}


# ------------------------------------------------------------------------------------------------ GFF.0's scattered store
SCATTER_TAG, SCATTER_CPG, SCATTER_GROUPS = "b1_gff0", 6, 12       # 72 output chunks as 12 groups of 6, one gap plane between groups
GUARD_HI, GUARD_LO = 1.5, 2.0 ** -13                               # what the gap planes hold before the call and must hold after


def planes_to_nchw(p):
    """A chunk-plane tensor [chunks, N, H, W, 16] (any device) as NCHW float64 on the CPU."""
    return wg.planes_to_nchw(p, p.shape[0] * 16).double()


def decode(cp):
    """A CP (hi [+ lo]) as NCHW float64 on the CPU: hi + lo, exact in float64."""
    v = planes_to_nchw(cp.hi)
    return v if cp.lo is None else v + planes_to_nchw(cp.lo)
