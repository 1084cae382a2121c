"""-m gpu: the fp16 range contract (include/binhip.h, "Dynamic range") on every store path that writes chunk planes, one launch per
(path, mode, value), against a float64 reference of the stored tensor (the layer output after bias, residual / accumulator, ReLU /
mask, as torch computes it):
  * |v| <= 65504: status bit clear; hi (and lo) are the split of fl32(v) bit for bit (the inputs are built so that the kernels' fp32
    arithmetic is exact: identity-like weights, fp16-exact operands);
  * |v| > 65504 or +-inf: bit set, hi = sign(v) * 65504 and lo = 0 at exactly those elements;
  * NaN of either sign, relu(NaN) included: bit set, hi and lo finite (and lo = 0);
  * ReLU of a value below -65504 / -inf, and a gradient behind a saved activation <= 0 (inf and NaN included), store 0 with the bit clear;
  * every other element is bit-identical to the same launch without the extreme value (saturation stays local);
  * FINAL (fp32 output) passes 1e30 / inf / NaN through exactly, bit clear.
Then whole RDN forward and backward calls must raise `fp16 range exceeded` from ops.check_status() on NaN / out-of-range values and stay
finite.  Case table: tests/range_cases.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from range_cases import CASES, EXTRA_VALUES, F16_MAX, NAN_NEG, NAN_POS, VALUES, runs

pytestmark = pytest.mark.gpu

N, H, W = 1, 6, 34          # 34 columns: one full 32-pixel tile and a ragged one
PIX = (0, 2, 33)            # (n, y, x) of the placed value: in the ragged tile
TARGET = 5                  # the output channel that receives it
_REF = {}                   # float64 references, shared between modes and the ReLU on / off cases
TOL = {1: 2e-3, 3: 2e-5}    # the per-op bar of tests/test_gpu_conv.py (max error / max |ref|) where fl32(v) is not exact
_WORST = [0.0]              # worst relative error of the elements that are not exactly constructed, since the last _worst()


def _worst():
    w, _WORST[0] = _WORST[0], 0.0
    return w


def _f32(v):
    """An fp32 value from a float or an fp32 bit pattern (int)."""
    if isinstance(v, int):
        return float(np.array([v], dtype=np.uint32).view(np.float32)[0])
    return float(v)


def _f16_bits(v):
    """fp16 bit pattern of `v` (fp32 NaN bit patterns keep their sign)."""
    if isinstance(v, int):
        return 0x7E00 if v == NAN_POS else 0xFE00
    return int(torch.tensor([v], dtype=torch.float16).view(torch.int16)[0]) & 0xFFFF


def _poke(plane, ch, pix, v):
    """Write fp16 `v` into element (channel ch, pixel pix) of a [chunk][N][H][W][16] plane."""
    n, y, x = pix
    b = _f16_bits(v)
    plane.view(torch.int16)[ch // 16, n, y, x, ch % 16] = b - 0x10000 if b >= 0x8000 else b


def _bias_tensor(vals):
    """fp32 tensor of floats and fp32 bit patterns (a NaN keeps its sign bit)."""
    bits = [int(np.array([v], np.float32).view(np.uint32)[0]) if not isinstance(v, int) else v for v in vals]
    return torch.from_numpy(np.array(bits, dtype=np.uint32).view(np.float32).copy())


def _set32(t, idx, how, val):
    """Write the value of a VALUES entry into fp32 tensor t at idx: a + b for "sum", else the value (bit pattern for a NaN)."""
    v = _f32(val[0]) + _f32(val[1]) if how == "sum" else val
    t[idx] = _bias_tensor([v])[0]


def _to_planes(t, nch=None):
    """NCHW -> [chunk][N][H][W][16] (channels padded with zeros)."""
    n, c, h, w = t.shape
    nch = nch or (c + 15) // 16
    if c < nch * 16:
        t = torch.cat([t, t.new_zeros(n, nch * 16 - c, h, w)], 1)
    return t.view(n, nch, 16, h, w).permute(1, 0, 3, 4, 2).contiguous()


def _from_planes(hi, lo, c):
    """[chunk][N][H][W][16] planes -> float64 NCHW of hi (+ lo)."""
    v = hi.double() + (lo.double() if lo is not None else 0)
    nch, n, h, w, _ = v.shape
    return v.permute(1, 0, 4, 2, 3).reshape(n, nch * 16, h, w)[:, :c].cpu()


def _grid(shape, gen, span=2.0):
    """fp16-exact values k / 64, |k| <= 64 * span."""
    k = int(64 * span)
    return torch.randint(-k, k + 1, shape, generator=gen).double() / 64


def _status():
    """Read and clear the status word of the current device."""
    from bin_amd import ops
    w = ops.status_word(torch.device("cuda"))
    v = int(w.item())
    w.zero_()
    return v & 1


def _same_bits(a, b):
    """fp16 tensors equal bit for bit, +0 / -0 counted as the same stored value."""
    return (a.view(torch.int16) == b.view(torch.int16)) | ((a == 0) & (b == 0))


def check_store(label, hi, lo, ref, flag, base=None, want=None, nterms=None, nan_hi=-F16_MAX):
    """The contract on one stored tensor.  hi / lo: the stored planes (lo None in the single-product mode); ref: float64 reference in
    plane layout; flag: the status bit of the launch; base: (hi, lo, ref) of the same launch without the extreme value; want: the
    expected bit when the launch stores more than this tensor; nan_hi: what a NaN stores (the lower clamp bound: -65504, 0 on a ReLU
    layer).  In-range elements whose reference is an fp32 number are the split of it
    bit for bit: hi always, lo (its last bits depend on how the matrix core aligns the addends) where the value is a multiple of 2^-19, so
    that no addend of |x| <= 16 loses a bit; the rest meet the mode's per-op bar.  Returns the number of elements checked bit for bit."""
    hi, lo = hi.cpu(), (lo.cpu() if lo is not None else None)
    v32 = ref.float()
    nan = torch.isnan(ref)
    big = ~nan & (v32.abs() > F16_MAX)
    inr = ~nan & ~big
    want = bool((nan | big).any()) if want is None else want
    nterms = nterms or (3 if lo is not None else 1)
    exact = inr & (v32.double() == ref)
    grid = exact & (((ref * 2.0 ** 19).frac() == 0) | (ref.abs() >= 16))
    loose = inr & ~grid
    if bool(loose.any()):
        got = hi.double() + (lo.double() if lo is not None else 0)
        scale = float(ref[inr].abs().max())
        err = float((got - ref)[loose].abs().max()) / max(scale, 1e-30)
        _WORST[0] = max(_WORST[0], err)
        assert err <= TOL[nterms], f"{label}: {err:.2e} relative error on {int(loose.sum())} inexact elements (bar {TOL[nterms]:.0e})"
    assert flag == want, f"{label}: status bit {flag}, expected {want} ({int(big.sum())} out of range, {int(nan.sum())} NaN)"
    assert bool(torch.isfinite(hi.float()).all()), f"{label}: hi holds inf / NaN"
    if lo is not None:
        assert bool(torch.isfinite(lo.float()).all()), f"{label}: lo holds inf / NaN"
        assert bool((lo[~inr] == 0).all()), f"{label}: lo != 0 after saturation"
    exp_hi = torch.where(exact, v32, torch.zeros_like(v32)).half()
    ok = _same_bits(hi, exp_hi) | ~exact
    assert bool(ok.all()), f"{label}: {int((~ok).sum())} in-range hi differ, first at {(~ok).nonzero()[0].tolist()}"
    if lo is not None:
        exp_lo = (torch.where(grid, v32, torch.zeros_like(v32)) - exp_hi.float()).half()
        ok = _same_bits(lo, exp_lo) | ~grid
        assert bool(ok.all()), f"{label}: {int((~ok).sum())} in-range lo differ"
    ok = (hi.float() == nan_hi) | ~nan
    assert bool(ok.all()), f"{label}: a NaN stored hi != {nan_hi} at {int((~ok).sum())} elements"
    sat_hi = torch.sign(v32) * F16_MAX
    ok = (hi.float() == sat_hi) | ~big
    assert bool(ok.all()), f"{label}: saturated hi != sign(v) * 65504 at {int((~ok).sum())} elements"
    if base is not None:
        bhi, blo, bref = base
        same = inr & (ref == bref)
        ok = _same_bits(hi, bhi.cpu()) | ~same
        assert bool(ok.all()), f"{label}: {int((~ok).sum())} untouched elements changed"
        if lo is not None:
            ok = _same_bits(lo, blo.cpu()) | ~same
            assert bool(ok.all()), f"{label}: {int((~ok).sum())} untouched lo elements changed"
    return int(exact.sum())


def _values(kinds):
    return [v for v in VALUES + EXTRA_VALUES if v[1] in kinds]


# ------------------------------------------------------------------------------------------------ packers
def _nchw_case(case, nterms, name, how, val):
    from bin_amd import ops, _lib as L
    gen = torch.Generator().manual_seed(3)
    x = _grid((N, 21, 5, 7), gen).float()
    sc = case["scale"]
    if name is not None:
        _set32(x, (0, 17, 4, 6), how, val)
    if sc is None:
        y = ops.nchw_to_planes(x.cuda(), nterms)
        ref = x.double()
    else:                       # the scale pushes finite inputs out of range: x / scale in, x out
        xin = (x / sc).cuda()           # (a NaN stays NaN, of the same sign)
        y = ops.CP.empty(2, N, 5, 7, nterms, "cuda", 21)
        s = torch.tensor([sc, 1.0 / sc], device="cuda")
        L.check(L.lib().binhip_nchw_to_planes_scaled(ops._ptr(xin), N, 21, 5, 7, ops._ptr(s), ops._ptr(y.hi), ops._ptr(y.lo),
                                                     ops._ptr(ops.status_word(xin.device)), ops._stream()), "scaled")
        ref = xin.cpu().double() * sc
    return y.hi, y.lo, _to_planes(ref)


def _pack_case(case, nterms, name, how, val):
    from bin_amd import ops
    k = case["frames"]
    gen = torch.Generator().manual_seed(4 + k)
    ims = [_grid((N, 3, 10, 14), gen).float() for _ in range(k)]
    if name is not None:
        _set32(ims[-1], (0, 2, 9, 13), how, val)
    y = ops.pack_inputs([im.cuda() for im in ims], nterms)
    ref = F.pixel_unshuffle(torch.cat(ims, 1).double(), 2)
    return y.hi, y.lo, _to_planes(ref)


# ------------------------------------------------------------------------------------------------ conv2d_fwd
def _conv_weights(cout, cin, ks):
    """Output o = x[o % cin] + x[(o + 7) % cin] (centre taps of 1, zeros elsewhere)."""
    w = torch.zeros(cout, cin, ks, ks, dtype=torch.float64)
    for o in range(cout):
        w[o, o % cin, ks // 2, ks // 2] += 1
        w[o, (o + 7) % cin, ks // 2, ks // 2] += 1
    return w


def _fwd_inputs(cin, cout, ks, residual, name, how, val, seed):
    """(x64 NCHW, bias values list, residual64 or None) of one launch: base operands plus the value placed as `how` says."""
    gen = torch.Generator().manual_seed(seed)
    x = _grid((N, cin, H, W), gen)
    bias = list((_grid((cout,), gen)).tolist())
    bias[TARGET % cout] = 0.0
    r = _grid((N, cout, H, W), gen) if residual else None
    return x, bias, r


def _conv_fwd_launch(case, nterms, name, how, val):
    from bin_amd import ops
    ks, cp, relu = case["ks"], case["cout_pad"], case["relu"]
    cin, cout = 32, cp
    x, bias, r = _fwd_inputs(cin, cout, ks, case["residual"], name, how, val, 7 + ks)
    xp = ops.nchw_to_planes(x.float().cuda(), nterms)
    a, b = TARGET % cin, (TARGET + 7) % cin
    if how == "sum":
        _poke(xp.hi, a, PIX, _f32(val[0]))
        _poke(xp.hi, b, PIX, _f32(val[1]))
    elif how == "bias":
        bias[TARGET] = val
    elif how == "plane":
        _poke(xp.hi, a, PIX, val)
    rp = None
    if r is not None:
        rp = ops.nchw_to_planes(r.float().cuda(), nterms)
        if how == "extra":
            _poke(rp.hi, TARGET, PIX, val)
    w = _conv_weights(cout, cin, ks)
    bt = _bias_tensor(bias)
    cw = ops.ConvWeights(w.float().cuda(), bt.cuda(), nterms=nterms, cout_pad=cp)
    y = ops.conv2d(xp, cw, relu=bool(relu), residual=rp)
    key = ("fwd", nterms, ks, cp, case["residual"], name, relu)
    if key not in _REF:
        ref = F.conv2d(_from_planes(xp.hi, xp.lo, cin), w, bt.double(), padding=ks // 2)
        if rp is not None:
            ref = ref + _from_planes(rp.hi, rp.lo, cout)
        if relu:
            ref = torch.relu(ref)
        _REF[key] = _to_planes(ref)
    return y.hi, y.lo, _REF[key]


def _shuffle_launch(case, nterms, name, how, val):
    from bin_amd import ops, _lib as L
    cin, cout = 32, 256
    x, bias, _ = _fwd_inputs(cin, cout, 3, False, name, how, val, 17)
    xp = ops.nchw_to_planes(x.float().cuda(), nterms)
    a, b = TARGET % cin, (TARGET + 7) % cin
    if how == "sum":
        _poke(xp.hi, a, PIX, _f32(val[0]))
        _poke(xp.hi, b, PIX, _f32(val[1]))
    elif how == "bias":
        bias[TARGET] = val
    elif how == "plane":
        _poke(xp.hi, a, PIX, val)
    w = _conv_weights(cout, cin, 3)
    bt = _bias_tensor(bias)
    cw = ops.ConvWeights(w.float().cuda(), bt.cuda(), nterms=nterms, shuffle=True)
    y = ops.conv2d(xp, cw, epilogue=L.EPI_SHUFFLE)
    key = ("shuffle", nterms, name)
    if key not in _REF:
        _REF[key] = _to_planes(F.pixel_shuffle(F.conv2d(_from_planes(xp.hi, xp.lo, cin), w, bt.double(), padding=1), 2))
    return y.hi, y.lo, _REF[key]


def _store_case(case, nterms, launch, values):
    """Baseline launch, then one launch per value; check_store on each."""
    from bin_amd import ops
    ops.check_status()                                # nothing left behind by earlier tests
    bhi, blo, bref = launch(case, nterms, None, None, None)
    torch.cuda.synchronize()
    nan_hi = 0.0 if case.get("relu") else -F16_MAX
    n_exact = check_store("baseline", bhi, blo, bref, _status(), nan_hi=nan_hi)
    for name, how, val in values:
        hi, lo, ref = launch(case, nterms, name, how, val)
        torch.cuda.synchronize()
        n_exact += check_store(f"{name}", hi, lo, ref, _status(), (bhi, blo, bref), nan_hi=nan_hi)
    return n_exact


@pytest.mark.parametrize("cid,nterms", runs(("nchw", "pack", "conv_fwd", "conv_shuffle")))
def test_plane_store_saturates_flags_and_stays_local(cid, nterms):
    """Packers and forward conv epilogues (no extras / residual / PixelShuffle), every tile variant, ReLU on and off."""
    case = CASES[cid]
    kind = case["kind"]
    if kind in ("nchw", "pack"):                      # fp32 inputs: every value is written as it is
        launch, values = (_nchw_case if kind == "nchw" else _pack_case), _values(("sum", "bias", "plane"))
    elif kind == "conv_shuffle":
        launch, values = _shuffle_launch, _values(("sum", "bias", "plane"))
    else:
        launch = _conv_fwd_launch
        values = _values(("sum", "bias", "plane", "extra") if case["residual"] else ("sum", "bias", "plane"))
    n = _store_case(case, nterms, launch, values)
    print(f"{cid} nterms={nterms}: {len(values)} values, {n} in-range elements bit-exact, worst error of the rest {_worst():.2e}")


@pytest.mark.parametrize("nterms", [3, 1])
def test_final_epilogue_passes_fp32_through(nterms):
    """FINAL stores fp32: 1e30, +-inf and NaN come out exactly as the reference computes them and the status bit stays clear."""
    from bin_amd import ops, _lib as L
    ops.check_status()
    cin, cout, t = 32, 3, 1
    for name, how, val in [("base", None, None)] + _values(("sum", "bias", "plane")):
        x, bias, _ = _fwd_inputs(cin, cout, 3, False, name, how, val, 27)
        bias[t] = 0.0
        xp = ops.nchw_to_planes(x.float().cuda(), nterms)
        a, b = t % cin, (t + 7) % cin
        if how == "sum":
            _poke(xp.hi, a, PIX, _f32(val[0]))
            _poke(xp.hi, b, PIX, _f32(val[1]))
        elif how == "bias":
            bias[t] = val
        elif how == "plane":
            _poke(xp.hi, a, PIX, val)
        w = _conv_weights(cout, cin, 3)
        bt = _bias_tensor(bias)
        cw = ops.ConvWeights(w.float().cuda(), bt.cuda(), nterms=nterms)
        y = ops.conv2d(xp, cw, epilogue=L.EPI_FINAL).cpu()
        torch.cuda.synchronize()
        assert _status() == 0, f"FINAL raised the status bit ({name})"
        ref = F.conv2d(_from_planes(xp.hi, xp.lo, cin), w, bt.double(), padding=1).float()
        same = (y == ref) | (torch.isnan(y) & torch.isnan(ref))
        assert bool(same.all()), f"FINAL {name}: {int((~same).sum())} elements differ from fl32(reference)"
    print(f"final nterms={nterms}: every element equals fl32(float64 reference), NaN / inf included")


# ------------------------------------------------------------------------------------------------ fused dense-block tail
def _tail_weights():
    """conv #3: o3[o] = blk[96 + 3o % 96] + blk[96 + (3o + 50) % 96] (3x3 centre); LFF: y[o] = blk[(o + 40) % 96] (1x1), its o3 and
    96..191 weights zero; the residual blk[0:96] is the kernel's own."""
    w3 = torch.zeros(32, 192, 3, 3, dtype=torch.float64)
    for o in range(32):
        w3[o, 96 + (3 * o) % 96, 1, 1] += 1
        w3[o, 96 + (3 * o + 50) % 96, 1, 1] += 1
    wl = torch.zeros(96, 224, 1, 1, dtype=torch.float64)
    for o in range(96):
        wl[o, (o + 40) % 96, 0, 0] = 1
    return w3, wl


def _tail_launch(case, nterms, name, how, val):
    from bin_amd import ops
    gen = torch.Generator().manual_seed(31)
    blk = torch.cat([_grid((N, 192, H, W), gen), torch.zeros(N, 32, H, W, dtype=torch.float64)], 1)
    b3, bl = _grid((32,), gen).tolist(), _grid((96,), gen).tolist()
    b3[TARGET] = bl[TARGET] = 0.0
    bp = ops.nchw_to_planes(blk.float().cuda(), nterms)
    o3_side = case["where"] == "o3"
    if o3_side:        # sources of o3[TARGET]
        a, b = 96 + (3 * TARGET) % 96, 96 + (3 * TARGET + 50) % 96
    else:              # sources of y[TARGET]: the residual and the LFF tap
        a, b = TARGET, (TARGET + 40) % 96
    if how == "sum":
        _poke(bp.hi, a, PIX, _f32(val[0]))
        _poke(bp.hi, b, PIX, _f32(val[1]))
    elif how == "bias":
        (b3 if o3_side else bl)[TARGET] = val
    elif how == "plane":
        _poke(bp.hi, a, PIX, val)
    w3, wl = _tail_weights()
    b3t, blt = _bias_tensor(b3), _bias_tensor(bl)
    cw3 = ops.ConvWeights(w3.float().cuda(), b3t.cuda(), nterms=nterms)
    cwl = ops.ConvWeights(wl.float().cuda(), blt.cuda(), nterms=nterms)
    x64 = _from_planes(bp.hi, bp.lo, 224)
    y = ops.rdb_tail(bp, cw3, cwl, store_o3=bool(case["store_o3"]))
    o3 = torch.relu(F.conv2d(x64[:, :192], w3, b3t.double(), padding=1))
    # the LFF reads the o3 that was stored (saturated, a NaN made finite): through its zero weights it must not reach y
    o3s = torch.nan_to_num(o3, nan=0.0).clamp(-F16_MAX, F16_MAX)
    yref = F.conv2d(torch.cat([x64[:, :192], o3s], 1), wl, blt.double()) + x64[:, :96]
    return y, bp, _to_planes(o3), _to_planes(yref)


@pytest.mark.parametrize("cid,nterms", runs(("rdb_tail",)))
def test_fused_tail_saturates_o3_and_output(cid, nterms):
    """binhip_rdb_tail_fwd: conv #3 with the ReLU folded into the clamp (o3, kept when store_o3) and the LFF + residual output.  The
    status bit covers o3 whether it is stored or not."""
    from bin_amd import ops
    ops.check_status()
    case = CASES[cid]
    base = None
    n = 0
    for name, how, val in [(None, None, None)] + _values(("sum", "bias", "plane")):
        y, bp, o3ref, yref = _tail_launch(case, nterms, name, how, val)
        torch.cuda.synchronize()
        flag = _status()
        want = any(bool(torch.isnan(r).any() or (r.float().abs() > F16_MAX).any()) for r in (o3ref, yref))
        label = f"{cid} nterms={nterms} {name}"
        lo = (lambda p: p.lo if nterms == 3 else None)
        if case["store_o3"]:
            n += check_store(label + " o3", bp.hi[12:14], lo(bp)[12:14] if nterms == 3 else None, o3ref, flag,
                             None if base is None else (base[1].hi[12:14], lo(base[1])[12:14] if nterms == 3 else None, base[2]), want,
                             nan_hi=0.0)
        n += check_store(label + " y", y.hi, lo(y), yref, flag, None if base is None else (base[0].hi, lo(base[0]), base[3]), want)
        if base is None:
            base = (y, bp, o3ref, yref)
    print(f"{cid} nterms={nterms}: {n} in-range elements bit-exact, worst error of the rest {_worst():.2e}")


# ------------------------------------------------------------------------------------------------ backward-data epilogues
def _bwd_launch(case, nterms, name, how, val, masksign=1.0):
    from bin_amd import ops
    lffd = case["lffd"]
    ks = 1 if lffd else 3
    if lffd:
        cf, cin = 96, 224
        res_chunks, mask_from = 6, 12
    elif case["y_unshuf"]:
        cf, cin, res_chunks, mask_from = 32, 64, 0, 0
    else:
        cf, cin = 32, 96
        res_chunks, mask_from = (6 if case["mask"] else 3), 2
    gen = torch.Generator().manual_seed(41 + cin)
    w = torch.zeros(cf, cin, ks, ks, dtype=torch.float64)
    for i in range(cin):
        w[i % cf, i, ks // 2, ks // 2] += 1
        w[(i + 7) % cf, i, ks // 2, ks // 2] += 1
    gy = _grid((N, cf, H, W), gen)
    gp = ops.nchw_to_planes(gy.float().cuda(), nterms)
    t = TARGET + 16 * mask_from if case["mask"] and not lffd else TARGET
    a, b = t % cf, (t + 7) % cf        # the two gy channels that feed gx[t]
    if how == "sum":
        _poke(gp.hi, a, PIX, _f32(val[0]))
        _poke(gp.hi, b, PIX, _f32(val[1]))
    elif how == "plane":
        _poke(gp.hi, a, PIX, val)
    nch = (cin + 15) // 16
    res = acc = mask = None
    if case["res"]:
        res = ops.nchw_to_planes(_grid((N, cin, H, W), gen).float().cuda(), nterms)
    if case["mask"]:
        m = _grid((N, cin, H, W), gen)
        m[0, t, PIX[1], PIX[2]] = masksign
        mask = ops.nchw_to_planes(m.float().cuda(), 1)
    dw = ops.DgradWeights(w.float().cuda(), nterms=nterms)
    out = None
    if case["acc"]:
        out = ops.nchw_to_planes(_grid((N, cin, H, W), gen).float().cuda(), nterms)
        acc = out
    if how == "extra":
        _poke((res if res is not None else acc).hi, t, PIX, val)
    # the reference, from what the planes hold
    ref = F.conv_transpose2d(_from_planes(gp.hi, gp.lo, cf), w, padding=ks // 2)
    if res is not None:
        ref[:, :16 * res_chunks] += _from_planes(res.hi, res.lo, cin)[:, :16 * res_chunks]
    if acc is not None:
        ref = ref + _from_planes(acc.hi, acc.lo, cin)
    if mask is not None:
        keep = _from_planes(mask.hi, None, cin) > 0
        keep[:, :16 * mask_from] = True
        ref = torch.where(keep, ref, torch.zeros_like(ref))    # torch's threshold backward: 0 whatever the gradient
    y = ops.conv2d_bwd_data(gp, dw, res=res, res_chunks=res_chunks, acc=acc, mask=mask, mask_from=mask_from, out=out,
                            y_unshuf=nch if case["y_unshuf"] else 0)
    if case["y_unshuf"]:
        ref = ref.view(N, cin, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(N, 4 * cin, H // 2, W // 2)
        return y.hi, y.lo, _to_planes(ref, 4 * nch)
    return y.hi, y.lo, _to_planes(ref, nch)


@pytest.mark.parametrize("cid,nterms", runs(("bwd_data",)))
def test_backward_data_store_saturates_flags_and_stays_local(cid, nterms):
    """binhip_conv2d_bwd_data: plain, residual, accumulator aliasing the output, ReLU mask, the inverse-PixelShuffle store and the LFF
    pattern's own instantiation.  Behind a saved activation <= 0 an inf / NaN gradient stores 0 with the bit clear."""
    from bin_amd import ops
    ops.check_status()
    case = CASES[cid]
    kinds = ("sum", "plane", "extra") if (case["res"] or case["acc"]) else ("sum", "plane")
    base = _bwd_launch(case, nterms, None, None, None)
    torch.cuda.synchronize()
    n = check_store("baseline", *base, _status())
    signs = (1.0, -1.0) if case["mask"] and not case["lffd"] else (1.0,)
    for ms in signs:
        for name, how, val in _values(kinds):
            hi, lo, ref = _bwd_launch(case, nterms, name, how, val, ms)
            torch.cuda.synchronize()
            n += check_store(f"{cid} {name} mask {ms:+}", hi, lo, ref, _status(), base if ms > 0 else None)
    print(f"{cid} nterms={nterms}: {n} in-range elements bit-exact, worst error of the rest {_worst():.2e}")


# ------------------------------------------------------------------------------------------------ null status word
@pytest.mark.parametrize("nterms", [3, 1])
def test_null_status_word_stores_the_same_planes(nterms, monkeypatch):
    """status = NULL through the C ABI: return code 0 (ops.L.check raises otherwise) and the same planes as with a status word."""
    from bin_amd import ops
    ops.check_status()

    class _Null:
        def data_ptr(self):
            return 0
    cases = [(_conv_fwd_launch, CASES["conv_planes_k3_c96_relu1"], ("-nan bias", "bias", NAN_NEG)),
             (_conv_fwd_launch, CASES["conv_residual_k3_relu1"], ("+inf extra", "extra", float("inf"))),
             (_pack_case, CASES["pack_inputs_3"], ("1e5", "sum", (F16_MAX, 34496.0)))]
    for launch, case, (name, how, val) in cases:
        hi, lo, _ = launch(case, nterms, name, how, val)
        torch.cuda.synchronize()
        assert _status() == 1
        with monkeypatch.context() as m:
            m.setattr(ops, "status_word", lambda dev: _Null())
            hi2, lo2, _ = launch(case, nterms, name, how, val)
            torch.cuda.synchronize()
        assert _status() == 0
        assert torch.equal(hi.view(torch.int16), hi2.view(torch.int16)), name
        if lo is not None:
            assert torch.equal(lo.view(torch.int16), lo2.view(torch.int16)), name
    tail = dict(CASES["rdb_tail_store1_o3"])
    y, bp, _, _ = _tail_launch(tail, nterms, "+nan bias", "bias", NAN_POS)
    torch.cuda.synchronize()
    assert _status() == 1
    with monkeypatch.context() as m:
        m.setattr(ops, "status_word", lambda dev: _Null())
        y2, bp2, _, _ = _tail_launch(tail, nterms, "+nan bias", "bias", NAN_POS)
        torch.cuda.synchronize()
    assert _status() == 0
    assert torch.equal(y.hi.view(torch.int16), y2.hi.view(torch.int16))
    assert torch.equal(bp.hi.view(torch.int16), bp2.hi.view(torch.int16))


# ------------------------------------------------------------------------------------------------ whole RDN
@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_rdn_forward_raises_on_a_nan_or_huge_bias_in_every_dense_conv(prec, canon_gpu):
    """A +-NaN or +1e30 bias in conv c of dense block d (every c, two blocks) must raise `fp16 range exceeded`; a -1e30 bias in these
    ReLU convs must not.  Per-conv path (NO_FUSE), fused tail (default), the three-phase dense-block launch (RDB3, f16x3), each with and
    without KEEP_ACTS; the output stays finite in every case."""
    from bin_amd import ops, _lib as L
    from bin_amd.models.archs.RDN import PRECISIONS
    from bin_amd.rdn_plan import RdnWeights, rdn_forward
    ops.check_status()
    nterms = PRECISIONS[prec]
    gen = torch.Generator().manual_seed(51)
    ins = [torch.rand(1, 3, 32, 48, generator=gen).cuda() for _ in range(3)]
    plans = [0, L.PLAN_NO_FUSE] + ([L.PLAN_RDB3] if nterms == 3 else [])
    runs = 0
    for d in (0, 11):
        for c in range(4):
            key = f"model2.RDBs.{d}.convs.{c}.conv.0.bias"
            for val, raises in ((NAN_POS, True), (NAN_NEG, True), (1e30, True), (-1e30, False)):
                params = dict(canon_gpu)
                b = params[key].clone()
                b[5] = _f32(val) if not isinstance(val, int) else _bias_tensor([val])[0]
                params[key] = b
                wts = RdnWeights(params, 3, nterms, prefix="model2.")
                for plan in plans:
                    for keep in (0, L.PLAN_KEEP_ACTS):
                        out = rdn_forward(wts, ins, flags=plan | keep)
                        torch.cuda.synchronize()
                        assert bool(torch.isfinite(out).all()), (d, c, val, plan, keep)
                        if raises:
                            with pytest.raises(RuntimeError, match="fp16 range exceeded"):
                                ops.check_status()
                        else:
                            ops.check_status()
                        runs += 1
    print(f"rdn forward {prec}: {runs} runs, bit raised exactly where expected")


@pytest.mark.parametrize("mode", ["f16x3", "mixed", "two_layer"])
def test_rdn_backward_raises_on_a_nan_or_inf_gradient(mode, canon_cpu, monkeypatch):
    """A gout with one NaN or +inf at an interior, a ring and a corner pixel must raise `fp16 range exceeded` (the fused UPNet's gsub
    packer and ring kernel, or the two-layer path's scaled packer); gout x 2^30 must not: the per-call power-of-two scale absorbs it and
    the gradients scale with it."""
    from bin_amd import ops
    from bin_amd.models.archs import RDN as A
    from bin_amd.weights import rdn_param_shapes
    if mode == "two_layer":
        monkeypatch.setenv("BIN_AMD_FUSED_UPNET_TRAIN", "0")
    else:
        monkeypatch.delenv("BIN_AMD_FUSED_UPNET_TRAIN", raising=False)
    ops.check_status()
    mod = A.RDN_residual_interp_2_1_input(G0=96, D=12)
    mod.load_state_dict({n: canon_cpu[f"model2.{n}"] for n in rdn_param_shapes(3)})
    mod = mod.cuda()
    mod.precision = "f16x3"
    mod.backward_precision = "f16" if mode == "mixed" else None
    gen = torch.Generator().manual_seed(61)
    ins = [torch.rand(1, 3, 16, 24, generator=gen).cuda() for _ in range(3)]
    gout = torch.randn(1, 3, 16, 24, generator=gen) * 1e-3

    def grads(g):
        xs = [t.clone().requires_grad_(True) for t in ins]
        mod(*xs).backward(g.cuda())
        torch.cuda.synchronize()
        out = [p.grad.detach().clone() for p in mod.parameters()] + [x.grad.clone() for x in xs]
        for p in mod.parameters():
            p.grad = None
        return out

    base = grads(gout)
    ops.check_status()
    assert (mod.kernel_weights(3).fused_graph is not None) == (mode != "two_layer")
    for where in ((1, 8, 12), (2, 0, 7), (0, 15, 23)):
        for val in (float("nan"), float("inf")):
            g = gout.clone()
            g[(0,) + where] = val
            grads(g)
            with pytest.raises(RuntimeError, match="fp16 range exceeded"):
                ops.check_status()
    big = grads(gout * 2.0 ** 30)
    ops.check_status()
    worst = max(float((b - a * 2.0 ** 30).abs().max() / (a.abs().max() * 2.0 ** 30).clamp_min(1e-30)) for a, b in zip(base, big))
    print(f"rdn backward {mode}: gout x 2^30 relative deviation {worst:.2e}")
    assert worst <= 1e-6


@pytest.mark.parametrize("mode", ["f16x3", "mixed", "two_layer"])
def test_gradient_glue_stores_saturate_flag_and_stay_local(mode, canon_cpu, monkeypatch):
    """The backward's own plane stores, read back from the backward workspace (binhip_rdn_backward_workspace_layout): the fused
    UPNet's gsub planes (pixel-unshuffled, ring-zeroed, scaled gout) and ring backward-data (upnet_ring_dgrad_kernel, read-modify-write
    of the G1 gradient), or the two-layer path's scaled gout planes (nchw_to_planes_scaled).  All weights are scaled by 2^-10, so that
    every later store stays far inside the range: the status bit can then only come from these kernels.  A NaN or +inf gout at an
    interior or a ring pixel: bit set; the planes against float64 gout x the call's scale (NaN -> -65504, lo = 0); with a NaN the scale
    is the clean call's (the amax ignores NaN), and every element outside the NaN's reach is bit-identical to the clean call."""
    from bin_amd import _lib as L, ops
    from bin_amd.models.archs import RDN as A
    from bin_amd.range_stats import _layout, _view
    from bin_amd.weights import rdn_param_shapes
    if mode == "two_layer":
        monkeypatch.setenv("BIN_AMD_FUSED_UPNET_TRAIN", "0")
    else:
        monkeypatch.delenv("BIN_AMD_FUSED_UPNET_TRAIN", raising=False)
    ops.check_status()
    mod = A.RDN_residual_interp_2_1_input(G0=96, D=12)
    mod.load_state_dict({n: canon_cpu[f"model2.{n}"] * 2.0 ** -10 for n in rdn_param_shapes(3)})
    mod = mod.cuda()
    mod.precision = "f16x3"
    mod.backward_precision = "f16" if mode == "mixed" else None
    fused = mode != "two_layer"
    n, Hf, Wf = 1, 16, 24
    h, w = Hf // 2, Wf // 2
    gen = torch.Generator().manual_seed(71)
    ins = [torch.rand(n, 3, Hf, Wf, generator=gen).cuda() for _ in range(3)]
    gout = torch.randn(n, 3, Hf, Wf, generator=gen) * 1e-3
    got = {}

    def hook(kind, module, dims, ws, info):
        if kind != "backward":
            return
        v = _layout(L.lib().binhip_rdn_backward_workspace_layout, dims, L.RDN_BWD_LAYOUT_WORDS, module.shape)
        nt, P = dims[4], v[0]
        base = (-ws.data_ptr()) % 256
        got["scale"] = float(ws[base + v[23]: base + v[23] + 8].view(torch.float32)[0])
        size = P if fused else v[4]                     # gsub: one half-resolution chunk; two-layer: one full-resolution one
        shape = (1, n, h, w, 16) if fused else (1, n, Hf, Wf, 16)
        got["g"] = (_view(ws, v[3], size).view(shape).clone(), _view(ws, v[3] + size, size).view(shape).clone() if nt == 3 else None)
        got["gg1"] = (_view(ws, v[9], v[10]).view(6, n, h, w, 16).clone(),
                      _view(ws, v[9] + v[10], v[10]).view(6, n, h, w, 16).clone() if nt == 3 else None)
    mod.debug_hook = hook

    def run(g):
        xs = [t.clone().requires_grad_(True) for t in ins]
        mod(*xs).backward(g.cuda())
        torch.cuda.synchronize()
        for p in mod.parameters():
            p.grad = None
        return dict(got), _status()

    def ref_planes(g, scale):
        g = g.double() * scale
        if not fused:
            return _to_planes(g)
        g = g.clone()
        g[:, :, 0, :] = g[:, :, -1, :] = 0
        g[:, :, :, 0] = g[:, :, :, -1] = 0
        return _to_planes(F.pixel_unshuffle(g, 2), 1)

    clean, flag = run(gout)
    assert flag == 0
    assert (mod.kernel_weights(3).fused_graph is not None) == fused, "the fused UPNet training path was (not) taken"
    cref = ref_planes(gout, clean["scale"])
    check_store(f"{mode} clean", *clean["g"], cref, flag)
    for where in ((1, 8, 12), (2, 0, 7)):
        ring = where[1] == 0
        for val in (float("nan"), float("inf")):
            g = gout.clone()
            g[(0,) + where] = val
            out, flag = run(g)
            label = f"{mode} gout {val} at {where}"
            assert flag == 1, f"{label}: no status bit"
            if val != val:
                assert out["scale"] == clean["scale"], f"{label}: the NaN changed the scale"
            ref = ref_planes(g, out["scale"])
            check_store(label + " g planes", *out["g"], ref, flag, (*clean["g"], cref) if val != val else None, want=True)
            hi, lo = out["gg1"]
            assert bool(torch.isfinite(hi.float()).all()) and (lo is None or bool(torch.isfinite(lo.float()).all())), label
            if fused and ring and val != val:
                # the ring kernel's reach from full-resolution (0, 7): half-resolution rows 0-2, columns 1-5, every channel
                reach = torch.zeros_like(hi, dtype=torch.bool)
                reach[:, :, 0:3, 1:6, :] = True
                bhi, blo = clean["gg1"]
                assert bool((hi[reach].float() == -F16_MAX).all()), f"{label}: ring backward-data did not store -65504 for NaN"
                assert bool(_same_bits(hi, bhi)[~reach].all()), f"{label}: ring backward-data changed elements out of its reach"
                if lo is not None:
                    assert bool((lo[reach] == 0).all()) and bool(_same_bits(lo, blo)[~reach].all()), label
    print(f"glue {mode}: scale {clean['scale']:.3g}; bit, planes and locality as expected, worst error of the rest {_worst():.2e}")
