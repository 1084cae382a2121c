"""-m gpu: every kernel of binhip_convlstm.hip, binhip_loss.hip and binhip_layout.hip — the fused ConvLSTM cell and its three-pass
backward, the elementwise gate kernels of the general cell, the pixel-loss reductions (one path for one and for many terms), the
gradient-scale reduction and the layout / frame glue — against float64 (or, where the contract is bit-exactness, numpy) at the shapes, sizes and
magnitudes where such kernels go wrong.  Case tables, references and bars: lstm_cases.py, loss_cases.py, glue_cases.py; their CPU
pins: test_cpu_small_kernels.py.  Each comparison prints e32 (float32 torch against float64), the bar max(B, 4 * e32) and the kernel's
error on a line that starts with `[small-kernels]`.

Measured on an MI355X when this module was written, largest error / bar over all cases: see DESIGN.md ("Small kernels")."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import glue_cases as GC
import loss_cases as LS
import lstm_cases as LC
import small_kernel_bit_cases as BC
from conftest import REPO

pytestmark = pytest.mark.gpu

NULL = C.c_void_p(0)


def _p(t):
    return NULL if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib():
    from bin_amd import _lib as L
    return L, L.lib()


def _nan_like(t):
    return torch.full_like(t, float("nan"))


# ------------------------------------------------------------------------------------------------------- A. fused ConvLSTM cell
def _run_fused(case, inp, conv):
    """binhip_convlstm_fwd + _bwd through the C ABI with the variant's NULL pointers; `conv` places every plane (identity copy =
    16-byte aligned = four pixels per thread when W % 4 == 0; lstm_cases.off1 = one pixel per thread).  Outputs start as NaN, so an element
    the kernels do not write fails the comparison."""
    L, lib = _lib()
    names = LC.wanted(case)
    dev = torch.device("cuda")
    D = lambda t: None if t is None else conv(t.to(dev))
    x, c0, h0, gh, gc = (D(inp[k]) for k in ("x", "c0", "h0", "gh", "gc"))
    w, b = inp["w"].to(dev), inp["b"].to(dev)
    if case.variant == "gh_only":
        gc = None
    if case.variant == "gc_only":
        gh = None
    out = {nm: conv(_nan_like(inp["x"].to(dev))) for nm in ("c", "h", "gx", "gcp", "ghp") if nm in names}
    if "dw" in names:
        out["dw"], out["db"] = _nan_like(w), _nan_like(b)
    n, h, ww = case.n, case.h, case.w
    L.check(lib.binhip_convlstm_fwd(_p(x), _p(c0), _p(h0), _p(w), _p(b), case.fb, n, h, ww, _p(out.get("c")), _p(out["h"]),
                                    _stream()), "convlstm_fwd")
    nbytes = lib.binhip_convlstm_bwd_workspace_bytes(n, h, ww)
    ws = torch.empty(nbytes + 512, dtype=torch.uint8, device=dev)
    L.check(lib.binhip_convlstm_bwd(_p(x), _p(c0), _p(h0), _p(w), _p(b), case.fb, n, h, ww, _p(gh), _p(gc), _p(ws), nbytes,
                                    _p(out.get("gx")), _p(out.get("ghp")), _p(out.get("gcp")), _p(out.get("dw")), _p(out.get("db")),
                                    _stream()), "convlstm_bwd")
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in out.items()}


@pytest.mark.parametrize("tag", [c.tag for c in LC.CASES])
def test_fused_convlstm_vs_float64(tag):
    """Both widths of the gate path against float64: aligned planes (four pixels per thread when W % 4 == 0) and every plane offset by
    one float (one pixel per thread); where both run they must also agree bit for bit."""
    case = LC.CASE_BY_TAG[tag]
    inp = LC.make_inputs(case)
    r64, r32 = LC.reference(case, inp, torch.float64), LC.reference(case, inp, torch.float32)
    names = LC.wanted(case)
    runs = [("aligned", lambda t: t.clone())]
    if case.w % 4 == 0:
        runs.append(("off1", LC.off1))
    got = {}
    for label, conv in runs:
        got[label] = _run_fused(case, inp, conv)
        assert sorted(got[label]) == sorted(names)
        LC.compare(f"{tag} [{label}]", names, got[label], r64, r32)
    if len(runs) == 2:
        for nm in names:
            assert torch.equal(got["aligned"][nm], got["off1"][nm]), (tag, nm)


# ------------------------------------------------------------------------------------------------------- A. general cell's gate kernels
@pytest.mark.parametrize("regime", LC.GATES_REGIMES)
@pytest.mark.parametrize("hidden", LC.GATES_HIDDEN)
def test_lstm_gate_kernels_vs_float64(hidden, regime):
    L, lib = _lib()
    gates, cp, gh, gc = LC.make_gates(hidden, regime)
    n, h, w = LC.GATES_SHAPE
    G, CP, GH, GC_ = (t.cuda() for t in (gates, cp, gh, gc))
    for fb in LC.GATES_FB:
        for cpv, CPv in ((None, None), (cp, CP)):
            for (a, A), (b, B) in (((gh, GH), (gc, GC_)), ((gh, GH), (None, None)), ((None, None), (gc, GC_))):
                r64 = LC.gates_reference(gates, cpv, fb, a, b, torch.float64)
                r32 = LC.gates_reference(gates, cpv, fb, a, b, torch.float32)
                out = {"c": _nan_like(CP), "h": _nan_like(CP), "dgates": _nan_like(G)}
                if cpv is not None:
                    out["gcp"] = _nan_like(CP)
                L.check(lib.binhip_lstm_gates_fwd(_p(G), _p(CPv), fb, n, hidden, h, w, _p(out["c"]), _p(out["h"]), _stream()), "gates_fwd")
                L.check(lib.binhip_lstm_gates_bwd(_p(G), _p(CPv), _p(A), _p(B), fb, n, hidden, h, w, _p(out["dgates"]),
                                                  _p(out.get("gcp")), _stream()), "gates_bwd")
                torch.cuda.synchronize()
                tag = f"gates h{hidden} {regime} fb{fb:g} cp={cpv is not None} gh={a is not None} gc={b is not None}"
                LC.compare(tag, list(r64), out, r64, r32, bars=LC.GATES_BARS)


# ------------------------------------------------------------------------------------------------------- A. item 5: state-only gradients
GENERAL_BARS = dict(LC.BARS, gcp=3e-5, ghp=3e-5, c=2e-6, h=2e-6)        # the general cell's gradients pass through the f16x3 convolution
                                                                         # kernels: 3e-5, the bar test_convlstm_cells_of_other_sizes applies


@pytest.mark.parametrize("kind", ["fused_3_3_k3", "general_5_7_k3"])
def test_state_gradients_flow_when_only_prev_state_requires_grad(kind):
    """A ConvLSTMCell with frozen weights and an input without grad, `prev_state` requiring grad: the state gradients must exist
    and be float64's (the cell once took the plain forward here and dropped them silently)."""
    from bin_amd.models.archs import RDN as A
    from oracle import rdn_oracle as O
    cin, hid = (3, 3) if kind.startswith("fused") else (5, 7)
    cell = A.ConvLSTMCell(cin, hid, forget_bias=0.5)
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():                                                   # (the constructor's Xavier draw uses the global RNG)
        cell.Gates.weight.copy_((torch.rand(cell.Gates.weight.shape, generator=g) - 0.5) * 0.4)
        cell.Gates.bias.copy_((torch.rand(4 * hid, generator=g) - 0.5) * 0.4)
    cell.requires_grad_(False)
    n, h, w = 2, 9, 20
    x = torch.rand(n, cin, h, w, generator=g)
    c0, h0 = (torch.rand(n, hid, h, w, generator=g) - 0.5) * 2, (torch.rand(n, hid, h, w, generator=g) - 0.5) * 2
    gh, gc = torch.rand(n, hid, h, w, generator=g) - 0.5, torch.rand(n, hid, h, w, generator=g) - 0.5
    ref = {}
    for dt in (torch.float64, torch.float32):
        cr, hr = c0.to(dt).clone().requires_grad_(True), h0.to(dt).clone().requires_grad_(True)
        hh, (cc, _) = O.convlstm_cell(x.to(dt), [cr, hr], cell.Gates.weight.detach().to(dt), cell.Gates.bias.detach().to(dt), forget_bias=0.5)
        ((hh * gh.to(dt)).sum() + (cc * gc.to(dt)).sum()).backward()
        ref[dt] = {"c": cc.detach(), "h": hh.detach(), "gcp": cr.grad, "ghp": hr.grad}
    cell = cell.cuda()
    cg, hg = c0.cuda().requires_grad_(True), h0.cuda().requires_grad_(True)
    hh, (cc, h_again) = cell(x.cuda(), [cg, hg])
    assert h_again is hh and hh.requires_grad and cc.requires_grad
    ((hh * gh.cuda()).sum() + (cc * gc.cuda()).sum()).backward()
    assert cg.grad is not None and hg.grad is not None
    assert cell.Gates.weight.grad is None and cell.Gates.bias.grad is None
    got = {"c": cc, "h": hh, "gcp": cg.grad, "ghp": hg.grad}
    bars = LC.BARS if kind.startswith("fused") else GENERAL_BARS
    LC.compare(f"state-only {kind}", ["c", "h", "gcp", "ghp"], got, ref[torch.float64], ref[torch.float32], bars=bars)


def test_lstm_gates_autograd_node_accepts_gates_that_are_not_float32():
    """_LstmGatesFn.backward hands the saved gates to the kernel through the .float() its forward applied (a float64 gates tensor
    was once read as float32 words there)."""
    from bin_amd.autograd import _LstmGatesFn
    gates, cp, gh, gc = LC.make_gates(3, "moderate")
    r64 = LC.gates_reference(gates, cp, 1.0, gh, gc, torch.float64)
    r32 = LC.gates_reference(gates, cp, 1.0, gh, gc, torch.float32)
    G, CP = gates.double().cuda().requires_grad_(True), cp.cuda().requires_grad_(True)
    h1, c1 = _LstmGatesFn.apply(G, CP, 1.0, 3)
    ((h1 * gh.cuda()).sum() + (c1 * gc.cuda()).sum()).backward()
    assert G.grad.dtype == torch.float64
    got = {"c": c1, "h": h1, "dgates": G.grad, "gcp": CP.grad}
    LC.compare("gates autograd node, float64 gates", list(got), got, r64, r32, bars=LC.GATES_BARS)


# ------------------------------------------------------------------------------------------------------- B. pixel losses
@pytest.mark.parametrize("numel", LS.NUMELS)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_pixel_loss_vs_float64(kind, numel):
    L, lib = _lib()
    x, y = LS.make_xy(numel)
    X, Y = x.cuda(), y.cuda()
    part = torch.empty(lib.binhip_charbonnier_partials(numel), dtype=torch.float32, device="cuda")
    gl = torch.tensor([LS.GLOSS], dtype=torch.float32, device="cuda")
    for eps in (LS.EPS_VALUES if (kind == "cb" and numel in (257, LS.FWD_CAP + 1)) else LS.EPS_VALUES[:1]):
        r64, r32 = (LS.reference(kind, x, y, eps, LS.GLOSS, dt) for dt in (torch.float64, torch.float32))
        tag = f"{kind} n={numel} eps={eps:g}"
        loss = torch.full((1,), float("nan"), device="cuda")
        L.check(lib.binhip_pixel_loss_fwd(LS.KIND_ID[kind], _p(X), _p(Y), numel, eps, _p(part), _p(loss), _stream()), "loss_fwd")
        LS.check_loss(tag, loss[0], r64["loss"], r32["loss"])
        for want_x, want_y in ((True, False), (False, True), (True, True)):
            gx = _nan_like(X) if want_x else None
            gy = _nan_like(X) if want_y else None
            L.check(lib.binhip_pixel_loss_bwd(LS.KIND_ID[kind], _p(X), _p(Y), numel, eps, _p(gl), _p(gx), _p(gy), _stream()), "loss_bwd")
            if want_x:
                LS.check_grad(f"{tag} gx(x={want_x},y={want_y})", gx, r64["gx"], r32["gx"])
            if want_y:
                LS.check_grad(f"{tag} gy(x={want_x},y={want_y})", gy, r64["gy"], r32["gy"])
        if kind == "l1":                                                   # sign(0) = 0 on the stretch of exact ties
            assert bool((gx[X == Y] == 0).all()) and bool((gy[X == Y] == 0).all())


@pytest.mark.parametrize("numel", [1, 257, LS.FWD_CAP + 1, LS.BWD_CAP + 1])
def test_charbonnier_entry_points_are_the_pixel_loss_ones(numel):
    """binhip_charbonnier_fwd / _bwd (the first ABI's names) == binhip_pixel_loss_* with BINHIP_LOSS_CHARBONNIER, bit for bit —
    which test_pixel_loss_vs_float64 pins to float64."""
    L, lib = _lib()
    x, y = (t.cuda() for t in LS.make_xy(numel))
    part = torch.empty(lib.binhip_charbonnier_partials(numel), dtype=torch.float32, device="cuda")
    gl = torch.tensor([LS.GLOSS], dtype=torch.float32, device="cuda")
    a, b = (torch.full((1,), float("nan"), device="cuda") for _ in range(2))
    ga, gb, ha, hb = (_nan_like(x) for _ in range(4))
    L.check(lib.binhip_charbonnier_fwd(_p(x), _p(y), numel, 1e-3, _p(part), _p(a), _stream()), "charbonnier_fwd")
    L.check(lib.binhip_pixel_loss_fwd(L.LOSS_CHARBONNIER, _p(x), _p(y), numel, 1e-3, _p(part), _p(b), _stream()), "pixel_loss_fwd")
    L.check(lib.binhip_charbonnier_bwd(_p(x), _p(y), numel, 1e-3, _p(gl), _p(ga), _p(ha), _stream()), "charbonnier_bwd")
    L.check(lib.binhip_pixel_loss_bwd(L.LOSS_CHARBONNIER, _p(x), _p(y), numel, 1e-3, _p(gl), _p(gb), _p(hb), _stream()), "pixel_loss_bwd")
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(ga, gb) and torch.equal(ha, hb)
    assert bool(torch.isfinite(ga).all()) and torch.equal(ga, -ha)


def test_device_cus_is_the_device_property():
    L, lib = _lib()
    assert lib.binhip_device_cus() == torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


@pytest.mark.parametrize("kind,T,numel,eps", LS.MULTI_CASES)
def test_multi_term_loss_vs_float64(kind, T, numel, eps):
    """binhip_multi_loss_fwd / _bwd: the `terms` vector, the loss and every gradient against float64 of the formula itself (the
    bit-for-bit agreement with the per-term path stays in test_gpu_loss.py)."""
    from bin_amd import ops
    ts = LS.make_multi(numel)
    r64, r32 = (LS.multi_reference(kind, T, ts, eps, LS.GLOSS, dt) for dt in (torch.float64, torch.float32))
    _, idx = LS.multi_pairs(T, ts)
    used = sorted(r64["grads"])
    dev = {i: ts[i].cuda() for i in used}
    pairs = [(dev[a], dev[b]) for a, b in idx]
    loss, terms = ops.multi_pixel_loss(LS.KIND_ID[kind], pairs, eps=eps)
    tag = f"multi {kind} T={T} n={numel} eps={eps:g}"
    LS.check_loss(tag, loss, r64["loss"], r32["loss"])
    LS.check_terms(tag, terms.cpu(), r64["terms"], r32["terms"])
    where = {i: [(t, 1.0) for t, (a, _) in enumerate(idx) if a == i] + [(t, -1.0) for t, (_, b) in enumerate(idx) if b == i] for i in used}
    gl = torch.tensor(LS.GLOSS, dtype=torch.float32, device="cuda")
    from bin_amd import _lib as L
    for k0 in range(0, len(used), L.LOSS_MAX_TERMS):                       # at most BINHIP_LOSS_MAX_TERMS gradient outputs per launch
        batch = used[k0:k0 + L.LOSS_MAX_TERMS]
        outs = ops.multi_pixel_loss_grad(LS.KIND_ID[kind], pairs, gl, [(dev[i], where[i]) for i in batch], eps=eps)
        for i, g in zip(batch, outs):
            LS.check_grad(f"{tag} g{i}", g, r64["grads"][i], r32["grads"][i])


@pytest.mark.parametrize("numel", LS.SCALE_NUMELS)
def test_grad_scale_vs_exact_exponent_arithmetic(numel):
    """amax in the LAST element (a grid-stride loop that stops early misses it), at a power of two, one ulp above and below, for a
    power-of-two and two other targets: (scale, 1 / scale) must be the exact pair.  All-zero input gives 1."""
    L, lib = _lib()
    base = LS.scale_input(numel, 1.0).cuda()
    part = torch.empty(lib.binhip_charbonnier_partials(numel), dtype=torch.float32, device="cuda")
    for k, amax in enumerate(LS.SCALE_AMAX):
        v = base * float(amax)
        v[-1] = float(amax) * (-1.0 if k % 2 else 1.0)
        assert numel == 1 or float(v[:-1].abs().max()) < float(amax)
        for target in LS.SCALE_TARGETS:
            sc = torch.full((2,), float("nan"), device="cuda")
            L.check(lib.binhip_grad_scale(_p(v), numel, target, _p(part), _p(sc), _stream()), "grad_scale")
            assert tuple(sc.tolist()) == LS.scale_reference(amax, target), (numel, float(amax), target, sc.tolist())
    sc = torch.full((2,), float("nan"), device="cuda")
    L.check(lib.binhip_grad_scale(_p(torch.zeros_like(base)), numel, 16.0, _p(part), _p(sc), _stream()), "grad_scale")
    assert sc.tolist() == [1.0, 1.0]


# ------------------------------------------------------------------------------------------------------- B'. the bit pin
def _recorded_small_kernel_bits():
    with open(os.path.join(REPO, "tests", "golden", "small_kernel_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("key", BC.KEYS)
def test_small_kernel_bits_are_the_recorded_ones(key):
    """The ConvLSTM, gate, pixel-criterion and gradient-scale entry points at the shapes of tests/small_kernel_bit_cases.py return bit
    for bit what tests/golden/make_small_kernel_bits.py recorded from the commit named in tests/golden/small_kernel_bits.json: these
    kernels may move between files and share their gate accumulation, their criterion and their block reductions; the roundings and
    the pairing of every sum may not change.  No atomics and no device-dependent summation order, so nothing may be left out."""
    rec = _recorded_small_kernel_bits()
    assert not rec["left_out"], f"cases that did not reproduce when the fixture was recorded: {rec['left_out']}"
    assert sorted(rec["bits"]) == sorted(BC.KEYS), "tests/golden/small_kernel_bits.json and tests/small_kernel_bit_cases.py name different cases"
    got = BC.bits(key)
    assert got == rec["bits"][key], f"{key}: the bits differ from those recorded from {rec['recorded_from']}"


# ------------------------------------------------------------------------------------------------------- C. layout glue
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def _planes_empty(nch, n, h, w, lo=True):
    hi = torch.full((nch, n, h, w, 16), float("nan"), dtype=torch.float16, device="cuda")
    return hi, (torch.full_like(hi, float("nan")) if lo else None)


def _assert_split(tag, x_planes, hi, lo, status, nterms):
    """hi / lo planes read back == numpy's split of the same values, bit for bit; the derived bound; status bit clear."""
    ehi, elo = GC.split_ref(x_planes)
    ghi = _bits(hi)
    bad = np.flatnonzero(ghi.reshape(-1) != ehi.view(np.uint16).reshape(-1))
    assert bad.size == 0, (tag, "hi", bad.size, x_planes.reshape(-1)[bad[:5]], ghi.reshape(-1)[bad[:5]])
    if nterms == 3:
        glo = _bits(lo)
        bad = np.flatnonzero(glo.reshape(-1) != elo.view(np.uint16).reshape(-1))
        assert bad.size == 0, (tag, "lo", bad.size, x_planes.reshape(-1)[bad[:5]], glo.reshape(-1)[bad[:5]], elo.view(np.uint16).reshape(-1)[bad[:5]])
    got_hi = hi.cpu().numpy()
    got_lo = lo.cpu().numpy() if nterms == 3 else None
    assert GC.split_bound_ok(x_planes, got_hi, got_lo, nterms).all(), tag
    assert int(status.item()) == 0, (tag, int(status.item()))


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("scale", [None, 2.0 ** -7, 2.0 ** 9], ids=["plain", "scaled_2^-7", "scaled_2^9"])
def test_split_store_contract_over_every_binade(scale, nterms):
    """include/binhip.h 'Dynamic range': the stored pair is hi = fp16(x), lo = fp16(x - hi), round-to-nearest-even with fp16
    subnormals kept — bit for bit over every binade from 2^-30 to 2^15 — hence |x - (hi + lo)| <= max(2^-23 |x|, 2^-25), and
    max(2^-11 |x|, 2^-25) for nterms = 1.  The scaled entry point states the same about x * scale (a power of two: exact)."""
    L, lib = _lib()
    v = GC.split_values()
    if scale is not None:
        v = v[np.abs(v.astype(np.float64) * scale) <= GC.F16_MAX]
    x = GC.as_nchw(v, 1, 37)
    n, c, h, w = x.shape
    X = torch.from_numpy(x).cuda()
    hi, lo = _planes_empty(3, n, h, w, nterms == 3)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    if scale is None:
        L.check(lib.binhip_nchw_to_planes(_p(X), n, c, h, w, _p(hi), _p(lo), _p(status), _stream()), "nchw_to_planes")
    else:
        sc = torch.tensor([scale, 1.0 / scale], dtype=torch.float32, device="cuda")
        L.check(lib.binhip_nchw_to_planes_scaled(_p(X), n, c, h, w, _p(sc), _p(hi), _p(lo), _p(status), _stream()), "nchw_to_planes_scaled")
    _assert_split(f"split scale={scale} nterms={nterms}", GC.planes_of(x * np.float32(scale or 1.0)), hi, lo, status, nterms)


@pytest.mark.parametrize("nterms", [3, 1])
def test_split_store_contract_through_pack_inputs(nterms):
    L, lib = _lib()
    v = GC.split_values()
    k = 2
    per = k * 3 * 2
    wd = 2 * (-(-len(v) // (per * 2)))
    buf = np.zeros(per * wd, np.float32)
    buf[:len(v)] = v
    imgs = [np.ascontiguousarray(a) for a in buf.reshape(k, 1, 3, 2, wd)]
    dev = [torch.from_numpy(a).cuda() for a in imgs]
    hi, lo = _planes_empty(2, 1, 1, wd // 2, nterms == 3)
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    arr = (C.c_void_p * k)(*[t.data_ptr() for t in dev])
    L.check(lib.binhip_pack_inputs(arr, k, 1, 2, wd, _p(hi), _p(lo), _p(status), _stream()), "pack_inputs")
    _assert_split(f"pack_inputs nterms={nterms}", GC.pack_inputs_ref(imgs), hi, lo, status, nterms)


@pytest.mark.parametrize("nhw", GC.NHW, ids=["%dx%dx%d" % s for s in GC.NHW])
@pytest.mark.parametrize("c", GC.CHANNELS)
def test_nchw_planes_both_ways_bit_for_bit(c, nhw):
    L, lib = _lib()
    n, h, w = nhw
    rng = np.random.RandomState(c * 100 + h)
    x = (rng.randn(n, c, h, w) * 3).astype(np.float32)
    X = torch.from_numpy(x).cuda()
    nch = (c + 15) // 16
    for nterms in (3, 1):
        hi, lo = _planes_empty(nch, n, h, w, nterms == 3)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(lib.binhip_nchw_to_planes(_p(X), n, c, h, w, _p(hi), _p(lo), _p(status), _stream()), "nchw_to_planes")
        _assert_split(f"nchw_to_planes c={c} {nhw}", GC.planes_of(x), hi, lo, status, nterms)
        # and back, from planes that hold arbitrary fp16 values in every slot (padded channels included): y = float(hi) + float(lo)
        ph = (rng.randn(nch, n, h, w, 16) * 5).astype(np.float16)
        pl = (rng.randn(nch, n, h, w, 16) * 0.01).astype(np.float16) if nterms == 3 else None
        y = torch.full((n, c, h, w), float("nan"), device="cuda")
        PH, PL = torch.from_numpy(ph).cuda(), (None if pl is None else torch.from_numpy(pl).cuda())
        L.check(lib.binhip_planes_to_nchw(_p(PH), _p(PL), n, c, h, w, _p(y), _stream()), "planes_to_nchw")
        want = ph.astype(np.float32) + (pl.astype(np.float32) if pl is not None else np.float32(0))
        assert np.array_equal(y.cpu().numpy().view(np.uint32), GC.nchw_of(want, c).view(np.uint32)), (c, nhw, nterms)


@pytest.mark.parametrize("nhw", GC.NHW_EVEN, ids=["%dx%dx%d" % s for s in GC.NHW_EVEN])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_pack_inputs_and_unpack_input_grads_bit_for_bit(k, nhw):
    L, lib = _lib()
    n, h, w = nhw
    rng = np.random.RandomState(k * 10 + h)
    imgs = [rng.rand(n, 3, h, w).astype(np.float32) for _ in range(k)]
    dev = [torch.from_numpy(a).cuda() for a in imgs]
    nch = (12 * k + 15) // 16
    arr = (C.c_void_p * k)(*[t.data_ptr() for t in dev])
    for nterms in (3, 1):
        hi, lo = _planes_empty(nch, n, h // 2, w // 2, nterms == 3)
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        L.check(lib.binhip_pack_inputs(arr, k, n, h, w, _p(hi), _p(lo), _p(status), _stream()), "pack_inputs")
        _assert_split(f"pack_inputs k={k} {nhw}", GC.pack_inputs_ref(imgs), hi, lo, status, nterms)
    # the inverse with the skip path: NULL outs entries, gx0 == NULL, scale == NULL, lo == NULL
    ph = (rng.randn(nch, n, h // 2, w // 2, 16) * 4).astype(np.float16)
    pl = (rng.randn(nch, n, h // 2, w // 2, 16) * 0.004).astype(np.float16)
    gout = rng.randn(n, 3, h, w).astype(np.float32)
    PH, PL, GO = torch.from_numpy(ph).cuda(), torch.from_numpy(pl).cuda(), torch.from_numpy(gout).cuda()
    sc = torch.tensor([2.0 ** 7, 2.0 ** -7], dtype=torch.float32, device="cuda")
    for label, hi_, lo_, sc_, skip_frames in (("all", PH, PL, sc, ()), ("no_lo", PH, None, sc, ()), ("no_scale", PH, PL, None, ()),
                                              ("skip_only", None, None, sc, ()), ("null_outs", PH, PL, sc, (0, k - 1))):
        outs = [None if i in skip_frames else torch.full((n, 3, h, w), float("nan"), device="cuda") for i in range(k)]
        oarr = (C.c_void_p * k)(*[0 if o is None else o.data_ptr() for o in outs])
        L.check(lib.binhip_unpack_input_grads(_p(hi_), _p(lo_), _p(GO), _p(sc_), k, n, h, w, oarr, _stream()), "unpack_input_grads")
        want = GC.unpack_input_grads_ref(None if hi_ is None else ph, None if lo_ is None else pl, gout, 2.0 ** -7 if sc_ is not None else 1.0, k)
        for i, o in enumerate(outs):
            if o is not None:
                assert np.array_equal(o.cpu().numpy().view(np.uint32), want[i].view(np.uint32)), (label, k, nhw, i)


@pytest.mark.parametrize("r", [2, 3, 4])
@pytest.mark.parametrize("c", GC.CHANNELS)
def test_pixel_unshuffle_f32_bit_for_bit(c, r):
    """Shapes: H and W must be multiples of r, so (1, r, r), (2, 3r, 5r) (= 2x6x10 at r = 2) and 3x18x30 / 3x20x28."""
    from bin_amd import ops
    rng = np.random.RandomState(c + r)
    for n, h, w in ((1, r, r), (2, 3 * r, 5 * r), (3, 18, 30) if r < 4 else (3, 20, 28)):
        x = rng.randn(n, c, h, w).astype(np.float32)
        y = ops.pixel_unshuffle(torch.from_numpy(x).cuda(), r)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), GC.pixel_unshuffle_ref(x, r).view(np.uint32)), (c, r, n, h, w)


@pytest.mark.parametrize("nhw", GC.NHW, ids=["%dx%dx%d" % s for s in GC.NHW])
@pytest.mark.parametrize("nch", [1, 2, 3])
def test_unshuffle_planes_bit_for_bit(nch, nhw):
    L, lib = _lib()
    n, h, w = nhw                                              # output size; the input planes are 2h x 2w
    rng = np.random.RandomState(nch + h)
    xh = rng.randint(0, 1 << 16, (nch, n, 2 * h, 2 * w, 16)).astype(np.uint16)       # any bit pattern: a pure 16-byte copy
    xl = rng.randint(0, 1 << 16, (nch, n, 2 * h, 2 * w, 16)).astype(np.uint16)
    T = lambda a: torch.from_numpy(a.view(np.int16)).cuda().view(torch.float16)
    XH, XL = T(xh), T(xl)
    for with_lo in (True, False):
        yh = torch.zeros((4 * nch, n, h, w, 16), dtype=torch.float16, device="cuda")
        yl = torch.zeros_like(yh) if with_lo else None
        L.check(lib.binhip_unshuffle_planes(_p(XH), _p(XL if with_lo else None), n, h, w, nch, _p(yh), _p(yl), _stream()), "unshuffle_planes")
        assert np.array_equal(_bits(yh), GC.unshuffle_planes_ref(xh))
        if with_lo:
            assert np.array_equal(_bits(yl), GC.unshuffle_planes_ref(xl))


# ------------------------------------------------------------------------------------------------------- C. frame glue
@pytest.mark.parametrize("h,w,pads", GC.frame_cases(), ids=["%dx%d_%s" % (h, w, "-".join(map(str, p))) for h, w, p in GC.frame_cases()])
def test_u8_to_frame_bit_for_bit(h, w, pads):
    from bin_amd import ops
    img = GC.u8_image(h, w)
    out = ops.u8_to_frame(torch.from_numpy(img).cuda(), pads)
    want = GC.u8_to_frame_ref(img, pads)
    assert tuple(out.shape) == want.shape
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_frame_to_u8_every_rounding_tie_bit_for_bit():
    """All 255 half-way values (k + 0.5) / 255 with their float32 neighbours, 0, 1, -0.0, negatives, values above 1, +-inf: the
    full frame and crops at its four corners against the oracle's tensor2img (round half to even)."""
    from bin_amd import ops
    from oracle import rdn_oracle as O
    f = GC.rounding_frame()
    F_ = torch.from_numpy(f).cuda()
    full = O.tensor2img(torch.from_numpy(f))                  # elementwise + a permutation: a crop of it is the crop's image
    for top, left, h, w in GC.ROUNDING_CROPS:
        out = ops.frame_to_u8(F_, top, left, h, w)
        assert np.array_equal(out.cpu().numpy(), full[top:top + h, left:left + w]), (top, left, h, w)
