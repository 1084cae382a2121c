"""Case table of the bit pin of the small kernels (binhip_convlstm.hip, binhip_loss.hip): the fused ConvLSTM cell and its three-pass
backward, the elementwise gate kernels of the general cell, the pixel criteria (single and multi-term) and the gradient-scale reduction,
each through its raw C entry point.  tests/golden/make_small_kernel_bits.py records the sha256 of every output buffer of every case into
tests/golden/small_kernel_bits.json; test_small_kernel_bits_are_the_recorded_ones (tests/test_gpu_small_kernels.py) computes them again.

None of these kernels has an atomic in its arithmetic and every reduction runs in a fixed order, so every digest is reproducible.  Inputs
are those of lstm_cases.make_inputs / make_gates, loss_cases.make_xy / make_multi / scale_input: all finite, so no digest hangs on a NaN
payload.  Output buffers (the loss kernels' `partials` among them) are zero-filled before the call, so words a kernel leaves alone cannot
change a digest.

Keys, the smallest shapes at which these kernels can go wrong:
  lstm/<N>x<H>x<W>/<state|nostate>/<aligned|off1>/<variant>[/overflow]   one pixel, one float4, one column, a ragged W, one
        weight-gradient tile, one tile +- 1, several tiles; `aligned` = 16-byte aligned planes (four pixels per thread when W % 4 == 0),
        `off1` = lstm_cases.off1 (one pixel per thread); the pointer variants of lstm_cases.VARIANTS at one ragged and one aligned shape
  gates/h<hidden>/<cp|nocp>/<gh|gc|both>
  ploss/<kind>/<numel>      forward, and the backward with gx only, gy only and both;  charb/257: the first ABI's names
  mloss/<kind>/T<T>/<numel> forward, and one backward launch per batch of outputs: tensors in two terms and targets (sign -1) among them
  gscale/<numel>
"""
import ctypes as C
import hashlib

import numpy as np
import torch

import loss_cases as LS
import lstm_cases as LC

LSTM_SHAPES = ((1, 1, 1), (1, 1, 4), (1, 4, 1), (3, 3, 5), (1, 7, 63), (1, 8, 64), (2, 9, 65), (2, 18, 70))
LSTM_VARIANT_SHAPES = ((2, 9, 65), (1, 16, 128))
LSTM_OVERFLOW_SHAPE = LC.OVERFLOW_SHAPES[0]
PLACEMENTS = ("aligned", "off1")
LOSS_NUMELS = (1, 2, 255, 256, 257, 65535, LS.FWD_CAP - 1, LS.FWD_CAP, LS.FWD_CAP + 1, LS.BWD_CAP + 1)
MULTI_NUMELS = (257, LS.FWD_CAP + 1)
SCALE_NUMELS = tuple(n for n in LS.SCALE_NUMELS if n <= LS.FWD_CAP + 1)
SCALE_AMAX, SCALE_TARGET = 1234.5, 16.0
CHARB_EPS, LOSS_EPS = 1e-3, 1e-6
GATES_DIRS = ("gh", "gc", "both")


def _keys():
    ks = []
    for n, h, w in LSTM_SHAPES:
        for st in ("nostate", "state"):
            ks += [f"lstm/{n}x{h}x{w}/{st}/{pl}/full" for pl in PLACEMENTS]
    for n, h, w in LSTM_VARIANT_SHAPES:
        for v in LC.VARIANTS[1:]:
            ks += [f"lstm/{n}x{h}x{w}/state/{pl}/{v}" for pl in PLACEMENTS]
    n, h, w = LSTM_OVERFLOW_SHAPE
    ks += [f"lstm/{n}x{h}x{w}/state/{pl}/full/overflow" for pl in PLACEMENTS]
    ks += [f"gates/h{hid}/{cp}/{d}" for hid in LC.GATES_HIDDEN for cp in ("nocp", "cp") for d in GATES_DIRS]
    ks += [f"ploss/{k}/{n}" for k in LS.KINDS for n in LOSS_NUMELS] + ["charb/257"]
    ks += [f"mloss/cb/T{T}/{n}" for T in LS.MULTI_T for n in MULTI_NUMELS]
    ks += [f"mloss/{k}/T17/{n}" for k in ("l1", "l2") for n in MULTI_NUMELS]
    ks += [f"gscale/{n}" for n in SCALE_NUMELS]
    return tuple(ks)


KEYS = _keys()
assert len(set(KEYS)) == len(KEYS)

NULL = C.c_void_p(0)


def _p(t):
    return NULL if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _sha(t):
    return hashlib.sha256(t.contiguous().cpu().numpy().view(np.uint8).tobytes()).hexdigest()


def lstm_case(key):
    """The lstm_cases.Case and the placement of an lstm/ key."""
    parts = key.split("/")
    n, h, w = (int(v) for v in parts[1].split("x"))
    state, variant = parts[2] == "state", parts[4]
    regime = "overflow" if parts[-1] == "overflow" else "moderate"
    fb = 0.0 if variant != "full" else 1.0                  # (the variants of lstm_cases.CASES run at forget_bias 0)
    return LC.Case(key, n, h, w, state, fb, regime, variant, 7), parts[3]


def lstm_buffers(key):
    """Names of the digests of an lstm/ key: lstm_cases.wanted under the names of include/binhip.h."""
    case, _ = lstm_case(key)
    return sorted({"gcp": "g_cprev", "ghp": "g_hprev"}.get(nm, nm) for nm in LC.wanted(case))


def _lstm_bits(lib, check, key):
    case, placement = lstm_case(key)
    conv = LC.off1 if placement == "off1" else (lambda t: t.clone())
    inp = LC.make_inputs(case)
    names = LC.wanted(case)
    D = lambda t: None if t is None else conv(t.cuda())
    x, c0, h0, gh, gc = (D(inp[k]) for k in ("x", "c0", "h0", "gh", "gc"))
    w, b = inp["w"].cuda(), inp["b"].cuda()
    if case.variant == "gh_only":
        gc = None
    if case.variant == "gc_only":
        gh = None
    out = {nm: conv(torch.zeros_like(inp["x"]).cuda()) for nm in ("c", "h", "gx", "gcp", "ghp") if nm in names}
    if "dw" in names:
        out["dw"], out["db"] = torch.zeros_like(w), torch.zeros_like(b)
    n, h, ww = case.n, case.h, case.w
    check(lib.binhip_convlstm_fwd(_p(x), _p(c0), _p(h0), _p(w), _p(b), case.fb, n, h, ww, _p(out.get("c")), _p(out["h"]), _stream()),
          "convlstm_fwd")
    nbytes = lib.binhip_convlstm_bwd_workspace_bytes(n, h, ww)
    ws = torch.zeros(nbytes + 512, dtype=torch.uint8, device="cuda")
    check(lib.binhip_convlstm_bwd(_p(x), _p(c0), _p(h0), _p(w), _p(b), case.fb, n, h, ww, _p(gh), _p(gc), _p(ws), nbytes,
                                  _p(out.get("gx")), _p(out.get("ghp")), _p(out.get("gcp")), _p(out.get("dw")), _p(out.get("db")),
                                  _stream()), "convlstm_bwd")
    torch.cuda.synchronize()
    return {{"gcp": "g_cprev", "ghp": "g_hprev"}.get(nm, nm): _sha(t) for nm, t in out.items()}


def _gates_bits(lib, check, key):
    _, hid, cpk, d = key.split("/")
    hidden = int(hid[1:])
    gates, cp, gh, gc = (t.cuda() for t in LC.make_gates(hidden, "moderate"))
    n, h, w = LC.GATES_SHAPE
    cpv = cp if cpk == "cp" else None
    a, b = (gh if d != "gc" else None), (gc if d != "gh" else None)
    out = {"c": torch.zeros_like(cp), "h": torch.zeros_like(cp), "dgates": torch.zeros_like(gates)}
    if cpv is not None:
        out["g_cprev"] = torch.zeros_like(cp)
    check(lib.binhip_lstm_gates_fwd(_p(gates), _p(cpv), 1.0, n, hidden, h, w, _p(out["c"]), _p(out["h"]), _stream()), "gates_fwd")
    check(lib.binhip_lstm_gates_bwd(_p(gates), _p(cpv), _p(a), _p(b), 1.0, n, hidden, h, w, _p(out["dgates"]), _p(out.get("g_cprev")),
                                    _stream()), "gates_bwd")
    torch.cuda.synchronize()
    return {k: _sha(v) for k, v in out.items()}


def _ploss_bits(lib, check, key):
    parts = key.split("/")
    charb = parts[0] == "charb"
    numel = int(parts[-1])
    kind = 0 if charb else LS.KIND_ID[parts[1]]
    eps = CHARB_EPS if charb else LOSS_EPS
    x, y = (t.cuda() for t in LS.make_xy(numel))
    part = torch.zeros(lib.binhip_charbonnier_partials(numel), dtype=torch.float32, device="cuda")
    gl = torch.tensor([LS.GLOSS], dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, device="cuda")
    if charb:
        check(lib.binhip_charbonnier_fwd(_p(x), _p(y), numel, eps, _p(part), _p(loss), _stream()), "charbonnier_fwd")
    else:
        check(lib.binhip_pixel_loss_fwd(kind, _p(x), _p(y), numel, eps, _p(part), _p(loss), _stream()), "pixel_loss_fwd")
    out = {"loss": loss, "partials": part}
    for label, want_x, want_y in (("only", True, False), ("only", False, True), ("both", True, True)):
        gx = torch.zeros_like(x) if want_x else None
        gy = torch.zeros_like(x) if want_y else None
        if charb:
            if label != "both":
                continue
            check(lib.binhip_charbonnier_bwd(_p(x), _p(y), numel, eps, _p(gl), _p(gx), _p(gy), _stream()), "charbonnier_bwd")
        else:
            check(lib.binhip_pixel_loss_bwd(kind, _p(x), _p(y), numel, eps, _p(gl), _p(gx), _p(gy), _stream()), "pixel_loss_bwd")
        if want_x:
            out["gx_" + label] = gx
        if want_y:
            out["gy_" + label] = gy
    torch.cuda.synchronize()
    return {k: _sha(v) for k, v in out.items()}


def multi_where(idx):
    """{tensor index: [(term, sign)]} of loss_cases.multi_pairs' index pairs: +1 where the tensor is a term's x, -1 where it is its y."""
    used = sorted({i for p in idx for i in p})
    return {i: [(t, 1.0) for t, (a, _) in enumerate(idx) if a == i] + [(t, -1.0) for t, (_, b) in enumerate(idx) if b == i] for i in used}


def _mloss_bits(L, lib, check, key):
    _, kind, T, numel = key.split("/")
    T, numel = int(T[1:]), int(numel)
    ts = LS.make_multi(numel)
    _, idx = LS.multi_pairs(T, ts)
    where = multi_where(idx)
    used = sorted(where)
    assert any(len(v) == 2 for v in where.values()) or T == 1
    dev = {i: ts[i].cuda() for i in used}
    t = L.BinLossTerms()
    t.n_terms = T
    for i, (a, b) in enumerate(idx):
        t.x[i], t.y[i] = dev[a].data_ptr(), dev[b].data_ptr()
    part = torch.zeros(T * lib.binhip_charbonnier_partials(numel), dtype=torch.float32, device="cuda")
    terms = torch.zeros(T, dtype=torch.float32, device="cuda")
    loss = torch.zeros(1, dtype=torch.float32, device="cuda")
    check(lib.binhip_multi_loss_fwd(LS.KIND_ID[kind], C.byref(t), numel, LOSS_EPS, _p(part), _p(terms), _p(loss), _stream()), "multi_loss_fwd")
    out = {"loss": loss, "terms": terms, "partials": part}
    gl = torch.tensor([LS.GLOSS], dtype=torch.float32, device="cuda")
    for k0 in range(0, len(used), L.LOSS_MAX_TERMS):
        batch = used[k0:k0 + L.LOSS_MAX_TERMS]
        g = L.BinLossGrads()
        g.n_out = len(batch)
        for k, i in enumerate(batch):
            o = out[f"g{i}"] = torch.zeros(numel, dtype=torch.float32, device="cuda")
            w = where[i]
            g.out[k] = o.data_ptr()
            g.term_a[k], g.sign_a[k] = w[0]
            g.term_b[k], g.sign_b[k] = w[1] if len(w) == 2 else (-1, 0.0)
        check(lib.binhip_multi_loss_bwd(LS.KIND_ID[kind], C.byref(t), numel, LOSS_EPS, _p(gl), C.byref(g), _stream()), "multi_loss_bwd")
    torch.cuda.synchronize()
    return {k: _sha(v) for k, v in out.items()}


def _gscale_bits(lib, check, key):
    numel = int(key.split("/")[1])
    v = LS.scale_input(numel, SCALE_AMAX, negative=True).cuda()
    part = torch.zeros(lib.binhip_charbonnier_partials(numel), dtype=torch.float32, device="cuda")
    sc = torch.zeros(2, device="cuda")
    check(lib.binhip_grad_scale(_p(v), numel, SCALE_TARGET, _p(part), _p(sc), _stream()), "grad_scale")
    torch.cuda.synchronize()
    return {"scale": _sha(sc), "partials": _sha(part)}


def bits(key):
    """{buffer name: sha256} of every output buffer of the case's calls into the library (needs a GPU)."""
    from bin_amd import _lib as L
    lib, family = L.lib(), key.split("/")[0]
    if family == "lstm":
        return _lstm_bits(lib, L.check, key)
    if family == "gates":
        return _gates_bits(lib, L.check, key)
    if family in ("ploss", "charb"):
        return _ploss_bits(lib, L.check, key)
    if family == "mloss":
        return _mloss_bits(L, lib, L.check, key)
    if family == "gscale":
        return _gscale_bits(lib, L.check, key)
    raise KeyError(key)
