"""-m gpu: every plane-addressed kernel at the TOP of its N H W < 2^26 domain (tests/domain_top_cases.py), every pixel held to float64:
periodic exact operands gathered on the device, float64 band references, an on-device compare of every other row against the verified
period; the weight-gradient kernels on a census and on exact bands; the layout glue as round trips against the period.  Equality is
required everywhere.  Every allocation a test makes sits between guard bands (tests/poison.py), which are checked after the call,
as is the status word.  One line per library call:
    [domain-top] case= nterms= family= shape= live=<GiB> call=<ms> test=<s so far> ref=<device of the float64 reference>
tests/test_cpu_domain_top.py shows that the same comparison reports a kernel that wraps a row offset, reads another image, drops the
last row, fetches a row as zeros or stores a row late."""
import ctypes as C
import gc
import math
import time

import pytest
import torch

import conv_ref_cases as rc
import domain_top_cases as dt
import glue_cases as glue
import poison

pytestmark = pytest.mark.gpu
CASE_SHAPES = [(c.tag, s) for c in dt.CASES for s in dt.shapes(c)]
POISON = 0x47


def _dev():
    return torch.device("cuda")


_ref_dev = []


def _reference_device():
    """Where the float64 band references run: the GPU if torch convolves float64 there and gives the CPU's integers, else the CPU
    (correct all the same, but far slower: the choice and its reason are printed once)."""
    if not _ref_dev:
        g = torch.Generator().manual_seed(1)
        x = torch.randint(-3, 4, (1, 5, 9, 11), generator=g).double()
        w = torch.randint(-2, 3, (4, 5, 3, 3), generator=g).double()
        want = torch.nn.functional.conv2d(x, w, padding=1)
        try:
            ok = torch.equal(torch.nn.functional.conv2d(x.cuda(), w.cuda(), padding=1).cpu(), want)
            why = "torch's float64 convolution on the GPU gives the CPU's integers" if ok else \
                "torch's float64 convolution on the GPU differs from the CPU's on an integer probe"
        except RuntimeError as e:
            ok, why = False, f"torch's float64 convolution on the GPU raised: {e}"
        _ref_dev.append(torch.device("cuda") if ok else torch.device("cpu"))
        print(f"[domain-top] float64 references run on {_ref_dev[0].type}: {why}"
              + ("" if ok else " -- expect tests far above their usual seconds"))
    return _ref_dev[0]


def _release():
    from bin_amd import rdn_plan
    rdn_plan.release_workspaces()
    gc.collect()
    torch.cuda.empty_cache()


def _timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3


def _line(case, nterms, family, shape, live, ms, t0, extra=""):
    print(f"[domain-top] case={case} nterms={nterms} family={family} shape={rc.shape_str(shape)} live={live / 2 ** 30:.2f}GiB "
          f"call={ms:.1f}ms test={time.perf_counter() - t0:.2f}s {extra}")


def _families(nterms):
    return ("A", "B") if nterms == 3 else ("A",)


# ------------------------------------------------------------------------------------------------ forward, backward data, fused tail
@pytest.mark.parametrize("nterms,family", [(nt, f) for nt in dt.NTERMS for f in _families(nt)])
@pytest.mark.parametrize("tag,shape", CASE_SHAPES)
def test_conv_path_at_the_top_of_the_domain(tag, shape, nterms, family):
    from bin_amd import ops
    case = dt.BY_TAG[tag]
    t0 = time.perf_counter()
    live = dt.live_bytes(case, nterms, shape)
    assert live <= dt.MAX_LIVE_BYTES
    ops.check_status()
    opnd = dt.period_operands(tag, family, shape[2])
    _release()
    with poison.poisoned(POISON) as rec:
        dev_in = dt.expand_operands(case, nterms, shape, opnd, _dev())
        outs, ms = _timed(lambda: dt.call_library(case, nterms, shape, opnd, dev_in))
        ops.check_status()
        rec.check_guards()
        _line(tag, nterms, family, shape, live, ms, t0, f"ref={_reference_device().type} row={case.rows[nterms]!r}")
        dt.check_outputs(case, nterms, family, shape, opnd, outs, _dev(), ref_dev=_reference_device())
    del dev_in, outs, rec
    _release()
    _line(tag, nterms, "-", shape, live, 0.0, t0, "done")


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad(x, g, ks, nterms):
    from bin_amd import ops
    return ops.conv2d_bwd_weight(ops.CP(x.hi, x.lo, dt.WGRAD_CIN), ops.CP(g.hi, g.lo, dt.WGRAD_COUT), dt.WGRAD_COUT, dt.WGRAD_CIN, ks, nterms)


@pytest.mark.parametrize("nterms", dt.NTERMS)
@pytest.mark.parametrize("shape", (dt.WIDE, dt.TALL), ids=rc.shape_str)
@pytest.mark.parametrize("ks", dt.WGRAD_KS)
def test_wgrad_census_counts_every_pixel_once(ks, shape, nterms):
    """dW[0, 0, tap] = the integer count of in-image pixel pairs; every other entry 0.  db[0] = N H W lies above 2^24 and is not part
    of the exact claim: every partial sum is an integer and exact while below 2^24 (a workgroup's share of the pixels is), so only the
    additions of the final reduction over at most 2^10 workgroup partials round, each by at most 2^-24 of the sum: 2^-14 in all."""
    from bin_amd import ops
    t0 = time.perf_counter()
    live, ws = dt.wgrad_live_bytes(shape, ks, nterms)
    assert live <= dt.MAX_LIVE_BYTES
    ops.check_status()
    _release()
    with poison.poisoned(POISON) as rec:
        x, g = dt.census_planes(shape, nterms, _dev())
        (dw, db), ms = _timed(lambda: _wgrad(x, g, ks, nterms))
        ops.check_status()
        rec.check_guards()
        dw, db = dw.cpu().double(), db.cpu().double()
    want = torch.zeros_like(dw)
    want[0, 0] = torch.from_numpy(dt.census_counts(shape, ks)).double()
    nhw = shape[0] * shape[1] * shape[2]
    _line(f"wgrad{ks}_census", nterms, "-", shape, live, ms, t0, f"workspace={ws} db0-NHW={float(db[0]) - nhw:+.0f}")
    assert torch.equal(dw[0, 0], want[0, 0]), (ks, shape, nterms, (dw[0, 0] - want[0, 0]).tolist())
    assert torch.equal(dw, want), "an entry that should be 0 is not"
    assert not bool(db[1:].any()) and abs(float(db[0]) - nhw) <= nhw * 2.0 ** -14
    del x, g, rec
    _release()


@pytest.mark.parametrize("nterms", dt.NTERMS)
@pytest.mark.parametrize("shape", (dt.WIDE, dt.TALL), ids=rc.shape_str)
@pytest.mark.parametrize("ks", dt.WGRAD_KS)
def test_wgrad_bands_at_the_offsets_that_change_a_bit(ks, shape, nterms):
    from bin_amd import ops
    t0 = time.perf_counter()
    live, ws = dt.wgrad_live_bytes(shape, ks, nterms)
    ops.check_status()
    for family in _families(nterms):
        runs, data, dwr, dbr, bound = dt.band_reference(shape, ks, family, nterms, dev=_dev())
        assert bound * (1.0 if family == "A" else 2.0 ** 11) < rc.EXACT_LIMIT, (ks, shape, family, bound)
        assert float(dwr.abs().max()) > 0 and float(dbr.abs().max()) > 0
        _release()
        with poison.poisoned(POISON) as rec:
            x, g = dt.band_planes(shape, nterms, runs, data, _dev())
            (dw, db), ms = _timed(lambda: _wgrad(x, g, ks, nterms))
            ops.check_status()
            rec.check_guards()
            dw, db = dw.cpu().double(), db.cpu().double()
        _line(f"wgrad{ks}_bands", nterms, family, shape, live, ms, t0, f"runs={runs}")
        assert torch.equal(dw, dwr), (ks, shape, nterms, family, float((dw - dwr).abs().max()))
        assert torch.equal(db, dbr), (ks, shape, nterms, family, float((db - dbr).abs().max()))
        del x, g, rec
    _release()


# ------------------------------------------------------------------------------------------------ layout glue
def _survivors(c, rows, width, seed):
    """fp32 [c, rows, width] of 21-bit integers times 2^-14: values whose hi / lo split decodes to themselves, with live lo planes."""
    gen = torch.Generator().manual_seed(seed + 31 * width)
    return torch.randint(-(1 << 20), 1 << 20, (c, rows, width), generator=gen).float() * 2.0 ** -14


def _plane_view(t):
    c, n, h, w, _ = t.shape
    return t.reshape(c, n, h, w * 16)


@pytest.mark.parametrize("shape", (dt.WIDE, dt.TALL), ids=rc.shape_str)
def test_nchw_planes_round_trip_at_the_top(shape):
    """binhip_nchw_to_planes, _scaled and binhip_planes_to_nchw: the planes against the period's split, the way back against the input,
    bit for bit."""
    from bin_amd import _lib as L, ops
    n, h, w = shape
    t0 = time.perf_counter()
    per = _survivors(dt.LAYOUT_C, dt.P, w, 5)
    ops.check_status()
    _release()
    phase = lambda i: dt.PHASES[i]
    live = n * h * w * (16 * 4 * 2 + 32 * 2)
    with poison.poisoned(POISON) as rec:
        x = dt.expand_rows(per.to(_dev()), n, h, dt.P, phase).permute(1, 0, 2, 3).contiguous()          # [N, 16, H, W]
        cp, ms = _timed(lambda: ops.nchw_to_planes(x, 3))
        ops.check_status()
        rec.check_guards()
        bad = []
        for scale, got in ((1.0, cp), (0.25, None)):
            if got is None:                                  # the scaled entry point into the same planes
                sc = torch.tensor([scale, 1 / scale], dtype=torch.float32, device=_dev())
                L.check(L.lib().binhip_nchw_to_planes_scaled(ops._ptr(x), n, dt.LAYOUT_C, h, w, ops._ptr(sc), ops._ptr(cp.hi), ops._ptr(cp.lo),
                                                             ops._ptr(ops.status_word(x.device)), ops._stream()), "nchw_to_planes_scaled")
                got = cp
            hi, lo = dt.split_planes((per * scale)[None].to(_dev()), 3)
            for nm, view, exp in (("hi", got.hi, hi), ("lo", got.lo, lo)):
                dt.compare_periodic(f"planes x{scale} {nm}", _plane_view(view), exp[:, 0].reshape(1, dt.P, w * 16), dt.P, phase, n, 0, h, bad)
            if scale == 1.0:
                back, ms2 = _timed(lambda: ops.planes_to_nchw(cp, dt.LAYOUT_C))
                assert poison.same_bits(back, x), "planes_to_nchw(nchw_to_planes(x)) is not x"
                del back
        ops.check_status()
        rec.check_guards()
        assert float(cp.lo.abs().max()) > 0
    _line("nchw_planes_round_trip", 3, "-", shape, live, ms, t0, f"planes_to_nchw={ms2:.1f}ms")
    assert not bad, bad
    del x, cp, rec
    _release()


@pytest.mark.parametrize("shape", (dt.EVEN_WIDE, dt.EVEN_TALL), ids=rc.shape_str)
def test_pack_unshuffle_unpack_at_the_top(shape):
    """binhip_pack_inputs (5 frames), binhip_unshuffle_planes and binhip_unpack_input_grads at the largest even frame: the packed
    half-resolution planes against the packed period; unshuffle_planes of a full-resolution plane against the same permutation of the
    period; unpack(pack(frames)) with a zero gout gives the frames back, bit for bit."""
    from bin_amd import _lib as L, ops
    n, h, w = shape
    t0 = time.perf_counter()
    k = 5
    pers = [_survivors(3, 2 * dt.P, w, 11 + i) for i in range(k)]                      # full-resolution period: 2 P rows
    ops.check_status()
    _release()
    phase2 = lambda i: dt.PHASES[i]                       # full-resolution rows: period 2 P, the even phase 2 q
    half = lambda i: dt.PHASES[i] // 2                    # half-resolution rows: period P, phase q
    bad = []
    with poison.poisoned(POISON) as rec:
        frames = [dt.expand_rows(p.to(_dev()), n, h, 2 * dt.P, phase2).permute(1, 0, 2, 3).contiguous() for p in pers]
        packed, ms = _timed(lambda: ops.pack_inputs(frames, 3))
        ops.check_status()
        rec.check_guards()
        want = torch.from_numpy(glue.pack_inputs_ref([p[None].numpy() for p in pers]))          # [4, 1, P, W/2, 16] fp32
        hi = want.half()
        lo = (want - hi.float()).half()
        for nm, view, exp in (("hi", packed.hi, hi), ("lo", packed.lo, lo)):
            dt.compare_periodic(f"pack_inputs {nm}", _plane_view(view), exp[:, 0].reshape(4, dt.P, (w // 2) * 16).to(_dev()), dt.P, half, n,
                                0, h // 2, bad)
        # the way back: outs[i] = unshuffle(packed)[frame i] * scale[1] + gout / k with gout = 0, scale = 1
        gout = torch.zeros_like(frames[0])
        sc = torch.ones(2, dtype=torch.float32, device=_dev())
        outs = [torch.empty_like(f) for f in frames]
        arr = (C.c_void_p * k)(*[o.data_ptr() for o in outs])
        _, ms2 = _timed(lambda: L.check(L.lib().binhip_unpack_input_grads(ops._ptr(packed.hi), ops._ptr(packed.lo), ops._ptr(gout), ops._ptr(sc),
                                                                         k, n, h, w, arr, ops._stream()), "unpack_input_grads"))
        rec.check_guards()
        for i in range(k):
            assert torch.equal(outs[i], frames[i]), f"unpack_input_grads(pack_inputs(frames))[{i}] is not the frame"
        del outs, gout, frames
        # unshuffle_planes: one full-resolution plane pair [1, N, H, W, 16] -> four at half resolution
        src = _survivors(16, 2 * dt.P, w, 29)
        shi, slo = dt.split_planes(src[None].to(_dev()), 3)                             # [1, 1, 2P, W, 16]
        xhi = dt.expand_rows(shi[:, 0], n, h, 2 * dt.P, phase2)
        xlo = dt.expand_rows(slo[:, 0], n, h, 2 * dt.P, phase2)
        yhi = torch.empty((4, n, h // 2, w // 2, 16), dtype=torch.float16, device=_dev())
        ylo = torch.empty_like(yhi)
        _, ms3 = _timed(lambda: L.check(L.lib().binhip_unshuffle_planes(ops._ptr(xhi), ops._ptr(xlo), n, h // 2, w // 2, 1, ops._ptr(yhi),
                                                                       ops._ptr(ylo), ops._stream()), "unshuffle_planes"))
        rec.check_guards()
        for nm, got, s in (("hi", yhi, shi), ("lo", ylo, slo)):
            exp = torch.from_numpy(glue.unshuffle_planes_ref(s.float().cpu().numpy())).half()   # [4, 1, P, W/2, 16]
            dt.compare_periodic(f"unshuffle_planes {nm}", _plane_view(got), exp[:, 0].reshape(4, dt.P, (w // 2) * 16).to(_dev()), dt.P, half, n,
                                0, h // 2, bad)
        ops.check_status()
    live = n * h * w * (2 * k * 3 * 4 + 4) + 4 * n * (h // 2) * (w // 2) * 64
    _line("pack_unshuffle_unpack", 3, "-", shape, live, ms, t0, f"unpack={ms2:.1f}ms unshuffle_planes={ms3:.1f}ms")
    assert not bad, bad
    del rec
    _release()


# ------------------------------------------------------------------------------------------------ ConvLSTM
def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


@pytest.mark.parametrize("shape", dt.LSTM_SHAPES, ids=rc.shape_str)
def test_convlstm_cell_at_its_top(shape):
    """binhip_convlstm_fwd and binhip_convlstm_bwd at N H W just under 2^24, with state: every pixel of c', h', gx, g_cprev, g_hprev and
    dw, db under the bars of lstm_cases.py (outputs start as NaN)."""
    from bin_amd import _lib as L, ops
    n, h, w = shape
    assert (1 << 24) - (1 << 13) <= n * h * w < (1 << 24)
    t0 = time.perf_counter()
    per = dt.lstm_period(w)
    lib = L.lib()
    nbytes = lib.binhip_convlstm_bwd_workspace_bytes(n, h, w)
    live = 10 * n * 3 * h * w * 4 + nbytes
    assert 0 < nbytes and live <= dt.MAX_LIVE_BYTES
    _release()
    with poison.poisoned(POISON) as rec:
        inp = dt.lstm_expand(per, shape, _dev())
        wt, b = per["w"].cuda(), per["b"].cuda()
        out = {nm: torch.empty_like(inp["x"]) for nm in dt.LSTM_PIXEL_OUTPUTS}
        out["dw"], out["db"] = torch.empty_like(wt), torch.empty_like(b)
        for t in out.values():
            t.fill_(float("nan"))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=_dev())
        _, ms = _timed(lambda: L.check(lib.binhip_convlstm_fwd(_p(inp["x"]), _p(inp["c0"]), _p(inp["h0"]), _p(wt), _p(b), dt.LSTM_FB, n, h, w,
                                                               _p(out["c"]), _p(out["h"]), ops._stream()), "convlstm_fwd"))
        _, ms2 = _timed(lambda: L.check(lib.binhip_convlstm_bwd(_p(inp["x"]), _p(inp["c0"]), _p(inp["h0"]), _p(wt), _p(b), dt.LSTM_FB, n, h, w,
                                                                _p(inp["gh"]), _p(inp["gc"]), _p(ws), nbytes, _p(out["gx"]), _p(out["ghp"]),
                                                                _p(out["gcp"]), _p(out["dw"]), _p(out["db"]), ops._stream()), "convlstm_bwd"))
        rec.check_guards()
        _line("convlstm", "-", "-", shape, live, ms, t0, f"bwd={ms2:.1f}ms workspace={nbytes / 2 ** 30:.2f}GiB ref={_reference_device().type}")
        dt.lstm_check(shape, per, out, _dev(), _reference_device())
    del inp, out, ws, rec
    _release()
    _line("convlstm", "-", "-", shape, live, 0.0, t0, "done")


@pytest.mark.parametrize("shape", dt.LSTM_SHAPES, ids=rc.shape_str)
def test_lstm_gate_kernels_at_their_top(shape):
    """binhip_lstm_gates_fwd / _bwd (hidden 3) on periodic gates at N H W just under 2^24: elementwise, so every row is held to the
    float64 period (lstm_cases.gates_reference) under GATES_BARS; the same bar on the periodicity compare."""
    import lstm_cases as lc
    from bin_amd import _lib as L, ops
    n, h, w = shape
    t0 = time.perf_counter()
    hid = 3
    g = torch.Generator().manual_seed(13 + 31 * w)
    gates = (torch.rand(1, 4 * hid, dt.P, w, generator=g) - 0.5) * 4.0
    cp, gh, gc = ((torch.rand(1, hid, dt.P, w, generator=g) - 0.5) * s for s in (2.0, 1.0, 1.0))
    r64, r32 = (lc.gates_reference(gates, cp, dt.LSTM_FB, gh, gc, d) for d in (torch.float64, torch.float32))
    phase = lambda i: dt.PHASES[i]
    lib = L.lib()
    live = n * h * w * 4 * (2 * 12 + 6 * 3)
    _release()
    with poison.poisoned(POISON) as rec:
        big = {k: dt.expand_rows(t[0].to(_dev()), n, h, dt.P, phase).permute(1, 0, 2, 3).contiguous()
               for k, t in (("gates", gates), ("cp", cp), ("gh", gh), ("gc", gc))}
        out = {"c": torch.empty_like(big["cp"]), "h": torch.empty_like(big["cp"]), "dgates": torch.empty_like(big["gates"]),
               "gcp": torch.empty_like(big["cp"])}
        for t in out.values():
            t.fill_(float("nan"))
        _, ms = _timed(lambda: L.check(lib.binhip_lstm_gates_fwd(_p(big["gates"]), _p(big["cp"]), dt.LSTM_FB, n, hid, h, w, _p(out["c"]),
                                                                 _p(out["h"]), ops._stream()), "gates_fwd"))
        _, ms2 = _timed(lambda: L.check(lib.binhip_lstm_gates_bwd(_p(big["gates"]), _p(big["cp"]), _p(big["gh"]), _p(big["gc"]), dt.LSTM_FB, n, hid,
                                                                  h, w, _p(out["dgates"]), _p(out["gcp"]), ops._stream()), "gates_bwd"))
        rec.check_guards()
        bad = []
        for nm in ("c", "h", "dgates", "gcp"):
            scale = 1.0 if nm in ("c", "h") else max(float(r64[nm].abs().max()), 1e-12)
            e32 = lc.err(nm, r32[nm], r64[nm])
            bb = lc.bar(nm, e32, lc.GATES_BARS)
            e = dt.max_diff_periodic(out[nm].permute(1, 0, 2, 3), r64[nm][0].float().to(_dev()), dt.P, phase, n, 0, h) / scale
            print(f"[domain-top] gates shape={rc.shape_str(shape)} {nm}: e32={e32:.3e} bar={bb:.3e} kernel={e:.3e} ratio={e / bb:.3f}")
            if not e <= bb:
                bad.append((nm, e, bb))
    _line("lstm_gates", "-", "-", shape, live, ms, t0, f"bwd={ms2:.1f}ms")
    assert not bad, bad
    del big, out, rec
    _release()


# ------------------------------------------------------------------------------------------------ one plan call
@pytest.mark.parametrize("prec", ("f16", "f16x3"))
def test_plan_forward_at_the_top(prec):
    """binhip_rdn_forward (inference: the fused UPNet's main launch and its ring kernel included) at 2 x 4096 x 8190, configuration
    (32, 1, 1, 32), 5 frames, against the float64 oracle under the bar of tests/test_gpu_rdn_configs.py for that precision."""
    from bin_amd import _lib as L, ops
    from bin_amd.models.archs import RDN as A
    from bin_amd.weights import general_rdn_weights
    from rdn_config_cases import FWD_BARS
    shape = dt.PLAN_SHAPE
    n, h, w = shape
    t0 = time.perf_counter()
    G0, D, Cc, G = dt.PLAN_CFG
    weights = general_rdn_weights(0, dt.PLAN_K, dt.PLAN_CFG)
    mod = A.RDN_residual_interp_4_1_input(G0=G0, D=D, C=Cc, G=G)
    mod.load_state_dict({nm: torch.from_numpy(v) for nm, v in weights.items()}, strict=True)
    mod = mod.cuda()
    mod.precision = prec
    s = L.BinRdnShape()
    s.G0, s.D, s.C, s.G = dt.PLAN_CFG
    ws = L.lib().binhip_rdn_workspace_bytes(n, h, w, dt.PLAN_K, 3 if prec == "f16x3" else 1, s)
    live = ws + (dt.PLAN_K + 1) * n * 3 * h * w * 4
    assert 0 < ws and live <= dt.MAX_LIVE_BYTES
    pers = dt.plan_periods(w)
    ops.check_status()
    _release()
    with poison.poisoned(POISON) as rec:
        frames = dt.plan_frames(pers, shape, _dev())
        with torch.no_grad():
            y, ms = _timed(lambda: mod(*frames))
        ops.check_status()
        rec.check_guards()
        _line("plan_forward", prec, "-", shape, live, ms, t0, f"workspace={ws / 2 ** 30:.2f}GiB ref={_reference_device().type}")
        dt.plan_check(shape, pers, weights, y, _dev(), _reference_device(), FWD_BARS[prec], label=prec)
    del frames, y, rec, mod
    _release()
    _line("plan_forward", prec, "-", shape, live, 0.0, t0, "done")


# ------------------------------------------------------------------------------------------------ upnet_gsub, through one plan backward
@pytest.mark.parametrize("shape", (dt.EVEN_WIDE, dt.EVEN_TALL), ids=rc.shape_str)
def test_upnet_gsub_plane_of_a_backward_at_the_top(shape):
    """upnet_gsub_kernel is reachable only through binhip_rdn_backward: one f16 training forward and backward of the smallest
    configuration (32, 1, 1, 32), 5 frames, at the largest even frame, with a periodic gout; the sub-pixel gradient plane the backward
    leaves in its workspace (hi; the f16 backward writes no lo plane, and an f16x3 backward does not fit the 96 GiB) must be the
    pixel-unshuffled, scaled, ring-zeroed gout bit for bit.  Nothing else of the backward is judged here beyond finite gradients and a
    clean status word: its kernels are covered per op above."""
    from bin_amd import _lib as L, ops
    from bin_amd.models.archs import RDN as A
    from bin_amd.range_stats import _layout, _view
    from bin_amd.weights import general_rdn_weights
    n, h, w = shape
    t0 = time.perf_counter()
    G0, D, Cc, G = dt.PLAN_CFG
    weights = general_rdn_weights(0, dt.PLAN_K, dt.PLAN_CFG)
    mod = A.RDN_residual_interp_4_1_input(G0=G0, D=D, C=Cc, G=G)
    mod.load_state_dict({nm: torch.from_numpy(v) for nm, v in weights.items()}, strict=True)
    mod = mod.cuda()
    mod.precision = "f16"
    mod.allow_f16_training = True            # the module's own switch: nothing is trained here, the plane under test is pure layout
    s = L.BinRdnShape()
    s.G0, s.D, s.C, s.G = dt.PLAN_CFG
    ws_f = L.lib().binhip_rdn_workspace_bytes(n, h, w, dt.PLAN_K, 1, s)
    ws_b = L.lib().binhip_rdn_backward_workspace_bytes(n, h, w, dt.PLAN_K, 1, s)
    live = ws_f + ws_b + (dt.PLAN_K + 2) * n * 3 * h * w * 4
    assert 0 < ws_f and 0 < ws_b and live <= dt.MAX_LIVE_BYTES, (ws_f, ws_b, live)
    pers, per_g = dt.plan_periods(w), dt.gsub_period(w)
    got = {}

    def hook(kind, module, dims, ws, info):
        if kind != "backward":
            return
        assert info["fused_upnet"], "the fused UPNet's backward was not taken"
        v = _layout(L.lib().binhip_rdn_backward_workspace_layout, dims, L.RDN_BWD_LAYOUT_WORDS, module.shape)
        base = (-ws.data_ptr()) % 256
        got["scale"] = float(ws[base + v[23]: base + v[23] + 8].view(torch.float32)[0])
        got["nt"] = dims[4]
        got["hi"] = _view(ws, v[3], v[0]).view(1, n, h // 2, w // 2, 16).clone()
    mod.debug_hook = hook
    ops.check_status()
    _release()
    with poison.poisoned(POISON) as rec:
        frames = dt.plan_frames(pers, shape, _dev())
        gout = dt.expand_rows(per_g.to(_dev()), n, h, 2 * dt.P, lambda i: dt.PHASES[i]).permute(1, 0, 2, 3).contiguous()
        y, ms = _timed(lambda: mod(*frames))
        _, ms2 = _timed(lambda: y.backward(gout))
        ops.check_status()
        rec.check_guards()
        _line("upnet_gsub", "f16", "-", shape, live, ms, t0, f"backward={ms2:.1f}ms workspaces={ws_f / 2 ** 30:.2f}+{ws_b / 2 ** 30:.2f}GiB "
              f"scale={got.get('scale')}")
        assert got and got["nt"] == 1
        sc = got["scale"]
        assert sc > 0 and math.frexp(sc)[0] == 0.5, f"the gradient scale {sc} is not a power of two"
        dt.gsub_check(shape, per_g, sc, got["hi"], None)
        assert float(got["hi"].abs().max()) > 0
        assert all(bool(torch.isfinite(p.grad).all()) for p in mod.parameters())
    del frames, gout, y, rec, mod, got
    _release()
    _line("upnet_gsub", "f16", "-", shape, live, 0.0, t0, "done")
