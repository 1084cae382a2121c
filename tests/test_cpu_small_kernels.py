"""CPU side of tests/test_gpu_small_kernels.py: (a) every float64 restatement in lstm_cases / loss_cases / glue_cases is pinned to
oracle/rdn_oracle.py or to torch's own modules, (b) every e32 (float32 torch against float64) is computed and the cap
4 * e32 <= 8 * B and the max|ref| >= 1e-3 condition are asserted, (c) the case tables cross the tile counts and grid caps they are
there for, (d) float32 torch runs through the very comparison code that judges the kernels — and passes."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as GC
import loss_cases as LS
import lstm_cases as LC
from oracle import rdn_oracle as O


# ------------------------------------------------------------------------------------------------------------------ ConvLSTM
def test_lstm_case_table_crosses_the_tile_counts_it_is_there_for():
    for shape, n_tiles in LC.EXPECTED_TILES.items():
        assert LC.tiles(*shape) == n_tiles, shape
    counts = sorted({LC.tiles(c.n, c.h, c.w) for c in LC.CASES})
    assert sum(t > LC.FINAL_STRIDE for t in counts) >= 2 and any(t > 1024 for t in counts)
    assert any(LC.FINAL_STRIDE < t < 2 * LC.FINAL_STRIDE for t in counts)           # one just past the first stride
    assert 1 in counts and 264 in counts and 1024 in counts and 1800 in counts
    shapes = {(c.n, c.h, c.w) for c in LC.CASES}
    assert set(LC.SMALL_SHAPES + LC.TILE_SHAPES + LC.LARGE_SHAPES) <= shapes
    assert any(c.n > 2 for c in LC.CASES) and any(c.w < 64 and c.h < 8 for c in LC.CASES)
    assert {c.fb for c in LC.CASES if c.state} == {1.0, 0.0, -2.5}
    assert all(c.state for c in LC.CASES if c.fb != 1.0)                           # forget_bias only matters with a state
    assert {c.variant for c in LC.CASES} == set(LC.VARIANTS)
    for v in LC.VARIANTS[1:]:                                                      # each at a ragged and at a four-pixel shape
        assert {c.w % 4 == 0 for c in LC.CASES if c.variant == v} == {True, False}
    for shape in LC.LARGE_SHAPES:                                                  # the large sizes: moderate, forget_bias 1.0 only
        assert {(c.state, c.fb, c.regime) for c in LC.CASES if (c.n, c.h, c.w) == shape} == {(False, 1.0, "moderate"), (True, 1.0, "moderate")}


def _gates_of(case, inp):
    xin = torch.cat((inp["x"], inp["h0"] if case.state else torch.zeros_like(inp["x"])), 1).double()
    return F.conv2d(xin, inp["w"].double(), inp["b"].double(), padding=1)


def test_lstm_regimes_are_what_the_table_says():
    sat = LC.CASE_BY_TAG["2x9x65_state_saturated"]
    g = _gates_of(sat, LC.make_inputs(sat))
    assert float(g.abs().max()) >= 20 and 0.10 <= float((g.abs() > 8).double().mean()) <= 0.35
    for tag in ("3x40x132_state_saturated", "3x40x132_state_saturated_fb-2.5", "3x40x132_nostate_saturated"):   # the first two re-drawn
        g = _gates_of(LC.CASE_BY_TAG[tag], LC.make_inputs(LC.CASE_BY_TAG[tag]))
        assert float(g.abs().max()) >= 20 and float((g.abs() > 8).double().mean()) >= 0.10, tag
    mod = LC.CASE_BY_TAG["2x9x65_state_moderate"]
    assert float(_gates_of(mod, LC.make_inputs(mod)).abs().max()) <= 2.5
    for shape in LC.OVERFLOW_SHAPES:
        ov = LC.CASE_BY_TAG["%dx%dx%d_state_overflow" % shape]
        inp = LC.make_inputs(ov)
        g = _gates_of(ov, inp)
        for k, v in LC.OVERFLOW_BIAS.items():                                      # whole gate planes at +-30, +-90, +-200 ...
            assert float((g[:, k] - v).abs().max()) <= 3.0 and abs(v) in (30.0, 90.0, 200.0)
        assert {abs(v) for v in LC.OVERFLOW_BIAS.values()} == {30.0, 90.0, 200.0}
        assert float(g[:, [0, 3, 6, 9]].abs().max()) <= 2.5                        # ... while hidden channel 0 stays moderate
        assert float(inp["c0"].abs().max()) > 3.5
        assert math.isinf(float(torch.exp(torch.tensor(200.0))))                   # 200 is past float32 exp's overflow


def test_gate_formula_is_the_oracle_cell():
    case = LC.CASE_BY_TAG["3x3x5_state_moderate_fb-2.5"]
    inp = LC.make_inputs(case)
    ref = LC.reference(case, inp, torch.float64)
    gates = _gates_of(case, inp)
    mine = LC.gates_reference(gates, inp["c0"], case.fb, inp["gh"], inp["gc"], torch.float64)
    assert torch.equal(mine["c"], ref["c"]) and torch.equal(mine["h"], ref["h"]) and torch.equal(mine["gcp"], ref["gcp"])
    db = mine["dgates"].sum((0, 2, 3))
    assert float((db - ref["db"]).abs().max()) <= 1e-12 * float(ref["db"].abs().max())
    nostate = LC.CASE_BY_TAG["3x3x5_nostate_moderate"]
    inp = LC.make_inputs(nostate)
    ref = LC.reference(nostate, inp, torch.float64)
    mine = LC.gates_reference(_gates_of(nostate, inp), None, 1.0, inp["gh"], inp["gc"], torch.float64)
    assert torch.equal(mine["c"], ref["c"]) and torch.equal(mine["h"], ref["h"])


@pytest.mark.parametrize("tag", [c.tag for c in LC.CASES])
def test_lstm_float32_torch_meets_the_bars_and_the_yardstick_cap(tag):
    case = LC.CASE_BY_TAG[tag]
    inp = LC.make_inputs(case)
    r64, r32 = LC.reference(case, inp, torch.float64), LC.reference(case, inp, torch.float32)
    for nm, t in r64.items():
        assert bool(torch.isfinite(t).all()) and bool(torch.isfinite(r32[nm]).all()), nm
        if nm not in ("c", "h"):
            assert float(t.abs().max()) >= LC.MIN_REF_MAX, (nm, float(t.abs().max()))
    names = [n for n in r64]
    res = LC.compare(tag, names, r32, r64, r32, label="float32")                   # asserts the cap for every output
    assert all(e <= b for _, b, e in res.values())


@pytest.mark.parametrize("regime", LC.GATES_REGIMES)
@pytest.mark.parametrize("hidden", LC.GATES_HIDDEN)
def test_gates_float32_torch_meets_the_bars_and_the_yardstick_cap(hidden, regime):
    gates, cp, gh, gc = LC.make_gates(hidden, regime)
    if regime == "overflow":
        assert {30.0, 90.0, 200.0} <= set(gates.abs().unique().tolist())
    for fb in LC.GATES_FB:
        for cpv in (None, cp):
            for a, b in ((gh, gc), (gh, None), (None, gc)):
                r64 = LC.gates_reference(gates, cpv, fb, a, b, torch.float64)
                r32 = LC.gates_reference(gates, cpv, fb, a, b, torch.float32)
                for nm in ("dgates", "gcp"):
                    if nm in r64:
                        assert float(r64[nm].abs().max()) >= LC.MIN_REF_MAX
                LC.compare(f"gates h{hidden} {regime} fb{fb:g}", list(r64), r32, r64, r32, bars=LC.GATES_BARS, label="float32")


def test_a_wrong_forget_bias_or_tap_is_far_outside_the_bars():
    """The comparison code bites: float32 torch with forget_bias ignored, or with one recurrent tap flipped, fails it."""
    case = LC.CASE_BY_TAG["2x9x65_state_moderate_fb-2.5"]
    inp = LC.make_inputs(case)
    r64, r32 = LC.reference(case, inp, torch.float64), LC.reference(case, inp, torch.float32)
    wrong = LC.reference(case._replace(fb=1.0), inp, torch.float32)
    with pytest.raises(AssertionError):
        LC.compare(case.tag, list(r64), wrong, r64, r32, label="wrong-fb")
    inp2 = dict(inp, w=inp["w"].clone())
    inp2["w"][:, 3:, :, 0], inp2["w"][:, 3:, :, 2] = inp["w"][:, 3:, :, 2], inp["w"][:, 3:, :, 0]
    wrong = LC.reference(case, inp2, torch.float32)
    with pytest.raises(AssertionError):
        LC.compare(case.tag, ["ghp"], wrong, r64, r32, label="wrong-tap")


# ------------------------------------------------------------------------------------------------------------------ losses
def test_loss_tables_sit_on_both_sides_of_the_grid_caps():
    for cap in (LS.FWD_CAP, LS.BWD_CAP):
        assert {cap - 1, cap, cap + 1} <= set(LS.NUMELS) and {cap - 1, cap, cap + 1} <= set(LS.CAP_NUMELS) <= set(LS.SCALE_NUMELS)
    assert (LS.FWD_CAP, LS.BWD_CAP) == (262144, 1048576)
    assert {1, 2, 255, 256, 257, 65535} <= set(LS.NUMELS) and max(LS.NUMELS) == 2 ** 24 + 3
    assert float(np.float32(2 ** 24 + 3)) != 2 ** 24 + 3                           # past the exact integers of float32
    assert set(LS.MULTI_T) == {1, 2, 17, 24}
    assert {(k, T, e) for k, T, n, e in LS.MULTI_CASES if e != 1e-6} == {("cb", 17, 1e-3), ("cb", 17, 1e-12)}
    assert {n > LS.FWD_CAP for k, T, n, e in LS.MULTI_CASES if e != 1e-6} == {True, False}
    few = LS.make_multi(257)
    by_eps = [float(LS.multi_reference("cb", 17, few, e, 1.0, torch.float64)["loss"]) for e in LS.EPS_VALUES]
    assert by_eps[1] > by_eps[0] * (1 + 1e-3) and by_eps[2] < by_eps[0] * (1 - 1e-6)         # far outside the 1e-6 bar: eps is seen
    for T in LS.MULTI_T:
        _, idx = LS.multi_pairs(T, list(range(34)))
        flat = [i for p in idx for i in p]
        assert max(flat.count(i) for i in set(flat)) <= 2
    _, idx = LS.multi_pairs(17, list(range(34)))
    xs, ys = {a for a, _ in idx}, {b for _, b in idx}
    assert {7, 8, 9} <= xs & ys                                                     # x of one term and y of another


def test_criteria_are_the_oracle_and_torch_modules():
    x, y = (t.double() for t in LS.make_xy(3001))
    assert float((x == y).sum()) >= 3001 // 8
    for eps in LS.EPS_VALUES:
        assert torch.equal(LS.criterion("cb", x, y, eps), O.charbonnier(x, y, eps))
    assert torch.equal(LS.criterion("l1", x, y, 0), torch.nn.L1Loss(reduction="sum")(x, y))
    assert torch.equal(LS.criterion("l2", x, y, 0), torch.nn.MSELoss(reduction="sum")(x, y))
    r = LS.reference("l1", x, y, 1e-6, LS.GLOSS, torch.float64)
    tie = x == y
    assert bool((r["gx"][tie] == 0).all()) and bool((r["gx"][~tie].abs() == LS.GLOSS).all()) and torch.equal(r["gx"], -r["gy"])
    r = LS.reference("cb", x, y, 1e-12, LS.GLOSS, torch.float64)
    assert bool((r["gx"][tie] == 0).all())
    # the 17-term pairing is bin_model.get_loss's (oracle bin_loss): outputs o0..o13 against gt order 2 4 6 8 3 5 7 4 6 5 10 9 8 7
    g = torch.Generator().manual_seed(1)
    outs = [torch.rand(500, generator=g).double() for _ in range(14)]
    I = {k: torch.rand(500, generator=g).double() for k in range(2, 11)}
    gts = [I[k] for k in (2, 4, 6, 8, 3, 5, 7, 4, 6, 5, 10, 9, 8, 7)]
    spare = [torch.zeros(500).double()] * 6
    ref = LS.multi_reference("cb", 17, outs + gts + spare, 1e-6, 1.0, torch.float64)
    loss, ll = O.bin_loss(outs, I)
    assert torch.equal(ref["loss"], loss) and torch.equal(ref["terms"][:14], torch.stack(ll))


@pytest.mark.parametrize("numel", LS.NUMELS)
@pytest.mark.parametrize("kind", LS.KINDS)
def test_loss_float32_torch_meets_the_bars_and_the_yardstick_cap(kind, numel):
    x, y = LS.make_xy(numel)
    for eps in (LS.EPS_VALUES if (kind == "cb" and numel in (257, LS.FWD_CAP + 1)) else LS.EPS_VALUES[:1]):
        r64, r32 = (LS.reference(kind, x, y, eps, LS.GLOSS, dt) for dt in (torch.float64, torch.float32))
        tag = f"{kind} n={numel} eps={eps:g}"
        LS.check_loss(tag, r32["loss"], r64["loss"], r32["loss"], label="float32")
        for nm in ("gx", "gy"):
            LS.check_grad(f"{tag} {nm}", r32[nm], r64[nm], r32[nm], label="float32")


@pytest.mark.parametrize("kind,T,numel,eps", LS.MULTI_CASES)
def test_multi_loss_float32_torch_meets_the_bars_and_the_yardstick_cap(kind, T, numel, eps):
    ts = LS.make_multi(numel)
    r64, r32 = (LS.multi_reference(kind, T, ts, eps, LS.GLOSS, dt) for dt in (torch.float64, torch.float32))
    tag = f"multi {kind} T={T} n={numel} eps={eps:g}"
    LS.check_loss(tag, r32["loss"], r64["loss"], r32["loss"], label="float32")
    LS.check_terms(tag, r32["terms"], r64["terms"], r32["terms"], label="float32")
    for i, g in r64["grads"].items():
        LS.check_grad(f"{tag} g{i}", r32["grads"][i], g, r32["grads"][i], label="float32")


def test_scale_reference_is_floor_log2_and_exact_at_the_edges():
    one = np.float32(1)
    assert LS.scale_reference(one, 16.0) == (16.0, 1 / 16.0)
    assert LS.scale_reference(np.nextafter(one, np.float32(2)), 16.0) == (8.0, 0.125)          # one ulp above a power of two
    assert LS.scale_reference(np.nextafter(one, np.float32(0)), 16.0) == (16.0, 1 / 16.0)
    assert LS.scale_reference(0.0, 16.0) == (1.0, 1.0)
    assert LS.scale_reference(np.float32(10.0), 10.0) == (1.0, 1.0)
    assert LS.scale_reference(np.nextafter(np.float32(10.0), np.float32(32)), 10.0) == (0.5, 2.0)
    assert LS.scale_reference(np.float32(1e-30), 16.0) == (2.0 ** 40, 2.0 ** -40)              # clamped
    for a in LS.SCALE_AMAX:
        for t in LS.SCALE_TARGETS:
            s, inv = LS.scale_reference(a, t)
            assert s * inv == 1.0 and float(a) * s <= float(np.float32(t))
            assert float(np.float32(t)) < 2 * float(a) * s or s == 2.0 ** 40                       # (the clamp of the exponent)
            if abs(math.log2(float(np.float32(t)) / float(a)) % 1.0 - 0.5) < 0.4:              # away from an integer: plain floor(log2)
                assert s == 2.0 ** min(40, math.floor(math.log2(float(np.float32(t)) / float(a))))
    v = LS.scale_input(LS.FWD_CAP + 1, np.float32(0.75), negative=True)
    assert float(v[-1]) == -0.75 and float(v[:-1].abs().max()) < 0.75 * 0.5


# ------------------------------------------------------------------------------------------------------------------ glue
def test_split_values_cover_every_binade_and_numpy_meets_the_derived_bound():
    v = GC.split_values()
    e = np.frexp(np.abs(v[v != 0]).astype(np.float64))[1] - 1
    for b in GC.BINADES:
        assert (e == b).sum() >= 100, b
    assert np.abs(v).max() == GC.F16_MAX and (v == 0).sum() == 2 and np.signbit(v[v == 0]).sum() == 1
    for want in (1 + 2.0 ** -11, 1 + 2.0 ** -10, 1 + 2.0 ** -23, 2 - 2.0 ** -23, 2.0 ** -14, 2.0 ** -24, -(2.0 ** -24)):
        assert (v == np.float32(want)).any(), want
    # numpy's conversion is round-to-nearest-even with subnormals kept
    assert np.float32(1 + 2.0 ** -11).astype(np.float16) == 1.0 and np.float32(1 + 3 * 2.0 ** -11).astype(np.float16) == np.float16(1 + 2.0 ** -9)
    assert np.float32(2.0 ** -24).astype(np.float16) == np.float16(2.0 ** -24) and np.float32(2.0 ** -25).astype(np.float16) == 0
    assert np.float32(1.5 * 2.0 ** -24).astype(np.float16) == np.float16(2.0 ** -23)
    for scale in (1.0, 2.0 ** -7, 2.0 ** 9):
        x = v * np.float32(scale)
        assert np.array_equal(x.astype(np.float64), v.astype(np.float64) * scale)              # the scaling is exact
        x = x[np.abs(x) <= GC.F16_MAX]
        hi, lo = GC.split_ref(x)
        assert np.isfinite(hi.astype(np.float32)).all() and np.isfinite(lo.astype(np.float32)).all()
        assert GC.split_bound_ok(x, hi, lo, 3).all() and GC.split_bound_ok(x, hi, lo, 1).all()
        worst = np.abs(x.astype(np.float64) - hi.astype(np.float64) - lo.astype(np.float64)) / np.maximum(np.abs(x.astype(np.float64)), 1e-300)
        assert worst[np.abs(x) >= 2.0 ** -13].max() > 2.0 ** -25                                # the bound is not slack by much
    bad_lo = (GC.split_ref(v)[1].view(np.uint16) & np.uint16(0xFFFE)).view(np.float16)          # a lost last bit breaks the bit-equality
    assert not np.array_equal(bad_lo.view(np.uint16), GC.split_ref(v)[1].view(np.uint16))


def test_layout_references_are_the_oracle_permutations():
    rng = np.random.RandomState(0)
    for c in GC.CHANNELS:
        x = rng.randn(2, c, 3, 5).astype(np.float32)
        p = GC.planes_of(x)
        assert p.shape == ((c + 15) // 16, 2, 3, 5, 16) and np.array_equal(GC.nchw_of(p, c), x)
        assert c % 16 == 0 or (p[-1, ..., c % 16:] == 0).all()                                  # zero-padded channels
        assert p[(c - 1) // 16, 1, 2, 4, (c - 1) % 16] == x[1, c - 1, 2, 4]
    for r in (2, 3, 4):
        x = rng.randn(2, 5, 3 * r, 2 * r).astype(np.float32)
        assert np.array_equal(GC.pixel_unshuffle_ref(x, r), O.pixel_reshuffle(torch.from_numpy(x), r).numpy())
    imgs = [rng.randn(2, 3, 6, 10).astype(np.float32) for _ in range(3)]
    want = GC.planes_of(O.pixel_reshuffle(torch.cat([torch.from_numpy(i) for i in imgs], 1), 2).numpy())
    assert np.array_equal(GC.pack_inputs_ref(imgs), want)
    # unshuffle_planes: output chunk sub * nch + c is F.pixel_unshuffle's channel (16 c + k) * 4 + sub
    x = rng.randn(2, 32, 6, 10).astype(np.float32)
    got = GC.nchw_of(GC.unshuffle_planes_ref(GC.planes_of(x)), 128)
    pu = F.pixel_unshuffle(torch.from_numpy(x), 2).numpy()
    for sub in range(4):
        for c in range(2):
            for k in (0, 7, 15):
                assert np.array_equal(got[:, (sub * 2 + c) * 16 + k], pu[:, (c * 16 + k) * 4 + sub])
    # unpack_input_grads: the inverse of pack_inputs plus the skip path
    for k in (2, 3, 5):
        imgs = [rng.randint(-50, 50, (2, 3, 6, 10)).astype(np.float32) for _ in range(k)]
        hi = GC.pack_inputs_ref(imgs).astype(np.float16)
        zero = np.zeros((2, 3, 6, 10), np.float32)
        outs = GC.unpack_input_grads_ref(hi, None, zero, 1.0, k)
        assert all(np.array_equal(a, b) for a, b in zip(outs, imgs))
        gout = rng.randn(2, 3, 6, 10).astype(np.float32)
        outs = GC.unpack_input_grads_ref(hi, hi, gout, 0.25, k)
        assert all(np.array_equal(a, gout / np.float32(k) + b * np.float32(0.5)) for a, b in zip(outs, imgs))
        assert all(np.array_equal(a, gout / np.float32(k)) for a in GC.unpack_input_grads_ref(None, None, gout, 1.0, k))


def test_frame_references_are_the_oracle_helpers():
    cases = GC.frame_cases()
    assert {(h, w) for h, w, _ in cases} == set(GC.FRAME_SIZES) and any(p[0] > w or p[2] > h for h, w, p in cases)
    img = GC.u8_image(5, 7)
    ref = GC.u8_to_frame_ref(img, (3, 5, 2, 7))
    plain = torch.from_numpy(img[:, :, [2, 1, 0]].transpose(2, 0, 1).copy()).float() / 255
    assert ref.shape == (1, 3, 14, 15) and np.array_equal(ref, O.replicate_pad(plain[None], (3, 5, 2, 7)).numpy())
    assert np.array_equal(ref[0, :, 2:7, 3:10], plain.numpy()) and ref[0, 0, 0, 0] == plain[0, 0, 0] and ref[0, 2, -1, -1] == plain[2, -1, -1]
    assert set(GC.u8_image(37, 53).reshape(-1).tolist()) == set(range(256))
    f = GC.rounding_frame()
    mid = ((np.arange(255) + 0.5) / 255.0).astype(np.float32)
    for m in (mid, np.nextafter(mid, np.float32(2)), np.nextafter(mid, np.float32(-1))):
        assert np.isin(m, f).all()
    assert np.isinf(f).sum() == 2 and not np.isnan(f).any() and (f > 1).any() and (f < 0).any()
    out = O.tensor2img(torch.from_numpy(f))
    assert out.shape == (16, 17, 3) and out.dtype == np.uint8
    t, l, h, w = GC.ROUNDING_CROPS[0]
    assert (t, l, h, w) == (0, 0, 16, 17) and len(GC.ROUNDING_CROPS) >= 5
    # round half to even is what distinguishes the oracle from floor(x + 0.5) on this frame
    naive = np.floor(np.clip(f, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)[[2, 1, 0]].transpose(1, 2, 0)
    assert (naive != out).any()
