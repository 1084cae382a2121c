"""CPU: output at any frame rate (--output_rate) without a device — libbinrate.so's ABI bookkeeping and its refusals before any
launch, the time grid of bin_amd/rate.py against its restatement in Fractions, rate.Resampler on stub frames through chain.Chain
for every cut set of every short stream, the entry point's argument checks, the Y4M header and the case table of the mix kernel
(rate_cases.py).  GPU side: test_gpu_rate.py."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import chain_cases as CC
import rate_cases as RC
import video_cases as VC
from conftest import REPO


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_rate_library_header_and_binding_agree():
    """What is binrate's own beside the bookkeeping of test_cpu_libraries.py: the codes against the binding, and sources that share
    binyuv's arithmetic where they could have copied it."""
    from bin_amd import _lib
    hdr = open(os.path.join(REPO, "include", "binrate.h")).read()
    for name, value, bound in (("BINRATE_E_ARG", -1, _lib.RATE_E_ARG), ("BINRATE_E_SHAPE", -2, _lib.RATE_E_SHAPE)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value == bound
    # the sources: the arithmetic is shared, not copied; plain HIP C++, no LDS, no switches
    csrc = os.path.join(REPO, "bin_amd", "csrc")
    src, yuv, common = (open(os.path.join(csrc, f)).read() for f in ("binrate.hip", "binyuv.hip", "binyuv_common.h"))
    assert '#include "binyuv_common.h"' in src and '#include "binyuv_common.h"' in yuv and "#pragma once" in common
    for name in ("rgb_pixel", "block_mean", "quantise", "coefficients", "clamp01"):
        defined = re.compile(rf"(?m)^[\w\s]*\b(?:void|float|uint32_t|int)\s+{name}\s*\([^;{{]*\)\s*\{{")
        assert len(defined.findall(common)) == 1 and not defined.findall(src) and not defined.findall(yuv), name
    for text in (src, yuv, common):
        assert not re.search(r"(?m)^\s*#\s*(if|ifdef|ifndef|elif|define)\b", text), "no preprocessor switches in the sources"
        assert "asm" not in re.sub(r"//.*", "", text) and "__shared__" not in text, "plain HIP C++, no LDS"
    assert "__fadd_rn(ca, __fmul_rn(w, __fsub_rn(cb, ca)))" in src, "every operation of the mix rounded on its own"


def test_rate_module_is_host_only():
    src = open(os.path.join(REPO, "bin_amd", "rate.py")).read()
    assert not re.search(r"(?m)^\s*(import|from)\s", src), "no imports at all: neither torch nor the device code"
    assert "float(" not in src, "integers only"
    from bin_amd import chain, rate
    assert rate.HOLD is chain.HOLD and rate.FACTORS == chain.FACTORS and rate.MODES == ("blend", "nearest")


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_blend_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.ratelib()
    Y, U, Vp, A, B = 0x100000, 0x200000, 0x300000, 0x4000000, 0x5000000
    fmt = lambda chroma=420, matrix=0, rng=0: C.byref(_lib.BinYuvFormat(chroma, matrix, rng))

    def call(a=A, b=B, w=0.25, hp=12, wp=16, top=3, left=1, h=6, w_=10, f=None, y=Y, u=U, v=Vp):
        return lib.binrate_blend_to_yuv(a, b, w, hp, wp, top, left, h, w_, f if f is not None else fmt(), y, u, v, None)
    for name in ("a", "b", "y", "u", "v"):
        assert call(**{name: None}) == -1, name
    assert call(a=A + 1) == -1 and call(b=B + 2) == -1 and call(a=A + 3, b=B + 3) == -1, "not a float's address"
    for w in (float("nan"), -0.1, 1.0, 1.5, float("inf"), float("-inf"), -1e-30):
        assert call(w=w) == -1, w
    for h, w_ in ((0, 10), (6, 0), (-1, 10), (6, -3)):
        assert call(h=h, w_=w_) == -1
    for bad in (fmt(chroma=422), fmt(chroma=0), fmt(matrix=2), fmt(matrix=-1), fmt(rng=2), fmt(rng=-1)):
        assert call(f=bad) == -1
    assert call(f=C.POINTER(_lib.BinYuvFormat)()) == -1, "a null format"
    for kw in (dict(hp=0), dict(wp=0), dict(hp=-4), dict(top=-1), dict(left=-1), dict(top=7), dict(left=7), dict(h=13), dict(w_=17),
               dict(top=2 ** 31 - 1), dict(left=2 ** 31 - 1)):
        assert call(**kw) == -1, kw
    big = 2 ** 31 - 1
    assert call(hp=big, wp=big, top=0, left=0) == -2 and call(hp=2 ** 20, wp=2 ** 20) == -2, "3*Hp*Wp beyond 2^40"
    # overlaps: an output plane on either input, planes on each other
    assert call(y=A + 64) == -1 and call(y=B + 64) == -1 and call(u=A) == -1 and call(v=B + 3 * 12 * 16 * 4 - 1) == -1
    assert call(u=Y + 59) == -1 and call(v=U + 14) == -1 and call(v=Y) == -1
    assert call(a=A, b=A, y=A + 8) == -1


def test_ops_blend_refuses_cpu_tensors_and_wrong_layouts():
    from bin_amd import ops
    fmt = (420, "bt601", "limited")
    x = torch.zeros(1, 3, 12, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.blend_to_yuv(x, x, 0.5, 3, 1, 6, 10, fmt)
    for bad in ((422, "bt601", "limited"), (420, "bt2020", "limited"), (420, "bt601", "tv")):
        with pytest.raises(ValueError, match="YUV format"):
            ops.blend_to_yuv(x, x, 0.5, 3, 1, 6, 10, bad)
    assert list(inspect.signature(ops.blend_to_yuv).parameters) == ["a", "b", "w", "top", "left", "h", "w_", "fmt", "out"]
    assert inspect.signature(ops.blend_to_yuv).parameters["out"].default is None


# ------------------------------------------------------------------------------------------------ the grid
@pytest.mark.parametrize("factor", RC.GRID_FACTORS)
@pytest.mark.parametrize("in_rate,out_rate", RC.RATE_PAIRS)
def test_grid_equals_its_restatement_in_fractions(in_rate, out_rate, factor):
    from bin_amd import rate
    T = RC.GRID_FRAMES
    F, M, want = RC.grid_ref(in_rate, out_rate, factor, T)
    for form in (out_rate, Fraction(*out_rate)):
        grid = rate.Grid(in_rate, form, factor)
        rho = RC.ratio(in_rate, out_rate)
        assert (grid.p, grid.q) == (rho.numerator, rho.denominator) and grid.F == F and grid.frames(T) == M
        got = [grid.at(m) for m in range(M)]
        assert [(a, Fraction(r, grid.p)) for a, r in got] == want
        assert all(0 <= r < grid.p for _, r in got) and all(grid.weight(m) == float(w) for m, (_, w) in enumerate(want))
        a_next, r_next = grid.at(M)
        assert a_next + (r_next > 0) > F * (T - 1) - 1, "frame M needs a dense position the stream does not emit"
    assert rate.Grid(in_rate, out_rate, factor).out_rate == tuple(out_rate), "the rate as written"


def test_grid_table_is_the_issues_and_its_named_ratios():
    rho = {pair: RC.ratio(*pair) for pair in RC.RATE_PAIRS}
    assert rho[((24, 1), (60, 1))] == Fraction(5, 2) and rho[((24, 1), (24, 1))] == 1 and rho[((60, 1), (24, 1))] == Fraction(2, 5)
    assert rho[((24, 1), (192, 1))] == 8 and rho[((30000, 1001), (60000, 1001))] == 2 and rho[((50, 1), (60, 1))] == Fraction(6, 5)
    assert rho[((24000, 1001), (60000, 1001))] == Fraction(5, 2) and rho[((25, 1), (60, 1))] == Fraction(12, 5)
    assert len(RC.RATE_PAIRS) == 9 and RC.GRID_FACTORS == (2, 8) and RC.GRID_FRAMES == 40
    from bin_amd import rate
    assert [rate.Grid((1, 1), (k, 1)).F for k in range(1, 9)] == [2, 2, 4, 4, 8, 8, 8, 8]
    assert rate.Grid((24, 1), (60, 1), 2).F == 4 and rate.Grid((24, 1), (60, 1), 8).F == 8 and rate.Grid((60, 1), (24, 1)).F == 2
    for F in (2, 4, 8):                                 # rho = F: today's length, every dense position once
        g = rate.Grid((30, 1), (30 * F, 1), 2)
        assert g.F == F and g.frames(7) == F * 6 and [g.at(m) for m in range(F * 6)] == [(m, 0) for m in range(F * 6)]


def test_grid_refusals():
    from bin_amd import rate
    with pytest.raises(ValueError, match="at most 8"):
        rate.Grid((24, 1), (193, 1))
    with pytest.raises(ValueError, match="at most 8"):
        rate.Grid((24000, 1001), (192, 1))
    rate.Grid((24, 1), (192, 1))
    for bad in ((0, 1), (-24, 1), (24, 0), (24, -1), (24.0, 1), (24,), (24, 1, 1), 24.0, "24", None, True, Fraction(0), Fraction(-5, 2)):
        with pytest.raises(ValueError):
            rate.Grid((24, 1), bad)
        with pytest.raises(ValueError):
            rate.Grid(bad, (24, 1))
    for bad in (3, 1, 0, 16, 4.0, "4", True):
        with pytest.raises(ValueError, match="factor"):
            rate.Grid((24, 1), (60, 1), bad)
    with pytest.raises(ValueError):
        rate.Grid((24, 1), (60, 1)).frames(1)
    with pytest.raises(ValueError, match="resample"):
        rate.Resampler(rate.Grid((24, 1), (60, 1)), lambda *a: None, "linear")
    assert rate.parse_rate("60") == (60, 1) and rate.parse_rate("60000:1001") == (60000, 1001) and rate.parse_rate("120:2") == (120, 2)
    for bad in ("", "60:", ":1", "0", "60:0", "-60", "59.94", "60/1", "60:1:1", "a", "60 "):
        with pytest.raises(ValueError, match="output_rate"):
            rate.parse_rate(bad)


# ------------------------------------------------------------------------------------------------ the resampler through chain.Chain
class _RateRun(CC.StubRun):
    """chain.run_stream on stub frames with its emit feeding rate.Resamplers (one per (rho, mode)), as the runners wire it."""

    def __init__(self, T, F, cuts, setups):
        from bin_amd import rate
        self.samplers, self.outputs = {}, {}
        for rho, mode in setups:
            key = (rho, mode)
            self.outputs[key] = []
            grid = rate.Grid((rho.denominator, 1), (rho.numerator, 1), F)
            assert grid.F == F
            self.samplers[key] = rate.Resampler(grid, lambda *out, key=key: self.outputs[key].append(out), mode)
        super().__init__(T, F, cuts)

    def emit(self, pos, frame):
        super().emit(pos, frame)
        for key, rs in self.samplers.items():
            n = len(self.outputs[key])
            rs.push(pos, frame)
            x_next = Fraction(n * self.F) / key[0]
            assert (len(self.outputs[key]) > n) == (x_next <= pos), "an output is emitted as soon as position ceil(x_m) has arrived"
            stubs = [v for v in vars(rs).values() if isinstance(v, CC.Stub)]
            assert len({id(v) for v in stubs}) <= 2, "at most two dense frames are referenced"
            assert not any(isinstance(v, (list, dict, set, tuple)) for v in vars(rs).values()), "nothing is collected"


@pytest.mark.parametrize("F", CC.FACTORS)
def test_resampler_on_every_cut_set_of_every_short_stream_equals_the_composition(F):
    rhos = sorted({r for r in (Fraction(1), Fraction(6, 5), Fraction(5, 2), Fraction(F, 2), Fraction(F)) if r <= F})
    assert Fraction(5, 2) in rhos or F == 2
    setups = [(rho, mode) for rho in rhos for mode in ("blend", "nearest")]
    n_mixed = n_suppressed = 0
    for T in range(2, 8):
        for cuts in CC.all_cut_sets(T):
            run = _RateRun(T, F, cuts, setups)
            # the invariant the resampler rests on: a real frame after a HOLD opens a scene, and only there
            opened = {pos for pos in range(1, len(run.emitted)) if run.emitted[pos] != CC.HOLD and run.emitted[pos - 1] == CC.HOLD}
            assert opened == {F * c for c in cuts if c < T - 1}, (T, cuts)
            assert run.emitted[0] != CC.HOLD and run.emitted == CC.expected_stream(T, cuts, F)
            for (rho, mode), outs in run.outputs.items():
                where = (T, cuts, F, rho, mode)
                want = RC.expected_outputs(T, cuts, F, rho, mode)
                M = ((F * (T - 1) - 1) * rho.numerator) // (F * rho.denominator) + 1
                assert [m for m, _, _, _ in outs] == list(range(M)) and len(want) == M, where
                got = [(left.t, None if right is None else right.t, w) for _, left, right, w in outs]
                assert got == want, where
                for m, left, right, w in outs:
                    assert (right is None) == (w == 0) and 0 <= w < 1, where
                    if right is not None:
                        assert mode == "blend" and left is not right and left.t != right.t, where
                        assert RC.scene_of_time(T, cuts, left.t) == RC.scene_of_time(T, cuts, right.t), where
                        assert 0 < right.t - left.t <= Fraction(1, F), "neighbours of the dense stream"
                        n_mixed += 1
                    if mode == "nearest":               # ties go left
                        x = Fraction(m * F) / rho
                        if x - (x.numerator // x.denominator) == Fraction(1, 2):
                            dense = RC.dense_stream(T, cuts, F)
                            assert left.t == dense[x.numerator // x.denominator][0], where
                n_suppressed += sum(1 for (m, _, right, _), x in ((o, Fraction(o[0] * F) / rho) for o in outs)
                                    if right is None and x.denominator != 1 and mode == "blend")
            if F == max(rhos):
                key = (Fraction(F), "blend")
                assert [left.t for _, left, _, _ in run.outputs[key]] == [t for t, _, _ in RC.dense_stream(T, cuts, F)]
    print(f"[rate] F = {F}: {n_mixed} mixes, {n_suppressed} frames kept alone between two dense positions")
    assert n_mixed > 100 and n_suppressed > 20, "both kinds of output were seen: mixes, and frames kept alone at cuts and holds"


def test_resampler_resolves_holds_to_the_same_object_and_checks_its_input():
    from bin_amd import rate
    outs = []
    rs = rate.Resampler(rate.Grid((2, 1), (3, 1), 2), lambda *o: outs.append(o))        # rho 3/2 on F = 2: x_m = 4m/3
    a, b, c = CC.Stub(0), CC.Stub(Fraction(1, 2)), CC.Stub(2)
    with pytest.raises(RuntimeError):
        rate.Resampler(rate.Grid((2, 1), (3, 1), 2), lambda *o: None).push(0, rate.HOLD)
    with pytest.raises(RuntimeError):
        rate.Resampler(rate.Grid((2, 1), (3, 1), 2), lambda *o: None).push(1, a)
    for pos, f in enumerate((a, b, rate.HOLD, rate.HOLD, c)):
        rs.push(pos, f)
    # x = 0, 4/3, 8/3, 4: a; b + 1/3 (hold - b) = b alone; hold alone; c
    assert outs == [(0, a, None, 0), (1, b, None, 0), (2, b, None, 0), (3, c, None, 0)]
    assert outs[1][1] is b and outs[2][1] is b, "a hold IS the last real frame"
    with pytest.raises(RuntimeError):
        rs.push(7, a)


# ------------------------------------------------------------------------------------------------ the entry point and the header
def test_cli_rate_arguments_and_their_refusals_come_before_the_model_is_built(monkeypatch, tmp_path):
    import argparse
    from bin_amd import harness, test as T, video as V
    monkeypatch.setattr(T, "create_model", lambda *a, **k: pytest.fail("the model must not be built"))
    monkeypatch.setattr(T.option, "parse", lambda *a, **k: pytest.fail("the options must not be read"))
    base = ["--opt", "c", "--input_video", "in.y4m", "--output_video", "-"]
    args = T.parse_args(base)
    assert args.output_rate is None and args.resample is None and args.factor == 2
    args = T.parse_args(base + ["--output_rate", "60000:1001", "--resample", "nearest", "--factor", "8"])
    assert (args.output_rate, args.resample, args.factor) == ("60000:1001", "nearest", 8)
    assert T.parse_args(base + ["--output_rate", "60"]).resample is None
    with pytest.raises(SystemExit):
        T.parse_args(base + ["--output_rate", "60", "--resample", "linear"])
    for bad in ("0", "60:0", "59.94", "60/1", "-1", "x", "60:"):
        with pytest.raises(ValueError, match="output_rate"):
            T.main(base + ["--output_rate=" + bad])
    with pytest.raises(ValueError, match="--resample goes with --output_rate"):
        T.main(base + ["--resample", "nearest"])
    folder = ["--opt", "c", "--input_path", "a", "--output_path", "b"]
    assert T.parse_args(folder).output_rate is None
    for extra in (["--output_rate", "60"], ["--resample", "blend"], ["--output_rate", "60", "--resample", "nearest"]):
        with pytest.raises(ValueError, match="--output_rate"):
            T.main(folder + extra)
    T.check_args(argparse.Namespace(input_video=None, output_video=None, input_path="a", output_path="b", gt_path=None, launcher="none"))
    with pytest.raises(ValueError, match="--output_rate"):
        T.check_args(argparse.Namespace(input_video=None, output_video=None, input_path="a", output_path="b", gt_path=None,
                                        launcher="none", output_rate="60"))
    # rho > 8 needs the stream's own rate: a file's header is looked at by check_args
    src = str(tmp_path / "in.y4m")
    header = V.parse_header(b"YUV4MPEG2 W40 H24 F24:1 Ip A1:1 C420jpeg")
    with V.Y4MWriter(src, header) as wr:
        for _ in range(2):
            wr.write(np.zeros(header.frame_bytes, np.uint8))
    on_file = ["--opt", "c", "--input_video", src, "--output_video", str(tmp_path / "out.y4m")]
    with pytest.raises(ValueError, match="at most 8"):
        T.main(on_file + ["--output_rate", "193"])
    with pytest.raises(ValueError, match="at most 8"):
        T.main(on_file + ["--output_rate", "193000:1001", "--factor", "8"])
    assert T.parse_args(on_file + ["--output_rate", "192"]).output_rate == "192"
    assert not os.path.exists(tmp_path / "out.y4m")
    # the signature: the new parameters come before factor, scene_cut stays last
    sig = inspect.signature(harness.interpolate_video).parameters
    assert list(sig)[-5:] == ["ensemble", "rate", "resample", "factor", "scene_cut"]
    assert (sig["rate"].default, sig["resample"].default, sig["factor"].default, sig["scene_cut"].default) == (None, "blend", 2, None)
    payloads = torch.zeros(3, header.frame_bytes, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at most 8"):
        harness.interpolate_video(None, payloads, header, rate=(193, 1))
    with pytest.raises(ValueError, match="resample"):
        harness.interpolate_video(None, payloads, header, rate=(60, 1), resample="linear")
    with pytest.raises(ValueError, match="resample"):
        harness.interpolate_video(None, payloads, header, resample="linear")
    for bad in ((0, 1), 59.94, "60", (60, 0)):
        with pytest.raises(ValueError, match="rate"):
            harness.interpolate_video(None, payloads, header, rate=bad)
    with pytest.raises(ValueError, match="at least 2 frames"):
        harness.interpolate_video(None, payloads[:1], header, rate=(60, 1))


def test_header_at_rate():
    from bin_amd import video as V
    h = V.parse_header(b"YUV4MPEG2 W40 H24 F24000:1001 Ip A1:1 C444 XCOLORRANGE=FULL")
    out = h.at_rate((60000, 1001))
    assert out.rate == (60000, 1001) and out.line() == b"YUV4MPEG2 W40 H24 F60000:1001 Ip A1:1 C444 XCOLORRANGE=FULL\n"
    assert h.at_rate((120, 2)).rate == (120, 2), "reduced only as far as the user wrote it"
    assert h.at_rate(60).rate == (60, 1) and h.at_rate(Fraction(60000, 1001)).rate == (60000, 1001) and h.at_rate(h.rate) == h
    assert V.parse_header(out.line()) == out
    for field in ("width", "height", "interlace", "aspect", "colorspace", "extra"):
        assert getattr(out, field) == getattr(h, field)
    for bad in ((0, 1), (60, 0), (-60, 1), 59.94, "60", (60,), True):
        with pytest.raises(ValueError):
            h.at_rate(bad)


# ------------------------------------------------------------------------------------------------ the case table
def test_safe_pairs_keep_the_mix_off_every_tie_and_replace_little():
    """The share condition of the table: at most 10 % of the pixels replaced in any case of 64 pixels or more, at most 5 % over the
    whole table (VC.CASES x the four (matrix, range) pairs x nine weights)."""
    replaced = pixels = 0
    worst = 0.0
    for h, w, chroma in VC.CASES:
        for matrix, rng in VC.MATRIX_RANGE:
            fmt = (chroma, matrix, rng)
            for k, weight in enumerate(RC.WEIGHTS):
                a, b, share = RC.safe_pair((h, w), fmt, weight, seed=1000 * h + 10 * w + k)
                assert a.dtype == b.dtype == np.float32 and a.shape == b.shape == (3, h, w)
                if h * w >= RC.SHARE_MIN_PIXELS:
                    assert share <= RC.MAX_SHARE_CASE, (h, w, fmt, weight, share)
                    worst = max(worst, share)
                replaced += share * h * w
                pixels += h * w
    print(f"[rate] safe_pair: replaced {replaced / pixels:.4f} of all pixels, worst case {worst:.4f}")
    assert replaced / pixels <= RC.MAX_SHARE_TABLE
    assert len(RC.WEIGHTS) == 9 and set(RC.GPU_WEIGHTS) == {Fraction(1, 5), Fraction(1, 2), Fraction(4, 5), Fraction(1, 60), Fraction(59, 60)}
    assert RC.TIE_MARGIN == VC.TIE_MARGIN == 2.0 ** -10


@pytest.mark.parametrize("chroma", VC.CHROMAS)
def test_safe_pairs_make_float32_and_float64_agree_on_every_byte(chroma):
    """The bar is not vacuous: the restatement in fp32 (every operation rounded on its own, as the kernel's) gives the float64 bytes
    on safe pairs, its pre-rounding values stay far inside the margin, the specials are there, and a crop is respected."""
    worst = 0.0
    for h, w in ((7, 16), (33, 130)):
        for matrix, rng in VC.MATRIX_RANGE:
            fmt = (chroma, matrix, rng)
            for weight in RC.GPU_WEIGHTS:
                t, l = 3, 1
                a, b, _ = RC.safe_pair((h + 5, w + 3), fmt, weight, seed=h + w, crop=(t, l, h, w))
                assert np.isnan(a).any() and np.isinf(a).any() and np.isnan(b).any() and (a < 0).any() and (b > 1).any()
                want = RC.blend_ref(a, b, weight, t, l, h, w, fmt)
                assert np.array_equal(RC.blend_ref(a, b, weight, t, l, h, w, fmt, np.float32), want), (fmt, weight)
                for p64, p32 in zip(RC.prerounding(a, b, weight, t, l, h, w, fmt), RC.prerounding(a, b, weight, t, l, h, w, fmt, np.float32)):
                    worst = max(worst, float(np.abs(p64 - p32.astype(np.float64)).max()))
    assert worst < RC.TIE_MARGIN / 4, worst
    print(f"[rate] fp32 restatement against float64: at most {worst:.3e} code units, the margin is {RC.TIE_MARGIN:.3e}")


def test_the_restatement_has_the_kernels_identities():
    """w = 0 and b = a give VC.from_frame_ref(a)'s bytes on UNSAFE frames, NaN and infinities included."""
    for chroma in VC.CHROMAS:
        fmt = (chroma, "bt709", "limited")
        a, b = RC.unsafe_pair((9, 14), seed=5)
        want = VC.from_frame_ref(a, 1, 2, 7, 11, fmt)
        assert np.array_equal(RC.blend_ref(a, b, 0, 1, 2, 7, 11, fmt), want)
        for weight in RC.GPU_WEIGHTS:
            assert np.array_equal(RC.blend_ref(a, a, weight, 1, 2, 7, 11, fmt), want)
        assert not np.array_equal(RC.blend_ref(a, b, Fraction(1, 2), 1, 2, 7, 11, fmt), want)
