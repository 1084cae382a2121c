"""CPU: scoring a video run against a ground-truth stream (--gt_video) without a device — libbinscore.so's ABI bookkeeping and its
refusals before any launch, the alignment rule, the classes and the tally of bin_amd/score.py against computations by hand, the
entry point's refusals, and chain.run_stream on stub frames with a recording scorer where the writer calls it.  GPU side:
test_gpu_score.py."""
import ctypes as C
import inspect
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

import chain_cases as CC
import score_cases as SC
from conftest import REPO


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_score_library_header_and_binding_agree():
    """What is binscore's own beside the bookkeeping of test_cpu_libraries.py: the codes and flags against the binding and against
    binhip.h's, the record's layout, and that libbinhip.so keeps its metrics source."""
    from bin_amd import _lib, build
    hdr = open(os.path.join(REPO, "include", "binscore.h")).read()
    assert build.SOURCES.count("binhip_metrics.hip") == 1
    for name, value, bound in (("BINSCORE_E_ARG", -1, _lib.SCORE_E_ARG), ("BINSCORE_E_SHAPE", -2, _lib.SCORE_E_SHAPE),
                               ("BINSCORE_E_WORKSPACE", -3, _lib.SCORE_E_WORKSPACE)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value == bound
    binhip = open(os.path.join(REPO, "include", "binhip.h")).read()
    for name, value, bound in (("SSIM_G11", 1, _lib.PLANE_SSIM_G11), ("SSIM_U7", 2, _lib.PLANE_SSIM_U7)):
        assert int(re.search(rf"#define\s+BINSCORE_{name}\s+(\d+)", hdr).group(1)) == value == bound
        assert int(re.search(rf"#define\s+BINHIP_SCORE_{name}\s+(\d+)", binhip).group(1)) == value, "1 and 2 in both headers"
    assert C.sizeof(_lib.BinPlaneScores) == 64 and _lib.BinPlaneScores.sad.offset == 24 and _lib.BinPlaneScores.ssim_g11.offset == 48


def test_the_tile_walk_has_one_definition():
    csrc = os.path.join(REPO, "bin_amd", "csrc")
    walk, metrics, planes = (open(os.path.join(csrc, f)).read() for f in ("binhip_score_walk.h", "binhip_metrics.hip", "binscore.hip"))
    assert "#pragma once" in walk and re.findall(r'(?m)^#include\s+(\S+)', walk) == ["<hip/hip_runtime.h>", "<stdint.h>"], \
        "the walk needs the HIP runtime only"
    for text in (metrics, planes):
        assert '#include "binhip_score_walk.h"' in text
        assert "static_assert(" in text and "SC_FLAG_G11" in text and "SC_FLAG_U7" in text, "the header's flags against the walk's"
    assert walk.count("\nscore_tile_kernel(const L ld") == 1 and "score_tile_kernel(const" not in metrics + planes
    for name in ("ssim_g11", "ssim_u7"):
        defined = re.compile(rf"(?m)^[\w\s]*\b(?:void|double)\s+{name}\s*\([^;{{]*\)\s*\{{")
        assert len(defined.findall(walk)) == 1 and not defined.findall(metrics) and not defined.findall(planes), name
    for name in ("ScoreTaps", "ScorePartial"):
        assert len(re.findall(rf"struct\s+{name}\s*\{{", walk)) == 1
        assert not re.search(rf"struct\s+{name}\s*\{{", metrics) and not re.search(rf"struct\s+{name}\s*\{{", planes)
    assert "struct U8Pairs" in metrics and "struct FramePairs" in metrics and "struct PlanePairs" in planes
    assert re.search(r"struct PlanePairs \{[^}]*STRIDE = 1", planes), "single u8 planes: a neighbour is one byte away"
    assert "plane_score_final_kernel" in planes and "image_score_final_kernel" in metrics, "each file keeps its final kernel"
    for text in (walk, planes):
        assert "asm" not in re.sub(r"//.*", "", text), "plain HIP C++"


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_planes_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced: every
    call here is one the library refuses, none reaches a launch)."""
    from bin_amd import _lib
    lib = _lib.scorelib()
    AY, AU, AV, BY, BU, BV, WS, OUT = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x8000000, 0x700000
    taps = (C.c_double * 11)(*([1.0 / 11] * 11))
    G11, U7 = _lib.PLANE_SSIM_G11, _lib.PLANE_SSIM_U7

    def need(h=24, w=40, chroma=420, flags=G11 | U7):
        return lib.binscore_workspace_bytes(h, w, chroma, flags)

    def call(ay=AY, au=AU, av=AV, by=BY, bu=BU, bv=BV, h=24, w=40, chroma=420, flags=G11 | U7, g=taps, ws=WS, nb=None, out=OUT):
        nb = need(h, w, chroma, flags) if nb is None else nb
        return lib.binscore_planes(ay, au, av, by, bu, bv, h, w, chroma, flags, g, ws, nb, out, None)

    # the workspace: one 64-byte slot per 16 x 246 tile of every plane
    assert need() == 64 * (2 + 2 * 1) and need(16, 246) == 64 * 3 and need(17, 247) == 64 * (4 + 2) and need(17, 247, 444) == 64 * 12
    assert need(33, 493, 420) == 64 * (9 + 2 * 4) and need(1, 1, 420, 0) == 64 * 3 and need(65535, 65535, 444, 0) == 64 * 3 * 4096 * 267
    for name in ("ay", "au", "av", "by", "bu", "bv", "ws", "out"):
        assert call(**{name: None}) == -1, name
    assert call(g=None) == -1 and call(g=None, flags=G11) == -1, "a null g11_taps with its flag"
    for flags in (4, 8, 7, -1, 1 << 30):
        assert call(flags=flags, nb=1 << 20) == -1 and need(flags=flags) == 0, flags
    for chroma in (0, 422, 411, 400, -420, 421):
        assert call(chroma=chroma, nb=1 << 20) == -1 and need(chroma=chroma) == 0, chroma
    for out in (OUT + 1, OUT + 4, OUT + 7):
        assert call(out=out) == -1, "out not 8-byte aligned"
    assert call(ws=WS + 4) == -1
    # overlaps: the record or the workspace on a plane (the planes of a 24 x 40 4:2:0 payload are 960, 240 and 240 bytes)
    assert call(out=AY) == -1 and call(out=AY + 952) == -1 and call(out=AU + 232) == -1 and call(out=BV + 8) == -1 and call(out=BY - 56) == -1
    assert call(ws=AY + 8) == -1 and call(ws=BU - 8) == -1 and call(ws=AV - need() + 8) == -1 and call(ws=OUT - 8) == -1
    # shapes
    for h, w in ((0, 40), (24, 0), (-1, 40), (24, -7), (65536, 40), (24, 65536), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert call(h=h, w=w, flags=0, nb=1 << 20) == -2 and need(h, w, 420, 0) == 0, (h, w)
    for h, w in ((10, 40), (24, 10), (7, 7)):
        assert call(h=h, w=w, flags=G11, nb=1 << 20) == -2 and call(h=h, w=w, flags=G11 | U7, nb=1 << 20) == -2 and need(h, w, 420, G11) == 0
    for h, w in ((6, 40), (24, 6), (1, 1)):
        assert call(h=h, w=w, flags=U7, nb=1 << 20) == -2 and need(h, w, 444, U7) == 0
    assert need(7, 7, 420, U7) > 0 and need(11, 11, 444, G11 | U7) > 0 and need(10, 40, 420, U7) > 0
    # the workspace size
    assert call(nb=need() - 1) == -3 and call(nb=0) == -3
    assert call(flags=4, nb=0) == -1 and call(h=0, nb=0) == -2, "argument and shape errors come first"


def test_ops_payload_scores_refuses_cpu_tensors_and_wrong_layouts():
    from bin_amd import ops
    n = SC.frame_bytes(24, 40, 420)[0]
    x = torch.zeros(n, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.payload_scores(x, x, 24, 40, 420)
    for bad in (422, 0, "420"):
        with pytest.raises(ValueError, match="chroma"):
            ops.payload_scores(x, x, 24, 40, bad)
    with pytest.raises(ValueError):
        ops.payload_scores(x, x, 0, 40, 420)
    assert list(inspect.signature(ops.payload_scores).parameters) == ["a", "b", "h", "w", "chroma", "ssim", "out"]
    sig = inspect.signature(ops.payload_scores).parameters
    assert sig["ssim"].default is True and sig["out"].default is None and ops.PLANE_SCORES_BYTES == 64
    rec = np.zeros(64, np.uint8)
    rec[:48].view(np.uint64)[:] = [5, 6, 7, 1, 2, 3]
    rec[48:].view(np.float64)[:] = [0.25, float("nan")]
    got = ops.read_plane_scores(rec)
    assert got[:7] == (5, 6, 7, 1, 2, 3, 0.25) and math.isnan(got[7]) and all(type(v) is int for v in got[:6])
    assert ops.read_plane_scores(torch.from_numpy(rec))[:7] == got[:7] and ops.read_plane_scores(rec.tobytes())[:7] == got[:7]
    with pytest.raises(ValueError):
        ops.read_plane_scores(rec[:32])


def test_case_table_reference():
    assert len(SC.CASES) == 104 and len({SC.case_id(c) for c in SC.CASES}) == 104
    for case in SC.CASES:
        flags, h, w, chroma, content = case
        ref = SC.reference(case)
        assert all(type(v) is int for v in ref[:6])
        assert math.isnan(ref[6]) == (flags != SC.BOTH) and math.isnan(ref[7]) == (flags == SC.NONE), case
        if content == "same":
            assert ref[:6] == (0,) * 6
        if content == "constant":
            n, ch, cw = SC.frame_bytes(h, w, chroma)
            assert ref[:6] == (0, 184 ** 2 * ch * cw, 184 ** 2 * ch * cw, 0, 184 * ch * cw, 184 * ch * cw)
            assert flags == SC.NONE or ref[7] == 1.0, "constant planes: SSIM is exactly 1"
            assert flags != SC.BOTH or ref[6] == 1.0
    assert SC.reference((SC.BOTH, 33, 493, 420, "random")) is SC.reference((SC.BOTH, 33, 493, 420, "random")), "computed once"


# ------------------------------------------------------------------------------------------------ alignment
def _header(text=b"W40 H24 F30:1 Ip A1:1 C420jpeg"):
    from bin_amd import video
    return video.parse_header(b"YUV4MPEG2 " + text)


def test_alignment_rule_and_its_refusals():
    from bin_amd import score
    assert score.stride((240, 1), (60, 1)) == 4 and score.stride((240, 1), (120, 1)) == 2 and score.stride((240, 1), (240, 1)) == 1
    assert score.stride((240000, 1001), (60000, 1001)) == 4 and score.stride((120, 2), (60, 1)) == 1 and score.stride((60, 1), (30000, 1000)) == 2
    for gt, out in (((240, 1), (100, 1)), ((60, 1), (120, 1)), ((240, 1), (60000, 1001)), ((30000, 1001), (30, 1)), ((75, 1), (30, 1))):
        with pytest.raises(ValueError) as e:
            score.stride(gt, out)
        assert f"{gt[0]}:{gt[1]}" in str(e.value) and f"{out[0]}:{out[1]}" in str(e.value), "the refusal names both values"
    out = _header().multiplied(2)
    assert score.align(out, _header(b"W40 H24 F240:1 Ip A1:1 C420jpeg")) == 4
    assert score.align(out, _header(b"W40 H24 F60:1 C420mpeg2"), 7) == 1, "the 4:2:0 sitings are one family"
    assert score.align(out, _header(b"W40 H24 F60:1"), 0) == 1, "no C tag is 4:2:0"
    assert score.align(_header().at_rate((75, 1)), _header(b"W40 H24 F150:1")) == 2, "against the written header's rate"
    for bad, names in ((b"W41 H24 F60:1", ("41", "40")), (b"W40 H26 F60:1", ("26", "24")), (b"W40 H24 F60:1 C444", ("444", "420")),
                       (b"W40 H24 F45:1", ("45:1", "60:1"))):
        with pytest.raises(ValueError, match="--gt_video") as e:
            score.align(out, _header(bad))
        assert all(n in str(e.value) for n in names), (bad, str(e.value))
    full, limited = _header(b"W40 H24 F60:1 XCOLORRANGE=FULL"), _header(b"W40 H24 F60:1 XCOLORRANGE=LIMITED")
    with pytest.raises(ValueError, match="XCOLORRANGE") as e:
        score.align(full, limited)
    assert "FULL" in str(e.value) and "LIMITED" in str(e.value)
    assert score.align(full, full) == 1 and score.align(full, _header(b"W40 H24 F60:1")) == 1 and score.align(out, limited) == 1, \
        "only two tags that disagree are refused"
    for bad in (-1, -100, 1.0, "1", None, True):
        with pytest.raises(ValueError, match="gt_offset"):
            score.align(out, _header(b"W40 H24 F60:1"), bad)
    plan = score.Plan(4, 3, 2)
    assert [plan.gt_index(m) for m in range(4)] == [3, 7, 11, 15]
    for bad in (0, -1, 2.0, None):
        with pytest.raises(ValueError):
            score.Plan(bad, 0, 2)


def test_classes_per_phase():
    from bin_amd import score
    L0, L1, L2, L3 = "deblurred", "interp_L1", "interp_L2", "interp_L3"
    assert [score.frame_class(m, 2) for m in range(4)] == [L0, L1, L0, L1]
    assert [score.frame_class(m, 4) for m in range(8)] == [L0, L2, L1, L2] * 2
    assert [score.frame_class(m, 8) for m in range(16)] == [L0, L3, L2, L3, L1, L3, L2, L3] * 2
    for F in (2, 4, 8):
        assert score.frame_class(F, F, is_hold=True) == "held" and score.frame_class(F + 1, F, is_hold=True) == "held"
        assert score.frame_class(5, F, at_rate=True) == "all"
        plan = score.Plan(1, 0, F)
        assert plan.frame_class(0) == L0 and plan.frame_class(F // 2) == L1 and plan.frame_class(1, True) == "held"
    assert score.Plan(1, 0, 4, at_rate=True).frame_class(3) == "all"
    with pytest.raises(ValueError):
        score.frame_class(1, 3)
    assert set(score.CLASSES) == {L0, L1, L2, L3, "held", "all"}


# ------------------------------------------------------------------------------------------------ the tally
def test_tally_equals_a_computation_by_hand(tmp_path):
    from bin_amd import score
    from bin_amd.utils import util
    ny, nc = 24 * 40, 12 * 20
    rows = [(0, 1, "deblurred", 960, 240, 480, 100, 20, 30, 0.9, 0.8),
            (1, 3, "interp_L1", 1920, 0, 240, 200, 0, 10, 0.7, 0.6),
            (2, 5, "deblurred", 0, 0, 0, 0, 0, 0, 1.0, 1.0),                    # identical to its ground truth
            (3, 7, "held", 9600, 2400, 2400, 900, 300, 300, 0.1, 0.2),
            (4, 9, "deblurred", 3840, 480, 240, 300, 40, 20, 0.5, float("nan"))]
    tally = score.Tally(ny, nc)
    for r in reversed(rows):                                                    # the order of the rows does not matter
        tally.add(r)
    tally.no_gt()
    tally.no_gt(2)
    s = tally.summary()
    assert set(s) == {"deblurred", "interp_L1", "held", "overall", "unscored"} and s["unscored"] == 3
    d = s["deblurred"]
    assert d["n"] == 3 and d["n_identical"] == 1
    assert d["psnr_y"] == util.psnr_from_mse((960 + 0 + 3840) / (3 * ny)) == 20 * math.log10(255.0 / math.sqrt(4800 / 2880))
    assert d["psnr_u"] == util.psnr_from_mse(720 / (3 * nc)) and d["psnr_v"] == util.psnr_from_mse(720 / (3 * nc))
    assert d["psnr_yuv"] == util.psnr_from_mse((4800 + 720 + 720) / (3 * (ny + 2 * nc)))
    assert d["mean_psnr_y"] == math.fsum([util.psnr_from_mse(960 / ny), util.psnr_from_mse(3840 / ny)]) / 2, "the infinite one left out"
    assert d["ssim_g11"] == math.fsum([0.9, 1.0, 0.5]) / 3 and d["ssim_u7"] == math.fsum([0.8, 1.0]) / 2
    o = s["overall"]
    assert o["n"] == 5 and o["n_identical"] == 1 and o["psnr_y"] == util.psnr_from_mse((960 + 1920 + 9600 + 3840) / (5 * ny))
    assert s["held"]["n"] == 1 and s["held"]["psnr_y"] == util.psnr_from_mse(9600 / ny) == s["held"]["mean_psnr_y"]
    assert s["interp_L1"]["psnr_u"] == float("inf"), "a plane identical over the whole class"
    forward = score.Tally(ny, nc)
    for r in rows:
        forward.add(r)
    forward.no_gt(3)
    assert repr(forward.summary()) == repr(s), "exact sums: no dependence on the order"
    only = score.Tally(ny, nc)
    only.add(rows[2])
    assert only.summary()["overall"]["n_identical"] == 1 and math.isnan(only.summary()["overall"]["mean_psnr_y"])
    assert score.Tally(ny, nc).summary() == {"overall": {"n": 0}, "unscored": 0}
    lines = score.table(s)
    assert lines[0].split()[:3] == ["class", "n", "psnr_y"] and [ln.split()[0] for ln in lines[1:5]] == ["deblurred", "interp_L1", "held", "overall"]
    assert "3 output frames" in lines[-1] and "not scored" in lines[-1]
    # the log file: a header line, one tab-separated row per scored frame, the doubles as they are
    path = str(tmp_path / "scores.tsv")
    score.write_log(path, reversed(rows))
    text = open(path).read().splitlines()
    assert text[0].split("\t") == ["out", "gt", "class", "sse_y", "sse_u", "sse_v", "sad_y", "sad_u", "sad_v", "ssim_g11", "ssim_u7"]
    assert len(text) == 6 and text[1].split("\t") == ["0", "1", "deblurred", "960", "240", "480", "100", "20", "30", "0.9", "0.8"]
    back = score.read_log(path)
    assert back[:4] == rows[:4] and back[4][:10] == rows[4][:10] and math.isnan(back[4][10])


# ------------------------------------------------------------------------------------------------ the entry point
def test_cli_gt_arguments_and_their_refusals_come_before_the_model_is_built(monkeypatch, tmp_path):
    import argparse
    from bin_amd import harness, test as T, video as V
    monkeypatch.setattr(T, "create_model", lambda *a, **k: pytest.fail("the model must not be built"))
    monkeypatch.setattr(T.option, "parse", lambda *a, **k: pytest.fail("the options must not be read"))
    base = ["--opt", "c", "--input_video", "in.y4m", "--output_video", "out.y4m"]
    args = T.parse_args(base)
    assert (args.gt_video, args.gt_offset, args.score_log) == (None, 0, None)
    args = T.parse_args(base + ["--gt_video", "gt.y4m", "--gt_offset", "3", "--score_log", "s.tsv"])
    assert (args.gt_video, args.gt_offset, args.score_log) == ("gt.y4m", 3, "s.tsv")
    assert T.parse_args(base + ["--gt_video", "-"]).gt_video == "-"
    with pytest.raises(ValueError, match="--score_log goes with --gt_video"):
        T.main(base + ["--score_log", "s.tsv"])
    with pytest.raises(ValueError, match="gt_offset"):
        T.main(base + ["--gt_video", "gt.y4m", "--gt_offset", "-1"])
    with pytest.raises(ValueError, match="gt_offset"):
        T.main(base + ["--gt_offset", "2"])
    with pytest.raises(ValueError, match="stdin"):
        T.main(["--opt", "c", "--input_video", "-", "--output_video", "out.y4m", "--gt_video", "-"])
    folder = ["--opt", "c", "--input_path", "a", "--output_path", "b"]
    for extra in (["--gt_video", "gt.y4m"], ["--score_log", "s.tsv"], ["--gt_video", "gt.y4m", "--score_log", "s.tsv"]):
        with pytest.raises(ValueError, match="--input_video"):
            T.main(folder + extra)
    with pytest.raises(ValueError):
        T.main(base + ["--gt_path", "g"])                          # a folder of frames does not score a video
    T.check_args(argparse.Namespace(input_video=None, output_video=None, input_path="a", output_path="b", gt_path=None, launcher="none"))
    # the two headers: refused once both are read, before the model is built
    def write(name, text, n=3):
        header = V.parse_header(b"YUV4MPEG2 " + text)
        with V.Y4MWriter(str(tmp_path / name), header) as wr:
            for _ in range(n):
                wr.write(np.zeros(header.frame_bytes, np.uint8))
        return str(tmp_path / name)
    src = write("in.y4m", b"W40 H24 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL")
    on_file = ["--opt", "c", "--input_video", src, "--output_video", str(tmp_path / "out.y4m")]
    for text, extra, names in ((b"W40 H24 F90:1 C420jpeg", [], ("90:1", "60:1")), (b"W40 H24 F60:1 C420jpeg", ["--factor", "4"], ("60:1", "120:1")),
                               (b"W40 H24 F100:1", ["--output_rate", "75"], ("100:1", "75:1")), (b"W48 H24 F60:1", [], ("48", "40")),
                               (b"W40 H22 F60:1", [], ("22", "24")), (b"W40 H24 F60:1 C444", [], ("444", "420")),
                               (b"W40 H24 F60:1 XCOLORRANGE=LIMITED", [], ("LIMITED", "FULL"))):
        with pytest.raises(ValueError, match="--gt_video") as e:
            T.main(on_file + ["--gt_video", write("gt.y4m", text)] + extra)
        assert all(n in str(e.value) for n in names), str(e.value)
    assert not os.path.exists(tmp_path / "out.y4m")
    # the signature: the new parameters come before ensemble, scene_cut stays last
    sig = inspect.signature(harness.interpolate_video).parameters
    assert list(sig)[-8:] == ["gt", "gt_offset", "gt_stride", "ensemble", "rate", "resample", "factor", "scene_cut"]
    assert (sig["gt"].default, sig["gt_offset"].default, sig["gt_stride"].default) == (None, 0, 1)
    header = V.parse_header(b"YUV4MPEG2 W40 H24 F24:1 Ip A1:1 C420jpeg")
    payloads = torch.zeros(3, header.frame_bytes, dtype=torch.uint8)
    with pytest.raises(ValueError, match="gt must be"):
        harness.interpolate_video(None, payloads, header, gt=torch.zeros(3, header.frame_bytes + 1, dtype=torch.uint8))
    with pytest.raises(ValueError, match="gt_offset"):
        harness.interpolate_video(None, payloads, header, gt=payloads, gt_offset=-1)


def test_gt_feed_hands_over_the_strided_frames_in_order_and_never_reads_ahead(monkeypatch):
    """The reader thread of the ground-truth feed on a fake reader: the frames offset, offset + s, ... reach the queue in order, the
    skipped ones do not, it never holds more page-locked buffers than it was given, and it reads no further than the frame it hands
    over next while the queue is full."""
    import threading
    from bin_amd import test as T, video
    header = video.parse_header(b"YUV4MPEG2 W4 H2 F30:1")

    class Reader:
        def __init__(self, n):
            self.n, self.i, self.header = n, 0, header
            self.lock = threading.Lock()

        def readinto(self, buf):
            with self.lock:
                if self.i >= self.n:
                    return False
                buf[:] = self.i
                self.i += 1
                return True
    allocated = []
    real_empty = torch.empty

    def empty(*a, **k):                                            # (no device here: ordinary memory stands in for page-locked)
        k.pop("pin_memory", None)
        t = real_empty(*a, **k)
        allocated.append(t)
        return t
    monkeypatch.setattr(torch, "empty", empty)
    for _ in (0,):
        reader = Reader(23)
        feed = T._GtFeed(reader, 4, 2)
        got = []
        while True:
            item = feed.filled.get(timeout=10)
            if item is None:
                break
            assert not isinstance(item, BaseException), item
            got.append(int(item[0]))
            assert (item.numpy() == got[-1]).all()
            # the frames read so far: never past the frames the bounded queue and the next hand-over can hold
            assert reader.i <= got[-1] + 1 + 4 * (feed.BUFFERS + 1)
            feed.free_in.put(item)
        assert got == [2, 6, 10, 14, 18, 22] and reader.i == 23
        assert len(allocated) <= feed.BUFFERS, "recycled buffers only"
        # a full queue stops the reader: with no buffer handed back it reads the frames of BUFFERS hand-overs and no further
        reader = Reader(1000)
        feed = T._GtFeed(reader, 3, 0)
        first = feed.filled.get(timeout=10)
        assert int(first[0]) == 0
        deadline = 200
        while feed.filled.qsize() < feed.BUFFERS - 1 and deadline:
            threading.Event().wait(0.01)
            deadline -= 1
        threading.Event().wait(0.05)
        assert feed.filled.qsize() == feed.BUFFERS - 1 and reader.i == 3 * (feed.BUFFERS - 1) + 1, "it stopped at the last buffer it had"


# ------------------------------------------------------------------------------------------------ the scorer where the writer calls it
class _ScoredRun(CC.StubRun):
    """chain.run_stream on stub frames; the emit is the writer's: pack, then call the scorer with (pos, row, is_hold).  With a grid,
    rate.Resampler sits in between as in the runners."""

    def __init__(self, T, F, cuts, plan, grid=None):
        from bin_amd import rate
        self.plan, self.calls, self.grid = plan, [], grid
        self.sampler = None if grid is None else rate.Resampler(grid, self.emit_at_rate)
        super().__init__(T, F, cuts)

    def scorer(self, pos, row, is_hold):
        self.calls.append((pos, self.plan.gt_index(pos), self.plan.frame_class(pos, is_hold), row))

    def emit(self, pos, frame):
        super().emit(pos, frame)
        if self.sampler is not None:
            self.sampler.push(pos, frame)
        else:
            self.scorer(pos, "row %d" % pos, frame is None)

    def emit_at_rate(self, m, left, right, w):
        self.scorer(m, "row %d" % m, False)


@pytest.mark.parametrize("F", (2, 4))
def test_scorer_sees_every_output_position_once_in_display_order(F):
    from bin_amd import rate, score
    L = {2: ["deblurred", "interp_L1"], 4: ["deblurred", "interp_L2", "interp_L1", "interp_L2"]}[F]
    for T in (2, 3, 5, 6):
        for cuts in ((), (2,), (1, 3)):
            cuts = tuple(c for c in cuts if c < T)
            for stride, offset in ((1, 0), (4 // F * 2, 3)):
                run = _ScoredRun(T, F, cuts, score.Plan(stride, offset, F))
                n = F * (T - 1)
                assert [c[0] for c in run.calls] == list(range(n)), "every position once, in display order"
                assert [c[1] for c in run.calls] == [stride * m + offset for m in range(n)]
                assert [c[3] for c in run.calls] == ["row %d" % m for m in range(n)], "the row that was just packed"
                want = ["held" if run.emitted[m] == CC.HOLD else L[m % F] for m in range(n)]
                assert [c[2] for c in run.calls] == want, (T, cuts)
                if cuts and cuts[0] < T - 1:
                    c = cuts[0]
                    assert want[F * (c - 1) + 1:F * c] == ["held"] * (F - 1) and want[F * c] == "deblurred", "the holds before a cut"
    # with a rate grid: the outputs of the grid, one class
    for T, cuts in ((5, ()), (6, (2,))):
        grid = rate.Grid((30, 1), (75, 1), F)
        run = _ScoredRun(T, grid.F, cuts, score.Plan(2, 1, grid.F, at_rate=True), grid)
        M = grid.frames(T)
        assert [c[0] for c in run.calls] == list(range(M)) and [c[1] for c in run.calls] == [2 * m + 1 for m in range(M)]
        assert {c[2] for c in run.calls} == {"all"}
