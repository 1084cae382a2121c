"""GPU: scoring a video run against a ground-truth stream (--gt_video) — binscore_planes (include/binscore.h) against numpy and the
host SSIMs over the whole table of score_cases.py, at every byte offset, with guard bytes around everything it touches;
harness.interpolate_video(gt=...) against ops.payload_scores called by hand on the returned bytes; and
`python -m bin_amd.test --gt_video ... --score_log ...` in a child process against the harness.  CPU side: test_cpu_score.py."""
import ctypes as C
import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chain_cases as CC
import score_cases as SC
from conftest import REPO

pytestmark = pytest.mark.gpu

SSIM_TOL = 1e-9                                        # the bar tests/test_gpu_metrics.py holds the same walk to
GUARD = 0xA5


def _record(a, b, h, w, chroma, flags, **kw):
    from bin_amd import ops
    rec = ops.payload_scores(a, b, h, w, chroma, ssim=flags != SC.NONE, **kw)
    assert rec.dtype == torch.uint8 and tuple(rec.shape) == (64,) and rec.is_cuda
    return rec


def _assert_scores(got, want, where):
    assert got[:6] == want[:6], (where, got, want)
    assert all(type(v) is int for v in got[:6]) and all(type(v) is float for v in got[6:])
    for name, g, r in (("ssim_g11", got[6], want[6]), ("ssim_u7", got[7], want[7])):
        if math.isnan(r):
            assert math.isnan(g), (where, name, "a field without its flag is NaN")
        else:
            print(f"{where} {name}: kernel {g!r} reference {r!r} |diff| {abs(g - r):.3e}")
            assert abs(g - r) <= SSIM_TOL, (where, name, g, r)


# ------------------------------------------------------------------------------------------------ 1. the kernel
_SHAPE_CASES = sorted({c[:4] for c in SC.CASES}, key=lambda c: (c[1], c[2], c[3], c[0]))


@pytest.mark.parametrize("flags,h,w,chroma", _SHAPE_CASES, ids=lambda v: str(v))
def test_kernel_equals_the_reference_over_the_table(flags, h, w, chroma):
    from bin_amd import ops
    for content in SC.CONTENTS:
        case = (flags, h, w, chroma, content)
        assert case in SC.CASES
        a, b = SC.payloads(h, w, chroma, content)
        da, db = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
        got = ops.read_plane_scores(_record(da, db, h, w, chroma, flags).cpu())
        want = SC.reference(case)
        _assert_scores(got, want, SC.case_id(case))
        if content == "constant" and flags != SC.NONE:
            assert want[7] == 1.0 and (flags != SC.BOTH or want[6] == 1.0), "constant planes: the reference's SSIM is exactly 1"
        if content == "same":
            assert got[:6] == (0,) * 6
            assert ops.read_plane_scores(_record(da, da, h, w, chroma, flags).cpu())[:6] == (0,) * 6, "a == b, the same memory"
        if content == "extremes":
            n, ch, cw = SC.frame_bytes(h, w, chroma)
            assert got[:6] == (65025 * h * w, 65025 * ch * cw, 65025 * ch * cw, 255 * h * w, 255 * ch * cw, 255 * ch * cw)


def test_table_is_the_issues():
    shapes = {(f, h, w) for f, h, w, _, _ in SC.CASES}
    assert {(SC.NONE, 1, 1), (SC.NONE, 2, 2), (SC.NONE, 3, 5), (SC.NONE, 5, 3), (SC.NONE, 7, 16), (SC.U7, 7, 16), (SC.U7, 7, 7), (SC.U7, 9, 10),
            (SC.BOTH, 11, 11), (SC.BOTH, 12, 13), (SC.BOTH, 16, 246), (SC.BOTH, 17, 247), (SC.BOTH, 33, 493)} == shapes
    assert {c[3] for c in SC.CASES} == {420, 444} and {c[4] for c in SC.CASES} == {"random", "same", "constant", "extremes"}
    assert len(SC.CASES) == 13 * 2 * 4
    assert SC.frame_bytes(33, 493, 420)[1:] == (SC.TILE_ROWS + 1, SC.TILE_COLS + 1)


def test_small_frames_and_ssim_requests():
    from bin_amd import ops
    a = torch.zeros(SC.frame_bytes(6, 9, 420)[0], dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="7 x 7"):
        ops.payload_scores(a, a, 6, 9, 420)
    got = ops.read_plane_scores(ops.payload_scores(a, a, 6, 9, 420, ssim=False).cpu())
    assert got[:6] == (0,) * 6 and math.isnan(got[6]) and math.isnan(got[7])
    with pytest.raises(ValueError):
        ops.payload_scores(a, a, 6, 9, 422)
    with pytest.raises(ValueError):
        ops.payload_scores(a[:-1], a[:-1], 6, 9, 420)
    with pytest.raises(ValueError):
        ops.payload_scores(a, a, 6, 9, 420, ssim=False, out=torch.zeros(32, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="downloaded"):
        ops.read_plane_scores(ops.payload_scores(a, a, 6, 9, 420, ssim=False))


@pytest.mark.parametrize("h,w,chroma", [(17, 247, 420), (12, 13, 444), (33, 493, 420)])
def test_any_byte_offset_gives_the_same_record_and_nothing_else_is_written(h, w, chroma):
    """The payloads as views at byte offsets 0, 1 and 3 of a guarded buffer, the workspace and the record guarded too (the library is
    called directly, with a workspace of exactly the bytes it asks for)."""
    from bin_amd import _lib, ops
    from bin_amd.utils.util import _gauss_taps
    lib = _lib.scorelib()
    taps = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    flags = _lib.PLANE_SSIM_G11 | _lib.PLANE_SSIM_U7
    n, ch, cw = SC.frame_bytes(h, w, chroma)
    a, b = SC.payloads(h, w, chroma, "random")
    nb = lib.binscore_workspace_bytes(h, w, chroma, flags)
    assert nb > 0 and nb % 64 == 0
    records = []
    for off_a, off_b in ((0, 0), (1, 0), (0, 3), (3, 1)):
        bufs = []
        for src, off in ((a, off_a), (b, off_b)):
            buf = torch.full((n + 256 + off,), GUARD, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 256 == 0
            buf[128 + off:128 + off + n].copy_(torch.from_numpy(src.copy()))
            bufs.append((buf, 128 + off))
        ws = torch.full((nb + 256,), GUARD, dtype=torch.uint8, device="cuda")
        rec = torch.full((64 + 256,), GUARD, dtype=torch.uint8, device="cuda")
        ptrs = []
        for buf, lo in bufs:
            p = buf.data_ptr() + lo
            ptrs += [p, p + h * w, p + h * w + ch * cw]
        rc = lib.binscore_planes(*ptrs, h, w, chroma, flags, taps, ws.data_ptr() + 128, nb, rec.data_ptr() + 128,
                                 torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        for (buf, lo), src in zip(bufs, (a, b)):
            host = buf.cpu().numpy()
            assert (host[:lo] == GUARD).all() and (host[lo + n:] == GUARD).all() and np.array_equal(host[lo:lo + n], src), "a payload written"
        hws, hrec = ws.cpu().numpy(), rec.cpu().numpy()
        assert (hws[:128] == GUARD).all() and (hws[128 + nb:] == GUARD).all(), "guard bytes around the workspace"
        assert (hrec[:128] == GUARD).all() and (hrec[192:] == GUARD).all(), "guard bytes around the record"
        records.append(hrec[128:192].tobytes())
    assert len(set(records)) == 1, "every offset gives the same 64 bytes"
    _assert_scores(ops.read_plane_scores(np.frombuffer(records[0], np.uint8)), SC.reference_scores(a, b, h, w, chroma, SC.BOTH), (h, w, chroma))
    # through ops, as views of one buffer: the same record
    buf = torch.zeros(n + 3, dtype=torch.uint8, device="cuda")
    buf[3:].copy_(torch.from_numpy(a.copy()))
    db = torch.from_numpy(b.copy()).cuda()
    assert ops.payload_scores(buf[3:], db, h, w, chroma).cpu().numpy().tobytes() == records[0]
    y, u, v = buf[3:3 + h * w], buf[3 + h * w:3 + h * w + ch * cw], buf[3 + h * w + ch * cw:]
    assert ops.payload_scores((y, u, v), db, h, w, chroma).cpu().numpy().tobytes() == records[0], "a (y, u, v) triple"


def test_two_calls_into_one_record_leave_the_second_and_a_repeat_gives_the_same_bytes():
    from bin_amd import ops
    h, w, chroma = 17, 247, 420
    a, b = (torch.from_numpy(x.copy()).cuda() for x in SC.payloads(h, w, chroma, "random"))
    z, f = (torch.from_numpy(x.copy()).cuda() for x in SC.payloads(h, w, chroma, "extremes"))
    rec = torch.empty(64, dtype=torch.uint8, device="cuda")
    assert ops.payload_scores(z, f, h, w, chroma, out=rec) is rec
    ops.payload_scores(a, b, h, w, chroma, out=rec)
    second = rec.cpu().numpy().tobytes()
    fresh = ops.payload_scores(a, b, h, w, chroma).cpu().numpy().tobytes()
    assert second == fresh, "the second call's values, nothing of the first"
    ops.payload_scores(a, b, h, w, chroma, ssim=False, out=rec)
    got = ops.read_plane_scores(rec.cpu())
    assert math.isnan(got[6]) and math.isnan(got[7]) and got[:6] == ops.read_plane_scores(np.frombuffer(fresh, np.uint8))[:6]
    for _ in range(3):
        assert ops.payload_scores(a, b, h, w, chroma).cpu().numpy().tobytes() == fresh, "two calls give the same bits"


# ------------------------------------------------------------------------------------------------ 2. interpolate_video(gt=...)
H, W, CHROMA, T = 24, 40, 420, 4                       # the frame of tests/test_gpu_chain.py: pads to 128 x 128


@functools.lru_cache(maxsize=None)
def _net():
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval()                                   # default precision


@functools.lru_cache(maxsize=None)
def _stream():
    from bin_amd import video
    return video.parse_header(CC.clip_header(H, W, CHROMA)), torch.from_numpy(CC.clip(H, W, CHROMA, T))


@functools.lru_cache(maxsize=None)
def _gt():
    """A ground truth long enough for every case below: the pattern of the clip at eight times its frame count, shifted."""
    return torch.from_numpy(CC.clip(H, W, CHROMA, 8 * T)[::-1].copy())


@functools.lru_cache(maxsize=None)
def _plain(**kw):
    from bin_amd import harness
    header, payloads = _stream()
    return harness.interpolate_video(_net(), payloads, header, **dict(kw))


_SCORED = {}


def _scored(gt, **kw):
    """(out, rows) of the clip scored against `gt`; the runs against the whole ground truth are shared between the tests."""
    from bin_amd import harness
    header, payloads = _stream()
    key = tuple(sorted(kw.items())) if gt is _gt() else None
    if key is None or key not in _SCORED:
        result = harness.interpolate_video(_net(), payloads, header, gt=gt, **kw)
        if key is None:
            return result
        _SCORED[key] = result
    return _SCORED[key]


def _rows_by_hand(out, gt, stride, offset):
    from bin_amd import ops
    rows = []
    for m in range(out.shape[0]):
        rec = ops.payload_scores(out[m], gt[stride * m + offset].cuda(), H, W, CHROMA)
        rows.append((m, stride * m + offset) + ops.read_plane_scores(rec.cpu()))
    return rows


def _same_rows(got, want):
    """Equal rows, NaN fields equal to NaN fields (bit for bit: the same kernel on the same bytes)."""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert np.array(g[-2:], np.float64).tobytes() == np.array(w[-2:], np.float64).tobytes() and tuple(g[:-2]) == tuple(w[:-2]), (g, w)


@pytest.mark.parametrize("factor,stride,offset", [(2, 1, 0), (2, 2, 1), (4, 1, 2), (4, 2, 3)])
def test_rows_equal_payload_scores_by_hand_and_the_bytes_do_not_change(factor, stride, offset):
    from bin_amd import score
    out, rows = _scored(_gt(), factor=factor, gt_stride=stride, gt_offset=offset)
    assert torch.equal(out, _plain(factor=factor)), "`out` with gt= is byte-identical to `out` without it"
    assert out.shape[0] == factor * (T - 1) == len(rows)
    want = _rows_by_hand(out, _gt(), stride, offset)
    _same_rows([r[:2] + r[3:] for r in rows], want)
    assert [r[2] for r in rows] == [score.frame_class(m, factor) for m in range(len(rows))]
    assert all(r[3] > 0 for r in rows) and all(-1 <= r[-1] < 1 and -1 <= r[-2] < 1 for r in rows), "real scores of real frames"


def test_frames_past_the_end_of_the_ground_truth_are_not_scored():
    out, rows = _scored(_gt()[:8], factor=2, gt_stride=2, gt_offset=1)       # output frame m needs frame 2 m + 1: m <= 3
    assert torch.equal(out, _plain(factor=2)) and [r[0] for r in rows] == [0, 1, 2, 3] and [r[1] for r in rows] == [1, 3, 5, 7]
    _same_rows([r[:2] + r[3:] for r in rows], _rows_by_hand(out, _gt(), 2, 1)[:4])


def test_a_held_frame_is_its_own_class():
    out, rows = _scored(_gt(), factor=2, scene_cut=(2,))
    assert torch.equal(out, _plain(factor=2, scene_cut=(2,)))
    assert [r[2] for r in rows] == ["deblurred", "interp_L1", "deblurred", "held", "deblurred", "interp_L1"]
    assert torch.equal(out[3], out[2]), "the held frame is the payload before it"
    _same_rows([r[:2] + r[3:] for r in rows], _rows_by_hand(out, _gt(), 1, 0))


def test_rows_at_an_output_rate_are_one_class():
    out, rows = _scored(_gt(), rate=(75, 1), gt_stride=1, gt_offset=1)       # rho 5/2 on the factor-4 stream
    assert torch.equal(out, _plain(rate=(75, 1))) and len(rows) == out.shape[0] > 4
    assert {r[2] for r in rows} == {"all"}
    _same_rows([r[:2] + r[3:] for r in rows], _rows_by_hand(out, _gt(), 1, 1))


# ------------------------------------------------------------------------------------------------ 3. the entry point
DRIVER = """\
import json, sys
from bin_amd import test as T
opt, out_json, src, gt, plain, scored, log = sys.argv[1:8]
base = ["--opt", opt, "--input_video", src]
assert T.main(base + ["--output_video", plain]) == 0
stats = {}
assert T.main(base + ["--output_video", scored, "--gt_video", gt, "--gt_offset", "1", "--score_log", log], stats) == 0
json.dump({"rows": stats["scores"]["rows"], "summary": stats["scores"]["summary"], "stride": stats["scores"]["stride"],
           "frames_out": stats["frames_out"]}, open(out_json, "w"))
"""


def test_cli_gt_video_equals_the_harness_and_writes_the_same_stream(tmp_path):
    from bin_amd import score, video
    from bin_amd.weights import reference_state_dict
    from host_fixtures import OPTION_YML
    header, payloads = _stream()
    src, gt_path = str(tmp_path / "in.y4m"), str(tmp_path / "gt.y4m")
    with video.Y4MWriter(src, header) as wr:
        for p in payloads:
            wr.write(p.numpy())
    with video.Y4MWriter(gt_path, header.multiplied(4)) as wr:             # twice the output's rate: stride 2
        for p in _gt():
            wr.write(p.numpy())
    weights = str(tmp_path / "w.pth")
    torch.save(reference_state_dict(0), weights)
    yml = str(tmp_path / "opt.yml")
    open(yml, "w").write(OPTION_YML.replace("/tmp/bin_amd_runs", str(tmp_path)).replace("~/w/adobe_bin.pth", weights)
                         .replace("name: debug_host", "name: adobe_stage4"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out_json, plain, scored, log = (str(tmp_path / n) for n in ("stats.json", "plain.y4m", "scored.y4m", "scores.tsv"))
    run = subprocess.run([sys.executable, "-c", DRIVER, yml, out_json, src, gt_path, plain, scored, log], stdin=subprocess.DEVNULL,
                         stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path), env=env, timeout=240)
    err = run.stderr.decode(errors="replace")
    assert run.returncode == 0, err[-3000:]
    assert run.stdout == b"", "the table goes to the log, never to stdout"
    assert open(plain, "rb").read() == open(scored, "rb").read(), "the written stream does not change with --gt_video"
    out, rows = _scored(_gt(), factor=2, gt_stride=2, gt_offset=1)
    frames = [bytes(p) for p in video.Y4MReader(scored)]
    assert frames == [p.tobytes() for p in out.cpu().numpy()]
    stats = json.load(open(out_json))
    assert stats["stride"] == 2 and stats["frames_out"] == len(rows) == 2 * (T - 1)
    logged = score.read_log(log)
    _same_rows(logged, rows)
    _same_rows([tuple(r) for r in stats["rows"]], rows)
    assert open(log).readline().rstrip("\n").split("\t") == list(score.LOG_COLUMNS)
    ch, cw = header.chroma_size
    tally = score.Tally(H * W, ch * cw)
    for r in rows:
        tally.add(r)
    want = tally.summary()
    assert stats["summary"]["overall"]["n"] == len(rows) and stats["summary"]["unscored"] == 0
    assert stats["summary"]["overall"]["psnr_y"] == want["overall"]["psnr_y"] and stats["summary"]["deblurred"] == want["deblurred"]
    assert "interp_L1" in err and "psnr_yuv" in err, "the per-class table is in the log"
