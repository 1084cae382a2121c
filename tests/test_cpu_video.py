"""CPU: what can be pinned about the video path (bin_amd/video.py, include/binyuv.h) without a device — Y4M header and stream
handling, the numpy restatement of the conversion (video_cases.py: exact in-gamut round trip in float64 and in fp32, and the
tie-free inputs on which fp32 and float64 agree on every byte), the ABI bookkeeping of libbinyuv.so, and every refusal that comes
before a launch.  GPU side: test_gpu_video.py."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest
import torch

import video_cases as VC
from bin_amd import video as V
from conftest import REPO


# ------------------------------------------------------------------------------------------------ headers and streams
HEADERS = [
    (b"YUV4MPEG2 W40 H24 F30:1 Ip A1:1 C420jpeg XYSCSS=420JPEG", 420, None),
    (b"YUV4MPEG2 W1280 H720 F30000:1001 Ip A1:1 C420mpeg2 XCOLORRANGE=LIMITED", 420, False),
    (b"YUV4MPEG2 W33 H17 F25:1 Ip A128:117 C420paldv XCOLORRANGE=FULL XFOO=bar", 420, True),
    (b"YUV4MPEG2 W5 H3 F24:1 C420", 420, None),
    (b"YUV4MPEG2 W5 H3 F24:1", 420, None),
    (b"YUV4MPEG2 W7 H9 F60:1 Ip C444 XCOLORRANGE=FULL", 444, True),
]
REFUSED = [(b"YUV4MPEG2 W4 H4 F30:1 It C420", "It"), (b"YUV4MPEG2 W4 H4 F30:1 Ib C420", "Ib"), (b"YUV4MPEG2 W4 H4 F30:1 Im", "Im"),
           (b"YUV4MPEG2 W4 H4 F30:1 C422", "C422"), (b"YUV4MPEG2 W4 H4 F30:1 Cmono", "Cmono"), (b"YUV4MPEG2 W4 H4 F30:1 C420p10", "C420p10"),
           (b"YUV4MPEG2 W4 H4 F30:1 C444p12", "C444p12"), (b"YUV4MPEG2 W4 H4 F30:1 C422p16", "C422p16"), (b"YUV4MPEG2 W4 H4 F30:1 Cmono16", "Cmono16")]


@pytest.mark.parametrize("line,chroma,full", HEADERS)
def test_header_parse_write_round_trip_and_rate_doubling(line, chroma, full):
    h = V.parse_header(line + b"\n")
    assert h.line() == line + b"\n" and V.parse_header(h.line()) == h
    assert h.chroma == chroma and h.full_range is full
    d = h.doubled()
    assert d.rate == (2 * h.rate[0], h.rate[1])
    assert (d.width, d.height, d.interlace, d.aspect, d.colorspace, d.extra) == (h.width, h.height, h.interlace, h.aspect, h.colorspace, h.extra)
    assert d.line() == line.replace(b"F%d:" % h.rate[0], b"F%d:" % (2 * h.rate[0])) + b"\n"
    assert h.frame_bytes == VC.frame_bytes(h.height, h.width, chroma)


@pytest.mark.parametrize("line,tag", REFUSED)
def test_header_refusals_name_the_tag(line, tag):
    with pytest.raises(ValueError, match=re.escape(tag) + r"\b"):
        V.parse_header(line)
    with pytest.raises(ValueError, match=re.escape(tag) + r"\b"):
        V.Y4MReader(io.BytesIO(line + b"\nFRAME\n" + bytes(24)))


def test_header_rejects_what_is_not_y4m():
    for bad in (b"RIFF W4 H4", b"YUV4MPEG2 H4 F30:1", b"YUV4MPEG2 W0 H4", b"YUV4MPEG2 W4 H4 Q1"):
        with pytest.raises(ValueError):
            V.parse_header(bad)
    with pytest.raises(ValueError):
        V.Y4MReader(io.BytesIO(b""))


def test_frame_bytes_for_odd_sizes():
    for (w, h, cs), want in (((5, 3, "420jpeg"), 15 + 2 * 2 * 3), ((1, 1, None), 3), ((3, 5, "444"), 45), ((40, 24, "420"), 1440),
                             ((130, 33, "420mpeg2"), 130 * 33 + 2 * 17 * 65)):
        hd = V.Y4MHeader(w, h, colorspace=cs)
        assert hd.frame_bytes == want and VC.frame_bytes(h, w, hd.chroma) == want


class _Pipe:
    """A non-seekable stand-in for a pipe: short reads, no readinto, and a count of what was taken from it."""

    def __init__(self, data, chunk=7):
        self.data, self.pos, self.chunk = data, 0, chunk

    def read(self, n=-1):
        n = self.chunk if n < 0 else min(n, self.chunk)
        out = self.data[self.pos:self.pos + n]
        self.pos += len(out)
        return out


def _stream(header, payloads, frame_line=b"FRAME"):
    out = io.BytesIO()
    with V.Y4MWriter(out, header) as wr:
        for p in payloads:
            wr.write(p)
    data = out.getvalue()
    return data.replace(b"FRAME\n", frame_line + b"\n") if frame_line != b"FRAME" else data


def test_reader_on_a_pipe_with_short_reads_and_frame_parameters():
    header = V.parse_header(b"YUV4MPEG2 W5 H3 F24:1 Ip C420jpeg XCOLORRANGE=FULL")
    payloads = [VC.random_payload(3, 5, 420, s).tobytes() for s in range(4)]
    assert b"FRAME" not in b"".join(payloads)
    for frame_line in (b"FRAME", b"FRAME Ip Xfoo"):
        data = _stream(header, payloads, frame_line) + b"trailing bytes of whatever follows"
        pipe = _Pipe(data)
        rd = V.Y4MReader(pipe)
        assert rd.header == header and pipe.pos == len(header.line()), "nothing past the header line is taken"
        buf = np.zeros(header.frame_bytes, np.uint8)
        for k, p in enumerate(payloads):
            assert rd.readinto(buf) and buf.tobytes() == p and rd.index == k + 1
            assert pipe.pos == len(header.line()) + (k + 1) * (len(frame_line) + 1 + header.frame_bytes), "never past what it yields"
    # a file object with readinto, a path, and iteration
    data = _stream(header, payloads)
    assert [bytes(p) for p in V.Y4MReader(io.BytesIO(data))] == payloads
    rd = V.Y4MReader(io.BytesIO(data))
    for _ in payloads:
        assert rd.readinto(bytearray(header.frame_bytes))
    assert rd.readinto(bytearray(header.frame_bytes)) is False


def test_writer_and_reader_on_paths(tmp_path):
    header = V.parse_header(b"YUV4MPEG2 W4 H2 F30:1 C444")
    payloads = [VC.ramp_payload(2, 4, 444, start=s).tobytes() for s in range(3)]
    path = str(tmp_path / "a.y4m")
    with V.Y4MWriter(path, header.doubled()) as wr:
        for p in payloads:
            wr.write(np.frombuffer(p, np.uint8))
        with pytest.raises(ValueError, match="frame 3"):
            wr.write(bytes(5))
    with V.Y4MReader(path) as rd:
        assert rd.header == header.doubled() and rd.header.rate == (60, 1)
        assert [bytes(p) for p in rd] == payloads
    assert open(path, "rb").read() == header.doubled().line() + b"".join(b"FRAME\n" + p for p in payloads)


def test_truncated_stream_names_the_frame():
    header = V.parse_header(b"YUV4MPEG2 W4 H4 F30:1 C420")
    data = _stream(header, [bytes(24), bytes(24), bytes(24)])
    rd = V.Y4MReader(_Pipe(data[:-5]))
    buf = bytearray(24)
    assert rd.readinto(buf) and rd.readinto(buf)
    with pytest.raises(ValueError, match="frame 2"):
        rd.readinto(buf)
    rd = V.Y4MReader(io.BytesIO(data[:len(header.line()) + 6 + 24 + 3]))
    assert rd.readinto(buf)
    with pytest.raises(ValueError):
        rd.readinto(buf)                                   # the stream ends inside the FRAME line
    rd = V.Y4MReader(io.BytesIO(header.line() + b"FRAMX\n" + bytes(24)))
    with pytest.raises(ValueError, match="frame 0"):
        rd.readinto(buf)


def test_resolve_format_auto_rules():
    mk = lambda w, h, extra=(): V.Y4MHeader(w, h, extra=tuple(extra))
    assert V.resolve_format(mk(1280, 720)) == (420, "bt709", "limited")
    assert V.resolve_format(mk(1279, 576)) == (420, "bt601", "limited")
    assert V.resolve_format(mk(720, 577)) == (420, "bt709", "limited")
    assert V.resolve_format(mk(40, 24, ["COLORRANGE=FULL"])) == (420, "bt601", "full")
    assert V.resolve_format(mk(40, 24, ["COLORRANGE=LIMITED"])) == (420, "bt601", "limited")
    assert V.resolve_format(mk(40, 24, ["COLORRANGE=FULL"]), "bt709", "limited") == (420, "bt709", "limited")
    assert V.resolve_format(V.Y4MHeader(4, 4, colorspace="444"), "bt601", "full") == (444, "bt601", "full")
    for bad in (("bt2020", "auto"), ("auto", "tv")):
        with pytest.raises(ValueError):
            V.resolve_format(mk(4, 4), *bad)


def test_video_slots_are_the_folder_runners_ownership_rule():
    from bin_amd import test as T
    assert [VC.video_slots(i, 4) for i in range(4)] == [(8, 13, 12), (13, 12), (13, 12), (13,)]
    assert VC.video_slots(0, 1) == (8, 13)
    for n_frames in (2, 3, 5):
        frames = [f"{8 * k:05d}.png" for k in range(n_frames)]
        names = []
        for i in range(n_frames - 1):
            interp, d0, d1 = T.output_names(frames, i)
            by_slot = {13: interp, 8: d0, 12: d1}
            names += [by_slot[k] for k in VC.video_slots(i, n_frames - 1)]
        assert names == sorted(names) and len(set(names)) == 2 * (n_frames - 1) and None not in names, "display order = name order"


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("matrix,rng", VC.MATRIX_RANGE)
def test_in_gamut_round_trip_is_exact_in_float64_and_in_float32(matrix, rng):
    codes = VC.in_gamut_codes(matrix, rng)
    assert 2_500_000 <= len(codes) <= 4_200_000, "2.6 to 4.1 million, depending on the pair"
    assert (codes == np.array(VC.SAFE_POINT, np.uint8)).all(1).any(), "SAFE_POINT is in gamut"
    n = len(codes)
    payload = np.concatenate([codes[:, 0], codes[:, 1], codes[:, 2]])
    for dtype in (np.float64, np.float32):
        frame = VC.to_frame_ref(payload, 1, n, (444, matrix, rng), (0, 0, 0, 0), dtype).astype(np.float32)
        planes = VC.prerounding(frame, 0, 0, 1, n, (444, matrix, rng), dtype)
        back = VC.from_frame_ref(frame, 0, 0, 1, n, (444, matrix, rng), dtype)
        assert np.array_equal(back, payload), (dtype, int((back != payload).sum()))
        off = max(float(np.abs(p - np.rint(p)).max()) for p in planes)
        print(f"[video] {matrix} {rng} {dtype.__name__}: {n} in-gamut code points, 0 mismatches, furthest pre-rounding value "
              f"{off:.2e} from its integer")
        assert off < 0.01, "every pre-rounding value sits half a unit from the nearest tie"
    # block-constant 4:2:0: replication up, box mean down
    sub = codes[:: max(1, n // 4096)][:4096]
    hb, wb = 2 * 64, 2 * 64
    assert len(sub) == 64 * 64
    Y = np.repeat(np.repeat(np.resize(sub[:, 0], (64, 64)), 2, 0), 2, 1)
    payload = np.concatenate([Y.reshape(-1), np.resize(sub[:, 1], 64 * 64), np.resize(sub[:, 2], 64 * 64)])
    for dtype in (np.float64, np.float32):
        frame = VC.to_frame_ref(payload, hb, wb, (420, matrix, rng), (3, 1, 2, 5), dtype).astype(np.float32)
        assert np.array_equal(VC.from_frame_ref(frame, 2, 3, hb, wb, (420, matrix, rng), dtype), payload)


@pytest.mark.parametrize("chroma", VC.CHROMAS)
@pytest.mark.parametrize("matrix,rng", VC.MATRIX_RANGE)
def test_safe_frames_make_float32_and_float64_agree_on_every_byte(matrix, rng, chroma):
    """The bar of the device test (every byte equal to the float64 restatement) is not vacuous: on safe_rgb_frame inputs an fp32
    evaluation has TIE_MARGIN = 9.8e-4 to spend and needs a few 1e-5; on the raw random draw it does not agree everywhere."""
    fmt = (chroma, matrix, rng)
    frame, share = VC.safe_rgb_frame((512, 1024), fmt, seed=5)
    finite = frame[np.isfinite(frame)]
    assert share < 0.05 and finite.size < frame.size and finite.min() < 0 and finite.max() > 1
    p64 = VC.prerounding(frame, 0, 0, 512, 1024, fmt, np.float64)
    p32 = VC.prerounding(frame, 0, 0, 512, 1024, fmt, np.float32)
    err = max(float(np.abs(a - b).max()) for a, b in zip(p32, p64))
    print(f"[video] {fmt}: replaced share {share:.4f}, fp32 pre-rounding error {err:.2e} (margin {VC.TIE_MARGIN:.2e})")
    assert err < VC.TIE_MARGIN / 8
    assert np.array_equal(VC.from_frame_ref(frame, 0, 0, 512, 1024, fmt, np.float32), VC.from_frame_ref(frame, 0, 0, 512, 1024, fmt))


def test_safe_frame_with_a_crop_and_the_specials():
    fmt = (420, "bt709", "limited")
    frame, share = VC.safe_rgb_frame((9, 14), fmt, seed=2, crop=(1, 3, 5, 7))
    assert frame.shape == (3, 9, 14) and frame.dtype == np.float32 and 0 <= share < 1
    assert np.isnan(frame).any() and np.isposinf(frame).any() and np.isneginf(frame).any()
    x = np.zeros((3, 1, 1), np.float32)
    x[:, 0, 0] = (np.nan, -np.inf, np.inf)                                     # -> (0, 0, 1): pure blue
    want = VC.from_frame_ref(np.array([0, 0, 1], np.float32).reshape(3, 1, 1), 0, 0, 1, 1, (444, "bt601", "full"))
    assert np.array_equal(VC.from_frame_ref(x, 0, 0, 1, 1, (444, "bt601", "full")), want) and list(want) == [29, 255, 107]


def test_case_table_covers_what_the_issue_names():
    assert VC.SHAPES == [(1, 1), (2, 2), (3, 5), (5, 3), (4, 4), (2, 8), (6, 10), (7, 16), (16, 64), (33, 130)]
    assert len(VC.CASES) == 20 and {c for _, _, c in VC.CASES} == {420, 444}
    assert VC.pads_of(16, 64) == [(0, 0, 0, 0), (1, 2, 3, 0), (4, 4, 2, 2), (32, 32, 56, 56)]
    assert [(t, l) for (l, r, t, b) in VC.crops_of(16, 64)] == [(0, 0), (56, 32), (1, 3)]
    assert VC.TO_FRAME_BAR == 8 * 2 * 2.0 ** -24 and len(VC.MATRIX_RANGE) == 4
    # the fp32 restatement of YUV -> frame sits well inside the bar
    for matrix, rng in VC.MATRIX_RANGE:
        p = VC.random_payload(33, 130, 444, 3)
        e = np.abs(VC.to_frame_ref(p, 33, 130, (444, matrix, rng), (1, 2, 3, 0), np.float32) - VC.to_frame_ref(p, 33, 130, (444, matrix, rng), (1, 2, 3, 0)))
        assert float(e.max()) < VC.TO_FRAME_BAR / 2


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_yuv_library_header_and_binding_agree():
    """What is binyuv's own beside the bookkeeping of test_cpu_libraries.py: the codes and constants, the format struct as the C
    compiler lays it out, and a source without switches or LDS."""
    from bin_amd import _lib
    hdr = open(os.path.join(REPO, "include", "binyuv.h")).read()
    for name, value in (("BINYUV_E_ARG", -1), ("BINYUV_E_SHAPE", -2)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1))
    assert (macro("BINYUV_CHROMA_420"), macro("BINYUV_CHROMA_444")) == (_lib.YUV_CHROMA_420, _lib.YUV_CHROMA_444) == (420, 444)
    assert (macro("BINYUV_MATRIX_BT601"), macro("BINYUV_MATRIX_BT709")) == (_lib.YUV_MATRIX_BT601, _lib.YUV_MATRIX_BT709) == (0, 1)
    assert (macro("BINYUV_RANGE_LIMITED"), macro("BINYUV_RANGE_FULL")) == (_lib.YUV_RANGE_LIMITED, _lib.YUV_RANGE_FULL) == (0, 1)
    # the struct: as the C compiler lays it out (the source asserts the size)
    assert re.search(r"typedef struct BinYuvFormat \{\s*int32_t chroma;\s*int32_t matrix;\s*int32_t range;\s*\} BinYuvFormat;", hdr)
    F = _lib.BinYuvFormat
    assert C.sizeof(F) == 12 and (F.chroma.offset, F.matrix.offset, F.range.offset) == (0, 4, 8)
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binyuv.hip")).read()
    assert "static_assert(sizeof(BinYuvFormat) == 12" in src
    assert not re.search(r"(?m)^\s*#\s*(if|ifdef|ifndef|elif|define)\b", src), "no preprocessor switches in the source"
    assert "__shared__" not in src


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.yuvlib()
    Y, U, Vp, X = 0x100000, 0x200000, 0x300000, 0x4000000
    fmt = lambda chroma=420, matrix=0, rng=0: C.byref(_lib.BinYuvFormat(chroma, matrix, rng))

    def to(y=Y, u=U, v=Vp, h=6, w=10, f=None, pads=(1, 2, 3, 0), out=X):
        return lib.binyuv_to_frame(y, u, v, h, w, f if f is not None else fmt(), *pads, out, None)

    def frm(x=X, hp=12, wp=16, top=3, left=1, h=6, w=10, f=None, y=Y, u=U, v=Vp):
        return lib.binyuv_from_frame(x, hp, wp, top, left, h, w, f if f is not None else fmt(), y, u, v, None)
    for call in (to, frm):
        for name in ("y", "u", "v"):
            assert call(**{name: None}) == -1, (call.__name__, name)
        for h, w in ((0, 10), (6, 0), (-1, 10), (6, -3)):
            assert call(h=h, w=w) == -1
        for bad in (fmt(chroma=422), fmt(chroma=0), fmt(matrix=2), fmt(matrix=-1), fmt(rng=2), fmt(rng=-1)):
            assert call(f=bad) == -1
        assert call(f=C.POINTER(_lib.BinYuvFormat)()) == -1, "a null format"
    assert to(out=None) == -1 and frm(x=None) == -1
    assert to(out=X + 2) == -1 and frm(x=X + 1) == -1, "not a float's address"
    for pads in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        assert to(pads=pads) == -1
    for kw in (dict(hp=0), dict(wp=0), dict(hp=-4), dict(top=-1), dict(left=-1), dict(top=7), dict(left=7), dict(h=13), dict(w=17),
               dict(top=2 ** 31 - 1), dict(left=2 ** 31 - 1)):
        assert frm(**kw) == -1, kw
    # element counts beyond 2^40, padded sides beyond 2^31 - 1
    big = 2 ** 31 - 1
    assert to(h=big, w=big, pads=(0, 0, 0, 0)) == -2 and to(h=2 ** 20, w=2 ** 20, pads=(0, 0, 0, 0)) == -2
    assert to(h=big, w=4, pads=(0, 0, 1, 0)) == -2 and to(h=4, w=big, pads=(0, 1, 0, 0)) == -2
    assert frm(hp=big, wp=big, top=0, left=0) == -2 and frm(hp=2 ** 20, wp=2 ** 20) == -2
    # overlaps: an output that covers an input, planes that cover each other
    assert to(out=Y - 64) == -1 and to(u=X + 16) == -1
    assert frm(y=X + 64) == -1 and frm(u=Y + 59) == -1 and frm(v=U + 14) == -1


def test_ops_refuse_cpu_tensors_and_wrong_layouts():
    from bin_amd import ops
    fmt = (420, "bt601", "limited")
    payload = torch.zeros(VC.frame_bytes(6, 10, 420), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.yuv_to_frame(payload, 6, 10, fmt, (0, 0, 0, 0))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.frame_to_yuv(torch.zeros(1, 3, 6, 10), 0, 0, 6, 10, fmt)
    for bad in ((422, "bt601", "limited"), (420, "bt2020", "limited"), (420, "bt601", "tv")):
        with pytest.raises(ValueError, match="YUV format"):
            ops.yuv_to_frame(payload, 6, 10, bad, (0, 0, 0, 0))
        with pytest.raises(ValueError, match="YUV format"):
            ops.frame_to_yuv(torch.zeros(1, 3, 6, 10), 0, 0, 6, 10, bad)
    with pytest.raises(ValueError):
        ops.yuv_to_frame(payload, 6, 10, fmt, (0, -1, 0, 0))
    with pytest.raises(ValueError):
        ops.yuv_to_frame(payload, 0, 10, fmt, (0, 0, 0, 0))
    assert ops.yuv_frame_bytes(3, 5, 420) == (27, 2, 3) and ops.yuv_frame_bytes(3, 5, 444) == (45, 3, 5)


def test_cli_video_arguments_and_their_conflicts_raise_before_the_model_is_built(monkeypatch):
    import inspect
    from bin_amd import harness, test as T
    monkeypatch.setattr(T, "create_model", lambda *a, **k: pytest.fail("the model must not be built"))
    monkeypatch.setattr(T.option, "parse", lambda *a, **k: pytest.fail("the options must not be read"))
    base = ["--opt", "c", "--input_video", "in.y4m", "--output_video", "-"]
    args = T.parse_args(base)
    assert (args.input_video, args.output_video, args.yuv_matrix, args.yuv_range, args.input_path) == ("in.y4m", "-", "auto", "auto", None)
    assert T.parse_args(base + ["--yuv_matrix", "bt709", "--yuv_range", "full"]).yuv_range == "full"
    for extra in (["--input_path", "a"], ["--output_path", "b"], ["--input_path", "a", "--output_path", "b"], ["--gt_path", "g"],
                  ["--launcher", "pytorch"]):
        with pytest.raises(ValueError):
            T.main(base + extra)
    for only in (["--input_video", "a"], ["--output_video", "b"]):
        with pytest.raises(ValueError, match="go together"):
            T.main(["--opt", "c"] + only)
    with pytest.raises(SystemExit):
        T.parse_args(base + ["--yuv_matrix", "bt2020"])
    folder = T.parse_args(["--input_path", "a", "--output_path", "b", "--opt", "c", "--gt_path", "g", "--launcher", "pytorch"])
    assert folder.input_video is None and folder.output_video is None, "the folder run's arguments are what they were"
    sig = inspect.signature(harness.interpolate_video).parameters
    assert [(k, sig[k].default) for k in ("matrix", "range", "reuse_stage1", "batch", "ensemble")] == \
        [("matrix", "auto"), ("range", "auto"), ("reuse_stage1", True), ("batch", 1), ("ensemble", None)]
    with pytest.raises(ValueError, match="at least 2 frames"):
        harness.interpolate_video(None, torch.zeros(1, 1440, dtype=torch.uint8), V.Y4MHeader(40, 24))
