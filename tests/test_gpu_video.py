"""GPU: the video path — binyuv_to_frame / binyuv_from_frame (include/binyuv.h) over the case table of video_cases.py against its
float64 restatement (YUV -> frame within 2^-20 on every element, pads included; frame -> YUV equal on every byte of tie-free inputs),
both data paths in bits, the guards, the exact round trip over every in-gamut code point; harness.interpolate_video against the
generator driven by hand; `python -m bin_amd.test --input_video` in a child process, file to file and pipe to pipe.
CPU side: test_cpu_video.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import video_cases as VC
from conftest import REPO

pytestmark = pytest.mark.gpu

FORMATS = VC.MATRIX_RANGE


def _dev(a, offset=0, guard=0):
    """`a` (numpy) on the device at `offset` elements past a 256-byte boundary, with `guard` guard elements on both sides; returns
    (view, whole buffer)."""
    a = np.ascontiguousarray(a)
    fill = VC.GUARD if a.dtype == np.uint8 else -7.0
    host = np.full(a.size + 2 * guard + offset, fill, a.dtype)
    host[guard + offset:guard + offset + a.size] = a.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    return buf[guard + offset:guard + offset + a.size].view(*a.shape), buf


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _planes_dev(payload, h, w, chroma):
    """Three separately allocated (aligned) plane tensors."""
    return tuple(torch.from_numpy(np.ascontiguousarray(p).reshape(-1)).cuda() for p in VC.split_planes(payload, h, w, chroma))


# ------------------------------------------------------------------------------------------------ 1. YUV -> frame
@pytest.mark.parametrize("h,w,chroma", VC.CASES, ids=VC.CASE_IDS)
def test_to_frame_against_float64_with_pads_and_both_data_paths(h, w, chroma):
    from bin_amd import ops
    worst = 0.0
    payloads = {"random": VC.random_payload(h, w, chroma, 100 * h + w), "ramp": VC.ramp_payload(h, w, chroma, step=7, start=h)}
    for kind, payload in payloads.items():
        contiguous = _dev(payload)[0]                       # U and V at H*W and H*W + ch*cw: misaligned for odd sizes by themselves
        shifted = _dev(payload, offset=1)[0]                # every plane off a dword boundary: the byte path whatever the size
        planes = _planes_dev(payload, h, w, chroma)         # every plane aligned: the dword path when W and the pads allow it
        assert contiguous.data_ptr() % 16 == 0 and shifted.data_ptr() % 4 == 1 and all(p.data_ptr() % 16 == 0 for p in planes)
        for pads in VC.pads_of(h, w):
            l, r, t, b = pads
            for matrix, rng in FORMATS:
                fmt = (chroma, matrix, rng)
                want = VC.to_frame_ref(payload, h, w, fmt, pads)
                got = [ops.yuv_to_frame(src, h, w, fmt, pads) for src in (contiguous, shifted, planes)]
                got = [g.cpu().numpy()[0] for g in got]
                assert got[0].shape == want.shape == (3, h + t + b, w + l + r) and got[0].dtype == np.float32
                err = float(np.abs(got[0].astype(np.float64) - want).max())
                worst = max(worst, err)
                assert err <= VC.TO_FRAME_BAR, (kind, pads, fmt, err)
                interior = got[0][:, t:t + h, l:l + w]
                assert np.array_equal(_bits(got[0]), _bits(np.pad(interior, ((0, 0), (t, b), (l, r)), mode="edge"))), "replicate pad, in bits"
                assert np.array_equal(_bits(got[1]), _bits(got[0])) and np.array_equal(_bits(got[2]), _bits(got[0])), "fast == slow"
    print(f"[video] to_frame {h}x{w} {chroma}: max err {worst:.3e} = {worst / VC.TO_FRAME_BAR:.3f} of the bar {VC.TO_FRAME_BAR:.3e}")


# ------------------------------------------------------------------------------------------------ 2. frame -> YUV
@pytest.mark.parametrize("h,w,chroma", VC.CASES, ids=VC.CASE_IDS)
def test_from_frame_equals_float64_on_every_byte_with_guards_and_both_data_paths(h, w, chroma):
    from bin_amd import ops
    n = VC.frame_bytes(h, w, chroma)
    for l, r, t, b in VC.crops_of(h, w):
        shape = (h + t + b, w + l + r)
        for matrix, rng in FORMATS:
            fmt = (chroma, matrix, rng)
            frame, share = VC.safe_rgb_frame(shape, fmt, seed=7 * h + w, crop=(t, l, h, w))
            want = torch.from_numpy(VC.from_frame_ref(frame, t, l, h, w, fmt))
            aligned = _dev(frame[None])[0]
            shifted = _dev(frame[None], offset=1)[0]            # 4 bytes past a 16-byte boundary: the single-float path
            assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
            # the payload in a guarded buffer, dword-aligned and not; and three separately aligned planes
            for x in (aligned, shifted):
                for offset in (0, 1):
                    out, whole = _dev(np.zeros(n, np.uint8), offset=offset, guard=16)
                    assert out.data_ptr() % 4 == offset
                    assert ops.frame_to_yuv(x, t, l, h, w, fmt, out=out) is out
                    whole = whole.cpu()
                    assert torch.equal(whole[16 + offset:16 + offset + n], want), (fmt, (t, l), offset, share)
                    assert (whole[:16 + offset] == VC.GUARD).all() and (whole[16 + offset + n:] == VC.GUARD).all(), "guard bytes written"
            planes = _planes_dev(np.zeros(n, np.uint8), h, w, chroma)
            ops.frame_to_yuv(aligned, t, l, h, w, fmt, out=planes)
            assert torch.equal(torch.cat(planes).cpu(), want)
            fresh = ops.frame_to_yuv(aligned[0], t, l, h, w, fmt)
            assert fresh.dtype == torch.uint8 and fresh.shape == (n,) and torch.equal(fresh.cpu(), want)


def test_from_frame_nan_and_infinities_land_where_the_clamp_puts_them():
    from bin_amd import ops
    for chroma in VC.CHROMAS:
        for matrix, rng in FORMATS:
            fmt = (chroma, matrix, rng)
            x = np.full((3, 4, 8), 0.5, np.float32)
            x[0, 1, 2], x[1, 1, 2], x[2, 1, 2] = np.nan, -np.inf, np.inf          # -> (0, 0, 1)
            x[0, 2, 5], x[1, 2, 5], x[2, 2, 5] = np.inf, np.nan, -np.inf          # -> (1, 0, 0)
            x[:, 3, 7] = np.nan                                                   # -> black
            x[:, 0, 0] = np.inf                                                   # -> white
            clean = x.copy()
            clean[:, 1, 2], clean[:, 2, 5], clean[:, 3, 7], clean[:, 0, 0] = (0, 0, 1), (1, 0, 0), 0, 1
            want = VC.from_frame_ref(clean, 0, 0, 4, 8, fmt)
            assert np.array_equal(VC.from_frame_ref(x, 0, 0, 4, 8, fmt), want)
            for src in (_dev(x[None])[0], _dev(x[None], offset=1)[0]):
                assert np.array_equal(ops.frame_to_yuv(src, 0, 0, 4, 8, fmt).cpu().numpy(), want), fmt


def test_wrappers_refuse_before_any_launch():
    from bin_amd import ops
    fmt = (420, "bt601", "limited")
    payload = torch.zeros(VC.frame_bytes(6, 10, 420), dtype=torch.uint8, device="cuda")
    frame = torch.zeros(1, 3, 12, 16, device="cuda")
    for bad in (payload[:-1], payload.view(2, -1), payload.to(torch.int8), (payload[:60], payload[60:75])):
        with pytest.raises(ValueError):
            ops.yuv_to_frame(bad, 6, 10, fmt, (0, 0, 0, 0))
    for crop in ((7, 0, 6, 10), (0, 7, 6, 10), (-1, 0, 6, 10), (0, 0, 0, 10)):
        with pytest.raises(ValueError):
            ops.frame_to_yuv(frame, *crop, fmt)
    with pytest.raises(ValueError):
        ops.frame_to_yuv(frame, 0, 0, 6, 10, fmt, out=payload[:-1])
    with pytest.raises(ValueError):
        ops.frame_to_yuv(torch.zeros(2, 3, 12, 16, device="cuda"), 0, 0, 6, 10, fmt)
    with pytest.raises(RuntimeError, match="bad argument"):               # the library's own refusal: the output inside the input
        ops.frame_to_yuv(frame, 0, 0, 6, 10, fmt, out=frame.view(-1).view(torch.uint8)[:payload.numel()])
    torch.cuda.synchronize()
    assert not frame.any() and not payload.any(), "nothing was launched"


# ------------------------------------------------------------------------------------------------ 3. the round trip
@functools.lru_cache(maxsize=None)
def _codes(matrix, rng):
    return VC.in_gamut_codes(matrix, rng)


def _round_trip(payload, h, w, fmt, pads):
    from bin_amd import ops
    l, r, t, b = pads
    src = torch.from_numpy(payload).cuda()
    frame = ops.yuv_to_frame(src, h, w, fmt, pads)
    back = ops.frame_to_yuv(frame, t, l, h, w, fmt)
    return frame, bool(torch.equal(back, src))


@pytest.mark.parametrize("matrix,rng", FORMATS)
def test_every_in_gamut_code_point_round_trips_on_the_device(matrix, rng):
    """YUV -> frame -> YUV returns the input bytes for every code point whose unclamped RGB lies in [0, 1]: as one 4:4:4 frame and as
    block-constant 4:2:0 frames (replication up, box mean down), without pads and through the pad_sizes pads and the matching crop."""
    codes = _codes(matrix, rng)
    cw = 2048
    ch = -(-len(codes) // cw)
    grid = np.resize(codes, (ch * cw, 3)).reshape(ch, cw, 3)            # (the tail repeats the first code points)
    p444 = np.concatenate([grid[..., k].reshape(-1) for k in range(3)])
    y420 = np.repeat(np.repeat(grid[..., 0], 2, 0), 2, 1)
    p420 = np.concatenate([y420.reshape(-1), grid[..., 1].reshape(-1), grid[..., 2].reshape(-1)])
    for chroma, payload, (h, w) in ((444, p444, (ch, cw)), (420, p420, (2 * ch, 2 * cw))):
        fmt = (chroma, matrix, rng)
        for pads in ((0, 0, 0, 0), tuple(VC.pad_sizes(h, w))):
            frame, same = _round_trip(payload, h, w, fmt, pads)
            assert same, (fmt, pads)
            if chroma == 444 and pads == (0, 0, 0, 0):                  # and the frame itself against float64, every code point
                want = VC.yuv_to_rgb(grid[..., 0], grid[..., 1], grid[..., 2], matrix, rng)
                err = float(np.abs(frame[0].cpu().numpy().astype(np.float64) - want).max())
                print(f"[video] to_frame {matrix} {rng}: {len(codes)} in-gamut code points, max err {err:.3e} = "
                      f"{err / VC.TO_FRAME_BAR:.3f} of the bar")
                assert err <= VC.TO_FRAME_BAR
    # odd sizes: an odd edge and an odd corner average 2 and 1 pixels of a block-constant frame, still exact
    h, w = 33, 131
    sub = codes[:: len(codes) // (17 * 66)][:17 * 66].reshape(17, 66, 3)
    y = np.repeat(np.repeat(sub[..., 0], 2, 0), 2, 1)[:h, :w]
    payload = np.concatenate([y.reshape(-1), sub[..., 1].reshape(-1), sub[..., 2].reshape(-1)])
    for pads in ((0, 0, 0, 0), (1, 2, 3, 0), tuple(VC.pad_sizes(h, w))):
        assert _round_trip(payload, h, w, (420, matrix, rng), pads)[1], pads


# ------------------------------------------------------------------------------------------------ 4. interpolate_video
@functools.lru_cache(maxsize=None)
def _net(prec):
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval().set_precision(prec)


CLIP_HEADER = b"YUV4MPEG2 W40 H24 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"


@functools.lru_cache(maxsize=None)
def _clip(T=5):
    """A smooth moving pattern (in gamut, unlike random bytes): [T, frame_bytes] uint8 payloads of a 40x24 4:2:0 stream."""
    from bin_amd import video
    header = video.parse_header(CLIP_HEADER)
    yy, xx = np.mgrid[0:24, 0:40]
    cy, cx = np.mgrid[0:12, 0:20]
    frames = []
    for k in range(T):
        Y = 110 + 70 * np.sin(0.31 * (xx + 2 * k)) * np.cos(0.23 * yy) + 8 * ((xx // 5 + yy // 4 + k) % 2)
        U = 128 + 30 * np.sin(0.4 * (cx - k))
        V = 128 + 30 * np.cos(0.35 * (cy + k))
        frames.append(np.concatenate([np.rint(p).astype(np.uint8).reshape(-1) for p in (Y, U, V)]))
    return header, torch.from_numpy(np.stack(frames))


def _by_hand(net, header, payloads, fmt, group=None):
    """The 2(T-1) output payloads from the generator driven by hand on yuv_to_frame frames."""
    import ensemble_cases as EC
    from bin_amd import harness, ops
    T, h, w = payloads.shape[0], header.height, header.width
    pads = VC.pad_sizes(h, w)
    l, r, t, b = pads
    assert (h + t + b, w + l + r) == (128, 128)
    padded = [ops.yuv_to_frame(payloads[i].cuda(), h, w, fmt, pads) for i in range(T)]
    out = []
    with torch.no_grad():
        for i in range(T - 1):
            inputs = [padded[j] for j in harness.window_frame_ids(i, T)]
            Ft_p = net(*inputs) if group is None else EC.by_hand(net, inputs, group)
            slots = (8, 13, 12) if i == 0 else ((13, 12) if i < T - 2 else (13,))
            out += [ops.frame_to_yuv(Ft_p[k], t, l, h, w, fmt) for k in slots]
    return torch.stack(out)


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_interpolate_video_equals_the_generator_driven_by_hand(prec):
    from bin_amd import harness
    header, payloads = _clip()
    net = _net(prec)
    fmt = (420, "bt601", "full")                        # auto: 40x24 -> bt601, XCOLORRANGE=FULL -> full
    want = _by_hand(net, header, payloads, fmt)
    got = harness.interpolate_video(net, payloads, header)
    assert got.shape == (8, header.frame_bytes) and got.dtype == torch.uint8 and got.is_cuda
    assert torch.equal(got, want)
    assert len({bytes(p.cpu().numpy()) for p in got}) == 8, "eight different frames"
    assert torch.equal(harness.interpolate_video(net, payloads.cuda(), header, reuse_stage1=False), want)
    assert torch.equal(harness.interpolate_video(net, payloads, header, batch=2), want)
    other = harness.interpolate_video(net, payloads, header, matrix="bt709", range="limited")
    assert torch.equal(other, _by_hand(net, header, payloads, (420, "bt709", "limited"))) and not torch.equal(other, want)
    with pytest.raises(ValueError, match="at least 2 frames"):
        harness.interpolate_video(net, payloads[:1], header)
    with pytest.raises(ValueError):
        harness.interpolate_video(net, payloads[:, :-1], header)


def test_interpolate_video_with_an_ensemble_equals_self_ensemble_driven_by_hand():
    from bin_amd import harness
    header, payloads = _clip()
    net = _net("f16x3")
    want = _by_hand(net, header, payloads, (420, "bt601", "full"), group="h")
    assert torch.equal(harness.interpolate_video(net, payloads, header, ensemble="h"), want)
    assert not torch.equal(want, _by_hand(net, header, payloads, (420, "bt601", "full")))


# ------------------------------------------------------------------------------------------------ 5. the entry point
DRIVER = """\
import sys
from bin_amd import test as T
common = ["--opt", sys.argv[1], "--precision", "f16x3"]
assert T.main(common + ["--input_video", sys.argv[2], "--output_video", sys.argv[3]]) == 0      # file to file
assert T.main(common + ["--input_video", "-", "--output_video", "-"]) == 0                      # stdin to stdout
"""


def test_cli_video_file_to_file_and_pipe_to_pipe_in_a_child_process(tmp_path):
    """One fresh child process runs the entry point twice: file to file, then from its stdin (a file object standing in for a pipe)
    to its stdout.  Nothing but the second run's stream may reach stdout, so the captured stdout is byte-identical to the file."""
    from bin_amd import harness, video
    from bin_amd.weights import reference_state_dict
    from host_fixtures import OPTION_YML
    header, payloads = _clip()
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out" / "out.y4m")
    with video.Y4MWriter(src, header) as wr:
        for p in payloads:
            wr.write(p.numpy())
    weights = str(tmp_path / "w.pth")
    torch.save(reference_state_dict(0), weights)
    yml = str(tmp_path / "opt.yml")
    open(yml, "w").write(OPTION_YML.replace("/tmp/bin_amd_runs", str(tmp_path)).replace("~/w/adobe_bin.pth", weights)
                         .replace("name: debug_host", "name: adobe_stage4"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    with open(src, "rb") as stdin:
        run = subprocess.run([sys.executable, "-c", DRIVER, yml, src, dst], stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                             cwd=str(tmp_path), env=env, timeout=240)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    data = open(dst, "rb").read()
    assert run.stdout == data, "stdout carries the stream and nothing else"
    assert b"In video:" in run.stderr and b"frames in: 5  out: 8" in run.stderr, "logging goes to stderr"
    logs = [f for f in os.listdir(tmp_path / "out") if f.endswith(".log")]
    assert logs and "frames in: 5  out: 8" in open(tmp_path / "out" / logs[0]).read()
    rd = video.Y4MReader(dst)
    assert rd.header == header.doubled() and rd.header.rate == (60, 1) and rd.header.line() == CLIP_HEADER.replace(b"F30:1", b"F60:1")
    frames = [bytes(p) for p in rd]
    want = harness.interpolate_video(_net("f16x3"), payloads, header).cpu().numpy()
    assert len(frames) == 2 * (payloads.shape[0] - 1) == 8
    assert all(f == w.tobytes() for f, w in zip(frames, want))
