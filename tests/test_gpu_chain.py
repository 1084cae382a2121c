"""GPU: the chained interpolation passes (--factor 4 | 8) — binchain_reframe (include/binchain.h) against numpy on every shape,
alignment and special value of chain_cases.py, exactly; harness.interpolate_video(factor=...) against what it promises (every second
frame of a factor is the stream of half the factor, factor 2 is today's stream, the added frames are the generator driven by hand on
frames reframed with torch), with batches, an ensemble and scene cuts; and `python -m bin_amd.test --input_video ... --factor 4` in
a child process against the harness.  CPU side: test_cpu_chain.py."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import chain_cases as CC
from conftest import REPO

pytestmark = pytest.mark.gpu

GUARD = np.float32(-777.25)
GUARD_FLOATS = 16


# ------------------------------------------------------------------------------------------------ 1. the kernel
def _values(shape, seed):
    """float32 values around [0, 1] on both sides, the specials sprinkled in (and at the corners, which the pads replicate)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.75, 1.75, size=shape).astype(np.float32)
    flat = x.reshape(-1)
    spots = rng.choice(flat.size, size=min(flat.size, 4 * len(CC.SPECIALS)), replace=False)
    flat[spots] = np.resize(np.array(CC.SPECIALS, np.float32), spots.size)
    return x


def _reframe_ref(x, top, left, h, w, pads):
    l, r, t, b = pads
    crop = x[..., top:top + h, left:left + w]
    with np.errstate(invalid="ignore"):
        crop = np.where(crop > 0, np.minimum(crop, 1), 0).astype(np.float32)
    return np.pad(crop, [(0, 0)] * (x.ndim - 2) + [(t, b), (l, r)], mode="edge")


def _arena(n_floats, offset):
    """A guard-filled device buffer and its view of n_floats floats `offset` floats past a 256-byte boundary, guards on both sides."""
    buf = torch.full((n_floats + 2 * GUARD_FLOATS + 64 + offset,), float(GUARD), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 256 == 0
    return buf, buf[64 + offset:64 + offset + n_floats]


def _run(case, n, src_off, dst_off, seed=0):
    """n items of one shape through ops.reframe, sources and destinations at the given float offsets: (outputs as numpy, expected)."""
    from bin_amd import ops
    name, planes, hs, ws, top, left, h, w, pads, _ = case
    l, r, t, b = pads
    out_shape = (planes, h + t + b, w + l + r)
    srcs, dsts, keep, want = [], [], [], []
    for i in range(n):
        x = _values((planes, hs, ws), seed + 31 * i)
        sbuf, sview = _arena(x.size, src_off)
        sview.copy_(torch.from_numpy(x).reshape(-1))
        dbuf, dview = _arena(int(np.prod(out_shape)), dst_off)
        assert sview.data_ptr() % 16 == 4 * (src_off % 4) and dview.data_ptr() % 16 == 4 * (dst_off % 4)
        srcs.append(sview.view(planes, hs, ws))
        dsts.append(dview.view(out_shape))
        keep.append((sbuf, dbuf, x))
        want.append(_reframe_ref(x, top, left, h, w, pads))
    got = ops.reframe(srcs, top, left, h, w, pads, out=dsts)
    assert all(g is d for g, d in zip(got, dsts))
    torch.cuda.synchronize()
    outs = []
    for (sbuf, dbuf, x), d in zip(keep, dsts):
        host = dbuf.cpu().numpy()
        lo = 64 + dst_off
        assert (host[:lo] == GUARD).all() and (host[lo + d.numel():] == GUARD).all(), (name, "guard floats around a destination written")
        shost = sbuf.cpu().numpy()
        assert np.array_equal(shost[64 + src_off:64 + src_off + x.size].view(np.int32), x.reshape(-1).view(np.int32)), "a source written"
        outs.append(host[lo:lo + d.numel()].reshape(out_shape))
    return outs, want


@pytest.mark.parametrize("case", CC.REFRAME_SHAPES, ids=lambda c: c[0])
def test_reframe_equals_numpy_on_both_data_paths(case):
    from bin_amd import _lib
    name, planes, hs, ws, top, left, h, w, pads, vec = case
    runs = {}
    for src_off, dst_off in ((0, 0), (1, 0), (0, 1), (3, 2)):
        outs, want = _run(case, 1, src_off, dst_off)
        assert np.array_equal(outs[0], want[0]), (name, src_off, dst_off)
        assert not np.isnan(outs[0]).any() and outs[0].min() >= 0 and outs[0].max() <= 1
        runs[(src_off, dst_off)] = outs[0]
    # (0, 0) takes the 16-byte path where the shape allows it, every other offset the 4-byte path: the same bits, zeros' signs included
    for key, out in runs.items():
        assert np.array_equal(out.view(np.int32), runs[(0, 0)].view(np.int32)), (name, key)
    shape_allows = ws % 4 == 0 and w % 4 == 0 and (w + pads[0] + pads[1]) % 4 == 0 and left % 4 == 0 and pads[0] % 4 == 0
    assert shape_allows == vec, "the table says which shapes are aligned"
    for n in (3, _lib.CHAIN_MAX_ITEMS):
        if n > 3 and planes * hs * ws > 3 * 128 * 128:
            continue                                           # (the largest shape: three items show the striding grid)
        outs, want = _run(case, n, 0, 0, seed=7)
        for i in range(n):
            assert np.array_equal(outs[i], want[i]), (name, n, i)


def test_reframe_table_covers_what_the_issue_names():
    cases = CC.REFRAME_SHAPES
    assert any(c[1:8] == (1, 1, 1, 0, 0, 1, 1) for c in cases), "1x1"
    assert any(c[9] for c in cases) and any(not c[9] for c in cases)
    assert any(c[9] and c[2] * c[3] * c[1] // 4 > 256 * 64 for c in cases), "more than one block"
    for side in range(4):
        assert any(c[8][side] == 0 and max(c[8]) > 0 for c in cases), f"a zero pad on side {side}"
    assert any(c[5] % 4 for c in cases) and any(c[4] % 4 for c in cases), "crop offsets that are no multiples of 4"
    assert {float("inf"), float("-inf")} <= set(CC.SPECIALS) and any(v != v for v in CC.SPECIALS)
    assert any(v < 0 for v in CC.SPECIALS) and any(1 < v < float("inf") for v in CC.SPECIALS)


def test_reframe_of_a_batch_tensor_and_fresh_outputs():
    from bin_amd import ops
    x = _values((2, 3, 128, 128), 5)
    dx = torch.from_numpy(x).cuda()
    pads = (44, 44, 52, 52)
    got = ops.reframe(dx, 52, 44, 24, 40, pads)
    assert got.shape == (2, 3, 128, 128) and got.data_ptr() != dx.data_ptr()
    assert np.array_equal(got.cpu().numpy(), _reframe_ref(x, 52, 44, 24, 40, pads))
    assert np.array_equal(dx.cpu().numpy().view(np.int32), x.view(np.int32)), "the input is only read"
    halves = ops.reframe([dx[0:1], dx[1:2]], 52, 44, 24, 40, pads)
    assert len(halves) == 2 and all(t.shape == (1, 3, 128, 128) for t in halves)
    assert torch.equal(torch.cat(halves, 0).view(torch.int32), got.view(torch.int32))
    with pytest.raises(RuntimeError, match="bad argument"):
        ops.reframe(dx, 52, 44, 24, 40, pads, out=dx)          # in place: a destination on its source
    with pytest.raises(ValueError):
        ops.reframe(dx, 120, 44, 24, 40, pads)                 # the crop leaves the frame
    with pytest.raises(ValueError):
        ops.reframe(dx[:, :, :, ::2], 0, 0, 24, 40, pads)      # not contiguous


# ------------------------------------------------------------------------------------------------ 2. interpolate_video(factor=...)
FORMATS = {"420": (24, 40, 420, 4), "444": (33, 47, 444, 4)}      # h, w, chroma, T: both pad to 128 x 128


@functools.lru_cache(maxsize=None)
def _net():
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval()                                   # default precision


@functools.lru_cache(maxsize=None)
def _stream(which, T=None):
    from bin_amd import video
    h, w, chroma, t = FORMATS[which]
    return video.parse_header(CC.clip_header(h, w, chroma)), torch.from_numpy(CC.clip(h, w, chroma, T or t))


@functools.lru_cache(maxsize=None)
def _out(which, factor, T=None, **kw):
    from bin_amd import harness
    header, payloads = _stream(which, T)
    out = harness.interpolate_video(_net(), payloads, header, factor=factor, **dict(kw))
    assert out.shape == (factor * (payloads.shape[0] - 1), header.frame_bytes) and out.dtype == torch.uint8 and out.is_cuda
    return out


def _fmt(header):
    return (header.chroma, "bt601", "full")                    # auto: small frames -> bt601, XCOLORRANGE=FULL -> full


@functools.lru_cache(maxsize=None)
def _level1_by_hand(which, T=None, group=None):
    """S1 = (D_0, I_0, D_1, ..., D_(T-1)) of a stream as one scene: the generator's padded fp32 outputs, driven by hand."""
    import ensemble_cases as EC
    from bin_amd import harness, ops
    from bin_amd.utils import util
    header, payloads = _stream(which, T)
    n, h, w = payloads.shape[0], header.height, header.width
    pads = util.pad_sizes(h, w)
    padded = [ops.yuv_to_frame(payloads[i].cuda(), h, w, _fmt(header), pads) for i in range(n)]
    assert tuple(padded[0].shape) == (1, 3, 128, 128)
    seq = []
    with torch.no_grad():
        for i in range(n - 1):
            inputs = [padded[j] for j in harness.window_frame_ids(i, n)]
            Ft_p = _net()(*inputs) if group is None else EC.by_hand(_net(), inputs, group)
            seq += [Ft_p[k].clone() for k in ((8, 13, 12) if i == 0 else (13, 12))]
    assert len(seq) == 2 * (n - 1) + 1
    return seq


def _reframe_torch(x, header):
    from bin_amd.utils import util
    h, w = header.height, header.width
    l, r, t, b = util.pad_sizes(h, w)
    crop = x[..., t:t + h, l:l + w].clamp(0.0, 1.0)
    return torch.nn.functional.pad(crop, (l, r, t, b), mode="replicate").contiguous()


def _added_frames_by_hand(which, seq, group=None):
    """The payloads of S2's odd frames from S1 = `seq`: slot 13 of the generator on windows of torch-reframed frames."""
    import ensemble_cases as EC
    from bin_amd import harness, ops
    from bin_amd.utils import util
    header, _ = _stream(which)
    h, w = header.height, header.width
    l, r, t, b = util.pad_sizes(h, w)
    inputs = [_reframe_torch(x, header) for x in seq]
    out = []
    with torch.no_grad():
        for j in range(len(seq) - 1):
            six = [inputs[i] for i in harness.window_frame_ids(j, len(seq))]
            Ft_p = _net()(*six) if group is None else EC.by_hand(_net(), six, group)
            out.append(ops.frame_to_yuv(Ft_p[13], t, l, h, w, _fmt(header)))
    return torch.stack(out)


@pytest.mark.parametrize("which", sorted(FORMATS))
def test_every_second_frame_of_a_factor_is_the_stream_of_half_the_factor(which):
    from bin_amd import harness
    header, payloads = _stream(which)
    today = harness.interpolate_video(_net(), payloads, header)
    out2, out4, out8 = _out(which, 2), _out(which, 4), _out(which, 8)
    assert torch.equal(out2, today), "factor 2 is today's stream"
    assert torch.equal(out4[::2], out2) and torch.equal(out8[::2], out4)
    T = payloads.shape[0]
    assert (out2.shape[0], out4.shape[0], out8.shape[0]) == (2 * (T - 1), 4 * (T - 1), 8 * (T - 1))
    assert len({bytes(p.cpu().numpy()) for p in out8}) == out8.shape[0], "all frames differ"


@pytest.mark.parametrize("which", sorted(FORMATS))
def test_added_frames_equal_the_generator_driven_by_hand_on_reframed_frames(which):
    from bin_amd import ops
    from bin_amd.utils import util
    header, _ = _stream(which)
    seq = _level1_by_hand(which)
    lo, hi = min(float(x.min()) for x in seq), max(float(x.max()) for x in seq)
    print(f"level-1 outputs of {which}: min {lo:.4f} max {hi:.4f}")
    h, w = header.height, header.width
    l, r, t, b = util.pad_sizes(h, w)
    # the hand-off kernel on real outputs against torch, bit for bit where no zero is involved
    mine = ops.reframe(seq, t, l, h, w, (l, r, t, b))
    for a, x in zip(mine, seq):
        assert torch.equal(a, _reframe_torch(x, header))
    want = _added_frames_by_hand(which, seq)
    out4 = _out(which, 4)
    assert torch.equal(out4[1::2], want)
    assert torch.equal(_out(which, 4, batch=2), out4), "batch=2 is bit-identical to batch=1"
    assert torch.equal(_out(which, 4, reuse_stage1=False), out4)


def test_added_frames_with_an_ensemble_equal_self_ensemble_driven_by_hand():
    seq = _level1_by_hand("420", group="h")
    want = _added_frames_by_hand("420", seq, group="h")
    out4 = _out("420", 4, ensemble="h")
    assert torch.equal(out4[1::2], want)
    assert torch.equal(out4[::2], _out("420", 2, ensemble="h"))
    assert not torch.equal(out4, _out("420", 4))


def test_scene_cuts_give_every_scene_as_if_it_ran_alone_and_holds():
    from bin_amd import harness
    header, payloads = _stream("420", 5)
    F, T = 4, 5
    got = harness.interpolate_video(_net(), payloads, header, factor=F, scene_cut=[2])
    assert got.shape == (F * (T - 1), header.frame_bytes)
    # scene [0, 2): its own run is F payloads (S2 without its last frame); the last frame D_1 and the holds follow.  D_1 is the
    # frame a stream of the scene and one more frame behind a cut emits at position F.
    first = harness.interpolate_video(_net(), payloads[0:2], header, factor=F)
    assert torch.equal(got[0:F], first)
    d1 = harness.interpolate_video(_net(), payloads[0:3], header, factor=2, scene_cut=[2])[2]     # today's path: D_1 before a cut
    assert torch.equal(got[F], d1)
    for pos in range(F + 1, 2 * F):
        assert torch.equal(got[pos], got[F]), "holds repeat the payload before them"
    # scene [2, 5) ends the stream: exactly its stand-alone run
    second = harness.interpolate_video(_net(), payloads[2:5], header, factor=F)
    assert torch.equal(got[2 * F:], second)
    assert not torch.equal(got, _out("420", F, 5)), "the cut changes the frames next to it"
    assert torch.equal(harness.interpolate_video(_net(), payloads, header, factor=F, scene_cut=[2], batch=2), got)
    assert torch.equal(got[::2], harness.interpolate_video(_net(), payloads, header, scene_cut=[2]))


# ------------------------------------------------------------------------------------------------ 3. the entry point
DRIVER = """\
import json, sys
from bin_amd import test as T
opt, out_json, extra = sys.argv[1], sys.argv[2], json.loads(sys.argv[3])
runs = {}
for name, src, dst in json.loads(sys.argv[4]):
    stats = {}
    assert T.main(["--opt", opt, "--input_video", src, "--output_video", dst, "--factor", "4"] + extra, stats) == 0
    runs[name] = {k: stats[k] for k in ("factor", "windows_per_pass", "frames_resident_peak", "frames_out", "windows")}
    runs[name]["cuts"] = stats.get("cuts")
json.dump(runs, open(out_json, "w"))
"""


def _cli(tmp_path, clips, extra, piped):
    """One fresh child process runs the entry point at --factor 4 on every clip of `clips` = {name: (header, payloads)}; the clip
    `piped` arrives on the child's stdin through a pipe (which cannot seek).  Returns ({name: stats}, {name: output path}, stderr)."""
    from bin_amd import video
    from bin_amd.weights import reference_state_dict
    from host_fixtures import OPTION_YML
    jobs, paths = [], {}
    for name, (header, payloads) in clips.items():
        src, dst = str(tmp_path / f"{name}.y4m"), str(tmp_path / "out" / f"{name}.y4m")
        with video.Y4MWriter(src, header) as wr:
            for p in payloads:
                wr.write(p.numpy())
        jobs.append((name, "-" if name == piped else src, dst))
        paths[name] = (src, dst)
    weights = str(tmp_path / "w.pth")
    torch.save(reference_state_dict(0), weights)
    yml = str(tmp_path / "opt.yml")
    open(yml, "w").write(OPTION_YML.replace("/tmp/bin_amd_runs", str(tmp_path)).replace("~/w/adobe_bin.pth", weights)
                         .replace("name: debug_host", "name: adobe_stage4"))
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out_json = str(tmp_path / "stats.json")
    run = subprocess.run([sys.executable, "-c", DRIVER, yml, out_json, json.dumps(extra), json.dumps(jobs)],
                         input=open(paths[piped][0], "rb").read(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path),
                         env=env, timeout=240)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    assert run.stdout == b"", "nothing reaches stdout in a run to a file"
    return json.load(open(out_json)), {name: dst for name, (_, dst) in paths.items()}, run.stderr.decode(errors="replace")


def _frames_of(path, header, factor):
    from bin_amd import video
    rd = video.Y4MReader(path)
    assert rd.header == header.multiplied(factor) and rd.header.rate == (factor * header.rate[0], header.rate[1])
    return [bytes(p) for p in rd]


def test_cli_factor_4_from_a_pipe_equals_the_harness_and_stays_resident_bounded(tmp_path):
    clips = {"t5": _stream("420", 5), "t9": _stream("420", 9)}
    stats, dst, err = _cli(tmp_path, clips, [], piped="t5")
    for name, (header, payloads) in clips.items():
        T = payloads.shape[0]
        frames = _frames_of(dst[name], header, 4)
        want = _out("420", 4, T).cpu().numpy()
        assert len(frames) == 4 * (T - 1) == want.shape[0] == stats[name]["frames_out"]
        assert all(f == w.tobytes() for f, w in zip(frames, want)), name
        assert stats[name]["factor"] == 4 and stats[name]["windows_per_pass"] == [T - 1, 2 * (T - 1)]
        assert f"frames in: {T}  out: {4 * (T - 1)}  factor: 4" in err
    assert stats["t5"]["frames_resident_peak"] == stats["t9"]["frames_resident_peak"] > 0, stats
    assert open(dst["t5"], "rb").read().startswith(CC.clip_header(24, 40, 420).replace(b"F30:1", b"F120:1"))


def test_cli_factor_4_with_scene_cuts_equals_the_harness(tmp_path):
    import scene_cases as SC
    from bin_amd import harness, video
    header = video.parse_header(SC.CLIP_HEADER)
    five, nine = SC.five_frame_clip(), SC.nine_frame_clip()
    clips = {"five": (header, torch.from_numpy(five[0])), "nine": (header, torch.from_numpy(nine[0]))}
    stats, dst, err = _cli(tmp_path, clips, ["--scene_cut", str(SC.THRESHOLD)], piped="nine")
    net = _net()
    for name, cuts in (("five", five[1]), ("nine", nine[1])):
        payloads = clips[name][1]
        T = payloads.shape[0]
        assert stats[name]["cuts"] == cuts and stats[name]["frames_out"] == 4 * (T - 1)
        want = harness.interpolate_video(net, payloads, header, factor=4, scene_cut=SC.THRESHOLD)
        assert torch.equal(want, harness.interpolate_video(net, payloads, header, factor=4, scene_cut=cuts))
        frames = _frames_of(dst[name], header, 4)
        assert len(frames) == want.shape[0] and all(f == w.tobytes() for f, w in zip(frames, want.cpu().numpy())), name
        for c in cuts:
            assert f"scene cut at input frame {c} (output frame {4 * c})" in err
        for c in cuts:                                         # the holds before every cut
            assert len({frames[pos] for pos in range(4 * (c - 1), 4 * c)}) == 1
    # both clips' longest scene has three frames: the same frames resident
    assert stats["five"]["frames_resident_peak"] == stats["nine"]["frames_resident_peak"] > 0, stats
