"""GPU: the scene-cut path — binscene_luma_stats (include/binscene.h) against numpy on every shape, content and alignment of
scene_cases.py, exactly; harness.detect_cuts on the clips whose distances the CPU side pins; harness.interpolate_video(scene_cut=...)
against the composition it promises (every scene as if it ran alone, its last deblurred frame, the holds), bit for bit; and
`python -m bin_amd.test --input_video ... --scene_cut` in a child process against the harness.  CPU side: test_cpu_scene.py."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import scene_cases as SC
import video_cases as VC
from conftest import REPO

pytestmark = pytest.mark.gpu

GUARD_BYTES = 64


def _view(a, offset):
    """`a` (numpy uint8) on the device at `offset` bytes past a 256-byte boundary, guard bytes on both sides: (view, whole buffer)."""
    a = np.ascontiguousarray(a).reshape(-1)
    host = np.full(a.size + offset + 2 * GUARD_BYTES + 256, SC.GUARD, np.uint8)
    start = 256 + offset                               # (the allocation is 256-byte aligned; the guard in front is 256 + offset bytes)
    host[start:start + a.size] = a
    buf = torch.from_numpy(host).cuda()
    assert buf.data_ptr() % 256 == 0
    return buf[start:start + a.size], buf


# ------------------------------------------------------------------------------------------------ 1. the kernel
@functools.lru_cache(maxsize=None)
def _contents(h, w):
    """[(name, cur, prev or None, expected record bytes)]: computed once per shape."""
    rnd, other = SC.plane("random", h, w, 31 * h + w), SC.plane("random", h, w, 17 * h + w + 1)
    zeros, full = SC.plane("zeros", h, w), SC.plane("full", h, w)
    cases = [("random", rnd, other), ("no prev", rnd, None), ("prev is cur", rnd, rnd), ("black", zeros, zeros), ("black after white", zeros, full),
             ("white", full, None), ("white after black", full, zeros)]
    return [(name, cur, prev, SC.record_ref(cur, prev)) for name, cur, prev in cases]


@pytest.mark.parametrize("h,w", SC.SHAPES + [SC.BIG_SHAPE], ids=lambda v: str(v))
def test_luma_stats_equals_numpy_exactly(h, w):
    from bin_amd import ops
    n = h * w
    if (h, w) == SC.BIG_SHAPE:
        assert n // 16 > 512 * 256, "more vectors than the grid cap has lanes: the blocks stride"
    stride = SC.RECORD_BYTES + 2 * GUARD_BYTES
    runs, keep = [], []
    contents = _contents(h, w)
    recs = torch.full((len(contents) * len(SC.OFFSETS) * 2, stride), SC.GUARD, dtype=torch.uint8, device="cuda")
    for name, cur, prev, want in contents:
        for offset in SC.OFFSETS:
            c, whole_c = _view(cur, offset)
            assert c.data_ptr() % 16 == offset % 16
            # prev at cur's offset within 16 bytes (it moves as vectors) and 5 bytes off it (it does not)
            for shift in ((0, 5) if prev is not None else (0,)):
                p, whole_p = _view(prev, offset + shift) if prev is not None else (None, None)
                rec = recs[len(runs), GUARD_BYTES:GUARD_BYTES + SC.RECORD_BYTES]
                assert rec.data_ptr() % 8 == 0
                assert ops.luma_stats(c, p, h, w, out=rec) is rec
                runs.append((name, offset, shift, want))
                keep.append((whole_c, whole_p))
    got = recs.cpu().numpy()
    for k, (name, offset, shift, want) in enumerate(runs):
        row = got[k]
        assert np.array_equal(row[GUARD_BYTES:GUARD_BYTES + SC.RECORD_BYTES], want), (name, offset, shift, ops.read_luma_record(
            row[GUARD_BYTES:GUARD_BYTES + SC.RECORD_BYTES])[0], ops.read_luma_record(want)[0])
        assert (row[:GUARD_BYTES] == SC.GUARD).all() and (row[GUARD_BYTES + SC.RECORD_BYTES:] == SC.GUARD).all(), "guard bytes written"
    assert (got[len(runs):] == SC.GUARD).all()
    for whole_c, whole_p in keep[:: max(1, len(keep) // 4)]:           # the planes' own guards: nothing is written around an input
        for whole in (whole_c, whole_p):
            if whole is not None:
                host = whole.cpu().numpy()
                assert (host[:256] == SC.GUARD).all() and (host[-GUARD_BYTES:] == SC.GUARD).all()
    sad, hist = ops.read_luma_record(got[0][GUARD_BYTES:GUARD_BYTES + SC.RECORD_BYTES])
    assert (sad, list(hist)) == (SC.luma_stats_ref(contents[0][1], contents[0][2])[0], list(np.bincount(contents[0][1].reshape(-1) >> 2, minlength=64)))
    assert hist.sum() == n


def test_luma_stats_clears_the_record_itself_and_returns_a_fresh_one():
    from bin_amd import ops
    h, w = 33, 130
    a, b = SC.plane("random", h, w, 1), SC.plane("random", h, w, 2)
    da, db = torch.from_numpy(a).cuda().view(-1), torch.from_numpy(b).cuda().view(-1)
    rec = torch.full((SC.RECORD_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")       # (never cleared by the caller)
    ops.luma_stats(da, None, h, w, out=rec)
    ops.luma_stats(db, da, h, w, out=rec)
    assert np.array_equal(rec.cpu().numpy(), SC.record_ref(b, a)), "two calls into one record: the second call's values"
    fresh = ops.luma_stats(da.view(h, w), db.view(h, w), h, w)
    assert fresh.dtype == torch.uint8 and fresh.shape == (SC.RECORD_BYTES,) and fresh.is_cuda
    assert np.array_equal(fresh.cpu().numpy(), SC.record_ref(a, b))
    sad, hist = ops.read_luma_record(fresh.cpu())
    assert sad == SC.luma_stats_ref(a, b)[0] and np.array_equal(hist, SC.luma_stats_ref(a, b)[1])
    with pytest.raises(ValueError, match="downloaded"):
        ops.read_luma_record(fresh)


def test_luma_stats_refuses_wrong_sizes_before_any_launch():
    from bin_amd import ops
    y = torch.zeros(60, dtype=torch.uint8, device="cuda")
    rec = torch.full((SC.RECORD_BYTES + 8,), SC.GUARD, dtype=torch.uint8, device="cuda")
    for cur, prev in ((y[:-1], None), (y, y[:-1]), (y.to(torch.int8), None), (y.view(6, 10)[:, :5], None), (y, y.float())):
        with pytest.raises(ValueError):
            ops.luma_stats(cur, prev, 6, 10, out=rec[:SC.RECORD_BYTES])
    for h, w in ((0, 10), (6, 0), (-6, -10)):
        with pytest.raises(ValueError):
            ops.luma_stats(y, None, h, w)
    for out in (rec[:100], rec.view(2, -1), rec[:SC.RECORD_BYTES].to(torch.int8)):
        with pytest.raises(ValueError):
            ops.luma_stats(y, None, 6, 10, out=out)
    with pytest.raises(RuntimeError, match="bad argument"):                # the library's own refusals: a misaligned record,
        ops.luma_stats(y, None, 6, 10, out=rec[4:4 + SC.RECORD_BYTES])
    big = torch.zeros(400, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="bad argument"):                # ... and a record inside a plane
        ops.luma_stats(big, None, 20, 20, out=big[8:8 + SC.RECORD_BYTES])
    torch.cuda.synchronize()
    assert (rec == SC.GUARD).all() and not big.any(), "nothing was launched"


# ------------------------------------------------------------------------------------------------ 2. detection
@functools.lru_cache(maxsize=None)
def _clip(which):
    from bin_amd import video
    payloads, cuts = SC.nine_frame_clip() if which == 9 else SC.five_frame_clip()
    return video.parse_header(SC.CLIP_HEADER), torch.from_numpy(payloads), cuts


@pytest.mark.parametrize("which", [9, 5])
def test_detect_cuts_finds_the_cuts_and_agrees_with_the_float64_reference(which):
    from bin_amd import harness, scene
    header, payloads, cuts = _clip(which)
    dist, ref = SC.clip_distances(payloads.numpy())
    assert [i for i, d in enumerate(dist, start=1) if d >= SC.THRESHOLD] == cuts, "the reference itself finds them"
    recs = harness.luma_records(payloads, header)
    assert len(recs) == which
    for got, want in zip(recs, ref):
        assert got[0] == want[0] and np.array_equal(got[1], want[1])
    assert [scene.distance(recs[i - 1][1], recs[i][1], SC.H, SC.W) for i in range(1, which)] == dist
    assert harness.detect_cuts(payloads, header, SC.THRESHOLD) == cuts
    assert harness.detect_cuts(payloads.cuda(), header, SC.THRESHOLD) == cuts
    assert harness.detect_cuts(payloads, header, 0.0) == list(range(1, which)), "threshold 0: every changed frame"
    assert harness.detect_cuts(payloads, header, 1.01) == []
    assert harness.detect_cuts(payloads, header, SC.THRESHOLD, min_mad=255.0) == [], "the min_mad guard"
    doubled = payloads[[0, 0, 1, 1]]
    assert harness.detect_cuts(doubled, header, 0.0) == [2], "a repeated frame is never a cut"
    if which == 9:
        assert cuts == [3, 6, 7]


# ------------------------------------------------------------------------------------------------ 3. interpolate_video
@functools.lru_cache(maxsize=None)
def _net(prec):
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval().set_precision(prec)


FMT = (420, "bt601", "full")                            # auto: 40x24 -> bt601, XCOLORRANGE=FULL -> full


def _forward_by_hand(net, header, payloads, ids, slot, group):
    """One output payload from the generator driven by hand on the frames `ids`."""
    import ensemble_cases as EC
    from bin_amd import ops
    from bin_amd.utils import util
    h, w = header.height, header.width
    pads = util.pad_sizes(h, w)
    l, r, t, b = pads
    padded = {i: ops.yuv_to_frame(payloads[i].cuda(), h, w, FMT, pads) for i in set(ids)}
    inputs = [padded[i] for i in ids]
    assert tuple(inputs[0].shape) == (1, 3, 128, 128)
    with torch.no_grad():
        Ft_p = net(*inputs) if group is None else EC.by_hand(net, inputs, group)
    return ops.frame_to_yuv(Ft_p[slot], t, l, h, w, FMT)


@functools.lru_cache(maxsize=None)
def _expected(which, prec, group=None):
    """The composition: interpolate_video (without the option) of every multi-frame scene alone, that scene's last deblurred frame
    from slot 12 of its last window by hand, the holds, and the forward on six equal frames for a one-frame scene."""
    from bin_amd import harness
    header, payloads, cuts = _clip(which)
    net = _net(prec)
    T = payloads.shape[0]
    edges = [0] + cuts + [T]
    out = []
    for s, e in zip(edges[:-1], edges[1:]):
        assert len(out) == 2 * s
        if e - s >= 2:
            alone = harness.interpolate_video(net, payloads[s:e], header, ensemble=group)
            assert alone.shape[0] == 2 * (e - s - 1)
            out += list(alone)
            if e < T:
                ids = [s + i for i in harness.window_frame_ids(e - s - 2, e - s)]
                last = _forward_by_hand(net, header, payloads, ids, 12, group)
                out += [last, last]                      # D_(e-1), and it again where the midpoint across the cut would be
        elif e < T:
            only = _forward_by_hand(net, header, payloads, [s] * 6, 8, group)
            out += [only, only]
    assert len(out) == 2 * (T - 1)
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def _one_clip(which, prec):
    """Today's output of the whole stream, the generator driven by hand."""
    from bin_amd import harness
    header, payloads, _ = _clip(which)
    T = payloads.shape[0]
    out = []
    for i in range(T - 1):
        out += [_forward_by_hand(_net(prec), header, payloads, harness.window_frame_ids(i, T), k, None)
                for k in VC.video_slots(i, T - 1)]
    return torch.stack(out)


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_interpolate_video_within_scenes_equals_the_composition(prec):
    from bin_amd import harness
    header, payloads, cuts = _clip(9)
    net = _net(prec)
    want = _expected(9, prec)
    got = harness.interpolate_video(net, payloads, header, scene_cut=SC.THRESHOLD)
    assert got.shape == (16, header.frame_bytes) and got.dtype == torch.uint8 and got.is_cuda
    assert torch.equal(got, want)
    # the holds repeat the payload before them; everything else differs
    frames = [bytes(p.cpu().numpy()) for p in got]
    assert frames[5] == frames[4] and frames[11] == frames[10] and frames[13] == frames[12] and len(set(frames)) == 13
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=[3, 6, 7]), want)
    assert torch.equal(harness.interpolate_video(net, payloads.cuda(), header, scene_cut=iter((7, 3, 6))), want)


def test_interpolate_video_within_scenes_without_reuse_and_batched():
    from bin_amd import harness
    header, payloads, cuts = _clip(9)
    net, want = _net("f16x3"), _expected(9, "f16x3")
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=SC.THRESHOLD, reuse_stage1=False), want)
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=SC.THRESHOLD, batch=2), want)
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=cuts, batch=4), want)


def test_interpolate_video_within_scenes_with_an_ensemble():
    from bin_amd import harness
    header, payloads, cuts = _clip(9)
    net = _net("f16x3")
    want = _expected(9, "f16x3", "h")
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=SC.THRESHOLD, ensemble="h"), want)
    assert not torch.equal(want, _expected(9, "f16x3"))


def test_interpolate_video_without_cuts_is_todays_and_differs_next_to_the_cuts():
    from bin_amd import harness
    header, payloads, cuts = _clip(9)
    net = _net("f16x3")
    today = _one_clip(9, "f16x3")
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=None), today)
    assert torch.equal(harness.interpolate_video(net, payloads, header), today)
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=[]), today)
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=1.01), today), "a threshold nothing reaches"
    aware = _expected(9, "f16x3")
    differs = [k for k in range(16) if not torch.equal(aware[k], today[k])]
    # the frames next to the cuts: a hold instead of a blend of two scenes (5, 11, 13), a first deblurred frame computed from its
    # own scene (6, 12, 14)
    assert set(differs) >= {5, 6, 11, 12, 13, 14}, differs
    for bad in ([0], [9], [3, 12]):
        with pytest.raises(ValueError):
            harness.interpolate_video(net, payloads, header, scene_cut=bad)


def test_interpolate_video_with_a_lone_first_and_a_lone_last_frame():
    from bin_amd import harness
    header, payloads, cuts = _clip(5)
    assert cuts == [1, 4]
    net, want = _net("f16x3"), _expected(5, "f16x3")
    got = harness.interpolate_video(net, payloads, header, scene_cut=SC.THRESHOLD)
    assert got.shape == (8, header.frame_bytes) and torch.equal(got, want)
    frames = [bytes(p.cpu().numpy()) for p in got]
    assert frames[1] == frames[0] and frames[7] == frames[6] and len(set(frames)) == 6
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=[1, 4], batch=2), want)
    assert torch.equal(harness.interpolate_video(net, payloads, header, scene_cut=[1, 4], reuse_stage1=False), want)
    assert not torch.equal(want, _one_clip(5, "f16x3"))


# ------------------------------------------------------------------------------------------------ 4. the entry point
DRIVER = """\
import sys
from bin_amd import test as T
stats = {}
assert T.main(["--opt", sys.argv[1], "--precision", "f16x3", "--input_video", sys.argv[2], "--output_video", sys.argv[3],
               "--scene_cut", "0.4"], stats) == 0
assert stats["cuts"] == [3, 6, 7] and stats["frames_out"] == 16 and stats["windows"] == 8, stats
"""


def test_cli_video_with_scene_cuts_in_a_child_process(tmp_path):
    """One fresh child process runs the entry point file to file with --scene_cut 0.4.  The runner streams: it decides window i from
    the frames up to i + 3 alone, so its output equal to the harness's, which sees the whole stream, is the check of the look-ahead."""
    from bin_amd import harness, video
    from bin_amd.weights import reference_state_dict
    from host_fixtures import OPTION_YML
    header, payloads, cuts = _clip(9)
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
    run = subprocess.run([sys.executable, "-c", DRIVER, yml, src, dst], stdin=subprocess.DEVNULL, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, cwd=str(tmp_path), env=env, timeout=240)
    assert run.returncode == 0, run.stderr.decode(errors="replace")[-3000:]
    assert run.stdout == b"", "nothing reaches stdout in a file-to-file run"
    err = run.stderr.decode(errors="replace")
    assert "scene cuts: 3 at input frames 3, 6, 7; duplicates: 0" in err and "frames in: 9  out: 16" in err
    for c in cuts:
        assert f"scene cut at input frame {c} (output frame {2 * c})" in err
    rd = video.Y4MReader(dst)
    assert rd.header == header.doubled()
    frames = [bytes(p) for p in rd]
    want = harness.interpolate_video(_net("f16x3"), payloads, header, scene_cut=SC.THRESHOLD).cpu().numpy()
    assert len(frames) == 16 == want.shape[0]
    assert all(f == w.tobytes() for f, w in zip(frames, want))
