"""CPU: the chained interpolation passes (--factor 4 | 8) without a device — libbinchain.so's ABI bookkeeping and its refusals before
any launch, chain.Chain on stub frames against the definition restated by brute force (chain_cases.py), the scene composition for
every cut set of every short stream, the entry point's argument checks and the Y4M header.  GPU side: test_gpu_chain.py."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import pytest
import torch

import chain_cases as CC
from conftest import REPO


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_chain_library_header_and_binding_agree():
    """What is binchain's own beside the bookkeeping of test_cpu_libraries.py: the codes and the limit, the item as the C compiler
    lays it out, and a source in plain HIP C++ without switches or LDS."""
    from bin_amd import _lib
    hdr = open(os.path.join(REPO, "include", "binchain.h")).read()
    for name, value in (("BINCHAIN_E_ARG", -1), ("BINCHAIN_E_SHAPE", -2)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value
    assert int(re.search(r"#define\s+BINCHAIN_MAX_ITEMS\s+(\d+)", hdr).group(1)) == _lib.CHAIN_MAX_ITEMS >= 8
    # the struct: as the C compiler lays it out (the source asserts the size)
    assert re.search(r"typedef struct BinChainItem \{\s*const float\* src;\s*float\* dst;\s*\} BinChainItem;", hdr)
    item = _lib.BinChainItem
    assert C.sizeof(item) == 16 and (item.src.offset, item.dst.offset) == (0, 8)
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binchain.hip")).read()
    assert "static_assert(sizeof(BinChainItem) == 16" in src
    assert not re.search(r"(?m)^\s*#\s*(if|ifdef|ifndef|elif|define)\b", src), "no preprocessor switches in the source"
    assert "asm" not in re.sub(r"//.*", "", src) and "__shared__" not in src, "plain HIP C++, no LDS"


def test_chain_module_is_host_only():
    src = open(os.path.join(REPO, "bin_amd", "chain.py")).read()
    assert not re.search(r"(?m)^\s*(import|from)\s", src), "no imports at all: neither torch nor the device code"


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_reframe_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.chainlib()
    SRC, DST = 0x1000000, 0x4000000
    src_bytes, dst_bytes = 3 * 12 * 16 * 4, 3 * 9 * 13 * 4

    def call(items=((SRC, DST),), n=None, planes=3, hs=12, ws=16, top=3, left=1, h=6, w=10, pads=(1, 2, 3, 0)):
        table = (_lib.BinChainItem * max(len(items), 1))()
        for it, (s, d) in zip(table, items):
            it.src, it.dst = s, d
        return lib.binchain_reframe(table, len(items) if n is None else n, planes, hs, ws, top, left, h, w, *pads, None)
    assert call(items=(), n=0) == 0 and lib.binchain_reframe(None, 0, 3, 12, 16, 3, 1, 6, 10, 1, 2, 3, 0, None) == 0, "n == 0: no launch"
    assert call(n=-1) == -1 and call(n=_lib.CHAIN_MAX_ITEMS + 1) == -1
    assert lib.binchain_reframe(None, 1, 3, 12, 16, 3, 1, 6, 10, 1, 2, 3, 0, None) == -1, "a null table"
    for s, d in ((None, DST), (SRC, None), (SRC + 2, DST), (SRC, DST + 1), (SRC + 3, DST + 3)):
        assert call(items=((s, d),)) == -1, (s, d)
    for kw in (dict(planes=0), dict(planes=-3), dict(hs=0), dict(ws=0), dict(h=0), dict(w=0), dict(h=-6), dict(w=-1), dict(hs=-12)):
        assert call(**kw) == -1, kw
        assert call(items=(), n=0, **kw) == -1, "a bad shape is refused whatever n"
    for pads in ((-1, 0, 0, 0), (0, -1, 0, 0), (0, 0, -1, 0), (0, 0, 0, -1)):
        assert call(pads=pads) == -1
    for kw in (dict(top=-1), dict(left=-1), dict(top=7), dict(left=7), dict(h=10), dict(w=16), dict(top=2 ** 31 - 1), dict(left=2 ** 31 - 1),
               dict(h=2 ** 31 - 1), dict(w=2 ** 31 - 1)):
        assert call(**kw) == -1, kw
    # element counts beyond 2^40, padded sides beyond 2^31 - 1
    big = 2 ** 31 - 1
    assert call(hs=2 ** 20, ws=2 ** 20, planes=3) == -2, "the source beyond 2^40"
    assert call(pads=(0, 0, big, 0)) == -2 and call(pads=(0, big, 0, 0)) == -2 and call(pads=(big, big, 0, 0)) == -2, "a side beyond 2^31 - 1"
    assert call(pads=(2 ** 20, 0, 2 ** 20, 0)) == -2, "the destination beyond 2^40"
    # overlaps: a destination on its source, on another item's source or destination; shared sources are fine (but not called: they
    # would launch)
    assert call(items=((SRC, SRC),)) == -1 and call(items=((SRC, SRC + src_bytes - 4),)) == -1 and call(items=((SRC, SRC - dst_bytes + 4),)) == -1
    far = DST + 0x1000000
    assert call(items=((SRC, DST), (far, SRC + 64))) == -1, "item 1's destination on item 0's source"
    assert call(items=((SRC, DST), (far, DST + dst_bytes - 4))) == -1, "two destinations overlap"
    assert call(items=((SRC, DST), (SRC, DST))) == -1


def test_ops_reframe_refuses_cpu_tensors_and_wrong_layouts():
    from bin_amd import _lib, ops
    x = torch.zeros(1, 3, 12, 16)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.reframe(x, 3, 1, 6, 10, (1, 2, 3, 0))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.reframe([x, x], 3, 1, 6, 10, (1, 2, 3, 0))
    for kw in (dict(pads=(0, -1, 0, 0)), dict(pads=(0, 0, 0)), dict(h=0), dict(w=0), dict(top=-1), dict(left=-2)):
        args = dict(top=3, left=1, h=6, w=10, pads=(1, 2, 3, 0))
        args.update(kw)
        with pytest.raises(ValueError):
            ops.reframe(x, **args)
    with pytest.raises(ValueError, match="at most"):
        ops.reframe([x] * (_lib.CHAIN_MAX_ITEMS + 1), 3, 1, 6, 10, (1, 2, 3, 0))
    assert ops.reframe([], 3, 1, 6, 10, (1, 2, 3, 0)) == []
    assert list(inspect.signature(ops.reframe).parameters) == ["frames", "top", "left", "h", "w", "pads", "out"]


# ------------------------------------------------------------------------------------------------ level arithmetic
def test_level_arithmetic():
    from bin_amd import chain, harness, scene
    assert [chain.levels(f) for f in (2, 4, 8)] == [1, 2, 3] and chain.FACTORS == CC.FACTORS
    assert chain.HOLD is None and not hasattr(scene, "HOLD") and harness.window_frame_ids is chain.window_ids, "one of each"
    for bad in (0, 1, 3, 6, 16, -2, 2.0, 4.0, True, "4", None):
        with pytest.raises(ValueError, match="factor"):
            chain.levels(bad)
    for n in range(1, 12):
        assert chain.sequence_length(n, 1) == 2 * (n - 1) + 1
        for p in (2, 3):
            assert chain.sequence_length(n, p) == 2 * chain.sequence_length(n, p - 1) - 1
        for j in range(n):
            assert chain.window_ids(j, n) == harness.window_frame_ids(j, n) == CC.window_ids(j, n)
    for T in range(2, 9):
        for F, k in ((2, 1), (4, 2), (8, 3)):
            levels, _ = CC.scene_levels(T, k)
            assert len(levels[-1]) == chain.sequence_length(T, k) == F * (T - 1) + 1
            assert levels[-1] == [Fraction(j, F) for j in range(F * (T - 1) + 1)], "the restatement itself: every 1/F"


def test_level1_plan_refuses_what_is_not_a_window_of_the_scene():
    """(What the plan gives for every window of every cut set: test_cpu_scene.py::test_plan_and_segments_over_every_cut_set.)"""
    from bin_amd import chain
    for i, s, e in ((3, 0, 3), (2, 3, 5), (-1, 0, 2), (5, 0, 5)):
        with pytest.raises(ValueError):
            chain.level1_plan(i, s, e)


# ------------------------------------------------------------------------------------------------ the scheduler on stub frames
def _forwards(run, level, scene_index=None):
    """[window ids] of the forwards of pass `level`, in order (of one scene of the run when given)."""
    out, scene_no = [], 0
    for entry in run.log:
        if entry == ("scene",):
            scene_no += 1
        elif entry[0] == "forward" and entry[1] == level and scene_index in (None, scene_no - 1):
            out.append(entry[2])
    return out


@pytest.mark.parametrize("F", CC.FACTORS)
@pytest.mark.parametrize("T", CC.LENGTHS)
def test_scheduler_equals_the_definition(T, F):
    from bin_amd import chain
    k = chain.levels(F)
    run = CC.StubRun(T, F)
    assert run.emitted == [Fraction(j, F) for j in range(F * (T - 1))], "every 1/F in display order, all but the last"
    levels, ids = CC.scene_levels(T, k)
    for p in range(2, k + 1):
        L = chain.sequence_length(T, p - 1)
        assert _forwards(run, p) == ids[p] == [chain.window_ids(j, L) for j in range(L - 1)]
    assert run.chain.windows == [chain.sequence_length(T, p - 1) - 1 for p in range(2, k + 1)]
    assert run.level1_ids == CC.expected_level1_ids(T, ()) == [chain.window_ids(i, T) for i in range(T - 1)]
    # every frame a pass consumes is reframed exactly once over the whole run: the level-1 frames and every pass's outputs but the last's
    n_consumed = chain.sequence_length(T, k - 1) if k > 1 else 0
    assert len(run.reframed) == len(set(run.reframed)) == n_consumed
    # the same object is handed over for the same frame in every window of a pass that names it
    assert run.seen or k == 1
    assert all(len(objs) == 1 for objs in run.seen.values())
    # ... and the passes share it: pass p + 1's sequence id 2j is pass p's j
    for (scene_no, level, i), objs in run.seen.items():
        if level < k and (scene_no, level + 1, 2 * i) in run.seen:
            assert run.seen[(scene_no, level + 1, 2 * i)] == objs
    assert sum(1 for entry in run.log if entry == ("scene",)) == 1


@pytest.mark.parametrize("F", CC.FACTORS)
@pytest.mark.parametrize("T", CC.LENGTHS)
def test_incremental_driver_equals_the_all_at_once_driver_and_runs_windows_as_early_as_it_may(T, F):
    from bin_amd import chain
    k = chain.levels(F)
    whole, single = CC.StubRun(T, F), CC.StubRun(T, F, step=1)
    strip = lambda log: [entry for entry in log if entry[0] != "push"]
    assert single.emitted == whole.emitted and strip(single.log) == strip(whole.log)
    # pass p runs window j in the push that makes frame j + 3 of its input exist, or when the end is known.  Its input's frames
    # exist in order: the level-1 frames as pushed, S(p)[0 .. 2c-1] after c windows of pass p (and the last one at the end).
    exist, ended = {1: 0}, False
    done = {p: 0 for p in range(2, k + 1)}
    for entry in single.log:
        if entry[0] == "push":
            exist[1] = entry[1]
        elif entry == ("end",):
            ended = True
        elif entry[0] == "forward":
            _, p, ids = entry
            j = done[p]
            have = exist[1] if p == 2 else 2 * done[p - 1]
            if not ended:
                assert j + 3 < have, "its frame j + 3 exists"
                assert j + 3 >= have - (1 if p == 2 else 2), "... and came with this very push"
            done[p] += 1
    assert ended and all(done[p] == chain.sequence_length(T, p - 1) - 1 for p in done)


def test_live_frames_do_not_grow_with_the_stream():
    for F in (4, 8):
        peaks = {T: CC.StubRun(T, F, step=1).chain.frames_resident_peak for T in (10, 40, 41)}
        assert peaks[10] == peaks[40] == peaks[41] > 0, peaks
        # per pass at most seven sequence ids (a window's six and the next one) with two objects each and the two frames being
        # handed on; the emitter holds one
        assert peaks[10] <= 16 * (F.bit_length() - 2) + 1
    assert CC.StubRun(10, 2).chain.frames_resident_peak == CC.StubRun(40, 2).chain.frames_resident_peak == 1


@pytest.mark.parametrize("batch", [2, 3, 8])
def test_batched_passes_emit_the_same_stream(batch):
    for F in (4, 8):
        for T in (2, 3, 6, 9):
            a, b = CC.StubRun(T, F), CC.StubRun(T, F, batch=batch)
            assert a.emitted == b.emitted
            for level in range(2, F.bit_length()):
                assert _forwards(a, level) == _forwards(b, level)


# ------------------------------------------------------------------------------------------------ scene cuts
@pytest.mark.parametrize("F", CC.FACTORS)
def test_every_cut_set_of_every_short_stream_equals_its_scenes_run_alone(F):
    from bin_amd import chain
    k = chain.levels(F)
    n_cases = 0
    for T in range(2, 7):
        for cuts in CC.all_cut_sets(T):
            run = CC.StubRun(T, F, cuts=cuts)
            want = CC.expected_stream(T, cuts, F)
            assert run.emitted == want and len(run.emitted) == F * (T - 1), (T, cuts)
            assert run.level1_ids == CC.expected_level1_ids(T, cuts), (T, cuts)
            begun = [(s, e) for s, e in CC.segments(T, cuts) if s < T - 1]        # (the stream's last frame alone is no scene of the run)
            assert sum(1 for entry in run.log if entry == ("scene",)) == len(begun)
            for index, (s, e) in enumerate(begun):
                _, ids = CC.scene_levels(e - s, k)
                for p in range(2, k + 1):
                    assert _forwards(run, p, index) == ids[p], (T, cuts, s, e, p)
                # positions: the scene's own stream from F s on, then the holds up to F e
                if e < T:
                    alone = CC.StubRun(e - s + 1, F, cuts=[e - s]).emitted       # the scene and one more frame behind a cut
                    assert [t if t == CC.HOLD else t + s for t in alone[:F * (e - s)]] == run.emitted[F * s:F * e]
                    assert run.emitted[F * (e - 1) + 1:F * e] == [CC.HOLD] * (F - 1) and run.emitted[F * (e - 1)] == e - 1
                else:
                    alone = CC.StubRun(e - s, F).emitted
                    assert [t + s for t in alone] == run.emitted[F * s:]
            n_cases += 1
    assert n_cases == sum(2 ** (T - 1) for T in range(2, 7))


def test_a_chain_refuses_a_scene_inside_a_scene():
    from bin_amd import chain
    c = chain.Chain(4, lambda level, jobs: [], lambda frames: [], lambda pos, f: None)
    c.begin(0)
    with pytest.raises(RuntimeError):
        c.begin(3)


# ------------------------------------------------------------------------------------------------ the loop's stream handling
def _level1_runs(run):
    return [entry[1] for entry in run.log if entry[0] == "run"]


def _short_streams():
    """(T, cuts): every cut set of T = 2 .. 6, and T = 7 .. 9 without cuts and with a few."""
    for T in range(2, 7):
        for cuts in CC.all_cut_sets(T):
            yield T, cuts
    for T in range(7, 10):
        for cuts in ((), (T - 1,), (1, 4), (3, 4, T - 2)):
            yield T, cuts


@pytest.mark.parametrize("F", CC.FACTORS)
def test_a_feed_that_learns_everything_late_gives_the_run_of_a_feed_that_knows_everything(F):
    for T, cuts in _short_streams():
        known, live = CC.StubRun(T, F, cuts=cuts), CC.StubRun(T, F, cuts=cuts, live=True)
        assert live.log == known.log and live.emitted == known.emitted == CC.expected_stream(T, cuts, F), (T, cuts)
        assert live.stats == known.stats and live.stats["windows"] == T - 1 == sum(live.flushes)
        assert live.stats["windows_per_pass"][0] == len(live.level1_ids) and live.stats["windows_per_pass"][1:] == live.chain.windows
        # window i asked for frame i + 3 and nothing beyond; the last question found the end
        assert live.feed.asked == [i + 3 for i in range(len(live.feed.asked))] and live.feed.asked[-1] >= T
        assert live.feed.n_frames == T and not live.feed.frames_dev.keys() - set(range(T - 6, T)), "frames are dropped as the windows pass"


def test_a_cut_is_honoured_as_soon_as_its_pair_is_in_sight_and_nothing_beyond_is_asked():
    """The cut at i + 3 comes into sight with frame i + 3, the last one window i waits for: window i must not name that frame.  The
    live feed raises when the loop asks about a frame that was not read (StubFeed.__contains__), and window i's forward is logged
    before the feed is asked for frame i + 4: no later frame and no later cut can have shaped it."""
    for F in CC.FACTORS:
        for T in range(5, 10):
            for i in range(T - 3):
                run = CC.StubRun(T, F, cuts=(i + 3,), live=True)
                mine = [ids for ids in run.level1_ids if ids[2] == i]
                assert mine == [[max(i - 2, 0), max(i - 1, 0), i, i + 1, i + 2, i + 2]], (T, i, mine)
                assert run.emitted == CC.expected_stream(T, (i + 3,), F)
                order = [entry for entry in run.log if entry[0] in ("read", "run")]
                for at, entry in enumerate(order):
                    if entry[0] == "run":
                        (ids,) = entry[1]
                        assert ("read", ids[2] + 3) in order[:at] and ("read", ids[2] + 4) not in order[:at], (T, i, ids)
    feed = CC.StubFeed(6, cuts=(2,), live=True)
    feed.read_to(3)
    feed.resolve_cuts()
    assert 2 in feed.cuts and 3 not in feed.cuts and list(feed.cuts) == [2]
    with pytest.raises(AssertionError, match="asked whether frame 4"):
        4 in feed.cuts


@pytest.mark.parametrize("batch", [1, 2, 3, 8])
def test_level1_forwards_are_the_forward_running_windows_in_groups_of_batch(batch):
    for F in CC.FACTORS:
        for T in range(2, 7):
            for cuts in CC.all_cut_sets(T):
                for live in (False, True):
                    run, one = CC.StubRun(T, F, cuts=cuts, batch=batch, live=live), CC.StubRun(T, F, cuts=cuts)
                    want = CC.expected_level1_ids(T, cuts)              # the forward-running windows in order, scene ends or not
                    groups = _level1_runs(run)
                    assert [ids for g in groups for ids in g] == want == one.level1_ids, (T, cuts)
                    assert [len(g) for g in groups] == [batch] * (len(want) // batch) + [len(want) % batch] * (len(want) % batch > 0)
                    assert run.emitted == one.emitted == CC.expected_stream(T, cuts, F)
                    for level in range(2, F.bit_length()):
                        assert _forwards(run, level) == _forwards(one, level)
                    assert run.stats["windows_per_pass"] == one.stats["windows_per_pass"] and sum(run.flushes) == T - 1


@pytest.mark.parametrize("F", CC.FACTORS)
def test_with_batch_1_a_scene_is_announced_between_the_forwards_of_two_scenes(F):
    """new_scene() drops the memos: it comes before the scene's first level-1 forward and after the last forward of every pass of the
    scene before."""
    for T, cuts in _short_streams():
        for live in (False, True):
            run = CC.StubRun(T, F, cuts=cuts, live=live)
            begun = [(s, e) for s, e in CC.segments(T, cuts) if s < T - 1]
            scene_no, per_scene = 0, {}
            for entry in run.log:
                if entry == ("scene",):
                    scene_no += 1
                elif entry[0] == "run":
                    assert scene_no >= 1, "a forward before any scene was announced"
                    per_scene.setdefault(scene_no - 1, []).append(("run", 1, entry[1][0]))
                elif entry[0] == "forward":
                    per_scene.setdefault(scene_no - 1, []).append(entry)
            assert scene_no == len(begun) == len(per_scene)
            # every forward logged after the n-th announcement and before the next belongs to the n-th scene
            for n, (s, e) in enumerate(begun):
                level1 = [entry[2] for entry in per_scene[n] if entry[0] == "run"]
                assert level1 == ([[s] * 6] if e - s == 1 else [[s + f for f in CC.window_ids(j, e - s)] for j in range(e - s - 1)]), (T, cuts, n)
                _, ids = CC.scene_levels(e - s, F.bit_length() - 1)
                for p in ids:
                    assert [entry[2] for entry in per_scene[n] if entry[0] == "forward" and entry[1] == p] == ids[p], (T, cuts, n, p)


# ------------------------------------------------------------------------------------------------ the entry point and the header
def test_cli_factor_argument_and_its_refusals_come_before_the_model_is_built(monkeypatch):
    from bin_amd import harness, test as T, video as V
    monkeypatch.setattr(T, "create_model", lambda *a, **k: pytest.fail("the model must not be built"))
    monkeypatch.setattr(T.option, "parse", lambda *a, **k: pytest.fail("the options must not be read"))
    base = ["--opt", "c", "--input_video", "in.y4m", "--output_video", "-"]
    assert T.parse_args(base).factor == 2
    assert [T.parse_args(base + ["--factor", str(f)]).factor for f in (2, 4, 8)] == [2, 4, 8]
    for bad in ("3", "16", "0", "4.0"):
        with pytest.raises(SystemExit):
            T.parse_args(base + ["--factor", bad])
    folder = ["--opt", "c", "--input_path", "a", "--output_path", "b"]
    assert T.parse_args(folder).factor == 2 and T.parse_args(folder + ["--factor", "2"]).factor == 2
    for f in ("4", "8"):
        with pytest.raises(ValueError, match="--factor"):
            T.main(folder + ["--factor", f])
    import argparse
    T.check_args(argparse.Namespace(input_video=None, output_video=None, input_path="a", output_path="b", gt_path=None, launcher="none"))
    with pytest.raises(ValueError, match="--factor"):
        T.check_args(argparse.Namespace(input_video=None, output_video=None, input_path="a", output_path="b", gt_path=None,
                                        launcher="none", factor=4))
    sig = inspect.signature(harness.interpolate_video).parameters
    assert sig["factor"].default == 2 and list(sig)[-2:] == ["factor", "scene_cut"], "scene_cut stays the last parameter"
    header = V.Y4MHeader(40, 24)
    for bad in (3, 1, 0, 16, 4.0, "4"):
        with pytest.raises(ValueError, match="factor"):
            harness.interpolate_video(None, torch.zeros(3, header.frame_bytes, dtype=torch.uint8), header, factor=bad)
    with pytest.raises(ValueError, match="at least 2 frames"):
        harness.interpolate_video(None, torch.zeros(1, header.frame_bytes, dtype=torch.uint8), header, factor=4)


def test_header_multiplied():
    from bin_amd import video as V
    h = V.parse_header(b"YUV4MPEG2 W40 H24 F30000:1001 Ip A1:1 C444 XCOLORRANGE=FULL")
    assert h.multiplied(2) == h.doubled() and h.doubled().rate == (60000, 1001)
    assert h.multiplied(4).rate == (120000, 1001) and h.multiplied(8).rate == (240000, 1001)
    assert h.multiplied(4).line() == b"YUV4MPEG2 W40 H24 F120000:1001 Ip A1:1 C444 XCOLORRANGE=FULL\n"
    assert h.multiplied(1) == h and h.multiplied(8) == h.multiplied(2).multiplied(4)
    for bad in (0, -2, 1.5):
        with pytest.raises(ValueError):
            h.multiplied(bad)
