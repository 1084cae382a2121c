"""CPU: what can be pinned about the scene-cut path without a device — the ABI bookkeeping of libbinscene.so (include/binscene.h),
every refusal that comes before a HIP call, the segments of bin_amd/scene.py and the plan of the shipped window loop
(bin_amd/chain.py) exhaustively for short streams, the
decision on hand-made records, and the command line's conflicts.  GPU side: test_gpu_scene.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import scene_cases as SC
from bin_amd import scene as S
from conftest import REPO


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_scene_library_header_and_binding_agree():
    """What is binscene's own beside the bookkeeping of test_cpu_libraries.py: the codes, the bins, the record as the C compiler lays
    it out, and a source in plain HIP C++ without switches."""
    from bin_amd import _lib
    hdr = open(os.path.join(REPO, "include", "binscene.h")).read()
    for name, value in (("BINSCENE_E_ARG", -1), ("BINSCENE_E_SHAPE", -2)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value
    assert int(re.search(r"#define\s+BINSCENE_BINS\s+(\d+)", hdr).group(1)) == _lib.SCENE_BINS == SC.BINS == 64
    # the struct: as the C compiler lays it out (the source asserts size and offset)
    assert re.search(r"typedef struct BinSceneRecord \{\s*uint64_t sad;[^}]*uint32_t hist\[BINSCENE_BINS\];[^}]*\} BinSceneRecord;", hdr)
    R = _lib.BinSceneRecord
    assert C.sizeof(R) == SC.RECORD_BYTES == 264 and (R.sad.offset, R.hist.offset) == (0, 8)
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binscene.hip")).read()
    assert "static_assert(sizeof(BinSceneRecord) == 264 && offsetof(BinSceneRecord, hist) == 8" in src
    assert not re.search(r"(?m)^\s*#\s*(if|ifdef|ifndef|elif|define)\b", src), "no preprocessor switches in the source"
    assert "asm" not in re.sub(r"//.*", "", src), "plain HIP C++"


def test_record_reader_and_restatement_agree_on_the_layout():
    from bin_amd import ops
    cur, prev = SC.plane("random", 5, 7, 1), SC.plane("random", 5, 7, 2)
    raw = SC.record_ref(cur, prev)
    assert raw.dtype == np.uint8 and raw.size == ops.LUMA_RECORD_BYTES == 264
    for form in (raw, torch.from_numpy(raw), raw.tobytes()):
        sad, hist = ops.read_luma_record(form)
        assert isinstance(sad, int) and sad == SC.luma_stats_ref(cur, prev)[0] and sad > 0
        assert hist.shape == (64,) and np.array_equal(hist, np.bincount(cur.reshape(-1) >> 2, minlength=64)) and hist.sum() == 35
    with pytest.raises(ValueError):
        ops.read_luma_record(raw[:-1])


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.scenelib()
    CUR, PREV, REC = 0x100000, 0x200000, 0x4000000

    def call(cur=CUR, prev=PREV, h=6, w=10, rec=REC):
        return lib.binscene_luma_stats(cur, prev, h, w, rec, None)
    assert call(cur=None) == -1 and call(rec=None) == -1
    for h, w in ((0, 10), (6, 0), (-1, 10), (6, -3), (0, 0)):
        assert call(h=h, w=w) == -1 and call(h=h, w=w, prev=None) == -1
    for off in (1, 2, 4, 7):
        assert call(rec=REC + off) == -1, "a record off an 8-byte boundary"
    # a record overlapping a plane: at its first and last byte, from either side
    for plane in ("cur", "prev"):
        base = CUR if plane == "cur" else PREV
        for rec in (base, base + 56, base - 256, base - 8, base + 8):
            assert (base - rec < 264 and rec - base < 60) and call(rec=rec) == -1, (plane, rec - base)
        assert base % 8 == 0
    # H*W beyond 2^31 - 1
    assert call(h=2 ** 16, w=2 ** 15) == -2 and call(h=2 ** 31 - 1, w=2) == -2 and call(h=1, w=2 ** 31 - 1, rec=None) == -1
    assert call(h=2 ** 16, w=2 ** 15, prev=None) == -2
    assert call(h=2 ** 31 - 1, w=2 ** 31 - 1) == -2


def test_op_refuses_cpu_tensors():
    from bin_amd import ops
    y = torch.zeros(60, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.luma_stats(y, None, 6, 10)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.luma_stats(y, y, 6, 10, out=torch.zeros(264, dtype=torch.uint8))


# ------------------------------------------------------------------------------------------------ the plan
def _cut_sets(T):
    positions = range(1, T)
    for n in range(T):
        for cuts in itertools.combinations(positions, n):
            yield set(cuts)


@pytest.mark.parametrize("T", range(2, 9))
def test_plan_and_segments_over_every_cut_set(T):
    """The plan as the shipped loop applies it: read off a factor-2 run of chain.run_stream on stub frames (chain_cases.StubRun), per
    output position the Ft_p slot or the hold and the window it came from, per forward its six ids."""
    import chain_cases as CC
    import video_cases as VC
    from bin_amd import chain, harness
    HOLD = "hold"
    n_sets = 0
    for cuts in _cut_sets(T):
        n_sets += 1
        segs = S.segments(T, cuts)
        # maximal runs: they tile 0 .. T, and a boundary lies exactly at every cut
        assert segs[0][0] == 0 and segs[-1][1] == T and all(a[1] == b[0] for a, b in zip(segs, segs[1:]))
        assert {s for s, _ in segs[1:]} == cuts and all(s < e for s, e in segs)
        run = CC.StubRun(T, 2, cuts=sorted(cuts))
        assert chain.HOLD is None and len(run.sources) == len(run.emitted)
        by_window = {}                                          # window -> [(position, slot or HOLD)] in display order
        for pos, src in enumerate(run.sources):
            window, slot = (pos // 2, HOLD) if src is None else src
            by_window.setdefault(window, []).append((pos, slot))
        ids_of = {ids[2]: ids for ids in run.level1_ids}
        assert len(ids_of) == len(run.level1_ids), "one forward per window at the most"
        positions, forwards = [], 0
        for s, e in segs:
            for i in range(s, min(e, T - 1)):
                ids, outputs = ids_of.get(i), by_window[i]
                plan_ids, plan_slots, plan_last = chain.level1_plan(i, s, e)
                assert plan_ids == ids and plan_last == (i + 1 == e)
                last = None
                for pos, slot in outputs:
                    assert slot in (8, 13, 12, HOLD)
                    if slot is HOLD:                         # a hold repeats D_i, which was emitted just before it
                        assert pos == 2 * i + 1 and positions and positions[-1] == 2 * i and i + 1 == e
                        assert run.emitted[pos] == CC.HOLD and run.emitted[pos - 1] == i
                    else:
                        assert ids is not None
                        assert pos == {8: 2 * i, 13: 2 * i + 1, 12: 2 * i + 2}[slot]
                    assert last is None or pos == last + 1
                    last = pos
                    positions.append(pos)
                slots = tuple(slot for _, slot in outputs if slot is not HOLD)
                if ids is None:
                    assert i + 1 == e and i > s and [slot for _, slot in outputs] == [HOLD] and plan_slots == ()
                else:
                    forwards += 1
                    assert len(ids) == 6 and all(s <= f < e for f in ids), "every id inside the window's scene"
                    assert ids == sorted(ids) and ids[2] == i
                    if i + 1 < e:
                        assert ids == [min(max(i + d, s), e - 1) for d in (-2, -1, 0, 1, 2, 3)] and ids[3] == i + 1
                        assert plan_slots == ((8,) if i == s else ()) + (13, 12)
                        # the stream's last window gives its slot 12 to the passes, never to the output
                        assert slots == (plan_slots[:-1] if i == T - 2 else plan_slots)
                    else:
                        assert ids == [i] * 6 and i == s, "a one-frame scene"
                        assert plan_slots == slots == (8,) and [slot for _, slot in outputs] == [8, HOLD]
        assert positions == list(range(2 * T - 2)), (T, sorted(cuts), positions)
        assert sorted(by_window) == [i for s, e in segs for i in range(s, min(e, T - 1))] == list(range(T - 1))
        # forwards: one per window that has a successor in its scene, one per one-frame scene that is not the last frame
        assert forwards == len(run.level1_ids) == run.stats["windows_per_pass"][0]
        assert forwards == sum(max(e - s - 1, 0) for s, e in segs) + sum(1 for s, e in segs if e - s == 1 and s < T - 1)
    assert n_sets == 2 ** (T - 1)
    # no cuts: the sliding window and the ownership rule as they are
    run = CC.StubRun(T, 2)
    for i in range(T - 1):
        assert run.level1_ids[i] == harness.window_frame_ids(i, T)
        assert tuple(slot for window, slot in run.sources if window == i) == VC.video_slots(i, T - 1)
    # a streaming caller that does not know the end yet (the scene end somewhere beyond i + 3) plans the same window, and runs the same
    for i in range(T - 4):
        assert chain.level1_plan(i, 0, i + 4) == chain.level1_plan(i, 0, T)
    live = CC.StubRun(T, 2, live=True)
    assert live.sources == run.sources and live.level1_ids == run.level1_ids


def test_plan_and_segments_refuse_what_is_not_a_window():
    from bin_amd import chain
    for bad in ([0], [5], [-1], [2, 9]):
        with pytest.raises(ValueError):
            S.segments(5, bad)
    assert S.segments(5, [4, 2, 2]) == [(0, 2), (2, 4), (4, 5)] and S.segments(3, ()) == [(0, 3)]
    for i, s, e in ((2, 3, 5), (3, 0, 3), (-1, 0, 2), (5, 0, 5)):
        with pytest.raises(ValueError):
            chain.level1_plan(i, s, e)


# ------------------------------------------------------------------------------------------------ the decision
def _rec(sad, counts):
    hist = np.zeros(64, np.int64)
    for k, c in counts.items():
        hist[k] = c
    return sad, hist


def test_is_cut_on_hand_made_records():
    h, w = 4, 25                                             # 100 pixels
    a = _rec(0, {0: 100})
    assert S.distance(a[1], a[1], h, w) == 0.0
    assert S.distance(a[1], _rec(0, {63: 100})[1], h, w) == 1.0, "disjoint histograms are at distance 1"
    quarter = _rec(500, {0: 75, 9: 25})                      # 25 pixels moved: sum |ha - hb| = 50 -> 0.25
    assert S.distance(a[1], quarter[1], h, w) == 0.25 and S.distance(quarter[1], a[1], h, w) == 0.25
    # the >= edge of the threshold (0.25 and 0.5 are exact in binary)
    assert S.is_cut(a, quarter, h, w, 0.25) and not S.is_cut(a, quarter, h, w, np.nextafter(0.25, 1.0))
    assert S.is_cut(a, quarter, h, w, 0.2) and not S.is_cut(a, quarter, h, w, 0.3)
    # the min_mad guard: sad / (h w) = 5.0, >= again
    assert S.is_cut(a, quarter, h, w, 0.25, min_mad=5.0) and not S.is_cut(a, quarter, h, w, 0.25, min_mad=np.nextafter(5.0, 6.0))
    assert S.is_cut(a, quarter, h, w, 0.25, min_mad=0.0)
    # sad == 0: a duplicate, never a cut, whatever the histograms or the threshold say
    for thr in (0.0, -1.0, 0.25):
        assert not S.is_cut(a, _rec(0, {9: 100}), h, w, thr) and not S.is_cut(a, a, h, w, thr)
    assert S.is_duplicate(_rec(0, {0: 100})) and not S.is_duplicate(quarter)
    assert S.is_cut(a, _rec(1, {0: 100}), h, w, 0.0), "threshold 0: every changed frame"
    # uint32 counts as the record holds them do not wrap in the difference
    big = (7, np.array([3_000_000_000] + [0] * 63, np.uint32)), (7, np.array([0, 3_000_000_000] + [0] * 62, np.uint32))
    assert S.distance(big[0][1], big[1][1], 60000, 50000) == 1.0


def test_the_clips_are_what_the_decision_is_checked_on():
    """The float64 reference of the end-to-end test, from numpy alone: inside a scene every distance is <= 0.19, across every boundary
    >= 0.65, so threshold 0.4 finds exactly the cuts."""
    for clip in (SC.nine_frame_clip, SC.five_frame_clip):
        payloads, cuts = clip()
        assert payloads.dtype == np.uint8 and payloads.shape[1] == 1440
        dist, recs = SC.clip_distances(payloads)
        for i, d in enumerate(dist, start=1):
            assert (d >= SC.ACROSS_BAR) if i in cuts else (d <= SC.INSIDE_BAR), (i, d)
            assert d == S.distance(recs[i - 1][1], recs[i][1], SC.H, SC.W)
        assert [i for i in range(1, len(recs)) if S.is_cut(recs[i - 1], recs[i], SC.H, SC.W, SC.THRESHOLD)] == cuts
        assert recs[0][0] == 0 and all(r[0] > 0 for r in recs[1:]) and all(r[1].sum() == SC.H * SC.W for r in recs)
    assert SC.nine_frame_clip()[1] == [3, 6, 7] and SC.five_frame_clip()[1] == [1, 4]


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_scene_arguments_and_their_conflicts_raise_before_the_model_is_built(monkeypatch):
    import inspect
    from bin_amd import harness, test as T
    monkeypatch.setattr(T, "create_model", lambda *a, **k: pytest.fail("the model must not be built"))
    monkeypatch.setattr(T.option, "parse", lambda *a, **k: pytest.fail("the options must not be read"))
    video = ["--opt", "c", "--input_video", "in.y4m", "--output_video", "-"]
    folder = ["--opt", "c", "--input_path", "a", "--output_path", "b"]
    args = T.parse_args(video)
    assert args.scene_cut is None and args.scene_cut_min_mad == 0.0, "off by default"
    args = T.parse_args(video + ["--scene_cut", "0.4", "--scene_cut_min_mad", "2.5"])
    assert args.scene_cut == 0.4 and args.scene_cut_min_mad == 2.5
    assert T.parse_args(video + ["--scene_cut", "0"]).scene_cut == 0.0, "threshold 0 is on"
    for extra in (["--scene_cut", "0.4"], ["--scene_cut", "0"], ["--scene_cut_min_mad", "1"], ["--scene_cut", "0.4", "--scene_cut_min_mad", "1"]):
        with pytest.raises(ValueError, match="--input_video"):
            T.main(folder + extra)
    with pytest.raises(ValueError, match="--scene_cut"):
        T.main(video + ["--scene_cut_min_mad", "1"])
    assert T.parse_args(folder).scene_cut is None, "the folder run's arguments are what they were"
    sig = inspect.signature(harness.interpolate_video).parameters
    assert sig["scene_cut"].default is None and list(sig)[-1] == "scene_cut"
    assert list(inspect.signature(harness.detect_cuts).parameters)[:4] == ["payloads", "header", "threshold", "min_mad"]
