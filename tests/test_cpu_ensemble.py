"""CPU: what can be pinned about the self-ensemble (bin_amd/ensemble.py, include/binens.h) without a device — the group spellings,
the slot table of the time reversal, the invariance of the sum tree under the group, our restatement of the reference's four-flip
helper against its recorded output, the host scheduler on a recording stand-in for the generator, the ABI bookkeeping of
libbinens.so and its refusals, and `train.val_self_ensemble`.  GPU side: test_gpu_ensemble.py."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ensemble_cases as EC
from bin_amd import ensemble as E
from conftest import REPO, load_golden


# ------------------------------------------------------------------------------------------------ the group
def test_parse_group_accepts_and_refuses():
    for s in (None, "", "none", "None", " NONE "):
        assert E.parse_group(s) == ""
    for k in (1, 2, 3):
        for perm in itertools.permutations("hvt", k):
            assert E.parse_group("".join(perm)) == "".join(c for c in "hvt" if c in perm)
    assert E.parse_group("flipx4") == "hv" and E.parse_group("x8") == "hvt" and E.parse_group("HV") == "hv"
    for bad in ("hh", "hvh", "x", "hx", "flipx8", "x4", "h v", "r", "hvtt", 4, True, ["h"]):
        with pytest.raises(ValueError):
            E.parse_group(bad)


def test_orientation_index_uses_only_the_bits_of_the_letters_present():
    W, H = E.FLIP_W, E.FLIP_H
    assert (W, H) == (1, 2)
    assert E.orientations("h") == [(0, False), (W, False)]
    assert E.orientations("v") == [(0, False), (H, False)]
    assert E.orientations("t") == [(0, False), (0, True)]
    assert E.orientations("hv") == [(0, False), (W, False), (H, False), (W | H, False)]
    assert E.orientations("ht") == [(0, False), (W, False), (0, True), (W, True)]
    assert E.orientations("vt") == [(0, False), (H, False), (0, True), (H, True)]
    assert E.orientations("hvt") == [(f, r) for r in (False, True) for f in (0, W, H, W | H)]
    for g in ("h", "hv", "ht", "hvt"):
        o = E.orientations(g)
        # the group acts on the index by XOR: composing two orientations is the orientation of the XOR of their indices
        for a in range(len(o)):
            for b in range(len(o)):
                assert (o[a][0] ^ o[b][0], o[a][1] ^ o[b][1]) == o[a ^ b]


def test_slot_table_of_the_time_reversal():
    frame, level, p = E.SLOT_FRAME, E.SLOT_LEVEL, E.SLOT_REVERSED
    assert list(p) == [10, 3, 2, 1, 11, 6, 5, 12, 8, 13, 0, 4, 7, 9]
    assert list(frame) == [2, 4, 6, 8, 3, 5, 7, 4, 6, 5, 10, 9, 8, 7] and list(level) == [1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 1, 2, 3, 4]
    assert len(set(zip(frame, level))) == 14, "every (frame, level) pair is distinct"
    for k in range(14):
        assert frame[p[k]] == 12 - frame[k] and level[p[k]] == level[k] and p[p[k]] == k
    derived = [next(j for j in range(14) if frame[j] == 12 - frame[k] and level[j] == level[k]) for k in range(14)]
    assert derived == list(p)
    # the frames the wrapper supervises the outputs with (bin_model.get_info) are the table's
    src = open(os.path.join(REPO, "bin_amd", "models", "bin_model.py")).read()
    names = re.search(r"gt_list = \[([^\]]+)\]", src).group(1)
    assert [int(n) for n in re.findall(r"self\.I(\d+)", names)] == list(frame)


def test_tree_sum_is_invariant_under_every_xor_and_the_sequential_sum_is_not():
    rng = np.random.Generator(np.random.PCG64(11))
    seq_mismatch = 0
    for M in (2, 4, 8):
        x = rng.uniform(-1, 2, size=(M, 4096)).astype(np.float32)
        want = E.tree_sum(list(x))
        for g in range(M):
            perm = [o ^ g for o in range(M)]
            assert np.array_equal(EC.bits(E.tree_sum([x[i] for i in perm])), EC.bits(want)), (M, g)
            seq = x[perm[0]].copy()
            for i in perm[1:]:
                seq = seq + x[i]
            base = x[0].copy()
            for i in range(1, M):
                base = base + x[i]
            seq_mismatch += int((EC.bits(seq) != EC.bits(base)).sum())
    assert seq_mismatch > 0, "a sequential sum does depend on the orientation of the input"
    assert np.float32(1 / 8) * np.float32(8) == 1 and all(np.float32(1.0 / M).view(np.uint32) & 0x7FFFFF == 0 for M in (1, 2, 4, 8))


# ------------------------------------------------------------------------------------------------ against the reference helper
def test_hv_on_the_stub_equals_the_recorded_reference_helper_bit_for_bit():
    g = load_golden("g14_flipx4")
    x = torch.from_numpy(g["x"])
    assert torch.equal(x, EC.grid_frame(int(g["seed"]), (1, 3, 6, 10)))
    net = EC.StubNet().eval()
    leaves = [EC.torch_flip(net(EC.torch_flip(x, f)), f) for f, _ in E.orientations("flipx4")]
    got = (E.tree_sum(leaves) * 0.25).numpy()
    assert got.dtype == np.float32 and np.array_equal(EC.bits(got), EC.bits(g["y"]))
    assert np.array_equal(EC.bits(EC.merge_ref32([net(EC.torch_flip(x, f)).numpy() for f in (0, 1, 2, 3)], [0, 1, 2, 3])), EC.bits(g["y"]))
    # not vacuous: the stub is not flip-equivariant, so leaving the un-flip out (or one orientation) is seen
    assert not np.array_equal(net(x).numpy(), g["y"])
    assert not np.array_equal((E.tree_sum([net(EC.torch_flip(x, f)) for f in (0, 1, 2, 3)]) * 0.25).numpy(), g["y"])


# ------------------------------------------------------------------------------------------------ the scheduler
def _frames(n=1, h=6, w=10, count=6, seed=50):
    return [EC.grid_frame(seed + i, (n, 3, h, w)) for i in range(count)]


@pytest.mark.parametrize("group", ["h", "v", "t", "hv", "ht", "vt", "hvt"])
@pytest.mark.parametrize("n", [1, 2])
def test_both_strategies_equal_the_composition_by_hand(group, n):
    frames = _frames(n)
    want = EC.by_hand(EC.FakeNetG(), frames, group)
    M = 1 << len(group)
    for small in (True, False):
        net, kern = EC.FakeNetG(small=small), EC.TorchKernels()
        ens = E.SelfEnsemble(net, group, kernels=kern)
        got = ens(frames)
        assert len(got) == 14 and all(torch.equal(a, b) for a, b in zip(got, want)), (group, small)
        assert kern.merge_launches == 1
        if small:       # batched: ONE call at batch M * N, one orient launch for all six frames
            assert ens.strategy_for(frames[0]) == "batched"
            assert [c["batch"] for c in net.calls] == [M * n] and kern.orient_launches == 1
        else:           # streamed: M calls at the input's own N, one orient launch per frame (none for a group without flips)
            assert ens.strategy_for(frames[0]) == "streamed"
            assert [c["batch"] for c in net.calls] == [n] * M
            assert kern.orient_launches == (0 if group == "t" else 6)
    some = E.SelfEnsemble(EC.FakeNetG(), group, kernels=EC.TorchKernels())(frames, slots=(13, 8, 12))
    assert [k for k, t in enumerate(some) if t is not None] == [8, 12, 13]
    assert all(torch.equal(some[k], want[k]) for k in (8, 12, 13))


@pytest.mark.parametrize("group", ["h", "v", "t", "hv", "ht", "vt", "hvt"])
def test_ensemble_of_an_oriented_input_is_the_oriented_ensemble_for_any_generator(group):
    """The ensemble symmetrises whatever deterministic generator it is given (the stand-in is equivariant under nothing): for every g
    of the group, E(g x) == g E(x) over all 14 slots, where g permutes the slots by SLOT_REVERSED when it reverses time.  Exact here
    because the stand-in's values are; on the device the tree makes it exact for the real generator (test_gpu_ensemble.py)."""
    frames = _frames(2)
    for small in (True, False):
        ens = E.SelfEnsemble(EC.FakeNetG(small=small), group, kernels=EC.TorchKernels())
        base = ens(frames)
        for flip, rev in E.orientations(group)[1:]:
            moved = [EC.torch_flip(f, flip) for f in (frames[::-1] if rev else frames)]
            got = ens(moved)
            for k in range(14):
                assert torch.equal(got[E.SLOT_REVERSED[k] if rev else k], EC.torch_flip(base[k], flip)), (group, flip, rev, k)
        plain = EC.FakeNetG()(*frames)
        assert not any(torch.equal(a, b) for a, b in zip(base, plain))


def test_explicit_strategy_overrides_the_rule():
    frames = _frames()
    net = EC.FakeNetG(small=True)
    E.SelfEnsemble(net, "hv", strategy="streamed", kernels=EC.TorchKernels())(frames)
    assert len(net.calls) == 4
    net = EC.FakeNetG(small=False)
    E.SelfEnsemble(net, "hv", strategy="batched", kernels=EC.TorchKernels())(frames)
    assert [c["batch"] for c in net.calls] == [4]
    with pytest.raises(ValueError):
        E.SelfEnsemble(net, "hv", strategy="both")
    with pytest.raises(ValueError):
        E.SelfEnsemble(net, "none")


def test_streamed_windows_keep_oriented_frames_and_one_cache_per_orientation():
    clip = _frames(count=9)
    net, kern = EC.FakeNetG(small=False), EC.TorchKernels()
    ens = E.SelfEnsemble(net, "hvt", kernels=kern)
    for first in (0, 1, 2):
        ids = list(range(first, first + 6))
        got = ens.window(ids, [clip[i] for i in ids], slots=(13, 8, 12))
        want = EC.by_hand(EC.FakeNetG(), [clip[i] for i in ids], "hvt")
        assert all(torch.equal(got[k], want[k]) for k in (13, 8, 12))
    assert len(net.calls) == 24 and kern.orient_launches == 8, "one orient launch per NEW frame: 6 + 1 + 1"
    w0, w1 = net.calls[:8], net.calls[8:16]
    caches = [c["cache"] for c in w0]
    assert all(isinstance(c, dict) for c in caches) and len({id(c) for c in caches}) == 8, "its own dict per orientation"
    assert [id(c["cache"]) for c in w1] == [id(c) for c in caches], "and the same one on the next window"
    for o, (flip, rev) in enumerate(E.orientations("hvt")):
        a, b = w0[o]["inputs"], w1[o]["inputs"]
        # consecutive windows hand over the SAME oriented objects, shifted by one frame: forwards in a forward orientation,
        # backwards in a reversed one
        if rev:
            assert all(a[j] is b[j + 1] for j in range(5))
            assert all(torch.equal(a[j], EC.torch_flip(clip[5 - j], flip)) for j in range(6)), "reversed: frames in order 5 - j"
        else:
            assert all(a[j + 1] is b[j] for j in range(5))
            assert all(torch.equal(a[j], EC.torch_flip(clip[j], flip)) for j in range(6))
        if flip == 0:
            assert all(a[j] is clip[5 - j if rev else j] for j in range(6)), "the identity orientation is the frame itself"
    assert sorted(ens._oriented) == [2, 3, 4, 5, 6, 7], "frames no window names any more are dropped"
    ens.reset()
    assert not ens._oriented and ens._caches is None
    # reuse off: no cache dict reaches the generator
    net2 = EC.FakeNetG(small=False)
    E.SelfEnsemble(net2, "h", kernels=EC.TorchKernels()).window(list(range(6)), clip[:6], reuse=False)
    assert [c["cache"] for c in net2.calls] == [None, None]


def test_batched_inputs_put_orientation_o_in_batch_rows_o_and_reversed_frames_in_slot_5_minus_j():
    frames = _frames(n=2)
    net = EC.FakeNetG(small=True)
    E.SelfEnsemble(net, "hvt", kernels=EC.TorchKernels())(frames)
    (call,) = net.calls
    for o, (flip, rev) in enumerate(E.orientations("hvt")):
        for j in range(6):
            assert torch.equal(call["inputs"][j][2 * o:2 * o + 2], EC.torch_flip(frames[5 - j if rev else j], flip)), (o, j)
    assert call["cache"] is None


def test_outputs_are_fresh_tensors():
    frames = _frames()
    net = EC.FakeNetG()
    outs = []
    real = net.forward
    net.forward = lambda *a, **k: outs.append(real(*a, **k)) or outs[-1]
    got = E.SelfEnsemble(net, "h", kernels=EC.TorchKernels())(frames)
    theirs = {t.data_ptr() for run in outs for t in run}
    assert all(t.data_ptr() not in theirs for t in got)


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_what_the_issue_names():
    assert len(set(EC.TAGS)) == len(EC.CASES)
    for shape in ((1, 1, 1), (3, 1, 2), (3, 2, 2), (3, 2, 6), (3, 3, 5), (6, 7, 9), (3, 6, 10), (6, 32, 48), (3, 4, 260), (3, 66, 130)):
        assert shape in EC.SHAPES
        assert {c.M for c in EC.CASES if c.shape == shape} == {1, 2, 4, 8}
    assert EC.FULL_CASE.shape == (3, 768, 1344) and EC.FULL_SIZE not in EC.SHAPES
    assert {4 * o for c in EC.CASES for o in c.offs} == {0, 4, 8, 12}
    assert any(c.special for c in EC.CASES)
    assert any(c.shape[2] % 4 == 0 and c.offs == (0,) for c in EC.CASES), "the 16 B path"
    assert any(c.shape[2] % 4 == 2 for c in EC.CASES) and any(c.shape[2] % 2 == 1 for c in EC.CASES)
    case = EC.CASE_BY_TAG["6x7x9_M8_inf_nan"]
    xs = EC.values(case, 8)
    assert sum(int(np.isinf(x).sum()) for x in xs) == 3 and sum(int(np.isnan(x).sum()) for x in xs) == 1
    r32 = EC.merge_ref32(xs, EC.flips_of(8))
    assert np.isnan(r32).any() and np.isinf(r32).any() and np.isfinite(r32).sum() > r32.size - 8, "they propagate, and only there"
    case = EC.CASE_BY_TAG["6x32x48_M8_mixed"]
    xs = EC.values(case, 8)
    assert all(x.dtype == np.float32 and -1 <= x.min() and x.max() <= 2 for x in xs)
    r32, r64 = EC.merge_ref32(xs, EC.flips_of(8)), EC.merge_ref64(xs, EC.flips_of(8))
    assert float(np.abs(r32 - r64).max()) <= 3 * 2.0 ** -24 * 2, "the tree: three roundings of sums below 16, scaled by 1/8"
    assert not np.array_equal(r32, EC.merge_ref32(xs, [0] * 8)), "the un-flip is seen"
    assert np.abs(r32[np.isfinite(r32)]).min() > 1e-30, "no denormal results (not covered)"
    a, s = EC.arena(xs[0], 3)
    assert s == EC.PAD + 3 and (a[:s] == EC.GUARD).all() and (a[s + xs[0].size:] == EC.GUARD).all() and a.size == xs[0].size + 2 * EC.PAD + 3
    for f in (0, 1, 2, 3):
        assert np.array_equal(EC.flip_np(EC.flip_np(xs[0], f), f), xs[0]), "a flip is an involution"
        assert np.array_equal(EC.flip_np(xs[0], f), EC.torch_flip(torch.from_numpy(xs[0]), f).numpy())


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def _header():
    return open(os.path.join(REPO, "include", "binens.h")).read()


def test_ens_library_header_and_binding_agree():
    """What is binens's own beside the bookkeeping of test_cpu_libraries.py: the codes, flags and limits, the two structs as the C
    compiler lays them out, and what the header says of the merge."""
    from bin_amd import _lib
    hdr = _header()
    for name, value in (("BINENS_E_ARG", -1), ("BINENS_E_SHAPE", -2)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1))
    assert (macro("BINENS_FLIP_W"), macro("BINENS_FLIP_H")) == (_lib.ENS_FLIP_W, _lib.ENS_FLIP_H) == (E.FLIP_W, E.FLIP_H) == (1, 2)
    assert (macro("BINENS_MAX_ORIENT"), macro("BINENS_MAX_SOURCES"), macro("BINENS_MAX_SLOTS")) == \
        (_lib.ENS_MAX_ORIENT, _lib.ENS_MAX_SOURCES, _lib.ENS_MAX_SLOTS) == (8, 6, 14)
    # the structs: sizes and offsets as the C compiler lays them out (the source asserts the sizes)
    assert re.search(r"typedef struct BinEnsOrient \{\s*const float\* src;\s*float\* dst\[BINENS_MAX_ORIENT\];\s*"
                     r"uint8_t flip\[BINENS_MAX_ORIENT\];\s*int32_t n_dst;\s*\} BinEnsOrient;", hdr)
    assert re.search(r"typedef struct BinEnsMerge \{\s*const float\* src\[BINENS_MAX_ORIENT\];\s*float\* dst;\s*\} BinEnsMerge;", hdr)
    O, M = _lib.BinEnsOrient, _lib.BinEnsMerge
    assert C.sizeof(O) == 88 and (O.src.offset, O.dst.offset, O.flip.offset, O.n_dst.offset) == (0, 8, 72, 80)
    assert C.sizeof(M) == 72 and (M.src.offset, M.dst.offset) == (0, 64)
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binens.hip")).read()
    assert "static_assert(sizeof(BinEnsOrient) == 88" in src and "static_assert(sizeof(BinEnsMerge) == 72" in src
    assert "propagate" in hdr and "balanced pairwise tree" in hdr and "Time reversal never reaches the library" in hdr


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.enslib()
    flips = (C.c_uint8 * 8)(0, 1, 2, 3, 0, 1, 2, 3)
    size = 3 * 4 * 8 * 4

    def merge_items(n=1, M=8):
        t = (_lib.BinEnsMerge * max(n, 1))()
        for i in range(n):
            for o in range(M):
                t[i].src[o] = 0x10000 + (i * 9 + o) * size
            t[i].dst = 0x10000 + (i * 9 + 8) * size
        return t

    def orient_items(n=1, nd=3):
        t = (_lib.BinEnsOrient * max(n, 1))()
        for i in range(n):
            t[i].src, t[i].n_dst = 0x10000 + i * 9 * size, nd
            for j in range(nd):
                t[i].dst[j], t[i].flip[j] = 0x10000 + (i * 9 + 1 + j) * size, j + 1
        return t
    merge = lambda t, n, M=8, f=flips, shape=(3, 4, 8): lib.binens_merge(t, n, M, f, *shape, None)
    orient = lambda t, n, shape=(3, 4, 8): lib.binens_orient(t, n, *shape, None)
    assert merge(merge_items(), 0) == 0 and orient(orient_items(), 0) == 0 and orient(None, 0) == 0      # nothing to do, nothing launched
    for M in (0, 3, 5, 6, 7, 9, 16, -1):
        assert merge(merge_items(), 1, M=M) == -1, M
    assert merge(merge_items(15), 15) == -1 and merge(merge_items(), -1) == -1 and merge(None, 1) == -1
    assert orient(orient_items(7), 7) == -1 and orient(orient_items(), -1) == -1 and orient(None, 1) == -1
    assert merge(merge_items(), 1, f=None) == -1
    assert merge(merge_items(), 1, f=(C.c_uint8 * 8)(0, 1, 2, 4)) == -1
    for shape in ((0, 4, 8), (3, 0, 8), (3, 4, 0), (-1, 4, 8)):
        assert merge(merge_items(), 1, shape=shape) == -1 and orient(orient_items(), 1, shape=shape) == -1
    assert merge(merge_items(), 1, shape=(2 ** 31 - 1, 2 ** 31 - 1, 4)) == -2 and orient(orient_items(), 1, shape=(2 ** 20, 2 ** 20, 2)) == -2
    t = merge_items()
    t[0].src[5] = None
    assert merge(t, 1) == -1
    t = merge_items(M=4)
    t[0].src[2] = None
    assert merge(t, 1, M=4) == -1
    t = merge_items()
    t[0].dst = None
    assert merge(t, 1) == -1
    t = merge_items()
    t[0].dst = t[0].src[3]                                                     # dst is a src
    assert merge(t, 1) == -1
    t = merge_items()
    t[0].dst = t[0].src[3] + size - 4                                          # ... or overlaps one by a single float
    assert merge(t, 1) == -1
    t = merge_items(2)
    t[1].dst = t[0].src[0]                                                     # ... of another item
    assert merge(t, 2) == -1
    t = merge_items()
    t[0].src[1] += 2                                                           # not a float's address
    assert merge(t, 1) == -1
    t = orient_items()
    t[0].dst[1] = t[0].src
    assert orient(t, 1) == -1
    t = orient_items()
    t[0].dst[2] = t[0].dst[0] + 4
    assert orient(t, 1) == -1
    t = orient_items()
    t[0].dst[1] = None
    assert orient(t, 1) == -1
    t = orient_items()
    t[0].src = None
    assert orient(t, 1) == -1
    for nd in (0, 9, -1):
        t = orient_items()
        t[0].n_dst = nd
        assert orient(t, 1) == -1
    t = orient_items()
    t[0].flip[0] = 4
    assert orient(t, 1) == -1


def test_ops_refuse_cpu_tensors_and_wrong_layouts():
    from bin_amd import ops
    x = torch.zeros(1, 3, 4, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ens_orient([x], None, [[1]])
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ens_merge([[x, x]], [0, 1])
    with pytest.raises(ValueError):
        ops.ens_merge([[x, x]], [0, 1, 2, 3])
    with pytest.raises(ValueError):
        ops.ens_orient([x], [[None, None]], [[1]])
    assert ops.ens_merge([], [0, 1]) == [] and ops.ens_orient([], None, []) == []


# ------------------------------------------------------------------------------------------------ the option
def test_val_self_ensemble_option():
    from bin_amd.options import options as option
    assert option.val_self_ensemble({}) == "" and option.val_self_ensemble({"train": {}}) == ""
    assert option.val_self_ensemble({"train": {"val_self_ensemble": None}}) == ""
    assert option.val_self_ensemble({"train": {"val_self_ensemble": "none"}}) == ""
    assert option.val_self_ensemble({"train": {"val_self_ensemble": "flipx4"}}) == "hv"
    assert option.val_self_ensemble({"train": {"val_self_ensemble": "tv"}}) == "vt"
    for bad in ("hh", "q", 4, True):
        with pytest.raises(ValueError, match="train.val_self_ensemble"):
            option.val_self_ensemble({"train": {"val_self_ensemble": bad}})
    for yml in ("bin_stage4_synthetic.yml", "bin_stage4_adobe240.yml"):
        text = open(os.path.join(REPO, "bin_amd", "options", yml)).read()
        assert re.search(r"(?m)^\s*# val_self_ensemble: hv", text), yml
        assert not re.search(r"(?m)^\s*val_self_ensemble:", text), "commented: off by default"


def test_cli_flag_and_harness_argument_exist_and_default_off():
    import inspect
    from bin_amd import harness, test as T
    args = T.parse_args(["--input_path", "a", "--output_path", "b", "--opt", "c"])
    assert args.self_ensemble is None
    assert T.parse_args(["--input_path", "a", "--output_path", "b", "--opt", "c", "--self_ensemble", "hvt"]).self_ensemble == "hvt"
    assert inspect.signature(harness.interpolate_clip).parameters["ensemble"].default is None
