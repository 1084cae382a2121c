"""Blurry training inputs synthesised from sharp frames (dataset option `blur_window`), host side: the arithmetic the kernel's
integer form rests on, the sharp-only window list against the reference script's rule and against today's make_window_list on
the written-out folders, the host loader on either tree, the option's validation and draws, and tools/make_blur_folder.py."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from blur_cases import SHARP_CLIPS, expected_windows, make_sharp_tree, script_blur, script_centres
from conftest import REPO


def _tool():
    spec = importlib.util.spec_from_file_location("make_blur_folder", os.path.join(REPO, "tools", "make_blur_folder.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------ 1. arithmetic
def test_float32_mean_truncated_is_the_integer_quotient_for_every_sum():
    """Every odd L in 1 .. 33 and every byte sum S in 0 .. 255 L: the script's float32(S) / float(L) truncated to uint8 is
    S // L (73 712 pairs), and so is the kernel's (S * ceil(2^23 / L)) >> 23, whose factors fit 24 bits."""
    pairs = 0
    for L in range(1, 34, 2):
        S = np.arange(0, 255 * L + 1, dtype=np.int64)
        script = (S.astype("float32") / float(L)).astype("uint8")
        assert script.dtype == np.uint8 and np.array_equal(script, S // L), L
        m = (2 ** 23 - 1) // L + 1
        assert m < 2 ** 24 and S.max() < 2 ** 24 and int(S.max()) * m < 2 ** 32
        assert np.array_equal((S * m) >> 23, S // L), L
        pairs += len(S)
    assert pairs == 73712


@pytest.mark.parametrize("L", [1, 3, 7, 11, 33])
def test_blur_average_equals_the_script_on_random_stacks(L):
    from bin_amd.data.BIN_dataset import blur_average
    g = np.random.Generator(np.random.PCG64(L))
    for stack in (g.integers(0, 256, (L, 9, 14, 3), dtype=np.uint8), np.full((L, 4, 5, 3), 255, np.uint8),
                  g.integers(250, 256, (L, 6, 6, 3), dtype=np.uint8)):
        got = blur_average(stack)
        assert got.dtype == np.uint8 and np.array_equal(got, script_blur(stack))
        assert np.array_equal(blur_average(list(stack)), got)
    with pytest.raises(ValueError):
        blur_average(np.zeros((34, 2, 2, 3), np.uint8))
    with pytest.raises(ValueError):
        blur_average(np.zeros((3, 2, 2, 3), np.float32))


# ------------------------------------------------------------------ 2. the window list
RULE_CLIPS = SHARP_CLIPS + (("clipF", 0, 64), ("clipG", 41, 71), ("clipH", 1, 96), ("clipI", 7, 23), ("clipJ", 1, 105))


@pytest.fixture(scope="module")
def small_tree(tmp_path_factory):
    """The clip lengths and first numbers of the rule, on 8 x 12 frames (the list does not look at the pixels)."""
    return make_sharp_tree(str(tmp_path_factory.mktemp("small")), clips=RULE_CLIPS, hw=(8, 12))


@pytest.mark.parametrize("window", [1, 7, 11, 15, 17, 33])
def test_sharp_only_list_follows_the_script_rule(small_tree, window):
    from bin_amd.data.BIN_dataset import clip_blur_centres, make_sharp_window_list
    h = (window - 1) // 2
    for clip, first, n in RULE_CLIPS:
        got_first, centres, usable = clip_blur_centres(os.path.join(small_tree, "train", clip), h)
        want_centres, want_usable = script_centres(first, n, window)
        assert (centres, usable) == (want_centres, want_usable), clip
        assert got_first == first
        assert centres == [first + 16 + 8 * i for i in range(n // 8 - 2)]
        if h <= 7:
            assert usable == centres                                              # the script's own range never leaves the clip
    kept, rest = make_sharp_window_list(small_tree, "train", shuffle=False, blur_window=window)
    want = expected_windows(RULE_CLIPS, window)
    assert rest == [] and len(kept) == len(want) and {w[3] for w in kept} == set(want)
    name = lambda clip, k: os.path.join(small_tree, "train", clip, f"{k:05d}.png")
    for blurry, sharp, mid, key in kept:
        clip = key[:5]
        cs, mids = want[key]
        assert sharp == [name(clip, c) for c in cs] and blurry == sharp and mid == [name(clip, c) for c in mids]
        assert all(os.path.isfile(p) for p in sharp + mid)
    if window == 11:
        assert {k[:5] for k in want} == {"clipA", "clipB", "clipC", "clipF", "clipG", "clipH", "clipJ"}    # D, E, I: too short
    if window == 33:
        assert want and len(want) < len(expected_windows(RULE_CLIPS, 11))          # the clip ends cost windows


def test_first_file_one_gives_the_centres_the_reference_lists(small_tree):
    """For a clip numbered from 00001 the centres are 17, 25, 33, ... (what the reference's test_list/*_im_list.txt hold)."""
    from bin_amd.data.BIN_dataset import clip_blur_centres
    _, centres, _ = clip_blur_centres(os.path.join(small_tree, "train", "clipA"), 5)
    assert centres == [17, 25, 33, 41, 49, 57, 65, 73]


def test_gap_in_the_sharp_files_is_refused(tmp_path):
    from bin_amd.data.BIN_dataset import make_sharp_window_list
    root = make_sharp_tree(str(tmp_path), clips=(("clipA", 1, 70),), hw=(4, 4))
    os.remove(os.path.join(root, "train", "clipA", "00033.png"))
    with pytest.raises(ValueError, match="not numbered consecutively"):
        make_sharp_window_list(root, "train", blur_window=11)


@pytest.mark.parametrize("window", [1, 11, 17, 33])
def test_written_out_folder_gives_the_same_windows_by_key(small_tree, tmp_path, window):
    """tools/make_blur_folder.py writes what the script would have; today's make_window_list reads it back to the same
    windows under the same keys (the blurry paths point into <mode>_blur there, at the same clip and number), and every
    written PNG is the script's mean of its sharp files."""
    import shutil
    from bin_amd.data.BIN_dataset import make_sharp_window_list, make_window_list
    from bin_amd.data.util import imread_u8
    root = str(tmp_path / "t")
    shutil.copytree(small_tree, root)
    written = _tool().make_blur_folder(root, "train", window)
    h = (window - 1) // 2
    for clip, first, n in RULE_CLIPS:
        _, usable = script_centres(first, n, window)
        assert written[clip] == [f"{c:05d}.png" for c in usable]
        assert open(os.path.join(root, "train_list", clip + "_im_list.txt")).read().split("\n") == (written[clip] or [""])
        for c in usable[:2] + usable[-1:]:
            stack = [imread_u8(os.path.join(root, "train", clip, f"{k:05d}.png")) for k in range(c - h, c + h + 1)]
            assert np.array_equal(imread_u8(os.path.join(root, "train_blur", clip, f"{c:05d}.png")), script_blur(stack))
    old, _ = make_window_list(root, "train", shuffle=False)
    new, _ = make_sharp_window_list(root, "train", shuffle=False, blur_window=window)
    old, new = {w[3]: w for w in old}, {w[3]: w for w in new}
    assert old.keys() == new.keys() and len(old) == len(expected_windows(RULE_CLIPS, window))
    for key, (blurry, sharp, mid, _) in old.items():
        assert new[key][1] == sharp and new[key][2] == mid
        assert [p.replace(os.sep + "train_blur" + os.sep, os.sep + "train" + os.sep) for p in blurry] == new[key][0]


# ------------------------------------------------------------------ 3. the host loader
@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    """(sharp-only tree, the same tree with the folders of window 11 written out), 352 x 640."""
    import shutil
    sharp = make_sharp_tree(str(tmp_path_factory.mktemp("sharp")))
    full = str(tmp_path_factory.mktemp("full") / "t")
    shutil.copytree(sharp, full)
    _tool().make_blur_folder(full, "train", 11)
    return sharp, full


def _dataset(root, blur_window=None, crop=(3, 64, 96)):
    from bin_amd.data import create_dataset
    random.seed(0)
    opt = {"mode": "BIN", "name": "train", "dataroot_GT": root, "dataroot_LQ": root, "LQ_size": list(crop),
           "data_type": "img", "phase": "train"}
    if blur_window is not None:
        opt["blur_window"] = blur_window
    return create_dataset(opt)


def _host_loader(ds, batch, sampler=None):
    from bin_amd.data import create_dataloader
    return create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": 0}, {"dist": False, "gpu_ids": [0]}, sampler)


class _InOrder(torch.utils.data.Sampler):
    def __init__(self, order):
        self.order = order

    def __iter__(self):
        return iter(self.order)

    def __len__(self):
        return len(self.order)


def test_host_loader_on_sharp_tree_equals_todays_on_written_tree(trees):
    """blur_window: 11 on the sharp-only tree against today's loader on the written-out tree: same `random` state, n_workers 0,
    3 batches, windows matched by key (the two lists are shuffled from different os.listdir orders), bit for bit."""
    sharp, full = trees
    assert not os.path.exists(os.path.join(sharp, "train_blur")) and not os.path.exists(os.path.join(sharp, "train_list"))
    new, old = _dataset(sharp, 11), _dataset(full)
    assert len(new) == len(old) == 7 and sorted(w[3] for w in new.all_paths) == sorted(w[3] for w in old.all_paths)
    by_key = {w[3]: i for i, w in enumerate(old.all_paths)}
    order = [by_key[w[3]] for w in new.all_paths]
    got = []
    for loader in (_host_loader(new, 2), _host_loader(old, 2, _InOrder(order))):
        random.seed(321)
        got.append([b for _, b in zip(range(3), loader)])
        assert len(got[-1]) == 3
    for nb, ob in zip(*got):
        assert nb["key"] == ob["key"]
        for k in ("LQs", "GTenh", "GTinp"):
            assert nb[k].dtype == torch.float32 and nb[k].shape == ob[k].shape
            assert torch.equal(nb[k].view(torch.int32), ob[k].view(torch.int32)), k
        assert not torch.equal(nb["LQs"], nb["GTenh"])                            # the blurry inputs are not the sharp frames


# ------------------------------------------------------------------ 4. the option
@pytest.mark.parametrize("bad", [0, 2, 10, 35, -3, [], [11, 12], [11, 35], "11", 11.0, True, [7, None]])
def test_blur_window_validation(trees, bad):
    with pytest.raises(ValueError, match="blur_window"):
        _dataset(trees[0], bad)


def test_even_window_error_names_the_reason(trees):
    with pytest.raises(ValueError, match="odd"):
        _dataset(trees[0], 12)


def test_absent_option_is_todays_dataset(trees):
    ds = _dataset(trees[1])
    assert ds.blur_window is None
    assert _dataset(trees[1], None).all_paths == ds.all_paths
    with pytest.raises(FileNotFoundError):
        _dataset(trees[0])                                                        # today's list needs <mode>_blur


def test_list_draws_one_more_value_per_sample_and_integer_none(trees):
    """After the same samples: an integer leaves `random` exactly where today's loader leaves it; a list has made one more
    random.choice per sample, after the four draws of draw_window_aug."""
    from bin_amd.data.BIN_dataset import draw_window_aug, load_window
    sharp, full = trees
    crop = (3, 64, 96)
    old, new_int, new_list = _dataset(full, None, crop), _dataset(sharp, 11, crop), _dataset(sharp, [3, 7, 11], crop)
    assert new_int.blur_window == 11 and new_list.blur_window == (3, 7, 11)
    random.seed(99)
    old[0], old[1]
    after_old = random.getstate()
    random.seed(99)
    new_int[0], new_int[1]
    assert random.getstate() == after_old
    random.seed(99)
    new_list[0], new_list[1]
    after_list = random.getstate()
    assert after_list != after_old
    random.seed(99)
    halves = []
    for _ in range(2):
        draw_window_aug(crop)
        halves.append(random.choice((3, 7, 11)) // 2)
    assert random.getstate() == after_list
    # and the drawn exposure is the one used
    random.seed(99)
    LQs, _, _, _ = load_window(new_list.all_paths[0], crop, blur_window=new_list.blur_window)
    random.seed(99)
    reverse, y0, x0, flip = draw_window_aug(crop)
    from bin_amd.data.BIN_dataset import exposure_paths
    from bin_amd.data.util import imread_u8
    centre = new_list.all_paths[0][0][-1 if reverse else 0]
    want = script_blur([imread_u8(p) for p in exposure_paths(centre, halves[0])])[y0:y0 + 64, x0:x0 + 96]
    want = (want[:, ::-1] if flip else want).astype(np.float32) / 255.
    assert np.array_equal(LQs[0], want)


def test_a_list_needs_every_centre_usable_at_its_largest_exposure(trees):
    """[5, 11, 17]: h = 8 reaches past the last file of a clip whose length is a multiple of 8."""
    ds = _dataset(trees[0], [5, 11, 17])
    assert sorted(w[3] for w in ds.all_paths) == sorted(expected_windows(SHARP_CLIPS, 17))
    assert len(ds) == 6 < len(_dataset(trees[0], 11))


# ------------------------------------------------------------------ 5. the tool, the table, the cache's host side
def test_tool_refuses_an_existing_output_folder(trees, tmp_path):
    import subprocess
    import sys
    tool = _tool()
    with pytest.raises(FileExistsError, match="train_blur"):
        tool.make_blur_folder(trees[1], "train", 11)
    root = make_sharp_tree(str(tmp_path), clips=(("clipA", 1, 24),), hw=(4, 6))
    os.makedirs(os.path.join(root, "train_list"))
    with pytest.raises(FileExistsError, match="train_list"):
        tool.make_blur_folder(root, "train", 11)
    assert not os.path.exists(os.path.join(root, "train_blur"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_blur_folder.py"), "--root", root, "--window", "11"],
                       capture_output=True, text=True)
    assert r.returncode != 0 and "exists" in r.stderr
    os.rmdir(os.path.join(root, "train_list"))
    r = subprocess.run([sys.executable, os.path.join(REPO, "tools", "make_blur_folder.py"), "--root", root, "--window", "11"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.listdir(os.path.join(root, "train_blur", "clipA")) == ["00017.png"]
    with pytest.raises(ValueError, match="odd"):
        tool.make_blur_folder(str(tmp_path / "x"), "train", 8)


def test_table_gains_the_h_column_only_when_asked(trees):
    from bin_amd.data.device_cache import N_SLOTS, window_table
    ds = _dataset(trees[0], 11)
    win = ds.all_paths[0]
    index = {p: i for i, p in enumerate(sorted(set(win[0] + win[1] + win[2])))}
    draws = [(False, 5, 7, False), (True, 1, 2, True)]
    plain = window_table([win, win], draws, index)
    rows = window_table([win, win], draws, index, [5, 0])
    assert plain.shape == (2, N_SLOTS + 3) and rows.shape == (2, N_SLOTS + 4) and rows.dtype == np.int32
    assert np.array_equal(rows[:, :N_SLOTS + 3], plain) and rows[:, N_SLOTS + 3].tolist() == [5, 0]
    assert rows[0, :6].tolist() == rows[0, 6:12].tolist()                         # a blurry id is its centre sharp frame


def test_cache_size_refusal_counts_the_sharp_arena(trees):
    """Per clip every file from the first centre - h_max to the last + h_max: refused from the headers alone, with the count."""
    from bin_amd.data.device_cache import DeviceFrameCache
    ds = _dataset(trees[0], 11)
    want = sum(cs[-1][0][-1] - cs[0][0][0] + 11 for cs in
               [sorted(v for k, v in expected_windows(SHARP_CLIPS, 11).items() if k.startswith(c)) for c in ("clipA", "clipB", "clipC")])
    with pytest.raises(ValueError, match=rf"{want} frames of 352x640x3 need .* more than device_cache_max_gb"):
        DeviceFrameCache(ds.all_paths, torch.device("cuda", 0), max_gb=0.001, blur_half=5)


def test_option_file_documents_blur_window():
    text = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_adobe240.yml")).read()
    assert "# blur_window: 11" in text and "device_cache_max_gb" in text
