"""Host side of the device frame cache (bin_amd/data/device_cache.py): the shared augmentation draws, the gather table, the
loader's index stream and the cache's refusals — none of it needs a GPU."""
import os
import random

import numpy as np
import pytest
import torch

from device_cache_cases import arena_of, bits, gather_reference
from host_fixtures import make_adobe_tree


@pytest.fixture(scope="module")
def adobe(tmp_path_factory):
    return make_adobe_tree(str(tmp_path_factory.mktemp("adobe")))


@pytest.fixture(scope="module")
def windows(adobe):
    from bin_amd.data.BIN_dataset import make_window_list
    kept, _ = make_window_list(adobe, mode="train", shuffle=False)
    return sorted(kept, key=lambda w: w[3])


@pytest.mark.parametrize("data_aug", [True, False])
@pytest.mark.parametrize("crop", [(64, 96), (32, 48), (17, 29)])
def test_shared_draws_and_kernel_formula_equal_load_window(windows, crop, data_aug):
    """draw_window_aug + window_table + the kernel's formula on imread_u8 frames == load_window + BINDataset._to_tensor,
    bit for bit, and both leave `random` in the same state."""
    from bin_amd.data.BIN_dataset import BINDataset, draw_window_aug, load_window
    from bin_amd.data.device_cache import window_table
    frames, index = arena_of(windows)
    size = (3,) + crop
    seen = set()
    for seed in range(6):
        win = windows[seed % len(windows)]
        random.seed(seed)
        draw = draw_window_aug(size, data_aug)
        after = random.getstate()
        seen.add((draw[0], draw[3]))
        out = gather_reference(frames, window_table([win], [draw], index), crop)
        random.seed(seed)
        LQs, GTenh, GTinp, key = load_window(win, size, data_aug)
        assert random.getstate() == after and key == win[3]
        for got, host in ((out[0:6, 0], LQs), (out[6:12, 0], GTenh), (out[12:17, 0], GTinp)):
            ref = BINDataset._to_tensor(host).numpy()
            assert got.shape == ref.shape
            assert np.array_equal(bits(got), bits(ref))
    if data_aug:
        assert len(seen) > 1                     # the seeds reach both orders / flips
    else:
        assert seen == {(True, False)}           # no aug: reversed (as in the reference), never flipped


def test_table_puts_reversed_windows_in_reverse_slot_order(windows):
    from bin_amd.data.device_cache import N_SLOTS, window_table
    _, index = arena_of(windows)
    win = windows[1]
    blurry, sharp, mid, _ = win
    rows = window_table([win, win], [(False, 5, 7, False), (True, 1, 2, True)], index)
    assert rows.dtype == np.int32 and rows.shape == (2, N_SLOTS + 3)
    assert rows[0, :N_SLOTS].tolist() == [index[p] for p in blurry + sharp + mid]
    assert rows[1, :N_SLOTS].tolist() == [index[p] for p in blurry[::-1] + sharp[::-1] + mid[::-1]]
    assert rows[0, N_SLOTS:].tolist() == [5, 7, 0] and rows[1, N_SLOTS:].tolist() == [1, 2, 1]


def _dataset(adobe, crop=(3, 32, 48)):
    from bin_amd.data import create_dataset
    random.seed(0)
    return create_dataset({"mode": "BIN", "name": "train", "dataroot_GT": adobe, "dataroot_LQ": adobe, "LQ_size": list(crop),
                           "data_type": "img", "phase": "train"})


@pytest.mark.parametrize("world_rank", [None, (2, 0), (2, 1)])
def test_loader_index_stream_matches_create_dataloader(adobe, world_rank):
    """Same batches of indices, same ragged-batch drop, same length as the host DataLoader (no sampler, DistIterSampler)."""
    from bin_amd.data import create_dataloader
    from bin_amd.data.data_sampler import DistIterSampler
    from bin_amd.data.device_cache import DeviceWindowLoader
    ds = _dataset(adobe)
    for batch in (2, 3):
        sampler = None if world_rank is None else DistIterSampler(ds, *world_rank, ratio=3)
        host = create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": 0}, {"dist": False, "gpu_ids": [0]},
                                 sampler)
        dev = DeviceWindowLoader(ds, batch, sampler, cache=object())            # no arena: the index stream only
        for epoch in (0, 1):
            if sampler is not None:
                sampler.set_epoch(epoch)
            want = [list(b) for b in host.batch_sampler]
            assert list(dev.index_batches()) == want and len(dev) == len(host) == len(want)
            n = len(sampler) if sampler is not None else len(ds)
            assert len(want) == n // batch                                        # drop_last


def _write(path, arr):
    from PIL import Image
    Image.fromarray(arr).save(path)
    return path


def _window(paths):
    return [paths[0:6], paths[6:12], paths[12:17], "k"]


@pytest.mark.parametrize("case", ["sizes", "grey", "max_gb"])
def test_cache_refuses_before_any_device_work(tmp_path, case):
    """Mixed sizes, a grey frame and an arena over max_gb raise ValueError from the headers alone: nothing is decoded and
    nothing is allocated (on a machine without a GPU, any device call would raise something else)."""
    from bin_amd.data.device_cache import DeviceFrameCache
    g = np.random.Generator(np.random.PCG64(0))
    paths = [_write(str(tmp_path / f"{i:02d}.png"), g.integers(0, 256, (20, 30, 3), dtype=np.uint8)) for i in range(17)]
    max_gb, match = 64, None
    if case == "sizes":
        paths[9] = _write(str(tmp_path / "big.png"), g.integers(0, 256, (20, 31, 3), dtype=np.uint8))
        match = r"differ in size: .* is 20x30, .*big\.png is 20x31"
    elif case == "grey":
        paths[3] = _write(str(tmp_path / "grey.png"), g.integers(0, 256, (20, 30), dtype=np.uint8))
        match = r"grey\.png has 1 channel"
    else:
        max_gb, match = 30000 / 1e9, r"17 frames of 20x30x3 need 0\.00 GB \(30600 bytes\), more than device_cache_max_gb"
    with pytest.raises(ValueError, match=match):
        DeviceFrameCache([_window(paths)], torch.device("cuda", 0), max_gb=max_gb)


def test_rgba_frames_count_as_colour(tmp_path):
    from bin_amd.data.device_cache import _frame_shape
    p = _write(str(tmp_path / "a.png"), np.zeros((5, 7, 4), np.uint8))
    assert _frame_shape(p) == (5, 7, 4)
    assert _frame_shape(_write(str(tmp_path / "b.png"), np.zeros((5, 7, 3), np.uint8))) == (5, 7, 3)


def test_option_file_documents_the_device_cache():
    from conftest import REPO
    text = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_adobe240.yml")).read()
    assert "# device_cache: true" in text and "# device_cache_max_gb: 64" in text
