"""-m gpu: binhip_gather_windows_blur against the numpy restatement of the reference's blurry-frame script (blur_cases.py), its
host-side checks and error codes, and the device-cache loader with `blur_window` against the host loader with it at
n_workers 0 (same `random` state => same batches bit for bit), down to one training step fed by each."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

from blur_cases import SHARP_CLIPS, bits, blur_gather_reference, expected_windows, make_sharp_tree
from device_cache_cases import gather_reference

pytestmark = pytest.mark.gpu

H, W = 24, 301               # odd width: source rows of 903 bytes start at every dword offset
NF = 40                      # frames: room for h = 16 around more than one centre
HALVES = {"h0": (0,), "h1": (1,), "h5": (5,), "h16": (16,), "mixed": (0, 1, 5, 16, 3, 8, 2, 16, 0)}


@pytest.fixture(scope="module")
def arenas():
    g = np.random.Generator(np.random.PCG64(3))
    host = {"random": g.integers(0, 256, (NF, H, W, 3), dtype=np.uint8), "all255": np.full((NF, H, W, 3), 255, np.uint8)}
    return {k: (v, torch.from_numpy(v).cuda()) for k, v in host.items()}


def _table(g, n, n_slots, n_blur, crop, where, flip, halves, n_frames=NF, frame=(H, W)):
    """Rows [ids, y0, x0, flip, h]; blurry centres are legal for the row's h, and the first two blurry slots of every row sit
    on the first and the last legal centre (h and n_frames - 1 - h)."""
    ch, cw = crop
    fh, fw = frame
    ys = {"tl": (0, 0), "tr": (0, fw - cw), "bl": (fh - ch, 0), "br": (fh - ch, fw - cw), "c": ((fh - ch) // 2, (fw - cw) // 2)}
    rows = np.empty((n, n_slots + 4), np.int32)
    for b in range(n):
        h = halves[b % len(halves)]
        rows[b, :n_slots] = g.integers(0, n_frames, n_slots)
        rows[b, :n_blur] = g.integers(h, n_frames - h, n_blur)
        rows[b, :min(n_blur, 2)] = (h, n_frames - 1 - h)[:min(n_blur, 2)]
        y0, x0 = ys[where] if where != "rand" else (g.integers(0, fh - ch + 1), g.integers(0, fw - cw + 1))
        rows[b, n_slots:] = (y0, x0, flip if flip is not None else b % 2, h)
    return rows


@pytest.mark.parametrize("n", [1, 9])
@pytest.mark.parametrize("cw", [1, 3, 5, 256])
@pytest.mark.parametrize("hs", list(HALVES))
def test_gather_windows_blur_matches_restatement(arenas, n, cw, hs):
    """Random bytes: h x cw x ch x crop position x flip x n x n_blur, every combination, compared as float bit patterns."""
    from bin_amd import ops
    host, frames = arenas["random"]
    g = np.random.Generator(np.random.PCG64(cw * 1000 + n * 10 + len(hs)))
    n_slots = 17
    for ch in (1, 7):
        for where in ("tl", "tr", "bl", "br", "c", "rand"):
            for flip in (0, 1, None):
                for n_blur in (0, 6, n_slots):
                    tab = _table(g, n, n_slots, n_blur, (ch, cw), where, flip, HALVES[hs])
                    out = ops.gather_windows_blur(frames, tab, (ch, cw), n_blur)
                    assert out.shape == (n_slots, n, 3, ch, cw) and out.dtype == torch.float32
                    ref = blur_gather_reference(host, tab, (ch, cw), n_blur)
                    assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), (ch, cw, where, flip, n_blur)


@pytest.mark.parametrize("cw", [1, 3, 5, 256])
@pytest.mark.parametrize("hs", list(HALVES))
def test_gather_windows_blur_largest_sums(arenas, cw, hs):
    """All-255 bytes: every sum is 255 L, the largest a 16-bit half of the packed accumulators has to hold; the mean is 255."""
    from bin_amd import ops
    host, frames = arenas["all255"]
    g = np.random.Generator(np.random.PCG64(cw))
    for n_blur in (0, 6, 17):
        for n, ch in ((9, 7), (1, 1)):
            tab = _table(g, n, 17, n_blur, (ch, cw), "rand", None, HALVES[hs])
            out = ops.gather_windows_blur(frames, tab, (ch, cw), n_blur).cpu().numpy()
            assert np.array_equal(bits(out), bits(blur_gather_reference(host, tab, (ch, cw), n_blur)))
            assert np.array_equal(bits(out), bits(np.ones_like(out)))


@pytest.mark.parametrize("frame", [(5, 7), (3, 9), (6, 10)])
def test_gather_windows_blur_frames_of_any_byte_size(frame):
    """H W 3 = 105, 81, 180 bytes: frames that start at every dword offset, so each frame of an exposure is realigned."""
    from bin_amd import ops
    fh, fw = frame
    g = np.random.Generator(np.random.PCG64(fh * fw))
    host = g.integers(0, 256, (NF, fh, fw, 3), dtype=np.uint8)
    frames = torch.from_numpy(host).cuda()
    for crop in ((fh, fw), (2, 5), (1, 1), (3, 4)):
        for flip in (0, 1, None):
            tab = _table(g, 9, 17, 6, crop, "rand", flip, HALVES["mixed"], frame=frame)
            out = ops.gather_windows_blur(frames, tab, crop, 6)
            assert np.array_equal(bits(out.cpu().numpy()), bits(blur_gather_reference(host, tab, crop, 6))), (crop, flip)


@pytest.mark.parametrize("cw", [1, 3, 5, 256])
def test_no_blurry_slot_equals_gather_windows(arenas, cw):
    """n_blur = 0: the same bits as ops.gather_windows on the same rows (whatever the h column holds), and as its restatement."""
    from bin_amd import ops
    host, frames = arenas["random"]
    g = np.random.Generator(np.random.PCG64(cw + 50))
    for n, n_slots in ((1, 17), (9, 17), (9, 1)):
        for ch in (1, 7):
            for flip in (0, 1, None):
                tab = _table(g, n, n_slots, 0, (ch, cw), "rand", flip, HALVES["mixed"])
                a = ops.gather_windows_blur(frames, tab, (ch, cw), 0)
                b = ops.gather_windows(frames, tab[:, :n_slots + 3], (ch, cw))
                assert torch.equal(a.view(torch.int32), b.view(torch.int32))
                assert np.array_equal(bits(a.cpu().numpy()), bits(gather_reference(host, tab[:, :n_slots + 3], (ch, cw))))


def test_h_zero_blurry_slot_is_a_plain_slot(arenas):
    from bin_amd import ops
    host, frames = arenas["random"]
    g = np.random.Generator(np.random.PCG64(77))
    tab = _table(g, 9, 17, 6, (7, 33), "rand", None, (0,))
    a = ops.gather_windows_blur(frames, tab, (7, 33), 6)
    assert torch.equal(a.view(torch.int32), ops.gather_windows(frames, tab[:, :20], (7, 33)).view(torch.int32))


def test_gather_windows_blur_rejects_bad_tables_on_the_host(arenas):
    from bin_amd import ops
    _, frames = arenas["random"]
    good = np.zeros((2, 21), np.int32)
    good[:, :17] = 20
    good[:, 20] = 5
    ops.gather_windows_blur(frames, good, (4, 10), 6)
    cases = ((3, NF, "frame id"), (9, -1, "frame id"), (17, H - 3, "offset"), (18, W - 9, "offset"), (19, 2, "flip"),
             (20, 17, r"h outside \[0, 16\]"), (20, -1, r"h outside \[0, 16\]"),
             (0, 4, "leaves the arena"), (5, NF - 5, "leaves the arena"))
    for col, val, msg in cases:
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError, match=msg):
            ops.gather_windows_blur(frames, bad, (4, 10), 6)
    edge = good.copy()
    edge[1, 0], edge[1, 5], edge[1, 8] = 5, NF - 6, 0                            # first / last legal centre; slot 8 is not blurry
    ops.gather_windows_blur(frames, edge, (4, 10), 6)
    with pytest.raises(ValueError, match="does not fit"):
        ops.gather_windows_blur(frames, good, (H + 1, 10), 6)
    for n_blur in (-1, 18):
        with pytest.raises(ValueError, match="n_blur"):
            ops.gather_windows_blur(frames, good, (4, 10), n_blur)
    with pytest.raises(ValueError, match=r"n_slots \+ 4"):
        ops.gather_windows_blur(frames, good[:, :4], (4, 10), 0)
    # clip extents: [0, 18) and [18, 40); a centre 20 with h 5 reads 15 .. 25 and crosses; 23 and 12 do not
    clips = np.array([[0, 18], [18, NF]])
    with pytest.raises(ValueError, match="crosses a clip boundary"):
        ops.gather_windows_blur(frames, good, (4, 10), 6, clip_ranges=clips)
    inside = good.copy()
    inside[:, :6] = (23, 12, 34, 5, 29, 12)
    ops.gather_windows_blur(frames, inside, (4, 10), 6, clip_ranges=clips)
    ops.gather_windows_blur(frames, inside, (4, 10), 6, clip_ranges=clips[::-1])
    for centre in (13, 22):                                                   # 8 .. 18 and 17 .. 27
        bad = inside.copy()
        bad[0, 2] = centre
        with pytest.raises(ValueError, match="crosses a clip boundary"):
            ops.gather_windows_blur(frames, bad, (4, 10), 6, clip_ranges=clips)
    with pytest.raises(ValueError, match="crosses a clip boundary"):           # a range before the first clip
        ops.gather_windows_blur(frames, inside, (4, 10), 6, clip_ranges=np.array([[8, NF]]))
    torch.cuda.synchronize()


def test_gather_windows_blur_error_codes(arenas):
    from bin_amd import _lib as L
    lib = L.lib()
    _, frames = arenas["random"]
    table = torch.zeros((2, 21), dtype=torch.int32, device="cuda")
    out = torch.empty((17, 2, 3, 8, 8), dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f, t, o = (C.c_void_p(x.data_ptr()) for x in (frames, table, out))
    fn = lib.binhip_gather_windows_blur
    assert fn(None, NF, H, W, t, 2, 17, 6, 8, 8, o, s) == -1                    # BINHIP_E_ARG
    assert fn(f, NF, H, W, None, 2, 17, 6, 8, 8, o, s) == -1
    assert fn(f, NF, H, W, t, 2, 17, 6, 8, 8, None, s) == -1
    assert fn(f, NF, H, W, t, 2, 17, 6, H + 1, 8, o, s) == -2                   # BINHIP_E_SHAPE: crop
    assert fn(f, NF, H, W, t, 2, 17, 6, 8, W + 1, o, s) == -2
    assert fn(f, NF, H, W, t, 2, 0, 0, 8, 8, o, s) == -2                        # n_slots
    assert fn(f, NF, H, W, t, 2, 33, 6, 8, 8, o, s) == -2
    assert fn(f, NF, H, W, t, 2, 17, -1, 8, 8, o, s) == -2                      # n_blur
    assert fn(f, NF, H, W, t, 2, 17, 18, 8, 8, o, s) == -2
    for nf, fh, fw in ((0, H, W), (NF, 0, W), (NF, H, 0)):
        assert fn(f, nf, fh, fw, t, 2, 17, 6, 8, 8, o, s) == -2
    for n, ch, cw in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert fn(f, NF, H, W, t, n, 17, 6, ch, cw, o, s) == -2
    for n_blur in (0, 6, 17):
        assert fn(f, NF, H, W, t, 2, 17, n_blur, 8, 8, o, s) == 0
    torch.cuda.synchronize()
    assert lib.binhip_version() == 622


# ------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def sharp(tmp_path_factory):
    return make_sharp_tree(str(tmp_path_factory.mktemp("sharp")))


def _dataset(root, blur_window, crop):
    from bin_amd.data import create_dataset
    random.seed(0)
    return create_dataset({"mode": "BIN", "name": "train", "dataroot_GT": root, "dataroot_LQ": root, "LQ_size": list(crop),
                           "data_type": "img", "phase": "train", "blur_window": blur_window})


def _loaders(ds, batch, sampler):
    from bin_amd.data import create_dataloader
    opt = {"dist": False, "gpu_ids": [0]}
    host = create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": 0}, opt, sampler)
    dev = create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": 0, "device_cache": True}, opt, sampler)
    return host, dev


def _expected_arena_paths(root, ds, window_max):
    """Per clip, in the order the dataset's list first names it: every file from the first centre - h to the last + h."""
    want = expected_windows(SHARP_CLIPS, window_max)
    h = window_max // 2
    paths, ranges, seen = [], [], []
    for w in ds.all_paths:
        if w[3][:5] not in seen:
            seen.append(w[3][:5])
    for clip in seen:
        cs = [c for k, (c6, _) in want.items() if k[:5] == clip for c in c6]
        ranges.append([len(paths), len(paths) + max(cs) - min(cs) + 2 * h + 1])
        paths += [os.path.join(root, "train", clip, f"{k:05d}.png") for k in range(min(cs) - h, max(cs) + h + 1)]
    return paths, ranges


@pytest.mark.parametrize("blur_window", [11, [5, 11, 17]])
@pytest.mark.parametrize("world_rank", [None, (2, 1)])
def test_device_loader_batches_equal_host_loader(sharp, world_rank, blur_window):
    from bin_amd.data.data_sampler import DistIterSampler
    from bin_amd.data.device_cache import DeviceWindowLoader
    from bin_amd.data.util import imread_u8
    ds = _dataset(sharp, blur_window, (3, 64, 96))
    sampler = None if world_rank is None else DistIterSampler(ds, *world_rank, ratio=4)
    host, dev = _loaders(ds, 2, sampler)
    assert isinstance(dev, DeviceWindowLoader) and len(dev) == len(host) >= 3
    paths, ranges = _expected_arena_paths(sharp, ds, blur_window if isinstance(blur_window, int) else max(blur_window))
    assert dev.cache.paths == paths and dev.cache.clip_ranges.tolist() == ranges
    assert dev.cache.shape == (len(paths), 352, 640, 3) and not any("_blur" in p for p in paths)
    if world_rank is None:                                                     # the arena's bytes are those files, in that order
        arena = dev.cache.frames.cpu().numpy()
        for i in range(0, len(paths), 7):
            assert np.array_equal(arena[i], imread_u8(paths[i])), paths[i]
        for a, b in ranges:
            assert np.array_equal(arena[b - 1], imread_u8(paths[b - 1]))
    got = []
    for loader in (host, dev):
        random.seed(123)
        got.append([b for _, b in zip(range(3), loader)])
        after = random.getstate()
    random.seed(123)
    [b for _, b in zip(range(3), host)]
    assert random.getstate() == after                                          # both loaders draw the same values
    assert len(got[0]) == len(got[1]) == 3
    for hb, db in zip(*got):
        assert hb["key"] == db["key"]
        for k in ("LQs", "GTenh", "GTinp"):
            assert db[k].is_cuda and db[k].shape == hb[k].shape
            assert db[k][:, 0].is_contiguous()                              # feed_data's LQs[:, i] is a plain device tensor
            assert torch.equal(db[k].cpu().view(torch.int32), hb[k].view(torch.int32)), k
        assert not torch.equal(hb["LQs"], hb["GTenh"])


def test_training_step_same_from_either_loader(sharp, tmp_path):
    """One optimize_parameters step fed by each loader with blur_window: identical loss and identical parameters afterwards."""
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    ds = _dataset(sharp, 11, (3, 64, 64))
    host, dev = _loaders(ds, 2, None)
    results = []
    for loader in (host, dev):
        random.seed(7)
        batch = next(iter(loader))
        opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
               "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
               "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp_path), "training_state": str(tmp_path)},
               "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "lr_G": 1e-4,
                         "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000], "restarts": None,
                         "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
        m = create_model(opt)
        m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
        m.feed_data(batch)
        m.optimize_parameters(1)
        torch.cuda.synchronize()
        results.append((float(m.loss.detach()), {k: v.detach().cpu().clone() for k, v in m.netG.module.state_dict().items()}))
        del m
    (la, pa), (lb, pb) = results
    assert la == lb
    assert pa.keys() == pb.keys() and all(torch.equal(pa[k], pb[k]) for k in pa)
