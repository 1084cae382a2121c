"""-m gpu: binhip_gather_windows against its numpy restatement, the device-cache loader against the host loader at n_workers 0
(same `random` state => same batches bit for bit), one training step fed by each, and the entry point's error codes."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from device_cache_cases import bits, gather_reference
from host_fixtures import make_adobe_tree

pytestmark = pytest.mark.gpu

H, W = 24, 301               # odd width: source rows of 903 bytes start at every dword offset


@pytest.fixture(scope="module")
def arena():
    g = np.random.Generator(np.random.PCG64(3))
    return g.integers(0, 256, (20, H, W, 3), dtype=np.uint8)


def _table(g, n, n_slots, crop, where, flip, n_frames=20):
    ch, cw = crop
    ys = {"tl": (0, 0), "tr": (0, W - cw), "bl": (H - ch, 0), "br": (H - ch, W - cw), "c": ((H - ch) // 2, (W - cw) // 2)}
    rows = np.empty((n, n_slots + 3), np.int32)
    for b in range(n):
        rows[b, :n_slots] = g.integers(0, n_frames, n_slots)
        y0, x0 = ys[where] if where != "rand" else (g.integers(0, H - ch + 1), g.integers(0, W - cw + 1))
        rows[b, n_slots:] = (y0, x0, flip if flip is not None else b % 2)
    return rows


@pytest.mark.parametrize("n,n_slots", [(1, 17), (9, 17), (9, 1)])
@pytest.mark.parametrize("cw", [1, 3, 5, 256])
def test_gather_windows_matches_restatement(arena, n, n_slots, cw):
    from bin_amd import ops
    frames = torch.from_numpy(arena).cuda()
    g = np.random.Generator(np.random.PCG64(cw * 100 + n * 10 + n_slots))
    for ch in (1, 7):
        for where in ("tl", "tr", "bl", "br", "c", "rand"):
            for flip in (0, 1, None):
                tab = _table(g, n, n_slots, (ch, cw), where, flip)
                out = ops.gather_windows(frames, tab, (ch, cw))
                assert out.shape == (n_slots, n, 3, ch, cw) and out.dtype == torch.float32
                ref = gather_reference(arena, tab, (ch, cw))
                assert np.array_equal(bits(out.cpu().numpy()), bits(ref)), (ch, cw, where, flip)


def test_gather_windows_rejects_bad_tables_on_the_host(arena):
    from bin_amd import ops
    frames = torch.from_numpy(arena).cuda()
    good = np.zeros((2, 20), np.int32)
    for col, val, msg in ((3, 20, "frame id"), (17, H - 3, "offset"), (18, W - 9, "offset"), (19, 2, "flip")):
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError, match=msg):
            ops.gather_windows(frames, bad, (4, 10))
    with pytest.raises(ValueError, match="does not fit"):
        ops.gather_windows(frames, good, (H + 1, 10))


def test_gather_windows_error_codes(arena):
    from bin_amd import _lib as L
    lib = L.lib()
    frames = torch.from_numpy(arena).cuda()
    table = torch.zeros((2, 20), dtype=torch.int32, device="cuda")
    out = torch.empty((17, 2, 3, 8, 8), dtype=torch.float32, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    f, t, o = (C.c_void_p(x.data_ptr()) for x in (frames, table, out))
    assert lib.binhip_gather_windows(None, 20, H, W, t, 2, 17, 8, 8, o, s) == -1             # BINHIP_E_ARG
    assert lib.binhip_gather_windows(f, 20, H, W, None, 2, 17, 8, 8, o, s) == -1
    assert lib.binhip_gather_windows(f, 20, H, W, t, 2, 17, 8, 8, None, s) == -1
    assert lib.binhip_gather_windows(f, 20, H, W, t, 2, 17, H + 1, 8, o, s) == -2           # BINHIP_E_SHAPE: crop
    assert lib.binhip_gather_windows(f, 20, H, W, t, 2, 17, 8, W + 1, o, s) == -2
    assert lib.binhip_gather_windows(f, 20, H, W, t, 2, 0, 8, 8, o, s) == -2                # n_slots
    assert lib.binhip_gather_windows(f, 20, H, W, t, 2, 33, 8, 8, o, s) == -2
    for n, ch, cw in ((0, 8, 8), (2, 0, 8), (2, 8, 0)):
        assert lib.binhip_gather_windows(f, 20, H, W, t, n, 17, ch, cw, o, s) == -2
    assert lib.binhip_gather_windows(f, 20, H, W, t, 2, 17, 8, 8, o, s) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the loader
@pytest.fixture(scope="module")
def adobe(tmp_path_factory):
    return make_adobe_tree(str(tmp_path_factory.mktemp("adobe")),
                           clips=(("clipA", 16, 9), ("clipB", 0, 7), ("clipC", 40, 8)))


def _dataset(adobe, crop):
    from bin_amd.data import create_dataset
    random.seed(0)
    return create_dataset({"mode": "BIN", "name": "train", "dataroot_GT": adobe, "dataroot_LQ": adobe, "LQ_size": list(crop),
                           "data_type": "img", "phase": "train"})


def _loaders(ds, batch, sampler):
    from bin_amd.data import create_dataloader
    opt = {"dist": False, "gpu_ids": [0]}
    host = create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": 0}, opt, sampler)
    dev = create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": 0, "device_cache": True}, opt, sampler)
    return host, dev


@pytest.mark.parametrize("world_rank", [None, (2, 1)])
def test_device_loader_batches_equal_host_loader(adobe, world_rank):
    from bin_amd.data.data_sampler import DistIterSampler
    from bin_amd.data.device_cache import DeviceWindowLoader
    ds = _dataset(adobe, (3, 64, 96))
    sampler = None if world_rank is None else DistIterSampler(ds, *world_rank, ratio=4)
    host, dev = _loaders(ds, 2, sampler)
    assert isinstance(dev, DeviceWindowLoader) and len(dev) == len(host) >= 3
    assert dev.cache.shape == (len(dev.cache.paths), 352, 640, 3)
    got = []
    for loader in (host, dev):
        random.seed(123)
        got.append([b for _, b in zip(range(3), loader)])
    for hb, db in zip(*got):
        assert hb["key"] == db["key"]
        for k in ("LQs", "GTenh", "GTinp"):
            assert db[k].is_cuda and db[k].shape == hb[k].shape
            assert db[k][:, 0].is_contiguous()                              # feed_data's LQs[:, i] is a plain device tensor
            assert torch.equal(db[k].cpu(), hb[k]), k


def test_training_step_same_from_either_loader(adobe, tmp_path):
    """One optimize_parameters step fed by each loader: identical loss and identical parameters afterwards."""
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    ds = _dataset(adobe, (3, 64, 64))
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
