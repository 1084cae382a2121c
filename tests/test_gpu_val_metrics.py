"""-m gpu: validation scores on the device.  binhip_frame_score through ops.frame_scores against the host metrics of
util.tensor2img images (exact sums, so PSNR and MAE to the bit; both SSIMs to 1e-9, the bar of tests/test_gpu_metrics.py for the
same u8 images) and against the u8 path (frame_to_u8 + image_scores); many pairs per call, repeats and streams; the entry
point's error codes; bin_model.compute_current_psnr_ssim and train.validate in device mode against host mode on the real HIP
bin_stage4; and validation windows served from the device frame cache."""
import ctypes as C
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from bin_amd import ops
from bin_amd.utils import util

pytestmark = pytest.mark.gpu

SHAPES = [(7, 7), (11, 11), (12, 300), (73, 101), (128, 128), (256, 256), (352, 640)]
KINDS = ("identical", "noise", "independent", "constant", "saturated", "out_of_range", "ties")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(kind, h, w, seed):
    """Two float32 [3, h, w] frames (numpy)."""
    g = np.random.default_rng(seed)
    x = g.random((3, h, w), dtype=np.float32)
    if kind == "identical":
        return x, x.copy()
    if kind == "noise":
        return x, (x + g.normal(0, 0.02, x.shape)).astype(np.float32)
    if kind == "independent":
        return x, g.random((3, h, w), dtype=np.float32)
    if kind == "constant":                                            # sigma = 0 everywhere
        return np.full((3, h, w), 37 / 255, np.float32), np.full((3, h, w), 219 / 255, np.float32)
    if kind == "saturated":                                           # 0 / 1 regions (and beyond) against each other
        x[:, : h // 2] = 1.0
        y = x.copy()
        y[:, : h // 2, : w // 2] = 0.0
        y[:, h // 2:, w // 3:] = 1.25
        return x, y
    if kind == "out_of_range":
        x = g.uniform(-0.5, 1.5, (3, h, w)).astype(np.float32)
        y = g.uniform(-0.5, 1.5, (3, h, w)).astype(np.float32)
        for a in (x, y):
            idx = g.choice(a.size, max(2, a.size // 50), replace=False)
            a.reshape(-1)[idx[::2]] = np.inf
            a.reshape(-1)[idx[1::2]] = -np.inf
        return x, y
    assert kind == "ties"
    # every rounding tie (k + 0.5) / 255, k = 0 .. 254, in both frames (a 7 x 7 frame has 147 values: x holds k = 0 .. 146
    # and y k = 254 .. 108, every tie in one of the two)
    i = np.arange(3 * h * w)
    x = ((i % 255 + 0.5) / 255).astype(np.float32).reshape(3, h, w)
    y = (((254 - i) % 255 + 0.5) / 255).astype(np.float32).reshape(3, h, w)
    if 3 * h * w >= 255:
        for a in (x, y):
            k = np.unique(np.rint(a.astype(np.float64) * 255 - 0.5)).astype(int)
            assert np.array_equal(k, np.arange(255))
    return x, y


def _with_nan(x, y, seed):
    g = np.random.default_rng(seed)
    x, y = x.copy(), y.copy()
    for a in (x, y):
        a.reshape(-1)[g.choice(a.size, max(1, a.size // 40), replace=False)] = np.nan
    return x, y


def _dev(a):
    return torch.from_numpy(a).cuda()


def _u8(a):
    return util.tensor2img(torch.from_numpy(a))


def _check_against_host(row, x, y, label):
    a, b = _u8(x), _u8(y)
    d = a.astype(np.int64) - b.astype(np.int64)
    g11 = util.calculate_ssim(a, b) if min(a.shape[:2]) >= 11 else float("nan")
    u7 = util.compare_ssim(a, b)
    print(f"{label}: sse {row[0]:.0f} / {(d * d).sum()}  sad {row[1]:.0f} / {np.abs(d).sum()}  "
          f"g11 {row[2]!r} / {g11!r}  u7 {row[3]!r} / {u7!r}")
    assert row[0] == float((d * d).sum()) and row[1] == float(np.abs(d).sum()), label
    r = util.score_row(row, a.size)
    assert r["psnr"] == util.calculate_psnr(a, b), label                               # bit for bit (inf included)
    assert r["mae"] == np.mean(np.abs(a.astype(np.float64) - b.astype(np.float64))), label
    if min(a.shape[:2]) < 11:
        assert np.isnan(row[2]), label
    else:
        assert abs(row[2] - g11) <= 1e-9, label
    assert abs(row[3] - u7) <= 1e-9, label


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_frame_scores_match_the_host_metrics(h, w):
    for i, kind in enumerate(KINDS):
        x, y = _pair(kind, h, w, 1000 + 7 * i + h)
        rows = ops.frame_scores([_dev(x)], [_dev(y)])
        assert rows.shape == (1, 4) and rows.dtype == torch.float64 and rows.is_cuda
        row = rows.cpu().numpy()[0]
        _check_against_host(row, x, y, f"{h}x{w} {kind}")
        if kind == "identical":
            assert row[0] == 0 and row[3] == 1.0 and (row[2] == 1.0 or min(h, w) < 11)
            assert util.score_row(row, x.size)["psnr"] == float("inf")
        # the [1,3,H,W] form is the same call
        assert np.array_equal(ops.frame_scores([_dev(x)[None]], [_dev(y)[None]]).cpu().numpy()[0], row, equal_nan=True)


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_frame_scores_match_the_u8_path(h, w):
    pairs = [_pair(kind, h, w, 2000 + 7 * i + w) for i, kind in enumerate(KINDS)]
    pairs += [_with_nan(*pairs[1], 5), _with_nan(*pairs[5], 6)]
    for label, (x, y) in zip(KINDS + ("noise+nan", "out_of_range+nan"), pairs):
        dx, dy = _dev(x), _dev(y)
        got = ops.frame_scores([dx], [dy]).cpu().numpy()[0]
        ref = ops.image_scores(ops.frame_to_u8(dx, 0, 0, h, w), ops.frame_to_u8(dy, 0, 0, h, w)).cpu().numpy()[0]
        print(f"{h}x{w} {label}: fused {got.tolist()}  u8 path {ref.tolist()}")
        assert got[0] == ref[0] and got[1] == ref[1], label
        for c in (2, 3):
            assert np.isnan(got[c]) == np.isnan(ref[c]), label
            assert np.isnan(ref[c]) or abs(got[c] - ref[c]) <= 1e-9, label
        assert np.isnan(got[2]) == (min(h, w) < 11) and not np.isnan(got[3])


def _window(h, w, seed):
    """14 (x, y) device pairs with get_info's repeat pattern of targets (I4 .. I8 twice) and one tensor on either side."""
    g = torch.Generator().manual_seed(seed)
    I = {k: torch.rand((3, h, w), generator=g).cuda() for k in range(2, 11)}
    order = [2, 4, 6, 8, 3, 5, 7, 4, 6, 5, 10, 9, 8, 7]
    xs = [(I[k] + 0.05 * torch.randn((3, h, w), generator=g).cuda()) for k in order]
    xs[3] = I[6]                                                       # I6 is y of pairs 2 and 8 and x of pair 3
    return xs, [I[k] for k in order]


def test_many_pairs_per_call_repeats_and_streams():
    h, w = 73, 101
    xs, ys = _window(h, w, 3)
    single = torch.cat([ops.frame_scores([x], [y]) for x, y in zip(xs, ys)]).cpu()
    got = ops.frame_scores(xs, ys)
    assert got.shape == (14, 4)
    assert torch.equal(got.cpu().view(torch.int64), single.view(torch.int64))            # every row: the bits of its n = 1 call
    _check_against_host(got.cpu().numpy()[3], xs[3].cpu().numpy(), ys[3].cpu().numpy(), "pair 3")
    sums = ops.frame_scores(xs, ys, ssim=False).cpu()
    assert torch.equal(sums[:, :2], single[:, :2]) and torch.isnan(sums[:, 2:]).all()
    # 33 pairs: more than one call of BINHIP_SCORE_MAX_PAIRS
    idx = [i % 14 for i in range(33)]
    many = ops.frame_scores([xs[i] for i in idx], [ys[i] for i in idx]).cpu()
    assert many.shape == (33, 4)
    assert torch.equal(many.view(torch.int64), single[idx].view(torch.int64))
    for _ in range(3):
        assert torch.equal(ops.frame_scores(xs, ys).cpu().view(torch.int64), single.view(torch.int64))
    # a non-contiguous frame is copied, not misread
    wide = torch.rand((3, h, 2 * w)).cuda()
    assert torch.equal(ops.frame_scores([wide[:, :, ::2]], [ys[0]]).cpu(),
                       ops.frame_scores([wide[:, :, ::2].contiguous()], [ys[0]]).cpu())
    # four host threads on four streams
    results, errors = {}, []
    start = threading.Barrier(4)

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                a = [t.clone() for t in xs[3 * i:3 * i + 3]]
                b = [t.clone() for t in ys[3 * i:3 * i + 3]]
                start.wait()
                outs = [ops.frame_scores(a, b) for _ in range(8)]
                results[i] = [o.cpu() for o in outs]
        except Exception as e:                                            # surfaced below
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(4):
        for o in results[i]:
            assert torch.equal(o.view(torch.int64), single[3 * i:3 * i + 3].view(torch.int64))


def test_frame_scores_argument_errors():
    x = torch.zeros((3, 16, 16), device="cuda")
    with pytest.raises(RuntimeError):
        ops.frame_scores([x.cpu()], [x])
    with pytest.raises(RuntimeError):
        ops.frame_scores([x[:, :6]], [x[:, :6]])                          # SSIM below 7 x 7
    assert torch.isnan(ops.frame_scores([x[:, :6]], [x[:, :6]], ssim=False)[0, 2:]).all()
    for bad in (x.double(), x.half()):
        with pytest.raises(ValueError):
            ops.frame_scores([bad], [bad])
    for bad in (x[0], x[None, None], torch.zeros((4, 16, 16), device="cuda"), torch.zeros((2, 3, 16, 16), device="cuda")):
        with pytest.raises(ValueError):
            ops.frame_scores([bad], [bad])
    with pytest.raises(ValueError):
        ops.frame_scores([x], [torch.zeros((3, 16, 17), device="cuda")])
    with pytest.raises(ValueError):
        ops.frame_scores([x, x], [x])


def test_frame_score_error_codes():
    from bin_amd import _lib as L
    from bin_amd.utils.util import _gauss_taps
    lib = L.lib()
    h, w, n = 16, 20, 2
    frames = torch.rand((4, 3, h, w), device="cuda")
    taps = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    px = (C.c_void_p * 2)(frames[0].data_ptr(), frames[1].data_ptr())
    py = (C.c_void_p * 2)(frames[2].data_ptr(), frames[3].data_ptr())
    hole = (C.c_void_p * 2)(frames[0].data_ptr(), None)
    nb = lib.binhip_frame_score_workspace_bytes(n, h, w, 3)
    assert nb == n * 3 * 64
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    pw, po = C.c_void_p(ws.data_ptr()), C.c_void_p(out.data_ptr())
    f = lib.binhip_frame_score
    E_ARG, E_SHAPE, E_WS = -1, -2, -3
    assert f(None, py, n, h, w, 3, taps, pw, nb, po, s) == E_ARG                        # null arrays
    assert f(px, None, n, h, w, 3, taps, pw, nb, po, s) == E_ARG
    assert f(hole, py, n, h, w, 3, taps, pw, nb, po, s) == E_ARG                        # a null element, either side
    assert f(px, hole, n, h, w, 3, taps, pw, nb, po, s) == E_ARG
    assert f(px, py, n, h, w, 3, None, pw, nb, po, s) == E_ARG                          # G11 without taps
    assert f(px, py, n, h, w, 2, None, pw, nb, po, s) == 0                              # U7 alone needs none
    assert f(px, py, n, h, w, 3, taps, None, nb, po, s) == E_ARG
    assert f(px, py, n, h, w, 3, taps, pw, nb, None, s) == E_ARG
    assert f(px, py, n, h, w, 4, taps, pw, nb, po, s) == E_ARG                          # unknown flag
    big = (C.c_void_p * (L.SCORE_MAX_PAIRS + 1))(*[frames[0].data_ptr()] * (L.SCORE_MAX_PAIRS + 1))
    for bad_n in (0, -1, L.SCORE_MAX_PAIRS + 1):
        assert f(big, big, bad_n, h, w, 0, taps, pw, nb, po, s) == E_SHAPE
        assert lib.binhip_frame_score_workspace_bytes(bad_n, h, w, 0) == 0
    for bh, bw, fl in ((0, w, 0), (h, 0, 0), (65536, w, 0), (h, 65536, 0), (-1, w, 0), (10, w, 1), (h, 10, 1), (6, w, 2), (h, 6, 2),
                       (10, w, 3)):
        assert f(px, py, n, bh, bw, fl, taps, pw, nb, po, s) == E_SHAPE, (bh, bw, fl)
        assert lib.binhip_frame_score_workspace_bytes(n, bh, bw, fl) == 0, (bh, bw, fl)
    assert lib.binhip_frame_score_workspace_bytes(n, h, w, 4) == 0
    assert lib.binhip_frame_score_workspace_bytes(1, 10, 10, 2) == 3 * 64 and lib.binhip_frame_score_workspace_bytes(1, 6, 6, 0) == 3 * 64
    assert lib.binhip_frame_score_workspace_bytes(L.SCORE_MAX_PAIRS, 65535, 65535, 3) > 0
    assert f(px, py, n, h, w, 3, taps, pw, nb - 1, po, s) == E_WS
    assert f(px, py, n, h, w, 3, taps, pw, nb, po, s) == 0
    torch.cuda.synchronize()
    ops.check_status()
    ref = ops.frame_scores([frames[0], frames[1]], [frames[2], frames[3]]).cpu()
    assert torch.equal(out.cpu()[:, :2].double(), ref[:, :2]) and torch.equal(out.cpu()[:, 2:].view(torch.float64), ref[:, 2:])


# ------------------------------------------------------------------ the wrapper and the training loop
def _model_opt(tmp, metrics=None):
    from bin_amd.options import options as option
    train = {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "lr_G": 1e-4,
             "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000], "restarts": None,
             "restart_weights": None, "lr_gamma": 0.5, "clear_state": False, "val_save_images": 1}
    if metrics is not None:
        train["val_metrics"] = metrics
    return option.dict_to_nonedict({
        "model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
        "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
        "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp),
                 "val_images": str(tmp)},
        "train": train})


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    m = create_model(_model_opt(tmp_path_factory.mktemp("model")))
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    return m


@pytest.fixture(scope="module")
def windows():
    """Two synthetic validation windows at 128 x 128, as the loader collates them (batch of 1)."""
    from bin_amd.data import create_dataset
    ds = create_dataset({"mode": "synthetic_texture", "name": "v", "phase": "val", "LQ_size": [3, 128, 128], "num_windows": 2,
                         "seed": None, "max_speed": None})
    return [{"LQs": s["LQs"][None], "GTenh": s["GTenh"][None], "GTinp": s["GTinp"][None], "key": [s["key"].replace("/", "_")]}
            for s in (ds[0], ds[1])]


def test_wrapper_device_scores_equal_host_scores(model, windows, tmp_path, monkeypatch):
    from bin_amd.data import util as du
    for k, batch in enumerate(windows):
        model.feed_data(batch)
        model.test()
        host_dir, dev_dir = tmp_path / f"host{k}", tmp_path / f"dev{k}"
        os.makedirs(host_dir), os.makedirs(dev_dir)
        psnr_h, ssim_h = model.compute_current_psnr_ssim(save=True, name="w", save_path=str(host_dir))
        assert (psnr_h, ssim_h) == model.compute_current_psnr_ssim(metrics="host")
        psnr_s, ssim_s = model.compute_current_psnr_ssim(save=True, name="w", save_path=str(dev_dir), metrics="device")
        names = sorted(os.listdir(host_dir))
        assert len(names) == 28 and names == sorted(os.listdir(dev_dir))
        for f in names:
            assert np.array_equal(du.imread_u8(str(host_dir / f)), du.imread_u8(str(dev_dir / f))), f
        with monkeypatch.context() as mp:                                  # no frame is copied to the host
            def boom(*a, **kw):
                raise AssertionError("the host path was reached in device mode")
            mp.setattr(model, "get_current_visuals", boom)
            mp.setattr(util, "tensor2img", boom)
            psnr_d, ssim_d = model.compute_current_psnr_ssim(metrics="device")
        assert (psnr_d, ssim_d) == (psnr_s, ssim_s)
        assert len(psnr_d) == len(ssim_d) == 14 and all(type(v) is float for v in psnr_d + ssim_d)
        print("psnr host", psnr_h, "\npsnr device", psnr_d, "\nssim host", ssim_h, "\nssim device", ssim_d)
        assert psnr_d == psnr_h                                            # bit for bit
        assert all(abs(a - b) <= 1e-9 for a, b in zip(ssim_d, ssim_h))
        assert all(np.isfinite(v) for v in ssim_d)


def test_validate_device_mode_equals_host_mode(model, windows, tmp_path):
    import logging
    from bin_amd import train
    log = logging.getLogger("test_val_metrics")
    runs = {}
    for mode in ("host", "device"):
        opt = _model_opt(tmp_path / mode, mode)
        loss = train.validate(model, list(windows), 7, opt, log)
        runs[mode] = (loss, [m.avg for m in model.psnr_interp], [m.avg for m in model.ssim_interp],
                      [m.count for m in model.psnr_interp])
        assert len(os.listdir(tmp_path / mode / "7")) == 28              # val_save_images: 1
    (lh, ph, sh, ch), (ld, pd, sd, cd) = runs["host"], runs["device"]
    print("psnr_interp host", ph, "\npsnr_interp device", pd, "\nssim_interp host", sh, "\nssim_interp device", sd)
    assert ch == cd == [2] * 14
    assert pd == ph
    assert all(abs(a - b) <= 1e-9 for a, b in zip(sd, sh))
    assert ld == lh
    for f in sorted(os.listdir(tmp_path / "host" / "7")):
        assert open(tmp_path / "host" / "7" / f, "rb").read() == open(tmp_path / "device" / "7" / f, "rb").read()


def test_train_script_validates_on_the_device(tmp_path):
    """python -m bin_amd.train on the shipped synthetic option file with val_metrics: device."""
    y = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    y = y.replace("save_path: ./runs", f"save_path: {tmp_path}").replace("num_windows: 4000", "num_windows: 64")
    y = y.replace("n_workers: 3", "n_workers: 0").replace("niter: 2000", "niter: 4")
    y = y.replace("val_freq: 500", "val_freq: 2\n  val_max_batches: 2").replace("  # val_metrics: device", "  val_metrics: device")
    assert "\n  val_metrics: device" in y
    p = str(tmp_path / "syn.yml")
    open(p, "w").write(y)
    r = subprocess.run([sys.executable, "-m", "bin_amd.train", "-opt", p], cwd=REPO, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exp = tmp_path / "experiments" / "synthetic_stage4"
    text = open(exp / [f for f in os.listdir(exp) if f.endswith(".log")][0]).read()
    lines = [ln for ln in text.splitlines() if "<val iter" in ln]
    print("\n".join(lines))
    assert len(lines) == 2 and "End of training." in text and "nan" not in "".join(lines).lower()
    assert (exp / "models" / "latest_G.pth").exists()


# ------------------------------------------------------------------ validation windows from the device frame cache
def test_validation_loader_honours_device_cache(tmp_path, monkeypatch):
    from host_fixtures import make_adobe_tree
    from bin_amd.data import create_dataloader, create_dataset
    from bin_amd.data import device_cache
    from bin_amd.data.device_cache import DeviceWindowLoader
    adobe = make_adobe_tree(str(tmp_path / "adobe"), clips=(("clipA", 16, 9), ("clipB", 0, 7), ("clipC", 40, 8)))
    random.seed(0)
    ds_opt = {"mode": "BIN", "name": "train", "dataroot_GT": adobe, "dataroot_LQ": adobe, "LQ_size": [3, 64, 96],
              "data_type": "img", "phase": "val", "device_cache": True}
    ds = create_dataset(ds_opt)
    built = []
    real = device_cache.DeviceFrameCache

    class Counting(real):
        def __init__(self, *a, **kw):
            built.append(1)
            super().__init__(*a, **kw)
    monkeypatch.setattr(device_cache, "DeviceFrameCache", Counting)
    loader = create_dataloader(ds, ds_opt, {"dist": False, "gpu_ids": [0]}, None)
    assert isinstance(loader, DeviceWindowLoader) and loader.batch == 1 and loader.sampler is None
    assert len(loader) == len(ds) >= 6
    passes = []
    for _ in range(2):
        random.seed(123)
        cache = loader.cache
        passes.append(list(loader))
        assert loader.cache is cache
    assert built == [1]                                                   # one cache for the run, not one per pass
    random.seed(123)
    items = [ds[i] for i in range(len(ds))]
    for got in passes:
        assert len(got) == len(ds)
        for b, item in zip(got, items):
            assert b["key"] == [item["key"]] and b["key"][0] == item["key"]
            for k in ("LQs", "GTenh", "GTinp"):
                assert b[k].is_cuda and b[k].shape == (1,) + tuple(item[k].shape)
                assert torch.equal(b[k][0].cpu().view(torch.int32), item[k].view(torch.int32)), k
    # without the key, and for other dataset kinds, the host loader as before
    host = create_dataloader(ds, dict(ds_opt, device_cache=None), {"dist": False, "gpu_ids": [0]}, None)
    assert isinstance(host, torch.utils.data.DataLoader) and host.batch_size == 1
    syn_opt = {"mode": "synthetic_texture", "name": "v", "phase": "val", "LQ_size": [3, 32, 32], "num_windows": 3, "seed": None,
               "max_speed": None, "device_cache": True}
    syn = create_dataloader(create_dataset(syn_opt), syn_opt, {"dist": False, "gpu_ids": [0]}, None)
    assert isinstance(syn, torch.utils.data.DataLoader) and syn.batch_size == 1
