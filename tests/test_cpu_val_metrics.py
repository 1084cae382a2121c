"""CPU: the host side of validation scoring on the device — the two binhip_frame_score entry points in the header, the library
and the binding, the `train.val_metrics` option, and train.validate on the oracle-backed CPU wrapper (device mode must refuse
a CPU model; host mode is the code path it always was)."""
import logging
import os
import re
import subprocess

import pytest
import torch

from conftest import REPO

NEW = ("binhip_frame_score_workspace_bytes", "binhip_frame_score")


def _header():
    return open(os.path.join(REPO, "include", "binhip.h")).read()


def test_header_declares_the_frame_score_entry_points():
    from bin_amd import build
    hdr = _header()
    for name in NEW:
        assert re.search(r"(?m)^BINHIP_API\s+[\w\s\*]+?\b%s\s*\(" % name, hdr), name
        assert name in build.abi_symbols()
    n_max = int(re.search(r"#define\s+BINHIP_SCORE_MAX_PAIRS\s+(\d+)", hdr).group(1))
    assert n_max >= 17                                       # the 14 outputs of a window and the 3 cycle pairs fit one call
    assert int(re.search(r"#define\s+BINHIP_VERSION\s+(\d+)", hdr).group(1)) == 622


def test_export_count_is_51():
    from bin_amd import build
    n = int(re.search(r"#define\s+BINHIP_ABI_EXPORTS\s+(\d+)", _header()).group(1))
    assert n == 51 == len(build.abi_symbols())


def test_library_exports_the_frame_score_symbols():
    from bin_amd import _lib
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    dyn = {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}
    for name in NEW:
        assert name in dyn, name


def test_binding_has_the_frame_score_signatures():
    import ctypes as C
    from bin_amd import _lib
    lib = _lib.lib()
    assert set(NEW) <= set(_lib.exported_symbols())
    assert lib.binhip_frame_score_workspace_bytes.restype is C.c_size_t
    assert len(lib.binhip_frame_score_workspace_bytes.argtypes) == 4
    assert lib.binhip_frame_score.restype is C.c_int and len(lib.binhip_frame_score.argtypes) == 11
    n_max = int(re.search(r"#define\s+BINHIP_SCORE_MAX_PAIRS\s+(\d+)", _header()).group(1))
    assert _lib.SCORE_MAX_PAIRS == n_max
    # arguments are checked before any HIP call, so the size query and the refusals run without a device
    f = lib.binhip_frame_score_workspace_bytes
    assert f(14, 256, 256, 3) == 14 * 3 * 16 * 2 * 64       # 16 row tiles x 2 column tiles (246 columns each) x 64-byte slots
    assert f(1, 7, 7, 2) == 3 * 64 and f(1, 7, 7, 3) == 0 and f(1, 6, 7, 2) == 0 and f(1, 6, 7, 0) == 3 * 64
    assert f(0, 16, 16, 0) == 0 and f(n_max + 1, 16, 16, 0) == 0 and f(n_max, 16, 16, 0) > 0
    assert f(1, 65536, 16, 0) == 0 and f(1, 16, 0, 0) == 0 and f(1, 16, 16, 4) == 0
    assert lib.binhip_frame_score(None, None, 1, 16, 16, 0, None, None, 0, None, None) == -1


def test_val_metrics_option_values(tmp_path):
    from bin_amd.options import options as option
    assert option.val_metrics({"train": {}}) == "host"
    assert option.val_metrics({}) == "host"
    assert option.val_metrics(option.dict_to_nonedict({"train": {"val_freq": 5}})) == "host"
    assert option.val_metrics({"train": {"val_metrics": "host"}}) == "host"
    assert option.val_metrics({"train": {"val_metrics": "device"}}) == "device"
    for bad in ("gpu", "Device", True, 1):
        with pytest.raises(ValueError, match="val_metrics"):
            option.val_metrics({"train": {"val_metrics": bad}})
    # a misspelt value stops the run when the option file is parsed
    y = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    assert "# val_metrics: device" in y
    assert "# val_metrics: device" in open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_adobe240.yml")).read()
    p = str(tmp_path / "bad.yml")
    open(p, "w").write(y.replace("  # val_metrics: device", "  val_metrics: gpu"))
    env = os.environ.get("CUDA_VISIBLE_DEVICES")
    try:
        with pytest.raises(ValueError, match="val_metrics"):
            option.parse(p, is_train=True)
        open(p, "w").write(y.replace("  # val_metrics: device", "  val_metrics: device"))
        assert option.parse(p, is_train=True)["train"]["val_metrics"] == "device"
        assert option.parse(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml"))["train"].get("val_metrics") is None
    finally:                                                 # parse() exports gpu_ids as CUDA_VISIBLE_DEVICES
        if env is None:
            os.environ.pop("CUDA_VISIBLE_DEVICES", None)
        else:
            os.environ["CUDA_VISIBLE_DEVICES"] = env


def _opt(tmp, metrics):
    from bin_amd.options import options as option
    train = {"pixel_criterion": "cb", "pixel_weight": 1.0, "lr_G": 1e-3, "beta1": 0.9, "beta2": 0.99,
             "lr_scheme": "MultiStepLR", "lr_steps": [100], "lr_gamma": 0.5, "val_save_images": 1}
    if metrics is not None:
        train["val_metrics"] = metrics
    return option.dict_to_nonedict({
        "model": "bin", "gpu_ids": None, "is_train": True, "dist": False,
        "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
        "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp),
                 "val_images": str(tmp / "val_images")},
        "train": train})


def _batches(n, hw=(16, 20)):
    g = torch.Generator().manual_seed(5)
    h, w = hw
    return [{"LQs": torch.rand((1, 6, 3, h, w), generator=g), "GTenh": torch.rand((1, 6, 3, h, w), generator=g),
             "GTinp": torch.rand((1, 5, 3, h, w), generator=g), "key": [f"clip_{i:05d}"]} for i in range(n)]


def test_validate_on_a_cpu_model_host_as_before_device_refused(tmp_path):
    from test_cpu_data import _tiny_factory
    from bin_amd import train
    from bin_amd.utils import util
    log = logging.getLogger("test_val_metrics")
    batches = _batches(2)
    losses = {}
    for mode in (None, "host"):
        opt = _opt(tmp_path / str(mode), mode)
        model = _tiny_factory(opt)
        losses[mode] = train.validate(model, batches, 3, opt, log)
        assert model.psnr_interp[0].count == 2 and all(m.avg > 0 for m in model.psnr_interp)
        # the meters hold what the host metrics give on the model's current outputs (the last window)
        model.feed_data(batches[-1])
        model.test()
        vis = model.get_current_visuals()
        psnr, ssim = model.compute_current_psnr_ssim()
        assert psnr[13] == util.calculate_psnr(util.tensor2img(vis["rlt"][13]), util.tensor2img(vis["GT"][13]))
        assert ssim[13] == util.calculate_ssim(util.tensor2img(vis["rlt"][13]), util.tensor2img(vis["GT"][13]))
        assert model.compute_current_psnr_ssim(metrics="host") == (psnr, ssim)
        saved = os.listdir(tmp_path / str(mode) / "val_images" / "3")
        assert len(saved) == 28 and "rlt_clip_00000_13.png" in saved
    assert losses[None] == losses["host"]
    opt = _opt(tmp_path / "device", "device")
    model = _tiny_factory(opt)
    with pytest.raises(RuntimeError, match="needs a CUDA model"):
        train.validate(model, batches, 3, opt, log)
    with pytest.raises(RuntimeError, match="needs a CUDA model"):
        model.compute_current_psnr_ssim(metrics="device")
    with pytest.raises(ValueError, match="val_metrics"):
        train.validate(model, batches, 3, _opt(tmp_path / "bad", "gpu"), log)
    with pytest.raises(ValueError):
        model.compute_current_psnr_ssim(metrics="gpu")


def test_frame_scores_refuses_cpu_tensors():
    from bin_amd import ops
    x = torch.zeros((3, 16, 16))
    with pytest.raises(RuntimeError):
        ops.frame_scores([x], [x])
    with pytest.raises(ValueError):
        ops.frame_scores([x], [x, x])
    with pytest.raises(ValueError):
        ops.frame_scores([], [])
