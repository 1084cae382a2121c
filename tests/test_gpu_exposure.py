"""-m gpu: binexpose_gather (libbinexpose.so) against the plain-integer restatement of include/binexpose.h (exposure_cases.py), bit
for bit on the case table; its sharp slots against ops.gather_windows and its h = 0 exposures against ops.gather_windows_blur;
that it is a function of its arguments alone (repeat, another key, poisoned buffers); the flip; the device loader with
`blur_gamma` / `blur_noise` against the host loader at n_workers 0; mode BIN_video against the restatement; and two steps of
`python -m bin_amd.train` with the options on.  CPU side: test_cpu_exposure.py."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_cases as CL
import exposure_cases as EC
import poison
from conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def arenas():
    return {(content, hw): torch.from_numpy(EC.arena(content, hw).copy()).cuda() for content in EC.CONTENTS for hw in EC.ARENAS.values()}


def _run(arenas, case, rows=None, noise="case"):
    from bin_amd import ops
    hw, crop, gamma, case_noise, content = EC.split(case)
    rows = EC.reference(case)[0] if rows is None else rows
    curve = ops.exposure_curve(gamma, case_noise if noise == "case" else noise)
    return ops.gather_windows_exposed(arenas[(content, hw)], EC.table_of(rows), crop, EC.N_BLUR, curve)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("case", EC.CASES)
def test_kernel_equals_the_restatement(arenas, case):
    from bin_amd import ops
    hw, crop, _, _, content = EC.split(case)
    rows, codes = EC.reference(case)
    out = _run(arenas, case)
    assert out.shape == (EC.N_SLOTS, 3, 3) + tuple(crop) and out.dtype == torch.float32
    got = out.cpu().numpy()
    assert np.array_equal(EC.bits(got), EC.bits(EC.as_float(codes))), np.argwhere(EC.bits(got) != EC.bits(EC.as_float(codes)))[:5]
    # the sharp slot is gather_windows' on the same row
    plain = ops.gather_windows(arenas[(content, hw)], rows[:, :EC.N_SLOTS + 3].astype(np.int32), crop)
    assert torch.equal(out[EC.N_BLUR:].view(torch.int32), plain[EC.N_BLUR:].view(torch.int32))


@pytest.mark.parametrize("gamma", [1.0, 2.2, "srgb"])
def test_one_frame_exposure_without_noise_is_gather_windows_blur(arenas, gamma):
    """h = 0, no noise: decode(LIN[v]) = v, so every slot is the plain crop, whatever the curve; at 17 slots, 6 of them blurry."""
    from bin_amd import ops
    hw, crop = (19, 27), (9, 13)
    g = np.random.Generator(np.random.PCG64(8))
    rows = np.zeros((5, 17 + 6), np.int64)
    rows[:, :17] = g.integers(0, EC.NF, (5, 17))
    rows[:, 17:] = [(int(g.integers(0, 11)), int(g.integers(0, 15)), b % 2, 0, int(g.integers(0, 2 ** 32)), 5) for b in range(5)]
    frames = arenas[("random", hw)]
    out = ops.gather_windows_exposed(frames, EC.table_of(rows), crop, 6, ops.exposure_curve(gamma))
    blur = ops.gather_windows_blur(frames, rows[:, :21].astype(np.int32), crop, 6)
    assert torch.equal(out.view(torch.int32), blur.view(torch.int32))


def test_same_table_same_bits_and_another_key_changes_the_blurry_slots_only(arenas):
    case = "19x27-whole-srgb-noisy-random"
    rows = EC.reference(case)[0]
    a, b = _run(arenas, case), _run(arenas, case)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    other = rows.copy()
    other[:, -1] ^= 1
    c = _run(arenas, case, other)
    assert torch.equal(c[EC.N_BLUR:].view(torch.int32), a[EC.N_BLUR:].view(torch.int32))
    for s in range(EC.N_BLUR):
        for smp in range(3):
            assert not torch.equal(c[s, smp], a[s, smp]), (s, smp)
    # without noise the key is not read at all
    clean = _run(arenas, case, rows, noise=None)
    assert torch.equal(_run(arenas, case, other, noise=None).view(torch.int32), clean.view(torch.int32))


def test_flip_mirrors_the_picture_and_the_noise_stays_on_output_coordinates(arenas):
    from bin_amd import ops
    rows = np.zeros((2, EC.N_SLOTS + 6), np.int64)
    rows[:, :EC.N_SLOTS] = (20, 9, 31)
    rows[:, EC.N_SLOTS:] = [(3, 5, 0, 5, 77, 99), (3, 5, 1, 5, 77, 99)]          # the same sample, unflipped and flipped
    case = "24x36-9x13-g2.2-noisy-random"
    clean = _run(arenas, case, rows, noise=None)
    assert torch.equal(clean[:, 1].flip(-1).view(torch.int32), clean[:, 0].view(torch.int32))
    noisy = _run(arenas, case, rows)
    assert not torch.equal(noisy[:EC.N_BLUR, 1].flip(-1), noisy[:EC.N_BLUR, 0])
    assert torch.equal(noisy[EC.N_BLUR:, 1].flip(-1).view(torch.int32), noisy[EC.N_BLUR:, 0].view(torch.int32))
    # a flat picture shows the field alone: it is the same whether the sample is flipped or not
    flat = torch.full((EC.NF, 24, 36, 3), 128, dtype=torch.uint8, device="cuda")
    out = ops.gather_windows_exposed(flat, EC.table_of(rows), (9, 13), EC.N_BLUR, ops.exposure_curve(2.2, (0.01, 0.002)))
    assert torch.equal(out[:, 1].view(torch.int32), out[:, 0].view(torch.int32))
    assert len(torch.unique(out[0, 0])) > 3 and bool((out[EC.N_BLUR:] == torch.tensor(128.0, device="cuda") / 255).all())


@pytest.mark.parametrize("case", ["19x27-whole-g2.2-noisy-random", "24x36-9x13-srgb-clean-shadows", "19x27-9x13-srgb-noisy-full"])
def test_every_output_byte_is_written(arenas, case):
    """Under poisoned allocations (0xFF: NaN; 0x47: finite) the result is the clean run's, and no guard band is touched."""
    want = _run(arenas, case)
    for byte in (0xFF, 0x47):
        with poison.poisoned(byte) as rec:
            got = _run(arenas, case)
            torch.cuda.synchronize()
        assert rec.count >= 1 and poison.same_bits(got, want), hex(byte)


def test_gather_windows_exposed_rejects_bad_tables_and_curves_on_the_host(arenas):
    from bin_amd import ops
    frames = arenas[("random", (24, 36))]
    curve = ops.exposure_curve(2.2, (0.01, 0.002))
    good = np.zeros((2, 23), np.int32)
    good[:, :17] = 20
    good[:, 20] = 5
    ops.gather_windows_exposed(frames, good, (4, 10), 6, curve)
    for col, val, msg in ((3, EC.NF, "frame id"), (17, 21, "offset"), (18, 27, "offset"), (19, 2, "flip"), (20, 17, r"h outside \[0, 16\]"),
                          (0, 4, "leaves the arena"), (5, EC.NF - 5, "leaves the arena")):
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(ValueError, match=msg):
            ops.gather_windows_exposed(frames, bad, (4, 10), 6, curve)
    with pytest.raises(ValueError, match=r"n_slots \+ 6"):
        ops.gather_windows_exposed(frames, good[:, :6], (4, 10), 0, curve)
    with pytest.raises(ValueError, match="n_blur"):
        ops.gather_windows_exposed(frames, good, (4, 10), 18, curve)
    with pytest.raises(ValueError, match="crosses a clip boundary"):
        ops.gather_windows_exposed(frames, good, (4, 10), 6, curve, clip_ranges=np.array([[0, 18], [18, EC.NF]]))
    broken = curve.copy()
    broken[1, 100] = broken[1, 99]
    with pytest.raises(ValueError, match="validity rule"):
        ops.gather_windows_exposed(frames, good, (4, 10), 6, broken)
    with pytest.raises(ValueError, match="tables"):
        ops.gather_windows_exposed(frames, good, (4, 10), 6, curve[:2])
    with pytest.raises(RuntimeError):
        ops.gather_windows_exposed(frames.cpu(), good, (4, 10), 6, curve)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the loaders
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return EC.make_toy_tree(str(tmp_path_factory.mktemp("toy")))


EXPOSURE = {"blur_window": [5, 11], "blur_gamma": "srgb", "blur_noise": [0.01, 0.002]}


def test_device_loader_batches_equal_host_loader(toy):
    from bin_amd.data import create_dataloader, create_dataset
    from bin_amd.data.device_cache import DeviceWindowLoader
    random.seed(0)
    ds = create_dataset(dict({"mode": "BIN", "name": "train", "dataroot_GT": toy, "dataroot_LQ": toy, "LQ_size": [3, 48, 64],
                              "data_type": "img", "phase": "train"}, **EXPOSURE))
    opt = {"dist": False, "gpu_ids": [0]}
    host = create_dataloader(ds, {"phase": "train", "batch_size": 2, "n_workers": 0}, opt, None)
    dev = create_dataloader(ds, {"phase": "train", "batch_size": 2, "n_workers": 0, "device_cache": True}, opt, None)
    assert isinstance(dev, DeviceWindowLoader) and len(dev) == len(host) == 3
    got, after = [], []
    for loader in (host, dev):
        random.seed(123)
        got.append(list(loader))
        after.append(random.getstate())
    assert after[0] == after[1], "both loaders draw the same values"
    assert len(got[0]) == len(got[1]) == 3
    for hb, db in zip(*got):
        assert hb["key"] == db["key"]
        for k in ("LQs", "GTenh", "GTinp"):
            assert db[k].is_cuda and db[k].shape == hb[k].shape
            assert torch.equal(db[k].cpu().view(torch.int32), hb[k].view(torch.int32)), k
        assert not torch.equal(hb["LQs"], hb["GTenh"])
    # a second pass draws other keys: other noise on the same windows is possible, equal bits are not expected
    assert not all(torch.equal(a["LQs"], b["LQs"]) for a, b in zip(list(dev), got[1]))


def test_video_loader_batch_equals_the_restatement(tmp_path):
    from bin_amd import ops
    from bin_amd.data import create_dataloader, create_dataset
    from bin_amd.data.BIN_dataset import draw_blur_half, draw_window_aug
    from bin_amd.data.exposure import sample_key
    fh, fw, crop = 48, 64, (3, 12, 20)
    payloads = CL.write_clip(str(tmp_path / "clipA.y4m"), 80, fh, fw, 420, seed=6)
    frames = ops.yuv_to_bgr(torch.from_numpy(payloads).cuda(), fh, fw, (420, "bt601", "limited")).cpu().numpy()
    for phase in ("train", "val"):
        opt = dict({"mode": "BIN_video", "name": "train", "dataroot_video": str(tmp_path), "LQ_size": list(crop), "phase": phase,
                    "batch_size": 2, "n_workers": 0, "device_cache": True}, **EXPOSURE)
        random.seed(0)
        ds = create_dataset(opt)
        loader = create_dataloader(ds, opt, {"dist": False, "gpu_ids": [0]}, None)
        n = 2 if phase == "train" else 1
        random.seed(55)
        batch = next(iter(loader))
        random.seed(55)
        draws = [(draw_window_aug(crop, src_size=(fh, fw)), draw_blur_half(ds.blur_window), sample_key(ds.exposure, phase == "train", i))
                 for i in range(n)]
        rows = loader.cache.table(ds.all_paths[:n], [d for d, _, _ in draws], [h for _, h, _ in draws], [k for _, _, k in draws])
        if phase == "val":
            assert rows[0, -2:].view(np.uint32).tolist() == [0x9E3779B9, 0]
        lo = int(os.path.basename(loader.cache.paths[0])[:-4]) - 1                # 0-based index of the arena's first frame
        arena = frames[lo:lo + loader.cache.shape[0]]
        assert np.array_equal(loader.cache.frames.cpu().numpy(), arena)
        want = EC.as_float(EC.gather_codes(arena, rows.tolist(), crop[1:], 6, EC.tables("srgb", (0.01, 0.002))))
        got = torch.cat([batch["LQs"], batch["GTenh"], batch["GTinp"]], dim=1).transpose(0, 1).cpu().numpy()
        assert got.shape == want.shape == (17, n, 3, 12, 20)
        assert np.array_equal(EC.bits(got), EC.bits(want)), phase


def test_train_script_runs_two_steps_with_the_options(toy, tmp_path):
    """python -m bin_amd.train --max_iter 2 with device_cache, blur_window, blur_gamma and blur_noise on the toy tree."""
    y = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_adobe240.yml")).read()
    y = y.replace("save_path: ./runs", f"save_path: {tmp_path}").replace("./Adobe_240fps_dataset/Adobe_240fps_blur", toy)
    y = y.replace("LQ_size: [3, 256, 256]", "LQ_size: [3, 64, 64]").replace("batch_size: 8 ", "batch_size: 2 ").replace("n_workers: 3 ", "n_workers: 0 ")
    y = y.replace("    # device_cache: true        # bin_amd extension: decode",
                  "    device_cache: true\n    blur_window: [5, 11]\n    blur_gamma: 2.2\n    blur_noise: [0.004, 0.0004]\n    # decode", 1)
    y = y.replace("print_freq: 100", "print_freq: 1")
    assert "\n    blur_noise: [0.004, 0.0004]\n" in y and "batch_size: 2 " in y
    p = str(tmp_path / "toy.yml")
    open(p, "w").write(y)
    r = subprocess.run([sys.executable, "-m", "bin_amd.train", "-opt", p, "--max_iter", "2"], cwd=REPO, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    exp = tmp_path / "experiments" / "adobe_stage4"
    text = open(exp / [f for f in os.listdir(exp) if f.endswith(".log")][0]).read()
    losses = [float(v) for v in re.findall(r"iter:\s+\d+, lr:\S+ loss (\S+)", text)]
    print(losses)
    assert len(losses) == 2 and all(np.isfinite(v) and v > 0 for v in losses) and "Device frame cache" in text


# ------------------------------------------------------------------------------------------------ the video tool
def test_make_blur_video_gamma_and_noise_write_the_host_functions_frames(tmp_path):
    """tools/make_blur_video.py --gamma srgb --noise ... --noise_seed 3: output frame i is expose_average of the BGR frames the
    planes convert to, key (3, i), converted back to planes."""
    from bin_amd import ops, video
    from bin_amd.data import exposure as X
    src, dst = str(tmp_path / "sharp.y4m"), str(tmp_path / "blurry.y4m")
    payloads = CL.write_clip(src, 40, 24, 40, 420, seed=12, tags=b"F240:1 Ip A1:1")
    tool = os.path.join(REPO, "tools", "make_blur_video.py")
    run = subprocess.run([sys.executable, tool, src, dst, "--window", "11", "--gamma", "srgb", "--noise", "0.01,0.002", "--noise_seed", "3"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    fmt = (420, "bt601", "limited")
    arena = ops.yuv_to_bgr(torch.from_numpy(payloads).cuda(), 24, 40, fmt).cpu().numpy()
    with video.Y4MReader(dst) as rd:
        written = [bytes(p) for p in rd]
    assert len(written) == 3
    for i, got in enumerate(written):
        c = 16 + 8 * i
        exposed = X.expose_average(arena[c - 5:c + 6], X.curve_tables("srgb", (0.01, 0.002)), (3, i))
        frame = torch.from_numpy(np.ascontiguousarray(exposed[:, :, ::-1].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)).cuda()
        assert got == ops.frame_to_yuv(frame, 0, 0, 24, 40, fmt).cpu().numpy().tobytes(), i
