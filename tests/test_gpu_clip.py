"""-m gpu: binclip_yuv_to_bgr (ops.yuv_to_bgr) against the composition it replaces and against the float64 restatement
(clip_cases.py), on both data paths; the device frame cache filled from a Y4M clip against the folder loader on the PNG tree of the
same frames (same `random` state => same batches bit for bit), down to a training step; tools/make_blur_video.py."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import clip_cases as CL
import video_cases as VC
from conftest import REPO

pytestmark = pytest.mark.gpu

LEAD = 64                        # guard bytes before and after every device buffer (a multiple of 16: the views stay aligned)


def _to_bgr(ops, host, n, stride, h, w, fmt, lead=LEAD):
    """ops.yuv_to_bgr on the staged bytes `host` (payloads at lead + i * stride) into a guarded output; returns uint8 [n, h, w, 3]."""
    src = torch.from_numpy(host).cuda()
    out = torch.full((2 * LEAD + n * h * w * 3,), VC.GUARD, dtype=torch.uint8, device="cuda")
    view = out[LEAD:LEAD + n * h * w * 3].view(n, h, w, 3)
    got = ops.yuv_to_bgr(src[lead:lead + n * stride].view(n, stride), h, w, fmt, out=view)
    assert got is view
    res = out.cpu().numpy()
    assert (res[:LEAD] == VC.GUARD).all() and (res[-LEAD:] == VC.GUARD).all(), "guard bytes around the output"
    assert torch.equal(src.cpu(), torch.from_numpy(host)), "the input is read only"
    return res[LEAD:-LEAD].reshape(n, h, w, 3)


def _composition(ops, payload, h, w, fmt):
    p = torch.from_numpy(np.ascontiguousarray(payload)).cuda()
    return ops.frame_to_u8(ops.yuv_to_frame(p, h, w, fmt, (0, 0, 0, 0)), 0, 0, h, w).cpu().numpy()


@pytest.mark.parametrize("h,w,chroma", VC.CASES, ids=VC.CASE_IDS)
def test_yuv_to_bgr_is_frame_to_u8_of_yuv_to_frame(h, w, chroma):
    """Random payloads, every (matrix, range), n in {1, 3}, three strides: byte for byte the composition, per frame; the guard bytes
    survive; the padding of a stride never reaches the result."""
    from bin_amd import ops
    fb = VC.frame_bytes(h, w, chroma)
    for matrix, rng in VC.MATRIX_RANGE:
        fmt = (chroma, matrix, rng)
        for n in (1, 3):
            payloads = [VC.random_payload(h, w, chroma, 100 * n + i) for i in range(n)]
            want = np.stack([_composition(ops, p, h, w, fmt) for p in payloads])
            for kind in CL.STRIDES:
                stride = CL.stride_of(kind, fb)
                got = [_to_bgr(ops, CL.staged(payloads, stride, fill, LEAD), n, stride, h, w, fmt) for fill in (0x00, 0xFF)]
                assert np.array_equal(got[0], want), (fmt, n, kind)
                assert np.array_equal(got[1], got[0]), "the padding bytes of a stride are never read into the result"
    made = ops.yuv_to_bgr(torch.from_numpy(np.stack(payloads)).cuda(), h, w, fmt)
    assert made.shape == (3, h, w, 3) and made.dtype == torch.uint8 and np.array_equal(made.cpu().numpy(), want), "without `out`"


def test_yuv_to_bgr_where_blocks_stride():
    """1030 x 2048 at 4:4:4: 527 360 items, more than 2048 blocks of 256 hold."""
    from bin_amd import ops
    h, w, chroma = CL.BIG_CASE
    fmt = (chroma, "bt709", "limited")
    payload = VC.random_payload(h, w, chroma, 77)
    fb = payload.size
    want = _composition(ops, payload, h, w, fmt)
    for stride in (fb, fb + 6):
        assert np.array_equal(_to_bgr(ops, CL.staged([payload], stride, 0x5A, LEAD), 1, stride, h, w, fmt)[0], want), stride


def _check_against_float64(got, payload, h, w, fmt):
    ref, mask = CL.ref_and_mask(payload, h, w, fmt)
    assert np.array_equal(got[~mask], ref[~mask]), (fmt, int((got != ref)[~mask].sum()))
    assert int(np.abs(got.astype(np.int16) - ref.astype(np.int16)).max()) <= 1
    return int(mask.sum()), int((got != ref).sum())


def test_yuv_to_bgr_against_float64_on_the_case_table():
    """Outside the near-tie mask every byte is the float64 restatement's, inside it at most one off; an aligned view and a view
    offset by one byte (the two data paths) give the same bytes."""
    from bin_amd import ops
    for h, w, chroma in VC.CASES:
        for matrix, rng in VC.MATRIX_RANGE:
            fmt = (chroma, matrix, rng)
            payloads = [VC.random_payload(h, w, chroma, 7 + i) for i in range(3)]
            stride = CL.stride_of("round16", payloads[0].size)
            aligned = _to_bgr(ops, CL.staged(payloads, stride, 0, LEAD), 3, stride, h, w, fmt)
            shifted = _to_bgr(ops, CL.staged(payloads, stride, 0, LEAD + 1), 3, stride, h, w, fmt, lead=LEAD + 1)
            assert np.array_equal(aligned, shifted), (h, w, fmt)
            for i, p in enumerate(payloads):
                _check_against_float64(aligned[i], p, h, w, fmt)


@pytest.mark.parametrize("matrix,rng", VC.MATRIX_RANGE)
def test_yuv_to_bgr_against_float64_on_every_code_point(matrix, rng):
    """All 2^24 (Y, U, V) as one 4096 x 4096 4:4:4 frame, on both data paths."""
    from bin_amd import ops
    fmt = (444, matrix, rng)
    payload = CL.all_code_points()
    fb = payload.size
    aligned = _to_bgr(ops, CL.staged([payload], fb, 0, LEAD), 1, fb, 4096, 4096, fmt)[0]
    shifted = _to_bgr(ops, CL.staged([payload], fb, 0, LEAD + 1), 1, fb, 4096, 4096, fmt, lead=LEAD + 1)[0]
    assert np.array_equal(aligned, shifted), "dwords and bytes give the same result"
    in_mask = off = 0
    for r0 in range(0, 4096, 512):                                # the float64 restatement in slabs of 512 rows
        rows = slice(r0, r0 + 512)
        a, b = _check_against_float64(aligned[rows], CL.all_code_points(rows), 512, 4096, fmt)
        in_mask, off = in_mask + a, off + b
    print(f"[clip] {fmt}: every code point; {in_mask} of {3 << 24} bytes in the near-tie mask, {off} of them one off")
    assert in_mask < 0.005 * (3 << 24)


# ------------------------------------------------------------------------------------------------ the cache and the loader
N_FRAMES, FH, FW = 80, 352, 640
BLUR = [7, 11, 15]


@pytest.fixture(scope="module")
def clip_and_tree(tmp_path_factory):
    """One 80-frame 640x352 4:2:0 clip, and the PNG tree <root>/<mode>/clipA/00001.png .. 00080.png of its frames as ops.yuv_to_bgr
    converts them.  Returns (folder of the clip, root of the tree, uint8 [80, 352, 640, 3] BGR frames)."""
    from PIL import Image
    from bin_amd import ops
    clips = tmp_path_factory.mktemp("clips")
    payloads = CL.write_clip(str(clips / "clipA.y4m"), N_FRAMES, FH, FW, 420, seed=4)
    frames = ops.yuv_to_bgr(torch.from_numpy(payloads).cuda(), FH, FW, (420, "bt601", "limited")).cpu().numpy()
    tree = tmp_path_factory.mktemp("tree")
    for mode in ("train", "test"):
        os.makedirs(tree / mode / "clipA")
    for k in range(N_FRAMES):
        Image.fromarray(np.ascontiguousarray(frames[k][:, :, ::-1])).save(str(tree / "train" / "clipA" / f"{k + 1:05d}.png"), compress_level=1)
        os.link(str(tree / "train" / "clipA" / f"{k + 1:05d}.png"), str(tree / "test" / "clipA" / f"{k + 1:05d}.png"))
    return str(clips), str(tree), frames


def _video_loader(clips, phase, batch, crop):
    from bin_amd.data import create_dataloader, create_dataset
    opt = {"mode": "BIN_video", "name": "train", "dataroot_video": clips, "LQ_size": list(crop), "phase": phase, "blur_window": BLUR,
           "batch_size": batch, "n_workers": 0, "device_cache": True}
    random.seed(0)
    ds = create_dataset(opt)
    return ds, create_dataloader(ds, opt, {"dist": False, "gpu_ids": [0]}, None)


def _folder_loader(tree, phase, batch, crop):
    from bin_amd.data import create_dataloader, create_dataset
    opt = {"mode": "BIN", "name": "train" if phase == "train" else "test", "dataroot_GT": tree, "dataroot_LQ": tree, "LQ_size": list(crop),
           "data_type": "img", "phase": phase, "blur_window": BLUR, "batch_size": batch, "n_workers": 0, "device_cache": True}
    random.seed(0)
    ds = create_dataset(opt)
    return ds, create_dataloader(ds, opt, {"dist": False, "gpu_ids": [0]}, None)


@pytest.mark.parametrize("phase,batch,passes", [("train", 3, 2), ("val", 1, 1)])
def test_video_loader_batches_equal_the_folder_loaders(clip_and_tree, phase, batch, passes):
    """80 frames give 3 windows: two passes of one batch of 3 in the train phase, one pass of three single windows in any other."""
    from bin_amd.data.device_cache import DeviceWindowLoader
    from bin_amd.data.video_dataset import VideoFrameCache
    clips, tree, frames = clip_and_tree
    crop = (3, 64, 96)
    vds, vloader = _video_loader(clips, phase, batch, crop)
    fds, floader = _folder_loader(tree, phase, batch, crop)
    assert isinstance(vloader, DeviceWindowLoader) and isinstance(vloader.cache, VideoFrameCache) and isinstance(floader, DeviceWindowLoader)
    assert [w[3] for w in vds.all_paths] == [w[3] for w in fds.all_paths] and len(vds) == 3
    assert len(vloader) == len(floader) == 3 // batch and vloader.src_size == (FH, FW)
    # the arena: files 10 .. 80 (first centre 17 - 7 to last centre 73 + 7), the frames the conversion of the whole clip gives
    cache = vloader.cache
    assert cache.shape == (71, FH, FW, 3) and cache.clip_ranges.tolist() == [[0, 71]] == floader.cache.clip_ranges.tolist()
    assert [os.path.basename(p) for p in cache.paths] == [f"{k:05d}.png" for k in range(10, 81)]
    assert os.path.dirname(cache.paths[0]) == os.path.join(clips, "clipA.y4m")
    arena = cache.frames.cpu().numpy()
    assert np.array_equal(arena, frames[9:80]) and np.array_equal(arena, floader.cache.frames.cpu().numpy())
    got = []
    for loader in (floader, vloader):
        random.seed(123)
        got.append([b for _ in range(passes) for b in loader])
        state = random.getstate()
    random.seed(123)
    [b for _ in range(passes) for b in floader]
    assert random.getstate() == state, "both loaders draw the same values"
    assert len(got[0]) == len(got[1]) == passes * (3 // batch)
    for fb, vb in zip(*got):
        assert fb["key"] == vb["key"] and len(vb["key"]) == batch and all(k.startswith("clipA_000") for k in vb["key"])
        for k in ("LQs", "GTenh", "GTinp"):
            assert vb[k].is_cuda and vb[k].shape == fb[k].shape and vb[k].shape[0] == batch
            assert torch.equal(vb[k].view(torch.int32), fb[k].view(torch.int32)), k
        assert not torch.equal(vb["LQs"], vb["GTenh"])


def test_training_step_fed_from_the_video_loader(clip_and_tree, tmp_path):
    from bin_amd import ops
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    clips, _, _ = clip_and_tree
    _, loader = _video_loader(clips, "train", 2, (3, 64, 64))
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
    before = {k: v.detach().clone() for k, v in m.netG.module.state_dict().items()}
    m.feed_data(batch)
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    ops.check_status()
    loss = float(m.loss.detach())
    assert np.isfinite(loss) and loss > 0
    after = m.netG.module.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before), "the step moved the weights"


# ------------------------------------------------------------------------------------------------ the tool
@pytest.mark.parametrize("window", [1, 11])
def test_make_blur_video_writes_the_truncated_means(tmp_path, window):
    from bin_amd import ops, video
    from bin_amd.data.BIN_dataset import blur_average
    src, dst = str(tmp_path / "sharp.y4m"), str(tmp_path / "blurry.y4m")
    payloads = CL.write_clip(src, 40, 24, 40, 420, seed=window, tags=b"F240:1 Ip A1:1")
    tool = os.path.join(REPO, "tools", "make_blur_video.py")
    run = subprocess.run([sys.executable, tool, src, dst, "--window", str(window)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert "--gt_video " + src in run.stdout and "--gt_offset 16" in run.stdout and "--input_video " + dst in run.stdout
    assert "0 centre(s) dropped at the front and 0 at the back" in run.stdout
    header, n = video.clip_info(dst)
    assert n == 40 // 8 - 2 == 3 and header.rate == (240, 8)
    assert (header.width, header.height, header.colorspace, header.interlace, header.aspect) == (40, 24, "420jpeg", "p", "1:1")
    fmt = (420, "bt601", "limited")
    arena = ops.yuv_to_bgr(torch.from_numpy(payloads).cuda(), 24, 40, fmt).cpu().numpy()
    h = window // 2
    with video.Y4MReader(dst) as rd:
        written = [bytes(p) for p in rd]
    for i, got in enumerate(written):
        c = 16 + 8 * i
        mean = blur_average(arena[c - h:c + h + 1])                                # uint8 [24, 40, 3] BGR
        frame = torch.from_numpy(np.ascontiguousarray(mean[:, :, ::-1].transpose(2, 0, 1)).astype(np.float32) / np.float32(255)).cuda()
        want = ops.frame_to_yuv(frame, 0, 0, 24, 40, fmt).cpu().numpy().tobytes()
        assert got == want, (window, i)
    # it refuses an existing output and leaves it as it is
    before = open(dst, "rb").read()
    again = subprocess.run([sys.executable, tool, src, dst, "--window", str(window)], capture_output=True, text=True)
    assert again.returncode != 0 and "exists" in again.stderr and open(dst, "rb").read() == before
