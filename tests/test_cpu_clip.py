"""CPU: what can be pinned about training from Y4M clips (dataset mode BIN_video) without a device — libbinclip.so's ABI bookkeeping and
its refusals before any launch, ops.yuv_to_bgr's refusals, video.clip_info, the window list of clips against the script's rule and
against make_sharp_window_list, the dataset's refusals, draw_window_aug's source size, and the restatement the device tests compare
with (clip_cases.py: the near-tie mask is small and an fp32 evaluation agrees with float64 outside it).  GPU side: test_gpu_clip.py."""
import ctypes as C
import inspect
import io
import os
import random
import re

import numpy as np
import pytest
import torch

import blur_cases as BC
import clip_cases as CL
import video_cases as VC
from conftest import REPO


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_clip_library_header_and_binding_agree():
    """What is binclip's own beside the bookkeeping of test_cpu_libraries.py: the format is binyuv.h's, included and not redeclared,
    the codes against the binding, and a source that shares binyuv's arithmetic."""
    from bin_amd import _lib
    hdr = open(os.path.join(REPO, "include", "binclip.h")).read()
    assert '#include "binyuv.h"' in hdr and "typedef" not in hdr
    for name, value, bound in (("BINCLIP_E_ARG", -1, _lib.CLIP_E_ARG), ("BINCLIP_E_SHAPE", -2, _lib.CLIP_E_SHAPE)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value == bound
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binclip.hip")).read()
    assert '#include "binyuv_common.h"' in src and "static_assert(sizeof(BinYuvFormat) == 12" in src
    for shared in ("coefficients(", "yuv_pixel(", "split(", "grid_for("):
        assert shared in src, f"{shared} is binyuv_common.h's"
    assert not re.search(r"(?m)^\s*#\s*(if|ifdef|ifndef|elif|define)\b", src), "no preprocessor switches in the source"
    assert "__shared__" not in src and "asm" not in re.sub(r"//.*", "", src)


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced: every
    call here is one the library refuses, none reaches a launch)."""
    from bin_amd import _lib
    lib = _lib.cliplib()
    P, X = 0x100000, 0x4000000
    fmt = lambda chroma=420, matrix=0, rng=0: C.byref(_lib.BinYuvFormat(chroma, matrix, rng))
    FB = VC.frame_bytes(6, 10, 420)                                # 90

    def call(p=P, n=3, stride=FB, h=6, w=10, f=None, out=X):
        return lib.binclip_yuv_to_bgr(p, n, stride, h, w, f if f is not None else fmt(), out, None)
    assert call(p=None) == -1 and call(out=None) == -1
    for n in (0, -1, -2 ** 31):
        assert call(n=n) == -1, n
    for h, w in ((0, 10), (6, 0), (-1, 10), (6, -3)):
        assert call(h=h, w=w) == -1
    for bad in (fmt(chroma=422), fmt(chroma=0), fmt(matrix=2), fmt(matrix=-1), fmt(rng=2), fmt(rng=-1)):
        assert call(f=bad) == -1
    assert call(f=C.POINTER(_lib.BinYuvFormat)()) == -1, "a null format"
    for stride in (FB - 1, 0, -FB, -2 ** 62):
        assert call(stride=stride) == -1, stride
    assert call(f=fmt(chroma=444), stride=179) == -1 and call(h=5, w=3, stride=26) == -1, "4:4:4 needs 180, 5 x 3 at 4:2:0 needs 27"
    assert call(n=1, h=2 ** 31 - 1, w=2 ** 31 - 1, stride=2 ** 62) == -1, "a frame of more than 2^62 bytes"
    # the output on the input range: 3 payloads at stride 96 end at P + 2 * 96 + 90; the output is 3 * 180 bytes
    assert call(stride=96, out=P) == -1 and call(stride=96, out=P + 281) == -1 and call(stride=96, out=P - 539) == -1
    assert call(n=1, out=P + 89) == -1 and call(n=1, out=P - 179) == -1
    # more than 2^40 output bytes, n * payload_stride beyond it; argument errors come first
    assert call(n=1, h=2 ** 20, w=2 ** 20, stride=2 ** 41) == -2 and call(n=2 ** 11, h=2 ** 14, w=2 ** 14, stride=2 ** 29) == -2
    assert call(n=2 ** 11, h=16, w=16, stride=2 ** 30) == -2 and call(n=1, h=16, w=16, stride=2 ** 40 + 1) == -2
    assert call(n=2 ** 31 - 1, h=16, w=16, stride=2 ** 62) == -2
    assert call(n=1, h=2 ** 20, w=2 ** 20, stride=2 ** 41, out=None) == -1 and call(n=2 ** 11, h=16, w=16, stride=2 ** 30, f=fmt(rng=7)) == -1


def test_ops_yuv_to_bgr_refuses_cpu_tensors_and_wrong_layouts():
    from bin_amd import ops
    fmt = (420, "bt601", "limited")
    fb = VC.frame_bytes(6, 10, 420)
    p = torch.zeros((3, fb), dtype=torch.uint8)
    assert list(inspect.signature(ops.yuv_to_bgr).parameters) == ["payloads", "h", "w", "fmt", "out"]
    assert inspect.signature(ops.yuv_to_bgr).parameters["out"].default is None
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.yuv_to_bgr(p, 6, 10, fmt)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.yuv_to_bgr(torch.zeros((3, fb + 6), dtype=torch.uint8), 6, 10, fmt, out=torch.zeros((3, 6, 10, 3), dtype=torch.uint8))
    for bad in ((422, "bt601", "limited"), (420, "bt2020", "limited"), (420, "bt601", "tv")):
        with pytest.raises(ValueError, match="YUV format"):
            ops.yuv_to_bgr(p, 6, 10, bad)
    for h, w in ((0, 10), (6, 0), (-6, 10)):
        with pytest.raises(ValueError, match="positive size"):
            ops.yuv_to_bgr(p, h, w, fmt)
    wide = torch.zeros((3, 2 * fb), dtype=torch.uint8)
    for bad in (p.int(), p[:, :fb - 1], p.reshape(-1), p[:0], p.reshape(3, fb, 1), wide[:, ::2], torch.zeros((fb, 3), dtype=torch.uint8).t()):
        with pytest.raises(ValueError, match="payloads"):
            ops.yuv_to_bgr(bad, 6, 10, fmt)
    for bad in (torch.zeros((3, 6, 10, 3)), torch.zeros((2, 6, 10, 3), dtype=torch.uint8), torch.zeros((3, 10, 6, 3), dtype=torch.uint8),
                torch.zeros((3, 6, 10, 4), dtype=torch.uint8)[..., :3], torch.zeros((6, 6, 10, 3), dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError, match="fills a contiguous uint8"):
            ops.yuv_to_bgr(p, 6, 10, fmt, out=bad)


# ------------------------------------------------------------------------------------------------ clips on disk
def test_clip_info_by_size_and_by_walking(tmp_path):
    from bin_amd import video as V
    bare = str(tmp_path / "bare.y4m")
    CL.write_clip(bare, 7, 6, 10, 420, seed=1)
    header, n = V.clip_info(bare)
    assert n == 7 and (header.width, header.height, header.chroma, header.rate) == (10, 6, 420, (240, 1))
    calls = []
    real = V.Y4MReader._line

    def counted(self):
        calls.append(1)
        return real(self)
    V.Y4MReader._line, keep = counted, real
    try:
        assert V.clip_info(bare)[1] == 7 and len(calls) == 1, "bare FRAME lines: the header line alone is read, the count is the size's"
        params = str(tmp_path / "params.y4m")
        payloads = CL.write_clip(params, 5, 5, 3, 444, seed=2, frame_line=b"FRAME Ip Xfoo")
        del calls[:]
        assert V.clip_info(params)[1] == 5 and len(calls) == 6, "FRAME lines with parameters: walked"
    finally:
        V.Y4MReader._line = keep
    with V.Y4MReader(params) as rd:
        assert [bytes(p) for p in rd] == [p.tobytes() for p in payloads], "the reader agrees with the count"
    # an open seekable object; an empty clip
    with open(bare, "rb") as f:
        assert V.clip_info(f)[1] == 7
    assert V.clip_info(io.BytesIO(b"YUV4MPEG2 W4 H4 F30:1\n"))[1] == 0
    # a truncated last frame names it, on both paths
    data = open(bare, "rb").read()
    for cut in (1, 50, 90, 93):                                   # in the payload, and in the FRAME line itself
        with pytest.raises(ValueError, match="frame 6"):
            V.clip_info(io.BytesIO(data[:-cut]))
    data = open(params, "rb").read()
    with pytest.raises(ValueError, match="frame 4"):
        V.clip_info(io.BytesIO(data[:-7]))
    # the size fits but the last offset is not FRAME: 2 frames of 24 bytes with `FRAME Ip` lines are 3 frames with bare ones by size alone
    header = b"YUV4MPEG2 W4 H4 F30:1\n"
    odd = header + b"FRAME Ip\n" + bytes(24) + b"FRAME Ip\n" + bytes(24) + bytes(24)
    assert (len(odd) - len(header)) % 30 == 0
    with pytest.raises(ValueError, match="frame 2"):
        V.clip_info(io.BytesIO(odd))
    fits = header + b"FRAME\n" + bytes(24) + b"FRAME Xabcde\n" + bytes(24) + b"FRAME\n" + bytes(17)
    assert (len(fits) - len(header)) % 30 == 0
    with pytest.raises(ValueError, match="frame 2 is truncated"):
        V.clip_info(io.BytesIO(fits))
    # refusals
    with pytest.raises(ValueError, match="seekable"):
        V.clip_info("-")

    class Pipe(io.RawIOBase):
        def seekable(self):
            return False
    with pytest.raises(ValueError, match="seekable"):
        V.clip_info(Pipe())
    with pytest.raises(ValueError, match="C422"):
        V.clip_info(io.BytesIO(b"YUV4MPEG2 W4 H4 F30:1 C422\n"))


# ------------------------------------------------------------------------------------------------ the window list
CLIP_LENGTHS = [(name, 1, n) for name, _, n in BC.SHARP_CLIPS]      # 80, 85, 65, 30 and 12 frames, numbered from 1


def _numbers(window):
    from bin_amd.data.BIN_dataset import frame_number
    return [frame_number(p) for p in window[0]], [frame_number(p) for p in window[1]], [frame_number(p) for p in window[2]], window[3]


@pytest.fixture(scope="module")
def clip_folder(tmp_path_factory):
    root = tmp_path_factory.mktemp("clips")
    for name, _, n in CLIP_LENGTHS:
        CL.write_clip(str(root / (name + ".y4m")), n, 6, 10, 420, seed=n)
    return str(root)


def _opt(root, **kw):
    opt = {"mode": "BIN_video", "name": "train", "dataroot_video": root, "LQ_size": [3, 4, 8], "phase": "train", "blur_window": 11}
    opt.update(kw)
    return opt


@pytest.mark.parametrize("window", [1, 11, 33])
def test_window_list_of_clips_is_the_scripts_rule(clip_folder, window):
    from bin_amd.data import create_dataset
    from bin_amd.data.video_dataset import VideoClipDataset, make_clip_window_list
    want = BC.expected_windows(CLIP_LENGTHS, window)
    assert len(want) == {1: 3 + 3 + 1, 11: 3 + 3 + 1, 33: 1 + 2 + 0}[window]
    ds = create_dataset(_opt(clip_folder, blur_window=window))
    assert isinstance(ds, VideoClipDataset) and len(ds) == len(want) and ds.frame_size == (6, 10)
    assert list(ds.clips) == [os.path.join(clip_folder, n + ".y4m") for n in ("clipA", "clipB", "clipC", "clipD", "clipE")], "sorted names"
    assert [n for _, n, _ in ds.clips.values()] == [80, 85, 65, 30, 12]
    got = {}
    for win in ds.all_paths:
        blurry, sharp, mid, key = _numbers(win)
        clip = os.path.join(clip_folder, key[:5] + ".y4m")
        assert all(os.path.dirname(p) == clip for p in win[0] + win[1] + win[2]), "pseudo-paths <clip.y4m>/<NNNNN>.png"
        assert blurry == sharp, "a blurry entry is its centre sharp frame"
        got[key] = (sharp, mid)
    assert got == {k: (list(cs), list(mid)) for k, (cs, mid) in want.items()}
    # a list of files, in its order; the unshuffled list and the split
    files = [os.path.join(clip_folder, n + ".y4m") for n in ("clipB", "clipA")]
    ds2 = create_dataset(_opt(files, blur_window=window))
    assert list(ds2.clips) == files and {w[3][:5] for w in ds2.all_paths} == {"clipA", "clipB"}
    plain, rest = make_clip_window_list([(f, ds2.clips[f][1]) for f in files], shuffle=False, blur_window=window)
    assert [w[3] for w in plain] == sorted((w[3] for w in plain), key=lambda k: (k[:5] != "clipB", k)) and rest == []
    a, b = make_clip_window_list([(f, ds2.clips[f][1]) for f in files], split=50, shuffle=False, blur_window=window)
    assert len(a) == len(plain) // 2 and a + b == plain


def test_one_clip_gives_the_folders_list_under_the_same_random_state(tmp_path):
    """A stream of n frames gives the windows, keys and order a folder of 00001.png .. n.png gives: one shuffle, the same draws."""
    from bin_amd.data.BIN_dataset import make_sharp_window_list
    from bin_amd.data.video_dataset import make_clip_window_list
    n = 200
    folder = tmp_path / "tree" / "train" / "clipA"
    folder.mkdir(parents=True)
    for k in range(1, n + 1):
        (folder / f"{k:05d}.png").touch()
    clip = str(tmp_path / "clipA.y4m")
    for window in (1, 11, [7, 11, 15], 33):
        for split in (100, 70):
            random.seed(5)
            want = make_sharp_window_list(str(tmp_path / "tree"), "train", split, True, window)
            state = random.getstate()
            random.seed(5)
            got = make_clip_window_list([(clip, n)], split, True, window)
            assert random.getstate() == state
            for w_list, g_list in zip(want, got):
                assert [_numbers(w) for w in w_list] == [_numbers(g) for g in g_list]
            assert len(got[0]) + len(got[1]) == n // 8 - 2 - 5 - (2 if window == 33 else 0) and len(got[0]) >= 10


def test_dataset_refusals_come_before_any_device_call(clip_folder, tmp_path, monkeypatch):
    from bin_amd import ops
    from bin_amd.data import create_dataloader, create_dataset
    monkeypatch.setattr(ops, "yuv_to_bgr", lambda *a, **k: pytest.fail("no device call"))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: pytest.fail("nothing is allocated"))
    with pytest.raises(ValueError, match="blur_window.*required"):
        create_dataset(_opt(clip_folder, blur_window=None))
    with pytest.raises(ValueError, match="blur_window"):
        create_dataset(_opt(clip_folder, blur_window=12))
    with pytest.raises(ValueError, match="dataroot_video"):
        create_dataset(_opt(None))
    with pytest.raises(ValueError, match="crop"):
        create_dataset(_opt(clip_folder, LQ_size=[3, 7, 8]))
    with pytest.raises(ValueError, match="crop"):
        create_dataset(_opt(clip_folder, LQ_size=[3, 4, 11]))
    create_dataset(_opt(clip_folder, LQ_size=[3, 6, 10]))
    empty = tmp_path / "none"
    empty.mkdir()
    with pytest.raises(ValueError, match="no \\*.y4m clip"):
        create_dataset(_opt(str(empty)))
    # clips that disagree: both files are named
    a = os.path.join(clip_folder, "clipA.y4m")
    for name, (h, w, chroma) in (("wide", (6, 12, 420)), ("tall", (8, 10, 420)), ("c444", (6, 10, 444))):
        other = str(tmp_path / (name + ".y4m"))
        CL.write_clip(other, 80, h, w, chroma)
        with pytest.raises(ValueError, match="differ") as e:
            create_dataset(_opt([a, other]))
        assert a in str(e.value) and other in str(e.value)
    with pytest.raises(ValueError, match="yuv_matrix|YUV matrix"):
        create_dataset(_opt(clip_folder, yuv_matrix="bt2020"))
    ds = create_dataset(_opt(clip_folder, yuv_matrix="bt709", yuv_range="full"))
    assert {f for _, _, f in ds.clips.values()} == {(420, "bt709", "full")}
    assert {f for _, _, f in create_dataset(_opt(clip_folder)).clips.values()} == {(420, "bt601", "limited")}
    # no host loader: the dataloader without device_cache, and an item
    for phase in ("train", "val"):
        with pytest.raises(ValueError, match="device_cache: true"):
            create_dataloader(ds, _opt(clip_folder, phase=phase, batch_size=2, n_workers=0), {"dist": False, "gpu_ids": [0]})
    with pytest.raises(ValueError, match="device_cache: true"):
        ds[0]
    # the cache's size check comes before any allocation, with the existing message
    from bin_amd.data.video_dataset import VideoFrameCache
    with pytest.raises(ValueError, match=r"more than device_cache_max_gb = 1e-06"):
        VideoFrameCache(ds, "cuda", max_gb=1e-6)
    with pytest.raises(NotImplementedError):
        create_dataset(_opt(clip_folder, mode="BIN_film"))


def test_shipped_option_file_names_the_mode():
    from bin_amd.options import options
    opt = options.parse(os.path.join(REPO, "bin_amd", "options", "bin_stage4_y4m.yml"))
    for phase in ("train", "val"):
        ds = opt["datasets"][phase]
        assert ds["mode"] == "BIN_video" and ds["device_cache"] is True and ds["dataroot_video"] and ds["blur_window"] and ds["phase"] == phase
    assert opt["datasets"]["train"]["blur_window"] == [7, 11, 15] and opt["datasets"]["train"]["batch_size"] == 8
    ref = options.parse(os.path.join(REPO, "bin_amd", "options", "bin_stage4_adobe240.yml"))
    assert opt["train"] == ref["train"] and opt["network_G"] == ref["network_G"] and opt["logger"] == ref["logger"]


# ------------------------------------------------------------------------------------------------ the crop draws
def test_draw_window_aug_default_is_unchanged_and_a_source_size_sets_the_ranges():
    from bin_amd.data.BIN_dataset import SRC_H, SRC_W, draw_window_aug
    sig = inspect.signature(draw_window_aug).parameters
    assert list(sig) == ["input_frame_size", "data_aug", "src_size"] and sig["src_size"].default == (SRC_H, SRC_W) == (352, 640)
    for crop in ((3, 128, 256), (3, 352, 640), (3, 1, 1)):
        for aug in (True, False):
            random.seed(11)
            want = []
            for _ in range(50):                                   # the draws as the function made them before it took a size
                reverse = not (aug and random.randint(0, 1))
                y0 = random.choice(range(352 - crop[1] + 1))
                x0 = random.choice(range(640 - crop[2] + 1))
                want.append((reverse, y0, x0, bool(aug and random.randint(0, 1))))
            state = random.getstate()
            random.seed(11)
            assert [draw_window_aug(crop, aug) for _ in range(50)] == want and random.getstate() == state
            random.seed(11)
            assert [draw_window_aug(crop, aug, (352, 640)) for _ in range(50)] == want
    random.seed(3)
    draws = [draw_window_aug((3, 4, 8), True, (6, 10)) for _ in range(400)]
    assert {d[1] for d in draws} == {0, 1, 2} and {d[2] for d in draws} == {0, 1, 2} and {d[0] for d in draws} == {True, False}
    random.seed(3)
    big = [draw_window_aug((3, 256, 256), True, (720, 1280)) for _ in range(400)]
    assert max(d[1] for d in big) > 352 - 256 and max(d[2] for d in big) > 640 - 256 and all(d[1] <= 464 and d[2] <= 1024 for d in big)
    assert draw_window_aug((3, 6, 10), False, (6, 10)) == (True, 0, 0, False)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("matrix,rng", VC.MATRIX_RANGE)
def test_near_tie_mask_is_small_and_float32_agrees_outside_it(matrix, rng):
    """The bar of the device test (every byte outside the mask equal to the float64 restatement) is not vacuous: the mask leaves
    more than 99.5 % of the bytes, and an fp32 evaluation of the same formulas has TIE_MARGIN = 9.8e-4 to spend and needs 1e-4."""
    fmt = (444, matrix, rng)
    payload = VC.random_payload(512, 2048, 444, 9)
    v64, v32 = CL.scaled_ref(payload, 512, 2048, fmt), CL.scaled_ref(payload, 512, 2048, fmt, np.float32)
    ref, mask = CL.ref_and_mask(payload, 512, 2048, fmt)
    assert np.array_equal(ref, CL.bgr_ref(payload, 512, 2048, fmt)) and np.array_equal(mask, CL.near_tie(payload, 512, 2048, fmt))
    err = float(np.abs(v32.astype(np.float64) - v64).max())
    got = CL.bgr_ref(payload, 512, 2048, fmt, np.float32)
    outside = int((got != ref)[~mask].sum())
    print(f"[clip] {fmt}: mask {mask.mean():.5f} of the bytes, fp32 error {err:.2e} on the 0..255 scale (margin {CL.TIE_MARGIN:.2e}), "
          f"{outside} mismatches outside the mask, {int((got != ref).sum())} inside")
    assert 0 < mask.mean() < 0.005
    assert err < CL.TIE_MARGIN / 8 and outside == 0
    assert int(np.abs(got.astype(np.int16) - ref.astype(np.int16)).max()) <= 1
    assert ref.shape == (512, 2048, 3) and ref.dtype == np.uint8 and 0 in ref and 255 in ref, "the clamp is reached at both ends"


def test_restatement_layout_and_inputs():
    fmt = (420, "bt601", "full")
    p = VC.random_payload(5, 7, 420, 1)
    rgb = VC.to_frame_ref(p, 5, 7, fmt, (0, 0, 0, 0))
    ref = CL.bgr_ref(p, 5, 7, fmt)
    for c in range(3):
        assert np.array_equal(ref[:, :, c], np.rint(255 * rgb[2 - c]).astype(np.uint8)), "HWC, B G R"
    grey = np.concatenate([np.arange(256, dtype=np.uint8), np.full(512, 128, np.uint8)])
    assert np.array_equal(CL.bgr_ref(grey, 1, 256, (444, "bt709", "full")), np.repeat(np.arange(256, dtype=np.uint8), 3).reshape(1, 256, 3))
    rows = CL.all_code_points(slice(4094, 4096))
    Y, U, V = VC.split_planes(rows, 2, 4096, 444)
    assert (Y == 255).all() and set(U[0]) == {0xE0 + i for i in range(16)} and U[1, -1] == 255 and list(V[1, -3:]) == [253, 254, 255]
    assert len(CL.all_code_points(slice(0, 16))) == 3 * 16 * 4096
    assert [CL.stride_of(k, 90) for k in CL.STRIDES] == [90, 96, 96] and [CL.stride_of(k, 1440) for k in CL.STRIDES] == [1440, 1446, 1440]
    buf = CL.staged([np.full(4, 1, np.uint8), np.full(4, 2, np.uint8)], 6, 9, lead=1)
    assert list(buf) == [9, 1, 1, 1, 1, 9, 9, 2, 2, 2, 2, 9, 9]
    h, w, c = CL.BIG_CASE
    assert (h * ((w + 3) // 4)) > 2048 * 256 and c == 444
