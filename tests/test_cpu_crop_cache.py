"""CPU: what can be pinned about the YUV device frame cache (`device_cache_format: yuv`) without a device — the planning function
(video_dataset.plan_crop_batch) against a numpy model of the decode and of both arenas, libbincrop.so's ABI bookkeeping and its
refusals before any launch, ops.yuv_crops_to_bgr's refusals of malformed rows, the option checks, the dataset's handling of clips of
different sizes, the cache's size refusal, and the stand-alone refusals program under host ASan / UBSan.  GPU side:
test_gpu_crop_cache.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import clip_cases as CL
import crop_cache_cases as CC
from conftest import REPO

NAME = "bincrop"
WANT = ["bincrop_version", "bincrop_yuv_crops_to_bgr"]


# ------------------------------------------------------------------------------------------------ the planning function
@pytest.fixture(scope="module")
def world():
    return CC.plan_world()


def _table(world, picks, keys=False):
    """window_table of `picks`: (window index, reverse, y0, x0, flip, h) per sample."""
    from bin_amd.data.device_cache import window_table
    windows = [world["windows"][i] for i, *_ in picks]
    draws = [(rev, y0, x0, flip) for _, rev, y0, x0, flip, _ in picks]
    halves = [h for *_, h in picks]
    return window_table(windows, draws, world["cache"].index, halves, [(7 + i, 2 ** 32 - 1 - i) for i in range(len(picks))] if keys else None)


def _plan(world, table):
    from bin_amd.data.video_dataset import plan_crop_batch
    return plan_crop_batch(table, world["offset"], world["h"], world["w"], world["format"], world["cache"].clip_ranges)


def test_plan_addresses_the_bytes_the_bgr_arena_holds(world):
    """h = 0, 3 and 16, reversed windows, flips, a span that starts at its clip's first cached frame and one that ends at its last,
    samples of two clips of different sizes and formats in one batch: every slot and every frame of every blurry range."""
    from bin_amd.data.device_cache import N_BLUR, N_SLOTS
    cache, windows = world["cache"], world["windows"]
    ranges = cache.clip_ranges.tolist()
    per_clip = [[i for i, w in enumerate(windows) if w[3].startswith(name[:5])] for name, *_ in CC.CLIPS]
    assert [len(p) for p in per_clip] == [6, 4] and ranges == [[0, 113], [113, 113 + 97]]
    a_first, a_last, b_first, b_last = per_clip[0][0], per_clip[0][-1], per_clip[1][0], per_clip[1][-1]
    ch, cw = CC.PLAN_CROP
    batches = [
        [(a_first, False, 0, 0, False, 16), (a_last, True, 6, 12, True, 16), (b_first, True, 8, 10, False, 16), (b_last, False, 3, 5, True, 16)],
        [(a_first, True, 1, 3, True, 0), (b_last, False, 0, 1, False, 0)],
        [(per_clip[0][2], False, 5, 7, True, 3), (per_clip[1][1], True, 2, 2, False, 3), (a_last, False, 6, 0, False, 0)],
        [(b_first, False, 8, 10, True, 7)],
    ]
    checked = 0
    for picks in batches:
        for keys in (False, True):
            table = _table(world, picks, keys)
            rows, local, rng = _plan(world, table)
            assert rows.dtype == np.int64 and rows.shape == (rng[-1, 1], 6)
            checked += CC.check_remap(world, table, (ch, cw), rows, local, rng)
            for r, (i, rev, y0, x0, flip, h) in enumerate(picks):
                lo, hi = int(table[r, :N_BLUR].min()) - h, int(table[r, :N_BLUR].max()) + h
                assert rng[r, 1] - rng[r, 0] == hi - lo + 1 == 41 + 2 * h <= 73, "first blurry centre - h .. last + h"
                assert (rows[rng[r, 0]:rng[r, 1], 3:5] == (y0, x0)).all() and int(local[r, N_SLOTS + 2]) == int(flip)
                k = cache.index[windows[i][0][0]]
                assert (rows[rng[r, 0]:rng[r, 1], 1:3] == (world["h"][k], world["w"][k])).all(), "the span's own clip's size"
                assert (rows[rng[r, 0]:rng[r, 1], 5] == world["format"][k]).all(), "and format"
                assert (np.diff(local[r, :6]) == (-8 if rev else 8)).all(), "a reversed window stays reversed"
    # the edges: with h = 16 the first window's span starts at its clip's first cached frame, the last one's ends at its last
    table = _table(world, batches[0])
    rows, _, rng = _plan(world, table)
    assert rows[rng[0, 0], 0] == world["offset"][0] and rows[rng[1, 1] - 1, 0] == world["offset"][112]
    assert rows[rng[2, 0], 0] == world["offset"][113] and rows[rng[3, 1] - 1, 0] == world["offset"][-1]
    assert checked == 2 * sum(6 * (2 * h + 1) + 11 for picks in batches for *_, h in picks) == 2188


def test_plan_refuses_a_span_that_leaves_its_clip(world):
    from bin_amd.data.device_cache import N_SLOTS
    good = _table(world, [(0, False, 0, 0, False, 16)])
    for change in (lambda t: t.__setitem__((0, slice(0, N_SLOTS)), t[0, :N_SLOTS] + 90),        # runs from clip A into clip B
                   lambda t: t.__setitem__((0, slice(0, N_SLOTS)), t[0, :N_SLOTS] - 1),         # one frame before the arena
                   lambda t: t.__setitem__((0, slice(0, N_SLOTS)), t[0, :N_SLOTS] + 170),       # past its end
                   lambda t: t.__setitem__((0, N_SLOTS + 3), -1)):
        bad = good.copy()
        change(bad)
        with pytest.raises(ValueError, match="span"):
            _plan(world, bad)
    with pytest.raises(ValueError, match="table must be"):
        _plan(world, good[:, :N_SLOTS + 3])


# ------------------------------------------------------------------------------------------------ the device tests' inputs
def test_kernel_test_payloads_hold_0_and_255_and_stay_off_rounding_ties():
    import video_cases as VC
    redrawn = 0
    for chroma in VC.CHROMAS:
        frames = CC.frame_payloads(chroma)
        assert [f[:2] for f in frames[::2]] == CC.FRAMES and len(frames) == 2 * len(CC.FRAMES)
        for h, w, p in frames:
            assert p.dtype == np.uint8 and p.size == VC.frame_bytes(h, w, chroma) and not CC.near_any_tie(p, h, w, chroma).any()
            if h * w > 1:
                assert all(pl.reshape(-1)[0] == 0 and pl.reshape(-1)[-1] == 255 for pl in VC.split_planes(p, h, w, chroma))
        redrawn += sum(int(CC.near_any_tie(VC.random_payload(h, w, chroma, 3), h, w, chroma).sum()) for h, w in CC.FRAMES)
        for crop in CC.CROPS:                                     # the rows of a launch: formats, sizes and origins are mixed
            _, offsets = CC.build_arena(frames, "plus6", 0)
            rows, which = CC.launch_rows(frames, offsets, crop)
            assert set(rows[:, 5]) == {0, 1, 2, 3} and len(set(which)) >= 6 and len({o % 4 for o in rows[:, 0]}) > 1
    assert redrawn > 0, "plain random payloads do hold near ties: the redraw is not idle"


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_header_binding_and_dynamic_symbols_agree():
    from bin_amd import _lib, build
    names = [row.name for row in build.ADDON_LIBRARIES]
    assert names[names.index("binlap") + 1] == NAME and list(_lib._ADDON_LIBRARIES) == names
    lib = build.ADDON_BY_NAME[NAME]
    assert build.row(NAME) is lib and lib.sources == ["bincrop.hip"] and lib.subdir == "extra" and lib.purpose and "\n" not in lib.purpose
    hdr = open(lib.header).read()
    declared = build.abi_symbols(NAME)
    assert declared == WANT and set(_lib.exported_symbols(NAME)) == set(declared) == _defined(lib.path)
    assert set(re.findall(rf"\b({NAME}_[a-z0-9_]+)\s*\(", hdr)) == set(declared)
    assert '#include "binyuv.h"' in hdr and all(m.startswith("BINCROP_") for m in re.findall(r"#\s*define\s+(\w+)", hdr))
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", hdr).group(1))
    assert _lib.croplib().bincrop_version() == macro("BINCROP_VERSION") == _lib.CROP_VERSION == 100 and _lib.croplib() is _lib.library(NAME)
    assert (macro("BINCROP_E_ARG"), macro("BINCROP_E_SHAPE")) == (_lib.CROP_E_ARG, _lib.CROP_E_SHAPE) == (-1, -2)
    assert macro("BINCROP_FORMATS") == _lib.CROP_FORMATS == 4 and C.sizeof(_lib.BinCropRow) == 32
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct BinCropRow \{(.*?)\}", hdr, re.S).group(1))
    assert [f for f, _ in _lib.BinCropRow._fields_] == re.findall(r"(\w+)\s*[,;]", body) and _lib.BinCropRow.format.offset == 24
    src = open(os.path.join(build.CSRC, "extra", "bincrop.hip")).read()
    assert '#include "../binyuv_common.h"' in src
    for shared in ("coefficients(", "yuv_pixel(", "split(", "grid_for(", "launch(", "ToCoef", "load_yuv4_vec<", "load_yuv4_bytes<"):
        assert shared in src, f"{shared} is binyuv_common.h's"
    assert not re.search(r"(?m)^\s*#\s*(if|ifdef|ifndef|elif|define)\b", src), "no preprocessor switches in the source"
    assert "__shared__" not in src and "asm" not in re.sub(r"//.*", "", src)
    from bin_amd import ops
    assert [ops.yuv_format_index((420, m, r)) for m, r in CC.FORMATS] == [0, 1, 2, 3]
    built = ["bin_amd/csrc/extra/libbincrop.so", "bin_amd/csrc/extra/binhip_exports.bincrop.map", "bin_amd/csrc/extra/bincrop.o"]
    ignored = subprocess.run(["git", "check-ignore"] + built, cwd=REPO, capture_output=True, text=True)
    if ignored.returncode != 128:                                 # (128: not a git checkout)
        assert len(ignored.stdout.split()) == len(built), "the built files stay out of git"


# ------------------------------------------------------------------------------------------------ refusals before any launch
def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the addresses are never dereferenced: every call
    here is one the library refuses, none reaches a launch)."""
    from bin_amd import _lib
    lib = _lib.croplib()
    A, T, OUT, AB = 0x100000, 0x200000, 0x300000, 4096

    def call(arena=A, nbytes=AB, rows=T, n=3, ch=4, cw=8, chroma=420, out=OUT):
        return lib.bincrop_yuv_crops_to_bgr(arena, nbytes, rows, n, ch, cw, chroma, out, None)
    assert call(arena=None) == -1 and call(rows=None) == -1 and call(out=None) == -1, "a null pointer"
    for bad in (0, -1, -2 ** 31):
        assert call(n=bad) == -1 and call(ch=bad) == -1 and call(cw=bad) == -1, bad
    for chroma in (0, 422, 411, -420, 2 ** 31 - 1):
        assert call(chroma=chroma) == -1, chroma
    for nbytes in (0, -1, -2 ** 63):
        assert call(nbytes=nbytes) == -1, nbytes
    assert call(rows=T + 4) == -1, "the table is 8-byte aligned"
    # sizes beyond 2^40: the arena, the output
    far = 0x7000000000000000
    assert call(nbytes=2 ** 40 + 1, out=far) == -2 and call(nbytes=2 ** 63 - 1, out=far) == -2
    assert call(n=1, ch=2 ** 20, cw=2 ** 20) == -2 and call(n=2 ** 11, ch=2 ** 14, cw=2 ** 14) == -2
    assert call(n=2 ** 31 - 1, ch=2 ** 31 - 1, cw=2 ** 31 - 1) == -2
    assert call(nbytes=2 ** 40 + 1, chroma=7) == -1 and call(n=1, ch=2 ** 20, cw=2 ** 20, out=None) == -1, "argument errors come first"
    # the output (3 * 4 * 8 * 3 = 288 bytes) on the arena, by one byte at either end; and on the table (96 bytes)
    for out in (A, A + AB - 1, A - 287, A + 100, T, T + 95, T - 287):
        assert call(out=out) == -1, hex(out)
    assert call(arena=A + 10, nbytes=20, out=A) == -1, "an arena inside the output"


def _rows(*rows):
    return np.array(rows, dtype=np.int64)


def test_ops_yuv_crops_to_bgr_refuses_malformed_rows_before_touching_a_device(monkeypatch):
    from bin_amd import _lib, ops
    monkeypatch.setattr(_lib, "croplib", lambda: pytest.fail("no library call"))
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda *a, **k: pytest.fail("nothing is uploaded"))
    fb = 90                                                       # a 10x6 4:2:0 frame
    arena = torch.zeros(2 * 96, dtype=torch.uint8)
    good = (96, 6, 10, 2, 2, 3)
    for bad, what in (((-1, 6, 10, 2, 2, 3), "payload leaves the arena"), ((103, 6, 10, 2, 2, 3), "payload leaves the arena"),
                      ((2 ** 40, 6, 10, 2, 2, 3), "payload leaves the arena"), ((96, 6, 20, 2, 2, 3), "payload leaves the arena"),
                      ((96, 0, 10, 0, 0, 0), "frame size"), ((96, 6, -10, 0, 0, 0), "frame size"), ((96, 2 ** 31, 10, 0, 0, 0), "frame size"),
                      ((96, 6, 10, 3, 2, 3), "crop leaves the frame"), ((96, 6, 10, 2, 3, 3), "crop leaves the frame"),
                      ((96, 6, 10, -1, 2, 3), "crop leaves the frame"), ((96, 6, 10, 2, -1, 3), "crop leaves the frame"),
                      ((96, 3, 10, 0, 0, 0), "crop leaves the frame"), ((96, 6, 7, 0, 0, 0), "crop leaves the frame"),
                      ((96, 6, 10, 2, 2, 4), "format index"), ((96, 6, 10, 2, 2, -1), "format index")):
        with pytest.raises(ValueError, match=what) as e:
            ops.yuv_crops_to_bgr(arena, _rows(good, bad, good), (4, 8), 420)
        assert "row 1" in str(e.value), "the row is named"
    assert 102 + fb == arena.numel(), "offset 102 is the last that fits, 103 the first that does not"
    with pytest.raises(ValueError, match="payload leaves the arena"):
        ops.yuv_crops_to_bgr(arena, _rows((13, 6, 10, 0, 0, 0)), (4, 8), 444)      # 180 bytes at 4:4:4
    for bad in (np.zeros((0, 6), np.int64), np.zeros((2, 5), np.int64), np.zeros(6, np.int64), np.zeros((2, 6), np.float32)):
        with pytest.raises(ValueError, match="rows must be"):
            ops.yuv_crops_to_bgr(arena, bad, (4, 8), 420)
    for bad in (arena.view(2, 96), arena.int(), arena[::2], arena[:0]):
        with pytest.raises(ValueError, match="arena must be"):
            ops.yuv_crops_to_bgr(bad, _rows(good), (4, 8), 420)
    with pytest.raises(ValueError, match="chroma"):
        ops.yuv_crops_to_bgr(arena, _rows(good), (4, 8), 422)
    for crop in ((0, 8), (4, 0), (-4, 8)):
        with pytest.raises(ValueError, match="a crop of"):
            ops.yuv_crops_to_bgr(arena, _rows(good), crop, 420)
    for out in (torch.zeros((1, 4, 8, 3)), torch.zeros((2, 4, 8, 3), dtype=torch.uint8), torch.zeros((1, 8, 4, 3), dtype=torch.uint8),
                torch.zeros((1, 4, 8, 4), dtype=torch.uint8)[..., :3]):
        with pytest.raises(ValueError, match="fills a contiguous uint8"):
            ops.yuv_crops_to_bgr(arena, _rows(good), (4, 8), 420, out=out)
    with pytest.raises(RuntimeError, match="HIP device"):         # a well-formed call gets as far as the device check
        ops.yuv_crops_to_bgr(arena, _rows(good), (4, 8), 420)


# ------------------------------------------------------------------------------------------------ options
def test_options_refuse_an_unknown_format_and_yuv_on_another_mode(tmp_path):
    import yaml
    from bin_amd.options import options
    assert options.device_cache_format({}) == "bgr" and options.device_cache_format({"device_cache_format": None}) == "bgr"
    assert options.device_cache_format({"device_cache_format": "bgr", "mode": "BIN"}) == "bgr"
    assert options.device_cache_format({"device_cache_format": "yuv", "mode": "BIN_video"}) == "yuv"
    for bad in ("rgb", "YUV", 420, True, ""):
        with pytest.raises(ValueError, match=r"datasets\.train\.device_cache_format.*not one of bgr, yuv"):
            options.device_cache_format({"device_cache_format": bad, "mode": "BIN_video", "phase": "train"})
    for mode in ("BIN", "synthetic_texture"):
        with pytest.raises(ValueError, match=r"datasets\.val\.device_cache_format: yuv .* mode BIN_video"):
            options.device_cache_format({"device_cache_format": "yuv", "mode": mode}, "val")
    # through parse: the shipped file, with the key set in one phase
    shipped = os.path.join(REPO, "bin_amd", "options", "bin_stage4_y4m.yml")
    text = open(shipped).read()
    assert re.search(r"(?m)^\s*# device_cache_format: yuv\b.*\n\s*#.*\n\s*#", text), "a commented line and two lines of explanation"
    opt = yaml.safe_load(text)
    for phase, value, mode, want in (("train", "yuv", None, None), ("val", "yuv", None, None), ("train", "yuv", "BIN", "mode BIN_video"),
                                     ("val", "rgb", None, r"datasets\.val\.device_cache_format")):
        changed = yaml.safe_load(text)
        changed["datasets"][phase]["device_cache_format"] = value
        if mode:
            changed["datasets"][phase]["mode"] = mode
        path = tmp_path / f"{phase}_{value}_{mode}.yml"
        path.write_text(yaml.safe_dump(changed))
        env = os.environ.get("CUDA_VISIBLE_DEVICES")
        try:
            if want is None:
                assert options.parse(str(path))["datasets"][phase]["device_cache_format"] == value
            else:
                with pytest.raises(ValueError, match=want):
                    options.parse(str(path))
        finally:
            if env is None:
                os.environ.pop("CUDA_VISIBLE_DEVICES", None)
            else:
                os.environ["CUDA_VISIBLE_DEVICES"] = env
    assert "device_cache_format" not in opt["datasets"]["train"], "the shipped file keeps the default"


# ------------------------------------------------------------------------------------------------ the dataset and the cache
def _opt(root, **kw):
    opt = {"mode": "BIN_video", "name": "train", "dataroot_video": root, "LQ_size": [3, 4, 8], "phase": "train", "blur_window": 11}
    opt.update(kw)
    return opt


def test_dataset_takes_clips_of_different_sizes_with_yuv_only(tmp_path, monkeypatch):
    from bin_amd import ops
    from bin_amd.data import create_dataset
    from bin_amd.data.video_dataset import VideoFrameCache, YuvFrameCache
    monkeypatch.setattr(ops, "yuv_to_bgr", lambda *a, **k: pytest.fail("no device call"))
    monkeypatch.setattr(ops, "yuv_crops_to_bgr", lambda *a, **k: pytest.fail("no device call"))
    monkeypatch.setattr(torch, "empty", lambda *a, **k: pytest.fail("nothing is allocated"))
    a, b, small, c444 = (str(tmp_path / n) for n in ("a.y4m", "b.y4m", "small.y4m", "c444.y4m"))
    CL.write_clip(a, 80, 6, 10, 420, seed=1)
    CL.write_clip(b, 80, 8, 12, 420, seed=2)
    CL.write_clip(small, 80, 3, 8, 420, seed=3)
    CL.write_clip(c444, 80, 6, 10, 444, seed=4)
    for fmt in (None, "bgr"):
        with pytest.raises(ValueError, match="the clips differ: ") as e:
            create_dataset(_opt([a, b], device_cache_format=fmt))
        assert str(e.value) == f"mode BIN_video: the clips differ: {a} is 10x6 420, {b} is 12x8 420", "word for word"
    ds = create_dataset(_opt([a, b], device_cache_format="yuv"))
    assert ds.cache_format == "yuv" and len(ds) == 6 and [(h.height, h.width) for h, _, _ in ds.clips.values()] == [(6, 10), (8, 12)]
    assert create_dataset(_opt([a], device_cache_format=None)).cache_format == "bgr"
    with pytest.raises(ValueError, match="chroma") as e:
        create_dataset(_opt([a, c444], device_cache_format="yuv"))
    assert a in str(e.value) and c444 in str(e.value)
    for fmt in ("yuv", None):                                      # a clip smaller than the crop is named, whichever it is
        with pytest.raises(ValueError, match="crop") as e:
            create_dataset(_opt([a, small] if fmt else [small], device_cache_format=fmt))
        assert small in str(e.value) and "8x3 frames" in str(e.value)
    with pytest.raises(ValueError, match="device_cache_format"):
        create_dataset(_opt([a], device_cache_format="nv12"))
    # the cache's size check comes before any allocation, with a message in the existing style; `make_device_cache` picks the class
    with pytest.raises(ValueError, match=r"need 0\.00 GB \(\d+ bytes\), more than device_cache_max_gb = 1e-06") as e:
        YuvFrameCache(ds, "cuda", max_gb=1e-6)
    frames = 2 * 67                                               # per clip the files 12 .. 78: first centre 17 - 5 to last centre 73 + 5
    assert f"{frames} YUV 420 frames" in str(e.value) and f"({67 * 96 + 67 * 144} bytes)" in str(e.value), "90 -> 96 and 144 -> 144 a frame"
    with pytest.raises(ValueError, match="YUV 420 frames"):
        ds.make_device_cache("cuda", 1e-6)
    with pytest.raises(ValueError, match=r"frames of 6x10x3 need"):
        create_dataset(_opt([a])).make_device_cache("cuda", 1e-6)
    assert issubclass(YuvFrameCache, object) and not issubclass(YuvFrameCache, VideoFrameCache)


# ------------------------------------------------------------------------------------------------ the stand-alone program
def test_refusals_program_ends_clean_under_host_sanitizers(tmp_path):
    """tools/bincrop_refusals.cpp with the library's source, host code under ASan and UBSan, run on its own: every refusal path, no
    device, nothing loaded into Python."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "bincrop_refusals")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(REPO, "bin_amd", "csrc", "extra", "bincrop.hip"),
                            os.path.join(REPO, "tools", "bincrop_refusals.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "bincrop refusals ok" in run.stdout and "runtime error" not in run.stderr, (run.stdout, run.stderr[-2000:])
