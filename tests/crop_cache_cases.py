"""Shared by tests/test_cpu_crop_cache.py and tests/test_gpu_crop_cache.py: the inputs of the crop-decode kernel tests (frames, crops,
offsets, strides, formats: bincrop_yuv_crops_to_bgr, include/bincrop.h), the numpy model of a decode launch on top of
clip_cases.bgr_ref, and the synthetic clips and window tables the planning function (video_dataset.plan_crop_batch) is driven with.

Sizes are written W x H in the prose and (h, w) in the code.  Every comparison made with these is exact: the kernel's per-pixel
function is the one binclip_yuv_to_bgr compiles, the planning is integer arithmetic, and the gathers run unchanged."""
import numpy as np

import clip_cases as CL
import video_cases as VC

FORMATS = VC.MATRIX_RANGE                        # format index i = 2 * matrix + range is FORMATS[i]
FRAMES = [(1, 1), (7, 5), (8, 6), (18, 33), (48, 64)]       # (h, w): 1x1, 5x7, 6x8, 33x18 and 64x48
CROPS = [(1, 1), (5, 3), (8, 4)]                 # (ch, cw): 1x1, 3x5, 4x8; the whole frame comes per frame size
BIG_ROWS = 700                                   # whole 64x48 frames: 700 * 48 * 16 = 537 600 items, more than 2048 blocks of 256 hold


def fmt_index(fmt):
    return FORMATS.index((fmt[1], fmt[2]))


def near_any_tie(p, h, w, chroma):
    """bool [h, w]: the pixels with a byte that clip_cases.near_tie flags under any of the four formats."""
    return np.any([CL.near_tie(p, h, w, (chroma,) + f).any(axis=2) for f in FORMATS], axis=0)


def payload(h, w, chroma, seed):
    """Random bytes with 0 and 255 planted in every plane (as far as the plane has room), kept away from rounding ties: the kernel
    evaluates 255 v in fp32 and the restatement (clip_cases.bgr_ref) in float64, so a byte whose float64 value lies within
    clip_cases.TIE_MARGIN of a half-integer may round either way (clip_cases.py; test_cpu_clip.py measures the fp32 error at a tenth
    of the margin).  An exact comparison with the restatement is a statement about every other byte, so the luma of a pixel that
    near_tie flags under any format is drawn again (and now and then the chroma under it) until none is flagged: the mask comes from the float64 restatement alone, as
    video_cases.safe_rgb_frame's does.  The comparison with ops.yuv_to_bgr needs no such care and the big launch does not take any."""
    g = np.random.Generator(np.random.PCG64(seed))
    p = g.integers(0, 256, VC.frame_bytes(h, w, chroma), dtype=np.uint8)
    for plane in VC.split_planes(p, h, w, chroma):               # views of p
        flat = plane.reshape(-1)
        flat[0] = 0
        flat[-1] = 255 if flat.size > 1 else flat[-1]
    if h * w == 1:
        p[:] = (255, 0, 255)
    luma, cu, cv = VC.split_planes(p, h, w, chroma)
    for attempt in range(64):
        flagged = near_any_tie(p, h, w, chroma)
        flagged.reshape(-1)[[0, -1]] = False                     # the planted pixels stay (they lie off every tie)
        if not flagged.any():
            break
        luma[flagged] = g.integers(1, 255, int(flagged.sum()), dtype=np.uint8)
        if attempt % 4 == 3:                                     # a chroma value can put a channel on a tie whatever the luma is
            ys, xs = np.nonzero(flagged)
            cy, cx = (ys >> 1, xs >> 1) if chroma == 420 else (ys, xs)
            free = ((cy != 0) | (cx != 0)) & ((cy != cu.shape[0] - 1) | (cx != cu.shape[1] - 1))
            cu[cy[free], cx[free]] = g.integers(1, 255, int(free.sum()), dtype=np.uint8)
            cv[cy[free], cx[free]] = g.integers(1, 255, int(free.sum()), dtype=np.uint8)
    assert not near_any_tie(p, h, w, chroma).any() and (h * w == 1 or (luma.reshape(-1)[0], luma.reshape(-1)[-1]) == (0, 255))
    return p


def frame_payloads(chroma, frames=FRAMES, per_size=2):
    """[(h, w, payload)]: `per_size` payloads of every frame size."""
    return [(h, w, payload(h, w, chroma, 1000 * i + 10 * k + (chroma == 444))) for i, (h, w) in enumerate(frames) for k in range(per_size)]


def build_arena(frames, kind, fill, lead=0):
    """The payloads of `frames` ([(h, w, payload)]) one after the other, each at stride_of(kind, its bytes), every other byte `fill`.
    Returns (uint8 [bytes], the offset of each payload)."""
    offsets, at = [], lead
    for _, _, p in frames:
        offsets.append(at)
        at += CL.stride_of(kind, p.size)
    buf = np.full(at, fill, np.uint8)
    for (_, _, p), o in zip(frames, offsets):
        buf[o:o + p.size] = p
    return buf, offsets


def offsets_for(h, w, ch, cw):
    """The crop origins of a ch x cw crop of an h x w frame that the tests use: both parities of y0 and x0 where there is room, a
    dword-aligned x0 past 0, and the origins that put the crop on the last row and the last column."""
    ys = sorted({y for y in (0, 1, h - ch - 1, h - ch) if 0 <= y <= h - ch})
    xs = sorted({x for x in (0, 1, 4, w - cw - 1, w - cw) if 0 <= x <= w - cw})
    return [(y, x) for y in ys for x in xs]


def launch_rows(frames, offsets, crop):
    """int64 [n, 6] rows (offset, H, W, y0, x0, format) of one launch: every frame that holds the crop at every origin of offsets_for,
    the format index cycling so that all four meet every frame size.  Also returns, per row, the index of its frame."""
    ch, cw = crop
    rows, which = [], []
    for i, ((h, w, _), off) in enumerate(zip(frames, offsets)):
        if ch > h or cw > w:
            continue
        for y0, x0 in offsets_for(h, w, ch, cw):
            rows.append((off, h, w, y0, x0, (len(rows) + i) % 4))
            which.append(i)
    return np.array(rows, dtype=np.int64), which


def decode_rows(arena, rows, crop, chroma, whole=None):
    """The numpy model of a launch: uint8 [n, ch, cw, 3], per row the crop of clip_cases.bgr_ref of the frame whose payload starts at
    the row's offset.  `whole`: a dict that keeps the decoded frames between calls."""
    ch, cw = crop
    whole = {} if whole is None else whole
    out = np.empty((len(rows), ch, cw, 3), np.uint8)
    for r, (off, h, w, y0, x0, f) in enumerate(np.asarray(rows).tolist()):
        key = (off, h, w, f)
        if key not in whole:
            fb = VC.frame_bytes(h, w, chroma)
            whole[key] = CL.bgr_ref(arena[off:off + fb], h, w, (chroma,) + FORMATS[f])
        out[r] = whole[key][y0:y0 + ch, x0:x0 + cw]
    return out


# ------------------------------------------------------------------------------------------------ the planning function
CLIPS = [("clipA.y4m", 120, 12, 20, (420, "bt601", "limited")),     # (file, frames, h, w, format): two sizes, two formats
         ("clipB.y4m", 100, 14, 18, (420, "bt709", "full"))]
PLAN_CROP = (6, 8)
HALF_MAX = 16


def plan_world(clips=CLIPS, half=HALF_MAX, seed=5):
    """What a YuvFrameCache of `clips` holds, without a device or files: the windows (unshuffled), the cache's index and clip_ranges
    (DeviceFrameCache._index_spans itself), the flat YUV arena with each payload at its clip's stride (frame bytes rounded up to 16)
    and the per-frame arrays, and the BGR frame of every arena id (bgr_ref)."""
    from bin_amd.data.device_cache import DeviceFrameCache
    from bin_amd.data.video_dataset import make_clip_window_list
    windows, _ = make_clip_window_list([(c[0], c[1]) for c in clips], shuffle=False, blur_window=2 * half + 1)
    cache = object.__new__(DeviceFrameCache)
    spans = cache._index_spans(windows, half)
    assert list(spans) == [c[0] for c in clips]
    n = len(cache.paths)
    off, fh, fw, ff = (np.zeros(n, np.int64) for _ in range(4))
    rng = np.random.Generator(np.random.PCG64(seed))
    chunks, bgr, at = [], [], 0
    for (name, _, h, w, fmt), (start, end) in zip(clips, cache.clip_ranges):
        fb = VC.frame_bytes(h, w, fmt[0])
        stride = CL.stride_of("round16", fb)
        for k in range(start, end):
            p = rng.integers(0, 256, fb, dtype=np.uint8)
            off[k], fh[k], fw[k], ff[k] = at, h, w, fmt_index(fmt)
            chunks.append(np.concatenate([p, np.full(stride - fb, 0xEE, np.uint8)]))
            bgr.append(CL.bgr_ref(p, h, w, fmt))
            at += stride
    return {"windows": windows, "cache": cache, "arena": np.concatenate(chunks), "offset": off, "h": fh, "w": fw, "format": ff, "bgr": bgr,
            "chroma": clips[0][4][0]}


def check_remap(world, table, crop, rows, local, ranges):
    """The remapped table addresses in the decoded mini-arena the bytes the original table addresses in the BGR frames: every slot,
    and every frame of every blurry range; the blocks are packed, disjoint and hold their samples' ranges."""
    from bin_amd.data.device_cache import N_BLUR, N_SLOTS
    ch, cw = crop
    mini = decode_rows(world["arena"], rows, crop, world["chroma"])
    assert ranges.shape == (len(table), 2) and ranges[0, 0] == 0 and ranges[-1, 1] == len(rows) and (ranges[1:, 0] == ranges[:-1, 1]).all()
    assert local.shape == table.shape and local.dtype == table.dtype
    assert (local[:, N_SLOTS:N_SLOTS + 2] == 0).all() and np.array_equal(local[:, N_SLOTS + 2:], table[:, N_SLOTS + 2:]), "flip, h, keys kept"
    checked = 0
    for r in range(len(table)):
        y0, x0, h = int(table[r, N_SLOTS]), int(table[r, N_SLOTS + 1]), int(table[r, N_SLOTS + 3])
        start, end = (int(v) for v in ranges[r])
        for s in range(N_SLOTS):
            for k in (range(-h, h + 1) if s < N_BLUR else (0,)):
                gid, lid = int(table[r, s]) + k, int(local[r, s]) + k
                assert start <= lid < end, (r, s, k)
                assert np.array_equal(mini[lid], world["bgr"][gid][y0:y0 + ch, x0:x0 + cw]), (r, s, k)
                checked += 1
    return checked
