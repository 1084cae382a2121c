"""Shared by tests/test_cpu_blur_synth.py and tests/test_gpu_blur_synth.py: the numpy restatement of how the reference's
data_scripts/adobe240fps/create_dataset_blur_N_frames_average.py makes a blurry frame, the restatement of
binhip_gather_windows_blur built on it, and a generator of sharp-only Adobe trees.

The script itself cannot be run to record a golden (it imports scipy.ndimage.imread and scipy.misc.imsave, both removed from
scipy, and drives ffmpeg), so there is no tests/golden/ fixture for the blurry frames: `script_blur` below, written line by
line as the script writes it, is the yardstick."""
import os

import numpy as np

SHARP_CLIPS = (("clipA", 1, 80),     # (name, first file number, number of consecutive sharp files): a multiple of 8,
               ("clipB", 0, 85),     # not a multiple, numbered from 0,
               ("clipC", 41, 65),    # numbered from 41, one window only,
               ("clipD", 1, 30),     # one blurry centre: too short for a window,
               ("clipE", 5, 12))     # too short for a blurry centre


def script_blur(stack):
    """The blurry frame of the uint8 frames stack[0], stack[1], ... (ascending file order), as the script computes it."""
    total = 0.0                                              # line 121: sum = 0.0
    for frame in stack:                                      # line 123: for loc in mid_list (ascending)
        total = total + frame.astype("float32")              # line 125: sum = sum + imread(...).astype("float32")
    total = total / float(len(stack))                        # line 131: sum = sum / float(len(mid_list))
    return total.astype("uint8")                             # line 132: sum = sum.astype("uint8")


def script_centres(first, n, window_size):
    """(every blurry centre, the usable ones) as file numbers, for a clip of n files numbered from `first` (script lines
    98-139: 0-based centre 16, step 8, floor(n / 8) - 2 of them, file name = index + 1 for a clip that starts at 00001)."""
    half = int((window_size - 1) / 2)                        # line 101
    total = n // 8 - 2                                       # line 104: math.floor(n_length / window_middle_delta) - 2
    centres = [first + 16 + 8 * i for i in range(max(total, 0))]
    return centres, [c for c in centres if first <= c - half and c + half <= first + n - 1]


def expected_windows(clips, window_size):
    """{key: ([6 blurry centre numbers], [5 half-way numbers])} of the windows the rule gives for `clips`."""
    out = {}
    for clip, first, n in clips:
        centres, usable = script_centres(first, n, window_size)
        for w in range(len(centres) - 5):
            cs = centres[w:w + 6]
            if all(c in usable for c in cs):
                out[f"{clip}_{cs[0]:05d}"] = (cs, [c + 4 for c in cs[:5]])
    return out


def blur_gather_reference(frames, table, crop, n_blur):
    """include/binhip.h, binhip_gather_windows_blur: a slot s < n_blur is script_blur of frames id - h .. id + h, every other
    slot frames[id]; then crop, flip, BGR -> RGB, CHW and float32 / float32(255).  table: int [n, n_slots + 4]."""
    ch, cw = crop
    table = np.asarray(table)
    n, n_slots = table.shape[0], table.shape[1] - 4
    out = np.empty((n_slots, n, 3, ch, cw), np.float32)
    for b in range(n):
        y0, x0, flip, h = (int(v) for v in table[b, n_slots:])
        xs = x0 + cw - 1 - np.arange(cw) if flip else x0 + np.arange(cw)
        for s in range(n_slots):
            i = int(table[b, s])
            src = frames[i - h:i + h + 1] if s < n_blur else frames[i:i + 1]
            win = script_blur([f[y0:y0 + ch][:, xs] for f in src])                 # ch, cw, 3 (BGR)
            out[s, b] = win[:, :, ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return out


def make_sharp_tree(root, mode="train", clips=SHARP_CLIPS, hw=(352, 640), seed=11):
    """<root>/<mode>/<clip>/NNNNN.png only: consecutive sharp frames, a gradient that moves a few pixels per frame plus
    seeded noise, so the mean of neighbouring frames is none of them."""
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(seed))
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    for ci, (clip, first, n) in enumerate(clips):
        d = os.path.join(root, mode, clip)
        os.makedirs(d)
        for k in range(first, first + n):
            base = ((xx * (ci + 1) + yy * 2 + 3 * k) % 256).astype(np.int16)
            img = np.stack([base, base[::-1], base[:, ::-1]], -1) + g.integers(-20, 21, (h, w, 3))
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(os.path.join(d, f"{k:05d}.png"), compress_level=1)
    return root


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
