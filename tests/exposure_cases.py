"""Shared by tests/test_cpu_exposure.py and tests/test_gpu_exposure.py: the case table of the exposure kernel (libbinexpose.so,
include/binexpose.h) and the restatement of its specification in plain Python integers — no numpy in the arithmetic, a Philox
written out.  numpy only carries the frames in and the codes out.

There is no reference implementation to compare with (the reference averages 8-bit codes and has no noise), so the header's
integer specification, restated here line by line, is the yardstick."""
import bisect
import functools
import itertools
import math

import numpy as np

ONE = 2 ** 24 - 1
Z_SIGMA = 53509.92

# ------------------------------------------------------------------------------------------------ the restatement
def dec(gamma, e):
    """Code value e in [0, 1] (float) -> linear light."""
    e = max(e, 0.0)
    if gamma == "srgb":
        return e / 12.92 if e <= 0.04045 else ((e + 0.055) / 1.055) ** 2.4
    return e ** gamma


def enc(gamma, x):
    """Linear light -> code value, the inverse of dec."""
    if gamma == "srgb":
        return 12.92 * x if x <= 0.0031308 else 1.055 * x ** (1 / 2.4) - 0.055
    return x ** (1.0 / gamma)


def tables(gamma, noise=None):
    """(LIN, MID, SIG) as lists of Python ints."""
    lin = [round(dec(gamma, v / 255) * ONE) for v in range(256)]                 # round(): half to even, as rint
    mid = [0] + [math.ceil(dec(gamma, (c - 0.5) / 255) * ONE) for c in range(1, 256)]
    if noise is None:
        sig = [0] * 256
    else:
        read, shot = noise
        sig = [round(math.sqrt(read * read + shot * (k + 0.5) / 256) * ONE * 65536 / Z_SIGMA) for k in range(256)]
    return lin, mid, sig


def curve_is_valid(lin, mid, sig):
    return (lin[0] == 0 and all(a <= b for a, b in zip(lin, lin[1:])) and lin[255] <= ONE
            and mid[0] == 0 and all(a < b for a, b in zip(mid, mid[1:]))
            and all(mid[c] <= lin[c] for c in range(256)) and all(lin[c] < mid[c + 1] for c in range(255))
            and all(0 <= s < 2 ** 23 for s in sig))


def decode(mid, m):
    """The largest c with MID[c] <= m."""
    return bisect.bisect_right(mid, m) - 1


def philox4x32_10(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def noise_int(sig, m, x, y, slot, c, key):
    """Steps 3-5: the noise integer n of linear value m at output position (x, y), channel c (RGB order) of `slot`."""
    z = sum((w & 0xFFFF) + (w >> 16) for w in philox4x32_10((x, y, 4 * slot + c, 0), key))
    return ((z - 262140) * sig[m >> 16]) >> 16               # Python's >> on a negative int is a floor


def element(codes, curve, x, y, slot, c, key):
    """Steps 1-7 for one element: `codes` are its 2h + 1 source codes."""
    lin, mid, sig = curve
    m = sum(lin[v] for v in codes) // len(codes)
    n = noise_int(sig, m, x, y, slot, c, key) if any(sig) else 0            # all-zero SIG: the generator is skipped
    return decode(mid, min(max(m + n, 0), ONE))


def gather_codes(frames, rows, crop, n_blur, curve):
    """binexpose_gather as 8-bit codes: uint8 [n_slots, n, 3, ch, cw] (RGB planes).  frames: uint8 [n_frames, H, W, 3] BGR;
    rows: [n, n_slots + 6] = ids, y0, x0, flip, h, k0, k1 (k as int32 or uint32 bits)."""
    ch, cw = crop
    f = np.asarray(frames).tolist()
    n, n_slots = len(rows), len(rows[0]) - 6
    out = np.zeros((n_slots, n, 3, ch, cw), np.uint8)
    for b, row in enumerate(rows):
        row = [int(v) for v in row]
        y0, x0, flip, h = row[n_slots:n_slots + 4]
        key = (row[n_slots + 4] & 0xFFFFFFFF, row[n_slots + 5] & 0xFFFFFFFF)
        for s, y, x, c in itertools.product(range(n_slots), range(ch), range(cw), range(3)):
            sy, sx = y0 + y, (x0 + cw - 1 - x) if flip else x0 + x
            if s < n_blur:
                codes = [f[i][sy][sx][2 - c] for i in range(row[s] - h, row[s] + h + 1)]
                out[s, b, c, y, x] = element(codes, curve, x, y, s, c, key)
            else:
                out[s, b, c, y, x] = f[row[s]][sy][sx][2 - c]
    return out


def as_float(codes):
    """Step 8: (float)code / 255.f."""
    return np.asarray(codes).astype(np.float32) / np.float32(255)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the case table
NF = 40                                                      # frames of an arena: room for h = 16 around more than one centre
N_SLOTS, N_BLUR = 3, 2                                       # two blurry slots and a sharp one
ARENAS = {"19x27": (19, 27), "24x36": (24, 36)}              # 19x27: rows of 81 bytes, frames of 1539: every byte alignment
CROPS = {"9x13": (9, 13), "8x16": (8, 16), "whole": None}
CURVES = {"g2.2": 2.2, "srgb": "srgb"}
NOISES = {"clean": None, "noisy": (0.01, 0.002)}
CONTENTS = ("random", "zeros", "full", "shadows")
HALVES = (0, 1, 2, 5, 16)
CASES = ["-".join(c) for c in itertools.product(ARENAS, CROPS, CURVES, NOISES, CONTENTS)]


def split(case):
    a, c, g, nz, content = case.split("-")
    return ARENAS[a], CROPS[c] or ARENAS[a], CURVES[g], NOISES[nz], content


@functools.lru_cache(maxsize=None)
def arena(content, hw):
    """uint8 [NF, H, W, 3], read-only."""
    g = np.random.Generator(np.random.PCG64(hw[0] * 100 + hw[1]))
    shape = (NF,) + tuple(hw) + (3,)
    a = {"random": lambda: g.integers(0, 256, shape, dtype=np.uint8), "zeros": lambda: np.zeros(shape, np.uint8),
         "full": lambda: np.full(shape, 255, np.uint8), "shadows": lambda: g.integers(0, 12, shape, dtype=np.uint8)}[content]()
    a.setflags(write=False)
    return a


def rows_of(case):
    """int64 [3, N_SLOTS + 6]: sample 0 unflipped, sample 1 flipped, sample 2 a reversed window (descending ids) whose flip
    alternates with the case; the three h walk through HALVES with the case, so every call mixes them."""
    hw, crop, _, _, _ = split(case)
    k = CASES.index(case)
    g = np.random.Generator(np.random.PCG64(1000 + k))
    rows = np.zeros((3, N_SLOTS + 6), np.int64)
    for b in range(3):
        h = HALVES[(k + 2 * b) % len(HALVES)]
        ids = sorted(int(v) for v in g.integers(h, NF - h, N_SLOTS))
        ids[0] = (h, NF - 1 - h)[k % 2]                      # the first or the last legal centre
        rows[b, :N_SLOTS] = ids[::-1] if b == 2 else ids
        y0, x0 = int(g.integers(0, hw[0] - crop[0] + 1)), int(g.integers(0, hw[1] - crop[1] + 1))
        rows[b, N_SLOTS:] = (y0, x0, (0, 1, k % 2)[b], h, int(g.integers(0, 2 ** 32)), int(g.integers(0, 2 ** 32)))
    return rows


def table_of(rows):
    """The int32 table ops.gather_windows_exposed takes: the key words keep their 32 bits."""
    return (np.asarray(rows, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


@functools.lru_cache(maxsize=None)
def reference(case):
    """(rows, the restatement's codes) of a case, computed once per process."""
    hw, crop, gamma, noise, content = split(case)
    rows = rows_of(case)
    codes = gather_codes(arena(content, hw), rows, crop, N_BLUR, tables(gamma, noise))
    codes.setflags(write=False)
    return rows, codes


# ------------------------------------------------------------------------------------------------ a toy tree
TOY_CLIPS = (("clipA", 1, 88), ("clipB", 0, 72))             # 4 + 2 windows at exposures up to 11


def make_toy_tree(root, mode="train", clips=TOY_CLIPS, hw=(352, 640), seed=5):
    """<root>/<mode>/<clip>/NNNNN.png: consecutive sharp frames, a moving gradient with dark and bright regions plus seeded
    jitter."""
    import os
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(seed))
    h, w = hw
    yy, xx = np.mgrid[0:h, 0:w]
    for ci, (clip, first, n) in enumerate(clips):
        d = os.path.join(root, mode, clip)
        os.makedirs(d)
        for k in range(first, first + n):
            base = ((xx * (ci + 1) + yy * 2 + 5 * k) % 256).astype(np.int16)
            img = np.stack([base, base[::-1], base[:, ::-1] // 8], -1) + g.integers(-6, 7, (h, w, 3))
            Image.fromarray(img.clip(0, 255).astype(np.uint8)).save(os.path.join(d, f"{k:05d}.png"), compress_level=1)
    return root
