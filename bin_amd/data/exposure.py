"""Blurry inputs synthesised as a camera exposure (bin_amd extension, dataset options `blur_gamma` and `blur_noise`, valid
wherever `blur_window` is): the host twin of libbinexpose.so in numpy, byte for byte.

A sensor integrates light, not gamma-encoded codes, and a real exposure carries read noise and shot noise.  With `blur_gamma` the
2h + 1 sharp frames of an exposure are decoded to linear light, averaged there and re-encoded, rounded to the nearest code; with
`blur_noise: [read, shot]` noise of variance read^2 + shot * lin (linear light, full scale = 1) is added before the encoding.  The
reference's recipe, the truncated mean of the 8-bit codes (BIN_dataset.blur_average), stays the default: with both options absent
this module is never imported.

Everything is exact integer arithmetic, specified in include/binexpose.h: a curve is three tables of 256 words (LIN, MID, SIG),
the noise is a Philox4x32-10 block per output element, keyed per sample.  Its sum of eight 16-bit halves is an Irwin-Hall
variable: kurtosis 2.85 instead of a normal variable's 3, tails cut at +-4.9 sigma."""
import functools
import math
import random
from typing import NamedTuple

import numpy as np

ONE = (1 << 24) - 1              # full scale in linear light (BINEXPOSE_ONE)
TABLE = 256                      # entries per table (BINEXPOSE_TABLE)
Z_MEAN = 262140                  # 8 * 65535 / 2: the mean of the sum of eight 16-bit halves
Z_SIGMA = 53509.92               # its standard deviation: sqrt(8 * (65536^2 - 1) / 12)
SIG_LIMIT = 1 << 23              # every SIG[k] is below it (BINEXPOSE_SIG_LIMIT)
GAMMA_MIN, GAMMA_MAX = 1.0, 2.4  # beyond 2.4 the integer result drifts from the real-number one in the shadows
READ_MAX, SHOT_MAX = 0.1, 0.01
VAL_KEY0 = 0x9E3779B9            # a validation window's key is (VAL_KEY0, window index)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


class Exposure(NamedTuple):
    """The parsed options: `gamma` a float in [1.0, 2.4] or "srgb", `noise` None or (read, shot)."""
    gamma: object
    noise: object

    @property
    def tables(self):
        return curve_tables(self.gamma, self.noise)


def parse_blur_gamma(value):
    """The `blur_gamma` option: None (absent), a number 1.0 .. 2.4 (codes e -> linear e^g), or "srgb"."""
    if value is None:
        return None
    if isinstance(value, str):
        if value.lower() != "srgb":
            raise ValueError(f"blur_gamma: {value!r} is not a number in {GAMMA_MIN} .. {GAMMA_MAX} or \"srgb\"")
        return "srgb"
    if isinstance(value, bool) or not isinstance(value, (int, float)) or not GAMMA_MIN <= value <= GAMMA_MAX:
        raise ValueError(f"blur_gamma: {value!r} is not a number in {GAMMA_MIN} .. {GAMMA_MAX} or \"srgb\"")
    return float(value)


def parse_blur_noise(value):
    """The `blur_noise` option: None (absent) or [read, shot], 0 <= read <= 0.1, 0 <= shot <= 0.01."""
    if value is None:
        return None
    ok = isinstance(value, (list, tuple)) and len(value) == 2 and all(
        not isinstance(v, bool) and isinstance(v, (int, float)) and math.isfinite(v) for v in value)
    if not ok or not 0 <= value[0] <= READ_MAX or not 0 <= value[1] <= SHOT_MAX:
        raise ValueError(f"blur_noise: {value!r} is not [read, shot] with 0 <= read <= {READ_MAX} and 0 <= shot <= {SHOT_MAX} "
                         f"(sigma^2 = read^2 + shot * lin in linear light, full scale = 1)")
    return float(value[0]), float(value[1])


def parse_options(opt, blur_window):
    """The Exposure of a dataset's options, or None when both are absent.  Either one without `blur_window`, and `blur_noise`
    without `blur_gamma`, are refused with a message that names the option."""
    gamma, noise = parse_blur_gamma(opt.get("blur_gamma")), parse_blur_noise(opt.get("blur_noise"))
    for name, value in (("blur_gamma", gamma), ("blur_noise", noise)):
        if value is not None and blur_window is None:
            raise ValueError(f"{name}: needs `blur_window`: it shapes the blurry inputs synthesised from sharp frames, and without "
                             f"`blur_window` the blurry frames are read from disk")
    if noise is not None and gamma is None:
        raise ValueError("blur_noise: needs `blur_gamma`: the noise is defined in linear light (`blur_gamma: 1.0` treats the codes as linear)")
    return None if gamma is None else Exposure(gamma, noise)


def decoder(gamma):
    """Code value in [0, 1] -> linear light in [0, 1], a function of one Python float (float64, the C library's pow: the tables do
    not depend on how an array library evaluates a power)."""
    if gamma == "srgb":
        return lambda e: max(e, 0.0) / 12.92 if e <= 0.04045 else math.pow((e + 0.055) / 1.055, 2.4)
    return lambda e: math.pow(max(e, 0.0), float(gamma))


def check_tables(tables):
    """The validity rules of include/binexpose.h (binexpose_check_curve's); raises ValueError naming the broken one."""
    t = np.asarray(tables)
    if t.shape != (3, TABLE) or t.dtype != np.uint32:
        raise ValueError(f"exposure curve: uint32 [3, {TABLE}] tables (LIN, MID, SIG), got {t.dtype} {t.shape}")
    lin, mid, sig = t.astype(np.int64)
    if lin[0] != 0 or (np.diff(lin) < 0).any() or lin[-1] > ONE:
        raise ValueError("exposure curve: LIN[0] = 0, LIN non-decreasing and LIN[255] <= 2^24 - 1 does not hold")
    if mid[0] != 0 or (np.diff(mid) <= 0).any():
        raise ValueError("exposure curve: MID[0] = 0 and MID strictly increasing does not hold")
    if (mid > lin).any() or (lin[:-1] >= mid[1:]).any():
        raise ValueError("exposure curve: MID[c] <= LIN[c] < MID[c + 1] does not hold")
    if (sig >= SIG_LIMIT).any():
        raise ValueError("exposure curve: SIG < 2^23 does not hold")
    return t


@functools.lru_cache(maxsize=None)
def curve_tables(gamma, noise=None):
    """uint32 [3, 256], read-only: LIN, MID and SIG of (parse_blur_gamma's gamma, parse_blur_noise's noise), checked."""
    dec = decoder(gamma)
    lin = [round(dec(v / 255.0) * ONE) for v in range(TABLE)]                # round(): half to even, rint
    mid = [0] + [math.ceil(dec((c - 0.5) / 255.0) * ONE) for c in range(1, TABLE)]
    read, shot = noise or (0.0, 0.0)
    sig = [round(math.sqrt(read * read + shot * (k + 0.5) / 256.0) * ONE * 65536.0 / Z_SIGMA) for k in range(TABLE)]
    t = check_tables(np.array([lin, mid, sig], dtype=np.uint32))
    t.setflags(write=False)
    return t


def decode(mid, m):
    """The largest c with MID[c] <= m, per element of `m`."""
    return np.searchsorted(np.asarray(mid, dtype=np.int64), np.asarray(m, dtype=np.int64), side="right") - 1


def philox4x32(counter, key, rounds=10):
    """Philox4x32 (Salmon et al., Random123) on arrays: `counter` four and `key` two uint32-valued arrays (or ints) that
    broadcast; returns the four output words as uint64 arrays below 2^32."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) for k in key)
    mask, m0, m1 = np.uint64(0xFFFFFFFF), np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                            # 32 x 32 -> 64 bits: no overflow
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & mask, (k1 + np.uint64(PHILOX_W1)) & mask
    return c0, c1, c2, c3


def noise_field(sig, m, key, slot, channels):
    """The noise integer n of every element of `m` (int64 [h, w, C] linear values): element (y, x, j) is output position (x, y),
    channel channels[j] in output RGB order, of slot `slot` under the sample's key (k0, k1)."""
    m = np.asarray(m, dtype=np.int64)
    h, w, _ = m.shape
    y, x = np.arange(h, dtype=np.uint64)[:, None, None], np.arange(w, dtype=np.uint64)[None, :, None]
    c = np.uint64(4 * slot) + np.asarray(channels, dtype=np.uint64)[None, None, :]
    words = philox4x32((x, y, c, 0), key)
    z = sum((wd & np.uint64(0xFFFF)) + (wd >> np.uint64(16)) for wd in words).astype(np.int64)
    s = np.asarray(sig, dtype=np.int64)[np.minimum(m >> 16, TABLE - 1)]
    return ((z - Z_MEAN) * s) >> 16                          # int64 >>: arithmetic, a floor


def default_channels(n):
    """The output RGB index of each channel of an imread_u8 frame: BGR (A), or grey."""
    return {1: (0,), 3: (2, 1, 0), 4: (2, 1, 0, 3)}[n]


def expose_average(frames_u8, tables, key=(0, 0), slot=0, channels=None):
    """The blurry frame of the L uint8 frames `frames_u8` ([L, h, w, C] or a list; C in BGR order as imread_u8 gives them) under the
    curve `tables` (curve_tables): the kernel's steps 1-7, uint8 [h, w, C].  The frames are in OUTPUT geometry already (cropped,
    flipped): element (y, x) is output position (x, y), which is what the noise field is tied to.  `key`: the sample's (k0, k1);
    `slot`: the blurry slot; `channels`: the output RGB index of each channel (default_channels)."""
    a = np.asarray(frames_u8)
    if a.dtype != np.uint8 or a.ndim != 4 or not 1 <= a.shape[0] <= 33:
        raise ValueError(f"expose_average: 1 .. 33 uint8 frames [L, h, w, C], got {a.dtype} {a.shape}")
    lin, mid, sig = (t.astype(np.int64) for t in np.asarray(tables))
    m = lin[a].sum(axis=0) // a.shape[0]
    if sig.any():
        m = m + noise_field(sig, m, key, slot, default_channels(a.shape[3]) if channels is None else channels)
    return decode(mid, np.clip(m, 0, ONE)).astype(np.uint8)


def sample_key(exposure, train, index):
    """The key (k0, k1) of one sample, for the host loader and the device loader alike.  Training: one random.getrandbits(64),
    made after the exposure's draw and only when `blur_noise` is set; any other phase: (VAL_KEY0, window index), no draw."""
    if exposure.noise is None:
        return 0, 0
    if train:
        r = random.getrandbits(64)
        return r & 0xFFFFFFFF, r >> 32
    return VAL_KEY0, int(index) & 0xFFFFFFFF
