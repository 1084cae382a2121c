"""Case table of the frame-rate resampler (bin_amd/rate.py, include/binrate.h), kept outside the package: the time grid and the
composition of the output stream restated by brute force in Fractions, the float64 restatement of the mix kernel, and the frame
pairs whose mixed pre-rounding values keep clear of every rounding tie.  Host side only."""
from fractions import Fraction
from math import ceil, floor

import numpy as np

import chain_cases as CC
import video_cases as VC

# (input rate, output rate) of the grid test, as (n, d) pairs; every one with factor 2 and factor 8
RATE_PAIRS = [((24, 1), (60, 1)), ((25, 1), (60, 1)), ((30000, 1001), (60000, 1001)), ((24000, 1001), (60000, 1001)), ((50, 1), (60, 1)),
              ((24, 1), (24, 1)), ((60, 1), (24, 1)), ((24, 1), (192, 1)), ((23, 1), (97, 1))]
GRID_FACTORS = (2, 8)
GRID_FRAMES = 40
GPU_WEIGHTS = (Fraction(1, 5), Fraction(1, 2), Fraction(4, 5), Fraction(1, 60), Fraction(59, 60))
WEIGHTS = GPU_WEIGHTS + (Fraction(1, 3), Fraction(2, 3), Fraction(1, 4), Fraction(3, 4))       # the nine of the share condition
FORMATS = [(c, m, r) for c in VC.CHROMAS for m, r in VC.MATRIX_RANGE]
# The mix adds three fp32 roundings of magnitudes up to 1 (cb - ca, w *, ca +) to a channel value before the conversion: at most
# 3 * 2^-25 each, times the largest scale 255, 2.3e-5 of a code unit, on top of the conversion's own error, which VC.TIE_MARGIN =
# 2^-10 already covers with a factor of tens to spare.  The table therefore keeps VC.TIE_MARGIN.
TIE_MARGIN = VC.TIE_MARGIN
MAX_SHARE_CASE, MAX_SHARE_TABLE, SHARE_MIN_PIXELS = 0.10, 0.05, 64


# ------------------------------------------------------------------------------------------------ the grid, by brute force
def ratio(in_rate, out_rate):
    return Fraction(out_rate[0], out_rate[1]) / Fraction(in_rate[0], in_rate[1])


def dense_factor(rho, factor):
    return min(F for F in (2, 4, 8) if F >= max(rho, factor))


def grid_ref(in_rate, out_rate, factor, T):
    """(F, M, [(a_m, w_m)]) of a T-frame stream: every x_m = m F / rho that lies on the dense positions 0 .. F(T-1)-1."""
    rho = ratio(in_rate, out_rate)
    F = dense_factor(rho, factor)
    last = F * (T - 1) - 1
    out, m = [], 0
    while Fraction(m * F) / rho <= last:
        x = Fraction(m * F) / rho
        out.append((floor(x), x - floor(x)))
        m += 1
    return F, len(out), out


# ------------------------------------------------------------------------------------------------ the output stream, by brute force
def dense_stream(T, cuts, F):
    """Per dense position: (timestamp of the frame shown there, holds resolved; index of its scene; whether it is a hold)."""
    stream = CC.expected_stream(T, cuts, F)
    scene_of = {}
    for index, (s, e) in enumerate(CC.segments(T, cuts)):
        for pos in range(F * s, min(F * e, F * (T - 1))):
            scene_of[pos] = index
    out, shown = [], None
    for pos, t in enumerate(stream):
        shown = shown if t == CC.HOLD else t
        out.append((shown, scene_of[pos], t == CC.HOLD))
    return out


def expected_outputs(T, cuts, F, rho, mode):
    """[(left timestamp, right timestamp or None, w)] per output frame of a T-frame stream with `cuts` at the ratio rho on the
    factor-F stream: the definition of bin_amd/rate.py's docstring, position by position."""
    dense = dense_stream(T, cuts, F)
    out, m = [], 0
    while Fraction(m * F) / rho <= len(dense) - 1:
        x = Fraction(m * F) / rho
        a, w = floor(x), x - floor(x)
        assert ceil(x) <= len(dense) - 1
        if w == 0:
            out.append((dense[a][0], None, 0))
        else:
            (left, ls, _), (right, rs, _) = dense[a], dense[a + 1]
            if ls != rs or left == right:
                out.append((left, None, 0))
            elif mode == "nearest":
                out.append((left if w <= Fraction(1, 2) else right, None, 0))
            else:
                out.append((left, right, float(w)))
        m += 1
    return out


def scene_of_time(T, cuts, t):
    return next(i for i, (s, e) in enumerate(CC.segments(T, cuts)) if s <= t <= e - 1)


# ------------------------------------------------------------------------------------------------ the mix kernel, in float64
def kernel_weight(w):
    """The weight as the kernel receives it: the fp32 nearest to w, as a float64."""
    return np.float64(np.float32(float(w)))


def blended(a, b, w, dtype=np.float64):
    """clamp01(a) + w (clamp01(b) - clamp01(a)) per element in `dtype` (fp32: every operation rounded on its own)."""
    ca = VC.clamp01(np.asarray(a, np.float32)).astype(dtype)
    cb = VC.clamp01(np.asarray(b, np.float32)).astype(dtype)
    return ca + dtype(kernel_weight(w)) * (cb - ca)


def prerounding(a, b, w, top, left, h, w_, fmt, dtype=np.float64):
    """(Y, U, V) planes of the crop of the mix BEFORE rounding: VC.prerounding's formulas on the mixed values, in `dtype`."""
    chroma, matrix, rng = fmt
    kr, kb = (dtype(k) for k in VC.KR_KB[matrix])
    one, two = dtype(1), dtype(2)
    kg = one - kr - kb
    ys, yo, cs = VC._scales(rng, dtype)
    x = blended(np.asarray(a)[:, top:top + h, left:left + w_], np.asarray(b)[:, top:top + h, left:left + w_], w, dtype)
    x = VC.clamp01(x)
    R, G, B = x[0], x[1], x[2]
    y = kr * R + kg * G + kb * B
    pb = (B - y) / (two * (one - kb))
    pr = (R - y) / (two * (one - kr))
    if chroma == 420:
        pb, pr = VC.box_mean(pb, dtype), VC.box_mean(pr, dtype)
    return yo + ys * y, dtype(128) + cs * pb, dtype(128) + cs * pr


def blend_ref(a, b, w, top, left, h, w_, fmt, dtype=np.float64):
    """The Y4M payload (uint8 [frame_bytes]) of the crop of the mix: rounded half to even, clamped to 0..255, Y then U then V."""
    planes = prerounding(a, b, w, top, left, h, w_, fmt, dtype)
    return np.concatenate([np.clip(np.rint(p), 0, 255).astype(np.uint8).reshape(-1) for p in planes])


def unsafe_pair(shape, seed):
    """Two fp32 [3, Hp, Wp] frames as VC.safe_rgb_frame draws them (-0.25 .. 1.25, NaN and +-inf), nothing replaced."""
    hp, wp = shape
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for _ in range(2):
        x = rng.uniform(-0.25, 1.25, (3, hp, wp)).astype(np.float32)
        n_special = min(6, x.size // 8)
        at = rng.choice(x.size, n_special, replace=False)
        x.reshape(-1)[at] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), n_special)
        out.append(x)
    return out


def safe_pair(shape, fmt, w, seed, crop=None):
    """Two fp32 [3, Hp, Wp] frames like VC.safe_rgb_frame's in which no pre-rounding Y, U or V of the MIX at weight `w` over the crop
    `(top, left, h, w)` (default: the whole frame) lies within TIE_MARGIN of a half-integer: every pixel (4:4:4) or whole 2x2 block
    (4:2:0) of the crop where one did is replaced IN BOTH frames by the frame-image of VC.SAFE_POINT, whose mix with itself sits on
    integers.  Returns (a, b, replaced share of the crop's pixels)."""
    hp, wp = shape
    top, left, h, w_ = crop if crop is not None else (0, 0, hp, wp)
    chroma, matrix, rng_name = fmt
    a, b = unsafe_pair(shape, seed)
    Y, U, V = prerounding(a, b, w, top, left, h, w_, fmt)
    near = lambda p: np.abs(p - np.floor(p) - 0.5) < TIE_MARGIN
    bad = near(Y)
    if chroma == 420:
        c_bad = near(U) | near(V)
        ch, cw = c_bad.shape
        y_bad = np.zeros((2 * ch, 2 * cw), bool)
        y_bad[:h, :w_] = bad
        c_bad |= y_bad[0::2, 0::2] | y_bad[0::2, 1::2] | y_bad[1::2, 0::2] | y_bad[1::2, 1::2]
        bad = np.repeat(np.repeat(c_bad, 2, 0), 2, 1)[:h, :w_]
    else:
        bad = bad | near(U) | near(V)
    safe = VC.yuv_to_rgb(*VC.SAFE_POINT, matrix, rng_name).astype(np.float32)
    for x in (a, b):
        x[:, top:top + h, left:left + w_][:, bad] = safe[:, None]
    for p in prerounding(a, b, w, top, left, h, w_, fmt):
        assert not near(p).any()
    return a, b, float(bad.mean())


# ------------------------------------------------------------------------------------------------ the clip (GPU)
def clip_at(rate, T=5):
    """(header, [T, frame_bytes] uint8 numpy payloads): chain_cases' 40x24 4:2:0 clip under a header of frame rate `rate`."""
    from dataclasses import replace
    from bin_amd import video
    header = replace(video.parse_header(CC.clip_header(24, 40, 420)), rate=tuple(rate))
    return header, CC.clip(24, 40, 420, T)
