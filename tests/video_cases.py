"""The case table of the video kernels (libbinyuv.so, include/binyuv.h) and the numpy restatement of their semantics, kept outside
the package: the tests hold the kernels to THIS, in float64.  `dtype=np.float32` restates the same formulas in fp32 (every
operation rounded to fp32, no fused multiply-add), which the CPU tests use to show that the bars are not vacuous."""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}
MATRIX_RANGE = [(m, r) for m in ("bt601", "bt709") for r in ("limited", "full")]
CHROMAS = (420, 444)
SHAPES = [(1, 1), (2, 2), (3, 5), (5, 3), (4, 4), (2, 8), (6, 10), (7, 16), (16, 64), (33, 130)]        # (h, w)
CASES = [(h, w, c) for (h, w) in SHAPES for c in CHROMAS]
CASE_IDS = [f"{h}x{w}_{c}" for h, w, c in CASES]
TO_FRAME_BAR = 2.0 ** -20           # at most eight fp32 roundings of magnitudes below 2: 8 * 2 * 2^-24
TIE_MARGIN = 2.0 ** -10             # safe_rgb_frame keeps every pre-rounding value this far from a rounding tie
GUARD = 0xA5
SAFE_POINT = (120, 110, 140)        # a code point in gamut under all four (matrix, range) pairs


def video_slots(index, n_windows):
    """The Ft_p slots window `index` of a clip contributes to the output video, in display order: the folder runner's ownership
    rule (bin_amd/test.py) — the first window opens with its first deblurred frame, the last one has no second."""
    return ((8,) if index == 0 else ()) + (13,) + ((12,) if index < n_windows - 1 else ())


def pad_sizes(h, w):
    from bin_amd.utils import util
    return util.pad_sizes(h, w)


def pads_of(h, w):
    """(left, right, top, bottom) sets of the table."""
    return [(0, 0, 0, 0), (1, 2, 3, 0), (4, 4, 2, 2), tuple(pad_sizes(h, w))]


def crops_of(h, w):
    """(pads around the crop) of the frame -> YUV cases: the crop at (0, 0), at the pad_sizes offset and at (top, left) = (1, 3)."""
    return [(0, 0, 0, 0), tuple(pad_sizes(h, w)), (3, 1, 1, 2)]


def chroma_size(h, w, chroma):
    return (h, w) if chroma == 444 else ((h + 1) // 2, (w + 1) // 2)


def frame_bytes(h, w, chroma):
    ch, cw = chroma_size(h, w, chroma)
    return h * w + 2 * ch * cw


def split_planes(payload, h, w, chroma):
    ch, cw = chroma_size(h, w, chroma)
    payload = np.asarray(payload).reshape(-1)
    assert payload.size == frame_bytes(h, w, chroma)
    return (payload[:h * w].reshape(h, w), payload[h * w:h * w + ch * cw].reshape(ch, cw), payload[h * w + ch * cw:].reshape(ch, cw))


def random_payload(h, w, chroma, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, frame_bytes(h, w, chroma), dtype=np.uint8)


def ramp_payload(h, w, chroma, step=1, start=0):
    """Every code value in turn, through all three planes (each plane of 256 bytes or more holds all of them)."""
    return ((np.arange(frame_bytes(h, w, chroma), dtype=np.int64) * step + start) % 256).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ YUV -> RGB
def _scales(rng, dtype):
    return (dtype(219), dtype(16), dtype(224)) if rng == "limited" else (dtype(255), dtype(0), dtype(255))


def yuv_to_rgb(Y, U, V, matrix, rng, dtype=np.float64, clamp=True):
    """Per sample (chroma already at the luma's resolution): the formulas of include/binyuv.h in `dtype`.  Returns [3, ...]."""
    kr, kb = (dtype(k) for k in KR_KB[matrix])
    one, two = dtype(1), dtype(2)
    kg = one - kr - kb
    ys, yo, cs = _scales(rng, dtype)
    y = (np.asarray(Y).astype(dtype) - yo) / ys
    pb = (np.asarray(U).astype(dtype) - dtype(128)) / cs
    pr = (np.asarray(V).astype(dtype) - dtype(128)) / cs
    R = y + two * (one - kr) * pr
    B = y + two * (one - kb) * pb
    G = (y - kr * R - kb * B) / kg
    out = np.stack([R, G, B])
    assert out.dtype == dtype
    return np.clip(out, dtype(0), dtype(1)) if clamp else out


def to_frame_ref(payload, h, w, fmt, pads, dtype=np.float64):
    """[3, Hp, Wp]: 4:2:0 chroma replicated (pixel (r, c) takes sample (r>>1, c>>1)), converted, clamped, replicate-padded."""
    chroma, matrix, rng = fmt
    Y, U, V = split_planes(payload, h, w, chroma)
    if chroma == 420:
        U = np.repeat(np.repeat(U, 2, 0), 2, 1)[:h, :w]
        V = np.repeat(np.repeat(V, 2, 0), 2, 1)[:h, :w]
    rgb = yuv_to_rgb(Y, U, V, matrix, rng, dtype)
    l, r, t, b = pads
    return np.pad(rgb, ((0, 0), (t, b), (l, r)), mode="edge")


# ------------------------------------------------------------------------------------------------ RGB -> YUV
def clamp01(x):
    """fminf(fmaxf(v, 0), 1): NaN -> 0, -inf -> 0, +inf -> 1."""
    with np.errstate(invalid="ignore"):
        return np.fmin(np.fmax(x, x.dtype.type(0)), x.dtype.type(1))


def box_mean(p, dtype):
    """[h, w] -> [ceil(h/2), ceil(w/2)]: the mean over the pixels of each 2x2 block that exist, summed (p00 + p01) + (p10 + p11)."""
    h, w = p.shape
    ch, cw = (h + 1) // 2, (w + 1) // 2
    q = np.zeros((2 * ch, 2 * cw), dtype)
    q[:h, :w] = p
    s = (q[0::2, 0::2] + q[0::2, 1::2]) + (q[1::2, 0::2] + q[1::2, 1::2])
    rows = np.where(2 * np.arange(ch) + 1 < h, 2, 1)[:, None]
    cols = np.where(2 * np.arange(cw) + 1 < w, 2, 1)[None, :]
    return (s / (rows * cols).astype(dtype)).astype(dtype)


def prerounding(frame, top, left, h, w, fmt, dtype=np.float64):
    """(Y, U, V) planes of the crop BEFORE rounding, in `dtype`."""
    chroma, matrix, rng = fmt
    kr, kb = (dtype(k) for k in KR_KB[matrix])
    one, two = dtype(1), dtype(2)
    kg = one - kr - kb
    ys, yo, cs = _scales(rng, dtype)
    x = clamp01(np.asarray(frame)[:, top:top + h, left:left + w].astype(np.float32)).astype(dtype)
    R, G, B = x[0], x[1], x[2]
    y = kr * R + kg * G + kb * B
    pb = (B - y) / (two * (one - kb))
    pr = (R - y) / (two * (one - kr))
    if chroma == 420:
        pb, pr = box_mean(pb, dtype), box_mean(pr, dtype)
    return yo + ys * y, dtype(128) + cs * pb, dtype(128) + cs * pr


def from_frame_ref(frame, top, left, h, w, fmt, dtype=np.float64):
    """The Y4M payload (uint8 [frame_bytes]) of the crop: rounded half to even, clamped to 0..255, Y then U then V."""
    planes = prerounding(frame, top, left, h, w, fmt, dtype)
    return np.concatenate([np.clip(np.rint(p), 0, 255).astype(np.uint8).reshape(-1) for p in planes])


# ------------------------------------------------------------------------------------------------ inputs
def in_gamut_codes(matrix, rng):
    """[n, 3] uint8: every (Y, U, V) whose unclamped RGB lies in [0, 1] (float64), in code order."""
    c = np.arange(256)
    out = []
    for Y in range(256):                                            # a [256, 256] slab per Y: small temporaries
        U, V = np.meshgrid(c, c, indexing="ij")
        rgb = yuv_to_rgb(np.full_like(U, Y), U, V, matrix, rng, clamp=False)
        ok = ((rgb >= 0) & (rgb <= 1)).all(0)
        u, v = np.nonzero(ok)
        out.append(np.stack([np.full(u.size, Y), u, v], 1).astype(np.uint8))
    return np.concatenate(out)


def safe_rgb_frame(shape, fmt, seed, crop=None):
    """fp32 [3, Hp, Wp] with values below 0 and above 1, NaN and +-inf, in which no pre-rounding Y, U or V of the crop `(top, left, h,
    w)` (default: the whole frame) lies within TIE_MARGIN of a half-integer: every pixel (4:4:4) or whole 2x2 block (4:2:0) of the
    crop where one did is replaced by the frame-image of SAFE_POINT, whose values sit on integers.  Returns (frame, replaced share
    of the crop's pixels).  After this nothing needs to be left out of any comparison."""
    hp, wp = shape
    top, left, h, w = crop if crop is not None else (0, 0, hp, wp)
    chroma, matrix, rng_name = fmt
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-0.25, 1.25, (3, hp, wp)).astype(np.float32)
    n_special = min(6, x.size // 8)
    at = rng.choice(x.size, n_special, replace=False)
    x.reshape(-1)[at] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), n_special)
    Y, U, V = prerounding(x, top, left, h, w, fmt)
    near = lambda p: np.abs(p - np.floor(p) - 0.5) < TIE_MARGIN
    bad = near(Y)
    if chroma == 420:
        c_bad = near(U) | near(V)
        ch, cw = c_bad.shape
        y_bad = np.zeros((2 * ch, 2 * cw), bool)
        y_bad[:h, :w] = bad
        c_bad |= y_bad[0::2, 0::2] | y_bad[0::2, 1::2] | y_bad[1::2, 0::2] | y_bad[1::2, 1::2]
        bad = np.repeat(np.repeat(c_bad, 2, 0), 2, 1)[:h, :w]
    else:
        bad = bad | near(U) | near(V)
    safe = yuv_to_rgb(*SAFE_POINT, matrix, rng_name).astype(np.float32)
    x[:, top:top + h, left:left + w][:, bad] = safe[:, None]
    for p in prerounding(x, top, left, h, w, fmt):
        assert not near(p).any()
    return x, float(bad.mean())
