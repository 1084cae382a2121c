"""Case table of the per-plane payload scores (include/binscore.h, ops.payload_scores) and their reference: the six integer sums in
numpy int64 and the two SSIMs as util.calculate_ssim / util.compare_ssim give them on the 2-D Y planes.  Host side only; a reference
is computed once per case and shared."""
import functools

import numpy as np

CHROMAS = (420, 444)
NONE, U7, BOTH = "none", "u7", "both"                   # which SSIMs a case is scored with

# (flags, (h, w)): every size at which the kernel takes another path
_SHAPES = (
    (NONE, (1, 1)), (NONE, (2, 2)), (NONE, (3, 5)), (NONE, (5, 3)),
    (NONE, (7, 16)), (U7, (7, 16)),
    (U7, (7, 7)), (U7, (9, 10)),
    (BOTH, (11, 11)), (BOTH, (12, 13)),                 # the smallest valid maps
    (BOTH, (16, 246)), (BOTH, (17, 247)),               # one past the walk's 16-row x 246-column tile in each direction
    (BOTH, (33, 493)),                                  # 4:2:0 chroma is 17 x 247 and crosses the tile too
)
CONTENTS = ("random", "same", "constant", "extremes")
CASES = tuple((flags, h, w, chroma, content) for flags, (h, w) in _SHAPES for chroma in CHROMAS for content in CONTENTS)
TILE_ROWS, TILE_COLS = 16, 246


def frame_bytes(h, w, chroma):
    ch, cw = (h, w) if chroma == 444 else ((h + 1) // 2, (w + 1) // 2)
    return h * w + 2 * ch * cw, ch, cw


def case_id(case):
    flags, h, w, chroma, content = case
    return f"{h}x{w}-{chroma}-{flags}-{content}"


@functools.lru_cache(maxsize=None)
def payloads(h, w, chroma, content):
    """(a, b): two uint8 payloads of an h x w frame (read-only arrays)."""
    n, _, _ = frame_bytes(h, w, chroma)
    rng = np.random.default_rng(1000 * h + 10 * w + chroma)
    if content == "random":
        a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
    elif content == "same":
        a = rng.integers(0, 256, n, dtype=np.uint8)
        b = a.copy()
    elif content == "constant":                         # constant planes: SSIM is exactly 1 where the constants agree
        a, b = np.full(n, 93, np.uint8), np.full(n, 93, np.uint8)
        a[h * w:], b[h * w:] = 17, 201
    elif content == "extremes":                         # the largest sums
        a, b = np.zeros(n, np.uint8), np.full(n, 255, np.uint8)
    else:
        raise ValueError(content)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def planes(payload, h, w, chroma):
    n, ch, cw = frame_bytes(h, w, chroma)
    assert payload.shape == (n,)
    return payload[:h * w].reshape(h, w), payload[h * w:h * w + ch * cw].reshape(ch, cw), payload[h * w + ch * cw:].reshape(ch, cw)


def reference_scores(a, b, h, w, chroma, flags):
    """(sse_y, sse_u, sse_v, sad_y, sad_u, sad_v, ssim_g11, ssim_u7): ints from int64 sums, SSIMs of the Y planes (NaN without flag)."""
    from bin_amd.utils import util
    pa, pb = planes(a, h, w, chroma), planes(b, h, w, chroma)
    d = [x.astype(np.int64) - y.astype(np.int64) for x, y in zip(pa, pb)]
    sse = tuple(int((v * v).sum()) for v in d)
    sad = tuple(int(np.abs(v).sum()) for v in d)
    g11 = float(util.calculate_ssim(pa[0], pb[0])) if flags == BOTH else float("nan")
    u7 = float(util.compare_ssim(pa[0], pb[0])) if flags in (U7, BOTH) else float("nan")
    return sse + sad + (g11, u7)


@functools.lru_cache(maxsize=None)
def reference(case):
    flags, h, w, chroma, content = case
    a, b = payloads(h, w, chroma, content)
    return reference_scores(a, b, h, w, chroma, flags)
