"""Shared by test_cpu_scene.py and test_gpu_scene.py: the numpy restatement of the luma statistics (include/binscene.h), the shape and
content table of the kernel test, and the two clips with scene cuts.  Pure numpy / Python: importable without a device."""
import numpy as np

BINS, RECORD_BYTES = 64, 264
GUARD = 0xA5

# sizes around the 16-byte vector (1, 15, 16, 17 bytes), ragged rows, whole vectors, several blocks
SHAPES = [(1, 1), (1, 15), (1, 16), (1, 17), (3, 5), (7, 16), (16, 64), (33, 130)]
# beyond the kernel's grid cap (512 blocks of 256 lanes, 16 bytes a lane = 2097152 bytes): the blocks stride
BIG_SHAPE = (1200, 1920)
OFFSETS = (0, 1, 3, 16)                      # byte offsets of a plane within a 256-byte aligned buffer

# the 40x24 4:2:0 stream of test_gpu_video.py
CLIP_HEADER = b"YUV4MPEG2 W40 H24 F30:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL\n"
H, W = 24, 40
THRESHOLD = 0.4
INSIDE_BAR, ACROSS_BAR = 0.19, 0.65          # every distance inside a scene is <= 0.19, across a boundary >= 0.65


def luma_stats_ref(cur, prev=None):
    """(sad, hist[64]) of a uint8 plane and the plane before it (or None), in integers."""
    cur = np.asarray(cur, np.uint8).reshape(-1)
    hist = np.bincount(cur >> 2, minlength=BINS).astype(np.int64)
    sad = 0 if prev is None else int(np.abs(cur.astype(np.int64) - np.asarray(prev, np.uint8).reshape(-1).astype(np.int64)).sum())
    return sad, hist


def plane(kind, h, w, seed=0):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    raise ValueError(kind)


def record_ref(cur, prev=None):
    """The 264 bytes of the record, as the C struct lays them out (little endian)."""
    sad, hist = luma_stats_ref(cur, prev)
    return np.concatenate([np.array([sad], "<u8").view(np.uint8), hist.astype("<u4").view(np.uint8)])


# ------------------------------------------------------------------------------------------------ the clips
def _payload(Y, k):
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    U = 128 + 30 * np.sin(0.4 * (cx - k))
    V = 128 + 30 * np.cos(0.35 * (cy + k))
    return np.concatenate([np.rint(p).astype(np.uint8).reshape(-1) for p in (Y, U, V)])


def frame_a(k):
    yy, xx = np.mgrid[0:H, 0:W]
    return _payload(110 + 70 * np.sin(0.31 * (xx + 2 * k)) * np.cos(0.23 * yy) + 8 * ((xx // 5 + yy // 4 + k) % 2), k)


def frame_b(k):
    yy, xx = np.mgrid[0:H, 0:W]
    return _payload(60 + 35 * np.cos(0.17 * (yy + 3 * k)) * np.sin(0.11 * xx + 0.5) + 6 * ((xx // 3 + k) % 2), k)


def nine_frame_clip():
    """A A A | B B B | a | B' B': [9, 1440] uint8, cuts at 3, 6 and 7."""
    frames = [frame_a(0), frame_a(1), frame_a(2), frame_b(0), frame_b(1), frame_b(2), frame_a(7), frame_b(5), frame_b(6)]
    return np.stack(frames), [3, 6, 7]


def five_frame_clip():
    """a | B B B | a': [5, 1440] uint8, cuts at 1 and 4: a lone first and a lone last frame."""
    frames = [frame_a(3), frame_b(0), frame_b(1), frame_b(2), frame_a(9)]
    return np.stack(frames), [1, 4]


def clip_distances(payloads):
    """The float64 reference of the decision: [distance(i-1, i)] for i = 1 .. T-1 and the records, from numpy alone."""
    recs = [luma_stats_ref(p[:H * W], payloads[i - 1][:H * W] if i else None) for i, p in enumerate(payloads)]
    dist = [float(np.abs(recs[i][1] - recs[i - 1][1]).sum()) / (2.0 * H * W) for i in range(1, len(recs))]
    return dist, recs
