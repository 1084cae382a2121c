"""Case tables and numpy / torch-indexing references for the layout and frame glue kernels (tests/test_gpu_small_kernels.py; pinned
to oracle/rdn_oracle.py by tests/test_cpu_small_kernels.py).  Everything here is bit-exact: permutations, one fp32 add, one fp32
divide, and the fp16 split

    hi = fp16(x), lo = fp16(x - float(hi)),    both round-to-nearest-even, fp16 subnormals kept    (binhip_internal.h split_hi / split_lo)

which numpy states as `x.astype(float16)`, `(x - hi.astype(float32)).astype(float16)`.  From that definition follows

    |x - (hi + lo)| <= max(2^-23 |x|, 2^-25)        (nterms = 3)        |x - hi| <= max(2^-11 |x|, 2^-25)        (nterms = 1)

(x - float(hi) is exact in fp32 and at most half an fp16 ulp of hi, i.e. <= 2^-11 |x|; rounding it to fp16 loses at most half an ulp
of a number below 2^-11 |x|, i.e. 2^-12 2^-11 |x| = 2^-23 |x| — a residual of exactly half an ulp of hi is a power of two and is kept
exactly; 2^-25 is half the fp16 subnormal step)."""
import numpy as np
import torch
import torch.nn.functional as F

F16_MAX = 65504.0
BINADES = range(-30, 16)                                   # 2^-30 .. 2^15
N_RANDOM_MANTISSAS = 300
CHANNELS = (1, 8, 9, 16, 17, 37)
NHW = ((1, 1, 1), (2, 6, 10), (3, 17, 31))
NHW_EVEN = ((1, 2, 2), (2, 6, 10), (3, 18, 30))            # where H and W must be even


def split_values(seed=1):
    """float32 vector: per binade 2^-30 .. 2^15 the mantissa edges 1, 1 + 2^-10, 1 + 2^-11 (an fp16 rounding tie), 1 + 2^-23,
    2 - 2^-23 and 300 random mantissas, in both signs; +-65504, +-0, the smallest fp16 normal and subnormal.  Magnitudes above
    65504 (the top of binade 2^15) are left out: they saturate, which tests/test_gpu_fp16_range.py covers."""
    rng = np.random.RandomState(seed)
    edges = np.array([1.0, 1 + 2.0 ** -10, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 1 + 2.0 ** -23, 2 - 2.0 ** -23], np.float64)
    vals = []
    for e in BINADES:
        m = np.concatenate([edges, 1.0 + rng.randint(0, 1 << 23, N_RANDOM_MANTISSAS).astype(np.float64) * 2.0 ** -23])
        vals.append(m * 2.0 ** e)
    v = np.concatenate(vals)
    v = v[v <= F16_MAX]
    v = np.concatenate([v, -v, [F16_MAX, -F16_MAX, 0.0, -0.0, 2.0 ** -14, -2.0 ** -14, 2.0 ** -24, -2.0 ** -24]])
    v32 = v.astype(np.float32)
    assert np.array_equal(v32.astype(np.float64), v)         # every value is a float32
    return v32


def split_ref(x):
    """(hi, lo) float16 arrays of a float32 array."""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_bound_ok(x, hi, lo, nterms):
    """The derived bound, in float64, per element."""
    x64 = np.asarray(x, np.float64)
    got = hi.astype(np.float64) + (lo.astype(np.float64) if nterms == 3 else 0.0)
    rel = 2.0 ** -23 if nterms == 3 else 2.0 ** -11
    return np.abs(x64 - got) <= np.maximum(rel * np.abs(x64), 2.0 ** -25)


def as_nchw(values, n, c, hh=1):
    """`values` laid into a float32 [n, c, hh, W] array, W as small as holds them, zero-padded."""
    per = n * c * hh
    w = -(-len(values) // per)
    buf = np.zeros(per * w, np.float32)
    buf[:len(values)] = values
    return buf.reshape(n, c, hh, w)


def planes_of(x):
    """fp32 NCHW -> fp32 chunk-plane order [ceil(C / 16), N, H, W, 16], channels zero-padded (include/binhip.h 'layout glue')."""
    x = np.asarray(x, np.float32)
    n, c, h, w = x.shape
    nch = (c + 15) // 16
    p = np.zeros((n, nch * 16, h, w), np.float32)
    p[:, :c] = x
    return np.ascontiguousarray(p.reshape(n, nch, 16, h, w).transpose(1, 0, 3, 4, 2))


def nchw_of(planes, c):
    """the inverse: [nch, N, H, W, 16] -> [N, c, H, W]."""
    nch, n, h, w, _ = planes.shape
    return np.ascontiguousarray(planes.transpose(1, 0, 4, 2, 3).reshape(n, nch * 16, h, w)[:, :c])


def pixel_unshuffle_ref(x, r):
    """out[b, c r r + i r + j, y, x] = in[b, c, y r + i, x r + j]  (reference RDN.py:123-132)."""
    x = np.asarray(x)
    n, c, h, w = x.shape
    out = np.empty((n, c * r * r, h // r, w // r), x.dtype)
    for ch in range(c):
        for i in range(r):
            for j in range(r):
                out[:, ch * r * r + i * r + j] = x[:, ch, i::r, j::r]
    return out


def pack_inputs_ref(images):
    """pixel_reshuffle(cat(images, 1), 2) in chunk-plane order."""
    return planes_of(pixel_unshuffle_ref(np.concatenate(images, 1), 2))


def unshuffle_planes_ref(x):
    """[nch, N, 2H, 2W, 16] -> [4 nch, N, H, W, 16]: output chunk sub * nch + c = input chunk c at (2y + (sub >> 1), 2x + (sub & 1))."""
    return np.concatenate([x[:, :, (sub >> 1)::2, (sub & 1)::2] for sub in range(4)], 0)


def unpack_input_grads_ref(hi, lo, gout, inv_scale, n_images):
    """outs[i][n, rgb, Y, X] = gout / n_images + (hi + lo)[channel 4 (3 i + rgb) + 2 (Y & 1) + (X & 1)] at (Y / 2, X / 2) * inv_scale, in
    float32 operation by operation (inv_scale a power of two: its product is exact).  hi None = the skip path alone."""
    gout = np.asarray(gout, np.float32)
    skip = gout / np.float32(n_images)
    if hi is None:
        return [skip.copy() for _ in range(n_images)]
    g = hi.astype(np.float32)
    if lo is not None:
        g = g + lo.astype(np.float32)
    g = nchw_of(g, 12 * n_images) * np.float32(inv_scale)              # [N, 12 k, h, w], channel = 4 cc + 2 i + j
    n, _, h, w = g.shape
    full = np.empty((n, 3 * n_images, 2 * h, 2 * w), np.float32)       # pixel-shuffle back
    for cc in range(3 * n_images):
        for i in range(2):
            for j in range(2):
                full[:, cc, i::2, j::2] = g[:, 4 * cc + 2 * i + j]
    return [skip + full[:, 3 * k:3 * k + 3] for k in range(n_images)]


# ---- frames -----------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = ((1, 1), (1, 7), (5, 1), (37, 53), (720, 1280))
FRAME_PADS = ((0, 0, 0, 0), (3, 0, 0, 0), (0, 0, 0, 9), (3, 5, 2, 7), (64, 64, 24, 24))          # left, right, top, bottom
FRAME_PADS_5x1 = ((4, 0, 9, 0), (0, 3, 0, 11))             # pads larger than the image


def frame_cases():
    out = [(h, w, p) for h, w in FRAME_SIZES for p in FRAME_PADS]
    return out + [(5, 1, p) for p in FRAME_PADS_5x1]


def u8_image(h, w, seed=2):
    img = np.random.RandomState(seed + h * 1301 + w).randint(0, 256, (h, w, 3)).astype(np.uint8)
    flat = img.reshape(-1)
    flat[:min(256, flat.size)] = np.arange(256, dtype=np.uint8)[:min(256, flat.size)]          # every byte value where there is room
    return img


def u8_to_frame_ref(img, pads):
    """read_image (test.py:44-56: float32 / 255, BGR -> RGB, CHW) + ReplicationPad2d (test.py:348-371)."""
    a = img.astype(np.float32) / 255.0
    a = np.ascontiguousarray(a[:, :, [2, 1, 0]].transpose(2, 0, 1))
    assert a.dtype == np.float32
    return F.pad(torch.from_numpy(a)[None], tuple(pads), mode="replicate").numpy()


def rounding_frame():
    """fp32 [3, 16, 17] frame: for every k in 0..254 the half-way value (k + 0.5) / 255 rounded to float32 and its two float32
    neighbours; 0, 1, -0.0, negatives, values above 1, +-inf; the rest uniform in [-0.1, 1.1).  (No NaN: numpy's cast of it to
    uint8 is not defined.)"""
    mid = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0).astype(np.float32)
    vals = np.concatenate([mid, np.nextafter(mid, np.float32(2)), np.nextafter(mid, np.float32(-1)),
                           np.array([0.0, 1.0, -0.0, -1.0, -1e-3, -1e-30, 1.5, 2.0, 1e30, np.inf, -np.inf,
                                     np.nextafter(np.float32(1), np.float32(0)), np.nextafter(np.float32(1), np.float32(2))], np.float32)])
    rng = np.random.RandomState(4)
    frame = (rng.rand(3 * 16 * 17).astype(np.float32) * np.float32(1.2) - np.float32(0.1))
    pos = rng.permutation(frame.size)[:len(vals)]           # scattered, so that every crop below holds some of them
    frame[pos] = vals
    return frame.reshape(3, 16, 17)


ROUNDING_CROPS = ((0, 0, 16, 17), (0, 0, 9, 8), (0, 9, 9, 8), (7, 0, 9, 8), (7, 9, 9, 8), (5, 6, 1, 1))    # top, left, H, W
