"""The case table of the YUV kernels' bit pin: binyuv_to_frame, binyuv_from_frame (include/binyuv.h), binrate_blend_to_yuv
(include/binrate.h) and binclip_yuv_to_bgr (include/binclip.h) over video_cases.CASES x video_cases.MATRIX_RANGE, each on both data
paths, plus one case per entry point whose blocks stride unevenly.  tests/golden/make_yuv_bits.py records the sha256 of every output
buffer into tests/golden/yuv_bits.json; test_gpu_yuv_bits.py computes them again.  The inputs are NOT kept away from rounding ties
(video_cases.safe_rgb_frame is not used): the pin holds the ties, NaN and the infinities too.

A key is "<op>/<h>x<w>_<chroma>/<matrix>_<range>" or "<op>/strided"; its value maps every sub-case (pads or crop, weight or stride,
`off<o>`: the device views start o elements past a 256-byte boundary, 0 the dword / float4 path where the shape allows it, 1 the byte /
single-float path) to the digest of the whole output buffer, guard bytes included where the caller passes the buffer."""
import functools
import hashlib

import numpy as np

import video_cases as VC

OPS = ("to_frame", "from_frame", "blend", "to_bgr")
OFFSETS = (0, 1)
BLEND_WEIGHTS = (0.0, 0.25, 0.6)
BGR_FRAMES = 3
BGR_STRIDES = ("plus5", "round16")               # frame_bytes + 5: rows at every alignment; rounded up to 16: the dword path
GUARD_BYTES = 16
# 2048 blocks of 256 lanes hold 524 288 items; between two and three times that some lanes loop twice and some three times
STRIDE_LANES = 2048 * 256
STRIDED_FRAME = (2731, 1920, 444)                # 2731 * 480 = 1 310 880 items of binyuv_to_frame, binyuv_from_frame, binrate_blend_to_yuv
STRIDED_CLIP = (5000, 16, 64, 444)               # n, h, w, chroma: 5000 * 16 * 16 = 1 280 000 items of binclip_yuv_to_bgr
STRIDED_FMT = ("bt709", "limited")
STRIDED_WEIGHT = 0.25

KEYS = [f"{op}/{h}x{w}_{c}/{m}_{r}" for op in OPS for h, w, c in VC.CASES for m, r in VC.MATRIX_RANGE] + [f"{op}/strided" for op in OPS]


def parse_key(key):
    """(op, h, w, chroma, matrix, range, strided)."""
    part = key.split("/")
    if part[1] == "strided":
        h, w, c = STRIDED_CLIP[1:] if part[0] == "to_bgr" else STRIDED_FRAME
        return (part[0], h, w, c) + STRIDED_FMT + (True,)
    size, chroma = part[1].split("_")
    h, w = size.split("x")
    matrix, rng = part[2].split("_")
    return part[0], int(h), int(w), int(chroma), matrix, rng, False


def strided_items(op):
    if op == "to_bgr":
        n, h, w, _ = STRIDED_CLIP
        return n * h * ((w + 3) // 4)
    h, w, _ = STRIDED_FRAME
    return h * ((w + 3) // 4)


def bgr_stride(kind, frame_bytes):
    return {"plus5": frame_bytes + 5, "round16": -(-frame_bytes // 16) * 16}[kind]


def _name(tag, four):
    return tag + ".".join(str(v) for v in four)


def subcases(key):
    """[(name, parameters)] of a key, in the order they run: parameters are (pads or crop, weight or stride kind, offset)."""
    op, h, w, _, _, _, strided = parse_key(key)
    if op == "to_bgr":
        kinds = ("round16",) if strided else BGR_STRIDES
        return [(f"{kind}/off{o}", (None, kind, o)) for kind in kinds for o in OFFSETS]
    zero = (0, 0, 0, 0)
    if op == "to_frame":
        pads = [zero] if strided else list(dict.fromkeys(VC.pads_of(h, w)))
        return [(f"{_name('pads', p)}/off{o}", (p, None, o)) for p in pads for o in OFFSETS]
    crops = [zero] if strided else list(dict.fromkeys(VC.crops_of(h, w)))
    if op == "from_frame":
        return [(f"{_name('crop', p)}/off{o}", (p, None, o)) for p in crops for o in OFFSETS]
    weights = (STRIDED_WEIGHT,) if strided else BLEND_WEIGHTS
    return [(f"{_name('crop', p)}/w{wt}/off{o}", (p, wt, o)) for p in crops for wt in weights for o in OFFSETS]


# ------------------------------------------------------------------------------------------------ inputs (host side, seeded)
@functools.lru_cache(maxsize=4)
def unsafe_frame(hp, wp, seed):
    """fp32 [1, 3, hp, wp]: uniform(-0.25, 1.25) with NaN, +inf and -inf planted; nothing is moved off a rounding tie."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = rng.uniform(-0.25, 1.25, (1, 3, hp, wp)).astype(np.float32)
    n_special = min(6, x.size // 8)
    at = rng.choice(x.size, n_special, replace=False)
    x.reshape(-1)[at] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), n_special)
    x.setflags(write=False)
    return x


def _dev(a, offset=0, guard=0):
    """test_gpu_video._dev: `a` on the device `offset` elements past a 256-byte boundary, `guard` guard elements on both sides;
    returns (view, whole buffer)."""
    import torch
    a = np.ascontiguousarray(a)
    fill = VC.GUARD if a.dtype == np.uint8 else -7.0
    host = np.full(a.size + 2 * guard + offset, fill, a.dtype)
    host[guard + offset:guard + offset + a.size] = a.reshape(-1)
    buf = torch.from_numpy(host).cuda()
    return buf[guard + offset:guard + offset + a.size].view(*a.shape), buf


def _sha(t):
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------------ the digests (need a GPU)
def digests(key):
    """{sub-case: sha256 of the output buffer} of one key."""
    from bin_amd import ops
    op, h, w, chroma, matrix, rng, strided = parse_key(key)
    fmt = (chroma, matrix, rng)
    seed = 1000 * h + 10 * w + (chroma == 444)
    out = {}
    if op == "to_frame":
        srcs = [_dev(VC.random_payload(h, w, chroma, seed), offset=o)[0] for o in OFFSETS]
        for name, (pads, _, o) in subcases(key):
            out[name] = _sha(ops.yuv_to_frame(srcs[o], h, w, fmt, pads))
    elif op == "to_bgr":
        n = STRIDED_CLIP[0] if strided else BGR_FRAMES
        fb = VC.frame_bytes(h, w, chroma)
        payloads = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, fb), dtype=np.uint8)
        for name, (_, kind, o) in subcases(key):
            stride = bgr_stride(kind, fb)
            host = np.full((n, stride), 0x5A, np.uint8)
            host[:, :fb] = payloads
            src = _dev(host, offset=o)[0]
            dst, whole = _dev(np.zeros((n, h, w, 3), np.uint8), offset=o, guard=GUARD_BYTES)
            ops.yuv_to_bgr(src, h, w, fmt, out=dst)
            out[name] = _sha(whole)
    else:
        nbytes = VC.frame_bytes(h, w, chroma)
        for name, ((l, r, t, b), weight, o) in subcases(key):
            shape = (h + t + b, w + l + r)
            xa = _dev(unsafe_frame(*shape, seed), offset=o)[0]
            dst, whole = _dev(np.zeros(nbytes, np.uint8), offset=o, guard=GUARD_BYTES)
            if op == "from_frame":
                ops.frame_to_yuv(xa, t, l, h, w, fmt, out=dst)
            else:
                xb = _dev(unsafe_frame(*shape, seed + 1), offset=o)[0]
                ops.blend_to_yuv(xa, xb, weight, t, l, h, w, fmt, out=dst)
            out[name] = _sha(whole)
    return out
