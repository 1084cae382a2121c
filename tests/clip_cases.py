"""Shared by tests/test_cpu_clip.py and tests/test_gpu_clip.py: the numpy restatement of binclip_yuv_to_bgr (include/binclip.h) on top
of video_cases.to_frame_ref, the near-tie mask that goes with it, the inputs of the device tests and a writer of Y4M clips.

A byte of the arena is rint(255 v), v the [0, 1] channel value of include/binyuv.h.  The kernel evaluates v and the product in fp32;
where 255 v (in float64) lies within TIE_MARGIN of a half-integer an fp32 evaluation may round the other way, so those bytes are
compared with a tolerance of 1 and every other byte exactly.  The fp32 error of 255 v is below 1e-4 (test_cpu_clip.py measures it),
a tenth of the margin, and the mask covers about a thousandth of the bytes."""
import numpy as np

import video_cases as VC

TIE_MARGIN = 2.0 ** -10
STRIDES = ("tight", "plus6", "round16")          # frame_bytes; + 6: rows at every alignment, the byte path; rounded up to 16
BIG_CASE = (1030, 2048, 444)                     # 527 360 items: more than 2048 blocks of 256, so blocks stride


def stride_of(kind, frame_bytes):
    return {"tight": frame_bytes, "plus6": frame_bytes + 6, "round16": -(-frame_bytes // 16) * 16}[kind]


def scaled_ref(payload, h, w, fmt, dtype=np.float64):
    """255 v before rounding, [h, w, 3] in B, G, R order, evaluated in `dtype`."""
    rgb = VC.to_frame_ref(payload, h, w, fmt, (0, 0, 0, 0), dtype)
    out = dtype(255) * rgb
    assert out.dtype == dtype
    return np.ascontiguousarray(out.transpose(1, 2, 0)[:, :, ::-1])


def bgr_ref(payload, h, w, fmt, dtype=np.float64):
    """uint8 [h, w, 3] HWC BGR: rint(255 * to_frame_ref) reordered."""
    return np.rint(scaled_ref(payload, h, w, fmt, dtype)).astype(np.uint8)


def near_tie(payload, h, w, fmt):
    """bool [h, w, 3]: the bytes whose float64 pre-rounding value lies within TIE_MARGIN of a rounding tie."""
    v = scaled_ref(payload, h, w, fmt)
    return np.abs(v - np.floor(v) - 0.5) < TIE_MARGIN


def ref_and_mask(payload, h, w, fmt):
    v = scaled_ref(payload, h, w, fmt)
    return np.rint(v).astype(np.uint8), np.abs(v - np.floor(v) - 0.5) < TIE_MARGIN


def all_code_points(rows=slice(0, 4096)):
    """The 4:4:4 payload of the rows `rows` of the 4096 x 4096 frame that holds every (Y, U, V) once: pixel p = 4096 y + x carries
    Y = p >> 16, U = (p >> 8) & 255, V = p & 255."""
    y = np.arange(4096)[rows]
    p = (y[:, None].astype(np.int64) << 12) + np.arange(4096)[None, :]
    return np.concatenate([(p >> 16).astype(np.uint8).reshape(-1), ((p >> 8) & 255).astype(np.uint8).reshape(-1),
                           (p & 255).astype(np.uint8).reshape(-1)])


def staged(payloads, stride, fill, lead=0):
    """uint8 [lead + n * stride]: the payloads at `lead` + i * stride, every other byte `fill`."""
    n = len(payloads)
    buf = np.full(lead + n * stride, fill, np.uint8)
    for i, p in enumerate(payloads):
        buf[lead + i * stride:lead + i * stride + p.size] = p
    return buf


def write_clip(path, n, h, w, chroma=420, seed=0, tags=b"F240:1 Ip A1:1", frame_line=b"FRAME"):
    """A Y4M file of n random frames; returns its payloads, uint8 [n, frame_bytes]."""
    cs = {420: b"C420jpeg", 444: b"C444"}[chroma]
    payloads = np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, VC.frame_bytes(h, w, chroma)), dtype=np.uint8)
    with open(path, "wb") as f:
        f.write(b"YUV4MPEG2 W%d H%d " % (w, h) + tags + b" " + cs + b"\n")
        for p in payloads:
            f.write(frame_line + b"\n")
            f.write(p.tobytes())
    return payloads
