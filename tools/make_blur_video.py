"""Write the blurry low-rate Y4M of a sharp high-frame-rate one: the video twin of tools/make_blur_folder.py.

    python tools/make_blur_video.py IN.y4m OUT.y4m --window 11

A sharp stream of n frames at F = r:d gives the blurry frames of the reference's
data_scripts/adobe240fps/create_dataset_blur_N_frames_average.py at F = r:8d: frame i is the truncated mean of the sharp frames
16 + 8 i - h .. 16 + 8 i + h (h = (window - 1) / 2, frames counted from 0), i < n // 8 - 2.  It is made on the device with the
functions training from clips uses (dataset mode BIN_video): ops.yuv_to_bgr, ops.gather_windows_blur on a one-slot, full-frame row,
ops.frame_to_yuv.  Centres whose exposure leaves the clip are dropped from the front and the back; the tool says how many, and
prints the `python -m bin_amd.test` arguments that score a run on OUT.y4m against IN.y4m.

With --gamma G (a number 1.0 .. 2.4 or srgb) a blurry frame is an exposure in linear light instead, and with --noise READ,SHOT
[--noise_seed N] it carries sensor noise: ops.gather_windows_exposed, the launch the `blur_gamma` / `blur_noise` training options
use (bin_amd.data.exposure.expose_average gives the same bytes on the host).  The planes are treated as training from clips treats
them: the Y plane and the chroma of every sharp frame are converted to 8-bit BGR first (ops.yuv_to_bgr), the exposure is made on
those B, G and R codes, noise per colour channel, and the result is converted back to Y and chroma by ops.frame_to_yuv; neither
the curve nor the noise is applied to a YUV plane directly.  The key of output frame i is (N, i).  Without the flags the bytes
are those of the truncated mean.

Refuses to overwrite: OUT.y4m must not exist."""
import argparse
import collections
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def blur_centres(n, h):
    """(every blurry centre of a clip of n frames, the usable ones), as 0-based frame indices."""
    centres = [16 + 8 * i for i in range(n // 8 - 2)]
    return centres, [c for c in centres if c - h >= 0 and c + h <= n - 1]


def make_blur_video(src, dst, window, matrix="auto", range_="auto", device="cuda", gamma=None, noise=None, noise_seed=0):
    """Returns (the sharp frame index of every blurry frame written, centres dropped at the front, at the back).  `gamma`, `noise`:
    the values of the dataset options `blur_gamma` and `blur_noise`; None (both): the reference's truncated mean."""
    import torch
    from bin_amd import ops, video
    from bin_amd.data.BIN_dataset import blur_half_max, parse_blur_window
    window = parse_blur_window(window)
    if not isinstance(window, int):
        raise ValueError(f"make_blur_video: one window size, got {window!r}")
    h = blur_half_max(window)
    curve = None
    if gamma is not None or noise is not None:
        from bin_amd.data import exposure as X
        curve = ops.exposure_curve(*X.parse_options({"blur_gamma": gamma, "blur_noise": noise}, window))
    if os.path.exists(dst):
        raise FileExistsError(f"make_blur_video: {dst} exists; remove it or choose another name")
    header, n = video.clip_info(src)
    fmt = video.resolve_format(header, matrix, range_)
    centres, kept = blur_centres(n, h)
    if not kept:
        raise ValueError(f"make_blur_video: {src} has {n} frames: too short for a blurry frame of {window}")
    front, back = centres.index(kept[0]), len(centres) - 1 - centres.index(kept[-1])
    H, W, L = header.height, header.width, 2 * h + 1
    stride = -(-header.frame_bytes // 16) * 16
    stage = torch.empty((L, stride), dtype=torch.uint8, pin_memory=True)
    row = np.array([[h, 0, 0, 0, h]], dtype=np.int32)         # one slot: the centre's id in the exposure's arena, y0, x0, flip, h
    recent = collections.deque(maxlen=L)
    want, written = set(kept), 0
    out_header = video.Y4MHeader(W, H, (header.rate[0], 8 * header.rate[1]), header.interlace, header.aspect, header.colorspace, header.extra)
    with video.Y4MReader(src) as rd, video.Y4MWriter(dst, out_header) as wr, torch.cuda.device(device):
        for k in range(kept[-1] + h + 1):
            buf = np.empty(header.frame_bytes, np.uint8)
            if not rd.readinto(buf):
                raise ValueError(f"make_blur_video: {src} ends at frame {k}: {n} were counted")
            recent.append(buf)
            if k - h not in want:
                continue
            for j, p in enumerate(recent):
                stage[j, :header.frame_bytes] = torch.from_numpy(p)
            arena = ops.yuv_to_bgr(stage.to(device, non_blocking=True), H, W, fmt)
            if curve is None:
                blurry = ops.gather_windows_blur(arena, row, (H, W), 1)
            else:                                            # the same row, then the key (seed, output frame index)
                keyed = np.concatenate([row, np.array([[int(noise_seed) & 0xFFFFFFFF, written]], np.uint32).view(np.int32)], axis=1)
                blurry = ops.gather_windows_exposed(arena, keyed, (H, W), 1, curve)
            written += 1
            wr.write(ops.frame_to_yuv(blurry[0], 0, 0, H, W, fmt).cpu().numpy())
    return kept, front, back


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("input", help="the sharp high-frame-rate Y4M file")
    ap.add_argument("output", help="the blurry Y4M to write")
    ap.add_argument("--window", type=int, default=11, help="odd exposure in sharp frames, 1 .. 33")
    ap.add_argument("--yuv_matrix", default="auto", help="auto | bt601 | bt709")
    ap.add_argument("--yuv_range", default="auto", help="auto | limited | full")
    ap.add_argument("--gamma", default=None, help="average in linear light: a number 1.0 .. 2.4 (code e -> e^G) or srgb; applied to the "
                    "B, G, R codes the YUV planes convert to, not to the planes")
    ap.add_argument("--noise", default=None, help="READ,SHOT: sensor noise of variance READ^2 + SHOT * lin in linear light, per colour "
                    "channel (needs --gamma)")
    ap.add_argument("--noise_seed", type=int, default=0, help="first key word of the noise; the second is the output frame index")
    args = ap.parse_args()
    try:
        from make_blur_folder import parse_gamma_flag, parse_noise_flag
        kept, front, back = make_blur_video(args.input, args.output, args.window, args.yuv_matrix, args.yuv_range,
                                            gamma=None if args.gamma is None else parse_gamma_flag(args.gamma),
                                            noise=None if args.noise is None else parse_noise_flag(args.noise), noise_seed=args.noise_seed)
    except (FileExistsError, FileNotFoundError, ValueError) as e:
        sys.exit(str(e))
    print(f"{len(kept)} blurry frames in {args.output}; {front} centre(s) dropped at the front and {back} at the back (their exposure "
          f"leaves the clip)")
    print(f"score a run on it against the sharp stream with: python -m bin_amd.test --input_video {args.output} --output_video OUT.y4m "
          f"--gt_video {args.input} --gt_offset {kept[0]}")


if __name__ == "__main__":
    main()
