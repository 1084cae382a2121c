"""Write the blurry frames of an Adobe-layout tree from its sharp frames, as the reference's
data_scripts/adobe240fps/create_dataset_blur_N_frames_average.py does (lines 95-148):

  <root>/<mode>/<clip>/NNNNN.png   ->   <root>/<mode>_blur/<clip>/NNNNN.png   one per usable blurry centre
                                        <root>/<mode>_list/<clip>_im_list.txt its names

with bin_amd.data.BIN_dataset.blur_average, the function the `blur_window` training option synthesises with.  Training does
not need these folders (set `blur_window`); `python -m bin_amd.test`, which takes a folder of blurry frames, does.

    python tools/make_blur_folder.py --root R --mode test --window 11

With --gamma G (a number 1.0 .. 2.4 or srgb) a blurry frame is an exposure in linear light instead, and with --noise READ,SHOT
[--noise_seed N] it carries sensor noise: bin_amd.data.exposure.expose_average, the function the `blur_gamma` / `blur_noise`
training options synthesise with, on whole frames.  The key of a frame is (N, its running index over the whole tree, clips in sorted
name order); every channel of a frame is treated alike (alpha included).  Without the flags the bytes are those of blur_average.

Refuses to overwrite: <mode>_blur and <mode>_list must not exist."""
import argparse
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402


def parse_noise_flag(text):
    """--noise READ,SHOT -> [read, shot] for exposure.parse_blur_noise."""
    try:
        return [float(v) for v in text.split(",")]
    except ValueError:
        raise ValueError(f"--noise: {text!r} is not READ,SHOT") from None


def parse_gamma_flag(text):
    """--gamma G -> a number or the word, for exposure.parse_blur_gamma."""
    try:
        return float(text)
    except ValueError:
        return text


def make_blur_folder(root, mode, window, gamma=None, noise=None, noise_seed=0):
    """Returns {clip: [names of the blurry frames written]}.  `gamma`, `noise`: the values of the dataset options `blur_gamma` and
    `blur_noise`; None (both): the reference's truncated mean."""
    from PIL import Image
    from bin_amd.data import util
    from bin_amd.data.BIN_dataset import blur_average, blur_half_max, clip_blur_centres, exposure_paths, parse_blur_window
    window = parse_blur_window(window)
    if not isinstance(window, int):
        raise ValueError(f"make_blur_folder: one window size, got {window!r}")
    h = blur_half_max(window)
    exposure = None
    if gamma is not None or noise is not None:
        from bin_amd.data import exposure as X
        exposure = X.parse_options({"blur_gamma": gamma, "blur_noise": noise}, window)
    sharp_root = os.path.join(root, mode)
    blur_root, list_root = os.path.join(root, mode + "_blur"), os.path.join(root, mode + "_list")
    for d in (blur_root, list_root):
        if os.path.exists(d):
            raise FileExistsError(f"make_blur_folder: {d} exists; remove it or choose another root")
    if not os.path.isdir(sharp_root):
        raise FileNotFoundError(f"make_blur_folder: no sharp frames at {sharp_root}")
    os.makedirs(blur_root), os.makedirs(list_root)
    written, count = {}, 0
    for clip in sorted(os.listdir(sharp_root)):
        sharp_dir = os.path.join(sharp_root, clip)
        _, _, usable = clip_blur_centres(sharp_dir, h)
        names = [str(c).zfill(5) + ".png" for c in usable]
        if names:                                            # as the script: a clip too short for a blurry frame gets no folder
            os.makedirs(os.path.join(blur_root, clip))
        for name in names:
            stack = [util.imread_u8(p) for p in exposure_paths(os.path.join(sharp_dir, name), h)]
            if exposure is None:
                img = blur_average(stack)
            else:
                img = X.expose_average(stack, exposure.tables, (int(noise_seed) & 0xFFFFFFFF, count & 0xFFFFFFFF))
            count += 1
            rgb = img[:, :, 0] if img.shape[2] == 1 else img[:, :, [2, 1, 0] + list(range(3, img.shape[2]))]
            Image.fromarray(np.ascontiguousarray(rgb)).save(os.path.join(blur_root, clip, name))
        with open(os.path.join(list_root, clip + "_im_list.txt"), "w") as f:
            f.write("\n".join(names))
        written[clip] = names
    return written


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="dataset root holding <mode>/")
    ap.add_argument("--mode", default="train")
    ap.add_argument("--window", type=int, default=11, help="odd exposure in sharp frames, 1 .. 33")
    ap.add_argument("--gamma", default=None, help="average in linear light: a number 1.0 .. 2.4 (code e -> e^G) or srgb; rounds to nearest")
    ap.add_argument("--noise", default=None, help="READ,SHOT: sensor noise of variance READ^2 + SHOT * lin in linear light (needs --gamma)")
    ap.add_argument("--noise_seed", type=int, default=0, help="first key word of the noise; the second is the frame's running index")
    args = ap.parse_args()
    try:
        written = make_blur_folder(args.root, args.mode, args.window, None if args.gamma is None else parse_gamma_flag(args.gamma),
                                   None if args.noise is None else parse_noise_flag(args.noise), args.noise_seed)
    except (FileExistsError, FileNotFoundError, ValueError) as e:
        sys.exit(str(e))
    print(f"{sum(len(v) for v in written.values())} blurry frames of {len(written)} clips under "
          f"{os.path.join(args.root, args.mode + '_blur')}")


if __name__ == "__main__":
    main()
