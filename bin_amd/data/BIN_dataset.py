"""Adobe240 blurry-interpolation training/validation dataset (reference data/BIN_dataset.py:12-287).

Directory contract (made by the reference's data_scripts/adobe240fps/create_dataset_blur_N_frames_average.py):
  <root>/<mode>/<clip>/NNNNN.png        sharp 240-fps frames
  <root>/<mode>_blur/<clip>/NNNNN.png   blurry 30-fps frames (every 8th index)
  <root>/<mode>_list/<clip>_im_list.txt names of the usable blurry frames
One sample = 6 blurry frames B1,B3,..,B11 (8 apart), the 6 sharp frames at the same indices (I1..I11) and the 5
sharp frames half-way (I2..I10); windows slide by one blurry frame.

bin_amd extension, option `blur_window` (an odd exposure 1 .. 33 in sharp frames, or a list of them to draw from per sample):
the window list is built from <root>/<mode>/ alone by that script's rule (make_sharp_window_list) and every blurry frame is
synthesised when it is loaded, as the script's truncated mean of the sharp frames around it (blur_average) — no <mode>_blur,
no <mode>_list.  On the host that costs 6 x L extra PNG decodes per sample; the device cache (device_cache.py), which averages
inside its gather launch, is the intended way to train with it.  With `blur_gamma` (and `blur_noise`) beside it the frames of an
exposure are averaged in linear light, with sensor noise, instead (exposure.py; ops.gather_windows_exposed on the device).

NOTE the reference's `_make_dataset_deep_long_` falls off its end without returning (BIN_dataset.py:283-287), so
`BINDataset(opt)` raises there; this class implements what that code computes up to that point (the window list,
shuffled, `split` % kept) and the loader's crop/flip/reverse draws in the same order, which the goldens pin."""
import math
import os
import random

import numpy as np
import torch
import torch.utils.data as data

from . import util

NUM_WIN_PER_BUNCH = 4
BLUR_STEP = 8                    # sharp frames per blurry frame
SRC_H, SRC_W = 352, 640          # frame size of the prepared dataset (crop offsets are drawn against it)


def make_window_list(root, mode="train", split=100, shuffle=True):
    """[[6 blurry paths], [6 sharp paths], [5 in-between sharp paths], key] per window, as the reference builds
    them; windows whose blurry frames are not all named in the clip's im_list are dropped."""
    sharp_root = os.path.join(root, mode)
    blur_root = os.path.join(root, mode + "_blur")
    list_root = os.path.join(root, mode + "_list")
    windows = []
    for clip in os.listdir(blur_root):
        blur_dir, sharp_dir = os.path.join(blur_root, clip), os.path.join(sharp_root, clip)
        blur_pics = sorted(os.listdir(blur_dir))
        with open(os.path.join(list_root, clip + "_im_list.txt")) as f:
            usable = set(f.read().split("\n"))
        first = int(blur_pics[0][:-4])
        for win in range(len(blur_pics) - NUM_WIN_PER_BUNCH - 1):
            base = first + BLUR_STEP * win
            name = lambda i: str(i).zfill(5) + ".png"
            blurry = [name(base + BLUR_STEP * k) for k in range(6)]
            if not all(b in usable for b in blurry):
                continue
            windows.append([[os.path.join(blur_dir, b) for b in blurry],
                            [os.path.join(sharp_dir, b) for b in blurry],
                            [os.path.join(sharp_dir, name(base + BLUR_STEP * k + BLUR_STEP // 2)) for k in range(5)],
                            clip + "_" + blurry[0][:-4]])
    if shuffle:
        random.shuffle(windows)
    keep = int(math.floor(len(windows) * split / 100.0))
    return windows[:keep], windows[keep:]


BLUR_FIRST_CENTRE = 16           # the script's first blurry centre, counted from the clip's first file (script line 100)
MAX_BLUR_WINDOW = 33             # longest exposure: half range 16, the limit of binhip_gather_windows_blur


def parse_blur_window(value):
    """The `blur_window` option: None (absent), an odd int 1 .. 33 (no draw), or a tuple of them (one random.choice per
    sample).  The reference's script halves `window_size - 1` with an integer division, so an even size silently means the
    next smaller odd one; only odd sizes are accepted here."""
    def one(v):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v <= MAX_BLUR_WINDOW or v % 2 == 0:
            raise ValueError(f"blur_window: {v!r} is not an odd integer in 1 .. {MAX_BLUR_WINDOW} (the exposure is centred: "
                             f"2h + 1 sharp frames; the reference's script turns an even size into the next smaller odd one)")
        return v
    if value is None:
        return None
    if isinstance(value, (list, tuple)):
        if not value:
            raise ValueError("blur_window: the list of exposures is empty")
        return tuple(one(v) for v in value)
    return one(value)


def blur_half_max(blur_window):
    """Largest half range h = (L - 1) / 2 the option can draw."""
    return (max(blur_window) if isinstance(blur_window, tuple) else blur_window) // 2


def draw_blur_half(blur_window):
    """Half range h of one sample's exposure: a list draws with one random.choice (made after draw_window_aug's four draws),
    an integer draws nothing."""
    return (random.choice(blur_window) if isinstance(blur_window, tuple) else blur_window) // 2


def blur_average(frames_u8):
    """The blurry frame of the L uint8 frames `frames_u8` ([L, ...] or a list): the script's float32 sum / float(L) truncated
    to uint8 (lines 121-132), computed as the integer quotient S // L, which equals it for every byte sum S <= 255 L, L <= 33
    (tests/test_cpu_blur_synth.py checks every pair)."""
    a = np.asarray(frames_u8)
    if a.dtype != np.uint8 or a.ndim < 1 or not 1 <= a.shape[0] <= MAX_BLUR_WINDOW:
        raise ValueError(f"blur_average: 1 .. {MAX_BLUR_WINDOW} uint8 frames, got {a.dtype} {a.shape}")
    return (a.sum(axis=0, dtype=np.uint32) // np.uint32(a.shape[0])).astype(np.uint8)


def exposure_options(opt, blur_window):
    """exposure.parse_options of a dataset's options; None, without importing that module, when both are absent."""
    if opt.get("blur_gamma") is None and opt.get("blur_noise") is None:
        return None
    from . import exposure
    return exposure.parse_options(opt, blur_window)


def frame_number(path):
    return int(os.path.basename(path)[:-4])


def exposure_paths(centre_path, h):
    """The 2h + 1 sharp files averaged into the blurry frame named after `centre_path`, in ascending order."""
    d, c = os.path.dirname(centre_path), frame_number(centre_path)
    return [os.path.join(d, str(k).zfill(5) + ".png") for k in range(c - h, c + h + 1)]


def read_blurry(centre_path, h):
    """float32 HWC BGR in [0, 1]: what util.read_img returns for the blurry PNG the script would have written."""
    img = blur_average([util.imread_u8(p) for p in exposure_paths(centre_path, h)])
    return (img.astype(np.float32) / 255.)[:, :, :3]


def clip_blur_centres(sharp_dir, h):
    """(first file number, every blurry centre of the clip, the usable ones) by the script's rule (lines 95-108): centres
    first + 16 + 8 i, i = 0 .. floor(n / 8) - 3; a centre is usable when c - h .. c + h stays inside the clip's files.  The
    files must be numbered consecutively (the device cache relies on "file number +- k" being "frame +- k")."""
    numbers = sorted(int(f[:-4]) for f in os.listdir(sharp_dir) if f.endswith(".png"))
    if not numbers:
        return 0, [], []
    first, n = numbers[0], len(numbers)
    if numbers != list(range(first, first + n)):
        raise ValueError(f"blur_window: the sharp files of {sharp_dir} are not numbered consecutively from {first:05d}.png")
    centres = [first + BLUR_FIRST_CENTRE + BLUR_STEP * i for i in range(n // BLUR_STEP - 2)]
    return first, centres, [c for c in centres if c - h >= first and c + h <= first + n - 1]


def make_sharp_window_list(root, mode="train", split=100, shuffle=True, blur_window=11):
    """make_window_list from <root>/<mode>/<clip>/ alone: the windows, keys, shuffle and split it gives for the <mode>_blur and
    <mode>_list folders the script would have written with this window size.  A window's blurry entries are the paths of the
    CENTRE sharp files (its blurry and sharp lists are equal); load_window averages exposure_paths() around them.  With a
    list of sizes a centre must be usable at the largest."""
    h = blur_half_max(parse_blur_window(blur_window))
    sharp_root = os.path.join(root, mode)
    windows = []
    for clip in os.listdir(sharp_root):
        sharp_dir = os.path.join(sharp_root, clip)
        _, centres, usable = clip_blur_centres(sharp_dir, h)
        usable = set(usable)
        name = lambda i: str(i).zfill(5) + ".png"
        for win in range(len(centres) - NUM_WIN_PER_BUNCH - 1):
            cs = centres[win:win + 6]
            if not all(c in usable for c in cs):
                continue
            sharp = [os.path.join(sharp_dir, name(c)) for c in cs]
            windows.append([list(sharp), sharp, [os.path.join(sharp_dir, name(c + BLUR_STEP // 2)) for c in cs[:5]],
                            clip + "_" + name(cs[0])[:-4]])
    if shuffle:
        random.shuffle(windows)
    keep = int(math.floor(len(windows) * split / 100.0))
    return windows[:keep], windows[keep:]


def draw_window_aug(input_frame_size=(3, 128, 256), data_aug=True, src_size=(SRC_H, SRC_W)):
    """The reference loader's augmentation draws for one window, in its order: temporal order (randint: 1 keeps it, 0
    reverses; no aug => reversed, as in the reference), crop offsets (choice, choice), horizontal flip (randint).
    Returns (reversed, y0, x0, flip).  load_window and the device-cache loader (device_cache.py) both draw through here.
    `src_size`: the (H, W) the offsets are drawn against; the prepared dataset's unless the frames come from a video clip
    (video_dataset.py), which has its own."""
    reverse = not (data_aug and random.randint(0, 1))
    _, ch, cw = input_frame_size
    src_h, src_w = src_size
    y0 = random.choice(range(src_h - ch + 1))
    x0 = random.choice(range(src_w - cw + 1))
    flip = bool(data_aug and random.randint(0, 1))
    return reverse, y0, x0, flip


def load_window(window, input_frame_size=(3, 128, 256), data_aug=True, blur_window=None, exposure=None, train=True, index=0):
    """Read the 17 frames of one window with the draws of draw_window_aug.  Returns ([B1..B11], [I1..I11], [I2..I10], key)
    as float32 HWC BGR crops.  With `blur_window` (parse_blur_window) the window is one of make_sharp_window_list and its
    blurry frames are averaged from the sharp files, after draw_blur_half's draw.  With `exposure` (exposure.parse_options)
    beside it they are exposures in linear light: the sample's key is drawn next (exposure.sample_key; `train` and the
    window's `index` decide it), and each exposure is made from the cropped and flipped frames, because its noise is tied to
    output coordinates."""
    blurry, sharp, mid, key = window
    reverse, y0, x0, flip = draw_window_aug(input_frame_size, data_aug)
    if reverse:
        blurry, sharp, mid = blurry[::-1], sharp[::-1], mid[::-1]
    _, ch, cw = input_frame_size

    def cut(f):
        f = f[y0:y0 + ch, x0:x0 + cw, :]
        return np.fliplr(f) if flip else f

    if blur_window is None:
        frames = [util.read_img(p) for p in list(blurry) + list(sharp) + list(mid)]
    elif exposure is None:
        h = draw_blur_half(blur_window)
        frames = [read_blurry(p, h) for p in blurry] + [util.read_img(p) for p in list(sharp) + list(mid)]
    else:
        from . import exposure as X
        h = draw_blur_half(blur_window)
        k = X.sample_key(exposure, train, index)
        exposed = [X.expose_average([cut(util.imread_u8(q)[:, :, :3]) for q in exposure_paths(p, h)], exposure.tables, k, slot)
                   for slot, p in enumerate(blurry)]
        frames = [e.astype(np.float32) / 255. for e in exposed] + [cut(util.read_img(p)) for p in list(sharp) + list(mid)]
        return frames[:6], frames[6:12], frames[12:], key
    frames = [f[y0:y0 + ch, x0:x0 + cw, :] for f in frames]
    if flip:
        frames = [np.fliplr(f) for f in frames]
    return frames[:6], frames[6:12], frames[12:], key


class BINDataset(data.Dataset):
    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.GT_root, self.LQ_root = opt["dataroot_GT"], opt["dataroot_LQ"]
        self.data_type = opt.get("data_type", "img")
        self.input_frame_size = tuple(opt["LQ_size"])
        self.blur_window = parse_blur_window(opt.get("blur_window"))
        if self.blur_window is None:
            self.all_paths, _ = make_window_list(self.LQ_root, mode=opt["name"])
        else:
            self.all_paths, _ = make_sharp_window_list(self.LQ_root, mode=opt["name"], blur_window=self.blur_window)
        self.exposure = exposure_options(opt, self.blur_window)
        self.train = opt.get("phase", "train") == "train"

    def __len__(self):
        return len(self.all_paths)

    @staticmethod
    def Adobe_BIN_loader(im_path_pair, input_frame_size=(3, 128, 256), data_aug=True, transform=None):
        return load_window(im_path_pair, input_frame_size, data_aug)

    @staticmethod
    def _to_tensor(frames):
        a = np.stack(frames, axis=0)[:, :, :, [2, 1, 0]]                    # T H W C, BGR -> RGB
        return torch.from_numpy(np.ascontiguousarray(a.transpose(0, 3, 1, 2))).float()

    def __getitem__(self, index):
        LQs, GTenh, GTinp, key = load_window(self.all_paths[index], self.input_frame_size, blur_window=self.blur_window,
                                             exposure=self.exposure, train=self.train, index=index)
        return {"LQs": self._to_tensor(LQs), "GTenh": self._to_tensor(GTenh), "GTinp": self._to_tensor(GTinp),
                "key": key}
