"""Training batches assembled on the GPU from a device-resident frame cache (bin_amd extension, opt-in with
`datasets.train.device_cache: true`).

The host loader (BIN_dataset.load_window) decodes the 17 whole PNGs of every sample, converts them to float32, crops them
and collates them, and feed_data then copies the batch to the device.  Consecutive windows share most of their frames and
every epoch revisits all of them.  Here every frame the training list touches is decoded ONCE into one uint8 arena on the
device (DeviceFrameCache), and each batch is one binhip_gather_windows launch (ops.gather_windows): crop, flip, BGR -> RGB,
/255 and the layout feed_data consumes.  The augmentation draws are the host loader's own (draw_window_aug), made in its
order in the main process, so with the same `random` state a batch equals the host loader's batch at n_workers 0 bit for
bit.

With the dataset option `blur_window` the arena holds sharp frames only, each clip's consecutively in file order, and the six
blurry inputs of a window are averaged from them inside the launch (ops.gather_windows_blur), with the exposure of each
sample in the table.  With `blur_gamma` / `blur_noise` beside it (exposure.py) the launch is ops.gather_windows_exposed: the frames
of an exposure are averaged in linear light, with sensor noise, and the table also carries each sample's key."""
import concurrent.futures as cf
import logging
import os

import numpy as np
import torch

from .. import ops
from .BIN_dataset import SRC_H, SRC_W, blur_half_max, draw_blur_half, draw_window_aug, frame_number
from .util import imread_u8

N_SLOTS = 17                     # 6 blurry + 6 sharp + 5 in-between sharp frames per window
N_BLUR = 6                       # the blurry slots come first
CHUNK_BYTES = 256 << 20          # host staging per pinned buffer while the arena fills


def _frame_shape(path):
    """(H, W, channels of imread_u8) from the file header, without decoding the pixels."""
    from PIL import Image
    with Image.open(path) as im:
        w, h = im.size
        return h, w, {"L": 1, "RGBA": 4}.get(im.mode, 3)


def _default_threads():
    return max(1, min(16, os.cpu_count() or 1))


def window_slots(window, reverse):
    """The 17 frame paths of a window in slot order ([B1..B11], [I1..I11], [I2..I10]), each group reversed when the
    window's temporal order is (as load_window reverses them)."""
    blurry, sharp, mid, _ = window
    if reverse:
        blurry, sharp, mid = blurry[::-1], sharp[::-1], mid[::-1]
    return list(blurry) + list(sharp) + list(mid)


class DeviceFrameCache:
    """Every unique frame of `window_list` decoded once (imread_u8 on a thread pool) into one uint8 [n_frames, H, W, 3]
    BGR arena on `device`.  Raises ValueError before allocating anything when the frames differ in size, a frame is not
    colour (an RGBA frame keeps its first 3 channels, as read_img does), or the arena would exceed `max_gb` (10^9 bytes).
    `blur_half` (the largest half range h of the dataset's `blur_window`): the windows are make_sharp_window_list's, and the
    arena holds per clip every sharp file from its first blurry centre - h to its last + h, consecutively in file order, so
    frame id +- k is file number +- k; `clip_ranges` keeps each clip's [start, end) ids."""

    def __init__(self, window_list, device, max_gb=64, threads=None, blur_half=None):
        self.paths, self.index, self.clip_ranges = [], {}, None
        if blur_half is None:
            for win in window_list:
                for p in window_slots(win, False):
                    if p not in self.index:
                        self.index[p] = len(self.paths)
                        self.paths.append(p)
        else:
            self._index_spans(window_list, blur_half)
        if not self.paths:
            raise ValueError("DeviceFrameCache: the window list is empty")
        threads = threads or _default_threads()
        with cf.ThreadPoolExecutor(threads) as pool:
            shapes = list(pool.map(_frame_shape, self.paths))
        h, w, _ = shapes[0]
        for p, (fh, fw, c) in zip(self.paths, shapes):
            if (fh, fw) != (h, w):
                raise ValueError(f"DeviceFrameCache: frames differ in size: {self.paths[0]} is {h}x{w}, {p} is {fh}x{fw}")
            if c < 3:
                raise ValueError(f"DeviceFrameCache: {p} has {c} channel(s); the cache holds 3-channel colour frames")
        self.shape = (len(self.paths), h, w, 3)
        self.nbytes = len(self.paths) * h * w * 3
        if self.nbytes > max_gb * 1e9:
            raise ValueError(f"DeviceFrameCache: {len(self.paths)} frames of {h}x{w}x3 need {self.nbytes / 1e9:.2f} GB ({self.nbytes} bytes), "
                             f"more than device_cache_max_gb = {max_gb}")
        self.device = torch.device(device)
        self.frames = torch.empty(self.shape, dtype=torch.uint8, device=self.device)
        self._fill(threads)

    def _index_spans(self, window_list, blur_half):
        """`paths`, `index` and `clip_ranges` of make_sharp_window_list's windows: per clip every file from its first blurry centre
        - blur_half to its last + blur_half.  Returns {clip folder: (first, last) blurry centre of any window}, in arena order."""
        self.paths, self.index = [], {}
        spans = {}
        for win in window_list:
            d, a, b = os.path.dirname(win[0][0]), frame_number(win[0][0]), frame_number(win[0][-1])
            lo, hi = spans.get(d, (a, b))
            spans[d] = (min(lo, a), max(hi, b))
        self.clip_ranges = np.empty((len(spans), 2), dtype=np.int64)
        for c, (d, (lo, hi)) in enumerate(spans.items()):
            clip = [os.path.join(d, str(k).zfill(5) + ".png") for k in range(lo - blur_half, hi + blur_half + 1)]
            self.clip_ranges[c] = (len(self.paths), len(self.paths) + len(clip))
            self.index.update((p, len(self.paths) + j) for j, p in enumerate(clip))
            self.paths += clip
        return spans

    def _fill(self, threads):
        """Decode into two pinned buffers in turn; each chunk's copy to the arena overlaps the next chunk's decoding."""
        n, h, w, _ = self.shape
        per = max(1, min(n, CHUNK_BYTES // (h * w * 3)))
        bufs = [torch.empty((per, h, w, 3), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        done = [None, None]

        def load(arg):
            buf, j, path = arg
            buf[j] = imread_u8(path)[:, :, :3]

        with torch.cuda.device(self.device), cf.ThreadPoolExecutor(threads) as pool:
            for k, start in enumerate(range(0, n, per)):
                m = min(per, n - start)
                buf = bufs[k % 2]
                if done[k % 2] is not None:
                    done[k % 2].synchronize()              # that buffer's previous copy has landed
                list(pool.map(load, [(buf.numpy(), j, self.paths[start + j]) for j in range(m)]))
                self.frames[start:start + m].copy_(buf[:m], non_blocking=True)
                done[k % 2] = torch.cuda.Event()
                done[k % 2].record()
            torch.cuda.current_stream().synchronize()

    def table(self, windows, draws, halves=None, keys=None):
        """window_table of these windows against this arena."""
        return window_table(windows, draws, self.index, halves, keys)


def window_table(windows, draws, index, halves=None, keys=None):
    """int32 [len(windows), 17 + 3] rows of binhip_gather_windows: the arena ids (`index`: path -> id) of each window's frames
    in slot order, a reversed window's in reverse order, then y0, x0, flip.  `draws`: one (reverse, y0, x0, flip) per window
    (draw_window_aug).  With `halves` (one half range h per window, draw_blur_half) the rows are binhip_gather_windows_blur's:
    [len(windows), 17 + 4], h last, the blurry ids being those of the centre sharp frames.  With `keys` as well (one (k0, k1) per
    window, exposure.sample_key) they are binexpose_gather's: [len(windows), 17 + 6], the 32 bits of k0 and k1 last."""
    extra = 3 if halves is None else 4 if keys is None else 6
    rows = np.empty((len(windows), N_SLOTS + extra), dtype=np.int32)
    for r, (win, (reverse, y0, x0, flip)) in enumerate(zip(windows, draws)):
        rows[r, :N_SLOTS] = [index[p] for p in window_slots(win, reverse)]
        rows[r, N_SLOTS:N_SLOTS + 3] = (y0, x0, int(flip))
    if halves is not None:
        rows[:, N_SLOTS + 3] = halves
    if keys is not None:
        rows[:, N_SLOTS + 4:] = np.array(keys, dtype=np.uint32).reshape(-1, 2).view(np.int32)
    return rows


class DeviceWindowLoader:
    """The training DataLoader of a BINDataset, served from a DeviceFrameCache: `len` batches, each a dict
    {"LQs", "GTenh", "GTinp", "key"} with device tensors [B, 6 | 6 | 5, 3, ch, cw] and the list of window keys.  As the
    host loader: indices from `sampler` (DistIterSampler) or in order, the ragged last batch dropped, `batch` samples per
    batch (data._train_loader_shape); the draws are made here, in the main process, in the order the host loader at
    n_workers 0 makes them."""

    def __init__(self, dataset, batch, sampler=None, device=None, max_gb=64, cache=None):
        self.dataset, self.batch, self.sampler = dataset, int(batch), sampler
        self.crop = tuple(dataset.input_frame_size)
        self.blur_window = getattr(dataset, "blur_window", None)
        self.exposure, self.train = getattr(dataset, "exposure", None), getattr(dataset, "train", True)
        blur_half = None if self.blur_window is None else blur_half_max(self.blur_window)
        from_clips = getattr(dataset, "make_device_cache", None)   # mode BIN_video (video_dataset.py): the frames come from its clips
        if cache is None:
            cache = from_clips(device, max_gb) if from_clips else DeviceFrameCache(dataset.all_paths, device, max_gb, blur_half=blur_half)
        self.cache = cache
        # crop offsets are drawn against the prepared dataset's frame size, as the host loader draws them; a clip's own for BIN_video
        # (None: each window's own clip's, from a cache that holds clips of different sizes: YuvFrameCache.src_size)
        self.src_size = (SRC_H, SRC_W) if not from_clips else None if hasattr(self.cache, "src_size") else tuple(self.cache.shape[1:3])

    def _src_size(self, window):
        return self.src_size or self.cache.src_size(window)

    def _gather(self, table, launch):
        """`launch(frames, table, clip_ranges)` on the arena, or on the batch's decoded crops when the cache keeps YUV (crop_batch)."""
        if hasattr(self.cache, "crop_batch"):
            return launch(*self.cache.crop_batch(table, self.crop[1:]))
        return launch(self.cache.frames, table, self.cache.clip_ranges)

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return n // self.batch

    def index_batches(self):
        """The index lists of the batches, as the host loader's batch sampler yields them (drop_last)."""
        it = iter(self.sampler) if self.sampler is not None else iter(range(len(self.dataset)))
        while True:
            idx = [i for _, i in zip(range(self.batch), it)]
            if len(idx) < self.batch:
                return
            yield idx

    def __iter__(self):
        _, ch, cw = self.crop
        for idx in self.index_batches():
            windows = [self.dataset.all_paths[i] for i in idx]
            if self.blur_window is None:
                draws = [draw_window_aug(self.crop, src_size=self._src_size(w)) for w in windows]
                out = ops.gather_windows(self.cache.frames, self.cache.table(windows, draws), (ch, cw))
            elif self.exposure is None:                      # per sample: the four draws, then the exposure's (load_window's order)
                both = [(draw_window_aug(self.crop, src_size=self._src_size(w)), draw_blur_half(self.blur_window)) for w in windows]
                table = self.cache.table(windows, [d for d, _ in both], [h for _, h in both])
                out = self._gather(table, lambda frames, tab, ranges: ops.gather_windows_blur(frames, tab, (ch, cw), N_BLUR, ranges))
            else:                                            # ... then the key's, when there is noise (exposure.sample_key)
                from .exposure import sample_key
                three = [(draw_window_aug(self.crop, src_size=self._src_size(w)), draw_blur_half(self.blur_window),
                          sample_key(self.exposure, self.train, i)) for w, i in zip(windows, idx)]
                table = self.cache.table(windows, [d for d, _, _ in three], [h for _, h, _ in three], [k for _, _, k in three])
                curve = ops.exposure_curve(*self.exposure)
                out = self._gather(table, lambda frames, tab, ranges: ops.gather_windows_exposed(frames, tab, (ch, cw), N_BLUR, curve, ranges))
            yield {"LQs": out[0:6].transpose(0, 1), "GTenh": out[6:12].transpose(0, 1), "GTinp": out[12:17].transpose(0, 1),
                   "key": [w[3] for w in windows]}


def create_device_loader(dataset, dataset_opt, batch, sampler=None):
    """DeviceWindowLoader on the current device (each rank's own under torch.distributed)."""
    device = torch.device("cuda", torch.cuda.current_device())
    max_gb = dataset_opt.get("device_cache_max_gb") or 64
    loader = DeviceWindowLoader(dataset, batch, sampler, device, max_gb)
    logging.getLogger("base").info("Device frame cache: %d frames, %.2f GB on %s, format %s", len(loader.cache.paths),
                                   loader.cache.nbytes / 1e9, device, "yuv" if hasattr(loader.cache, "crop_batch") else "bgr")
    return loader
