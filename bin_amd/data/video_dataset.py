"""Training from sharp high-frame-rate video (bin_amd extension, dataset mode `BIN_video`): the clips are YUV4MPEG2 files, one
240-fps clip each, and nothing else is on disk — no PNG tree, no blurry frames, no lists.

The windows are make_sharp_window_list's (BIN_dataset.py): frame index k of a clip plays the part of the file number k + 1, so a
stream of n frames gives the windows and keys a folder of 00001.png .. n.png gives.  A frame is named by the pseudo-path
`<clip.y4m>/<NNNNN>.png`, which keeps window_slots, frame_number and the cache's index as they are.  The blurry inputs are
synthesised from the sharp frames (`blur_window`, required), so the only loader is the device one (device_cache.py): the arena
(VideoFrameCache) is filled from the payloads by ops.yuv_to_bgr (libbinclip.so), nothing of a frame is converted on the host, and
every batch is the one ops.gather_windows_blur launch of the folder path (ops.gather_windows_exposed with `blur_gamma`)."""
import math
import os
import queue
import random
import threading

import torch
import torch.utils.data as data

from .. import ops, video
from .BIN_dataset import BLUR_FIRST_CENTRE, BLUR_STEP, NUM_WIN_PER_BUNCH, blur_half_max, exposure_options, parse_blur_window
from .device_cache import CHUNK_BYTES, DeviceFrameCache

NO_HOST_LOADER = ("mode BIN_video: there is no host loader for video clips; the batches are cut out of the device frame cache: "
                  "set `device_cache: true` for this dataset")
STAGING_ALIGN = 16               # a staged payload row starts at a multiple of this, so ops.yuv_to_bgr moves dwords


def frame_path(clip, number):
    """The pseudo-path of frame `number` (counted from 1, as the files of a prepared clip are) of the clip file `clip`."""
    return os.path.join(clip, str(number).zfill(5) + ".png")


def clip_key(clip):
    name = os.path.basename(clip)
    return name[:-4] if name.lower().endswith(".y4m") else name


def clip_files(root):
    """The clips of `dataroot_video`: a list of files as it is, or the *.y4m files of a folder in sorted name order."""
    if isinstance(root, (list, tuple)):
        files = [os.path.expanduser(str(f)) for f in root]
    else:
        root = os.path.expanduser(str(root))
        files = [os.path.join(root, f) for f in sorted(os.listdir(root)) if f.lower().endswith(".y4m")]
    if not files:
        raise ValueError(f"mode BIN_video: no *.y4m clip in dataroot_video = {root!r}")
    return files


def make_clip_window_list(clips, split=100, shuffle=True, blur_window=11):
    """make_sharp_window_list over `clips`, (file, number of frames) pairs, instead of the folders of <root>/<mode>/: the script's
    rule with the first file number 1, one shuffle over the whole list, then the split."""
    h = blur_half_max(parse_blur_window(blur_window))
    windows = []
    for clip, n in clips:
        centres = [1 + BLUR_FIRST_CENTRE + BLUR_STEP * i for i in range(n // BLUR_STEP - 2)]
        usable = {c for c in centres if c - h >= 1 and c + h <= n}
        for win in range(len(centres) - NUM_WIN_PER_BUNCH - 1):
            cs = centres[win:win + 6]
            if not all(c in usable for c in cs):
                continue
            sharp = [frame_path(clip, c) for c in cs]
            windows.append([list(sharp), sharp, [frame_path(clip, c + BLUR_STEP // 2) for c in cs[:5]],
                            clip_key(clip) + "_" + str(cs[0]).zfill(5)])
    if shuffle:
        random.shuffle(windows)
    keep = int(math.floor(len(windows) * split / 100.0))
    return windows[:keep], windows[keep:]


class VideoClipDataset(data.Dataset):
    """The windows of the sharp Y4M clips of `dataroot_video`.  Everything is checked from the headers and the file sizes, before any
    device call: the clips agree in W, H and chroma, the frames hold the crop, `blur_window` is there."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        self.input_frame_size = tuple(opt["LQ_size"])
        self.blur_window = parse_blur_window(opt.get("blur_window"))
        if self.blur_window is None:
            raise ValueError("mode BIN_video: `blur_window` is required: the clips hold sharp frames only, the blurry inputs are "
                             "averaged from them")
        self.exposure = exposure_options(opt, self.blur_window)   # blur_gamma, blur_noise: exposures in linear light (exposure.py)
        self.train = opt.get("phase", "train") == "train"
        if opt.get("dataroot_video") is None:
            raise ValueError("mode BIN_video: `dataroot_video` (a folder of *.y4m clips, or a list of files) is required")
        matrix, rng = opt.get("yuv_matrix") or "auto", opt.get("yuv_range") or "auto"
        self.clips = {}                                      # file -> (header, number of frames, (chroma, matrix, range))
        first = None
        for f in clip_files(opt["dataroot_video"]):
            header, n = video.clip_info(f)
            if first is None:
                first = (f, header)
            elif (header.width, header.height, header.chroma) != (first[1].width, first[1].height, first[1].chroma):
                raise ValueError(f"mode BIN_video: the clips differ: {first[0]} is {first[1].width}x{first[1].height} {first[1].chroma}, "
                                 f"{f} is {header.width}x{header.height} {header.chroma}")
            self.clips[f] = (header, n, video.resolve_format(header, matrix, rng))
        self.frame_size = (first[1].height, first[1].width)
        _, ch, cw = self.input_frame_size
        if ch > self.frame_size[0] or cw > self.frame_size[1]:
            raise ValueError(f"mode BIN_video: LQ_size asks for a {cw}x{ch} crop of {self.frame_size[1]}x{self.frame_size[0]} frames ({first[0]})")
        self.all_paths, _ = make_clip_window_list([(f, n) for f, (_, n, _) in self.clips.items()], blur_window=self.blur_window)

    def __len__(self):
        return len(self.all_paths)

    def __getitem__(self, index):
        raise ValueError(NO_HOST_LOADER)

    def make_device_cache(self, device, max_gb=64):
        """The arena DeviceWindowLoader serves this dataset from."""
        return VideoFrameCache(self, device, max_gb)


class VideoFrameCache(DeviceFrameCache):
    """DeviceFrameCache whose frames come from the clips of a VideoClipDataset: per clip the span from its first used centre - h to
    its last + h, consecutively, so `clip_ranges`, window_table and ops.gather_windows_blur are used as they are.  A reader thread
    takes the payloads into two page-locked staging buffers in turn; each chunk is uploaded and converted by one ops.yuv_to_bgr
    launch straight into its arena slice while the next one is read.  Raises ValueError before allocating anything when the arena
    would exceed `max_gb` (10^9 bytes)."""

    def __init__(self, dataset, device, max_gb=64):
        half = blur_half_max(dataset.blur_window)
        spans = self._index_spans(dataset.all_paths, half)
        if not self.paths:
            raise ValueError("DeviceFrameCache: the window list is empty")
        h, w = dataset.frame_size
        self.shape = (len(self.paths), h, w, 3)
        self.nbytes = len(self.paths) * h * w * 3
        if self.nbytes > max_gb * 1e9:
            raise ValueError(f"DeviceFrameCache: {len(self.paths)} frames of {h}x{w}x3 need {self.nbytes / 1e9:.2f} GB ({self.nbytes} bytes), "
                             f"more than device_cache_max_gb = {max_gb}")
        self.device = torch.device(device)
        self.frames = torch.empty(self.shape, dtype=torch.uint8, device=self.device)
        # (clip, its format, 0-based index of its first cached frame, arena id of that frame, frames)
        self._fill([(clip, dataset.clips[clip][2], lo - half - 1, int(start), int(end - start))
                    for (clip, (lo, _)), (start, end) in zip(spans.items(), self.clip_ranges)])

    def _fill(self, plan):
        _, h, w, _ = self.shape
        frame_bytes = ops.yuv_frame_bytes(h, w, plan[0][1][0])[0]
        stride = -(-frame_bytes // STAGING_ALIGN) * STAGING_ALIGN
        per = max(1, min(max(n for *_, n in plan), CHUNK_BYTES // stride))
        host = [torch.empty((per, stride), dtype=torch.uint8, pin_memory=True) for _ in range(2)]
        free, filled = queue.Queue(), queue.Queue()

        def read():
            """Every chunk of every clip in arena order: (buffer, format, arena id, frames), then None; an exception goes to the consumer."""
            try:
                scratch = bytearray(frame_bytes)
                for clip, fmt, skip, start, n in plan:
                    with video.Y4MReader(clip) as rd:
                        for _ in range(skip):                # the frames before the first exposure: read and dropped
                            if not rd.readinto(scratch):
                                raise ValueError(f"{clip} ends at frame {rd.index}")
                        for at in range(0, n, per):
                            b = free.get()
                            if b is None:
                                return
                            m = min(per, n - at)
                            rows = host[b].numpy()
                            for j in range(m):
                                if not rd.readinto(rows[j, :frame_bytes]):
                                    raise ValueError(f"{clip} ends at frame {rd.index}: {skip + n} were counted")
                            filled.put((b, fmt, start + at, m))
                filled.put(None)
            except BaseException as e:                       # noqa: B902 (handed over, raised by the consumer)
                filled.put(e)

        free.put(0)
        free.put(1)
        reader = threading.Thread(target=read, name="clip-reader", daemon=True)
        reader.start()
        try:
            with torch.cuda.device(self.device):
                dev = [torch.empty((per, stride), dtype=torch.uint8, device=self.device) for _ in range(2)]
                last = None                                  # (buffer, event behind its upload and conversion) of the previous chunk
                while True:
                    item = filled.get()
                    if item is None:
                        break
                    if isinstance(item, BaseException):
                        raise item
                    b, fmt, start, m = item
                    dev[b][:m].copy_(host[b][:m], non_blocking=True)
                    ops.yuv_to_bgr(dev[b][:m], h, w, fmt, out=self.frames[start:start + m])
                    done = torch.cuda.Event()
                    done.record()
                    if last is not None:                     # the previous chunk has left its page-locked buffer: read into it again
                        last[1].synchronize()
                        free.put(last[0])
                    last = (b, done)
                torch.cuda.current_stream().synchronize()
        finally:
            free.put(None)
            free.put(None)
            reader.join()
