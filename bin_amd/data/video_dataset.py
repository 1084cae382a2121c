"""Training from sharp high-frame-rate video (bin_amd extension, dataset mode `BIN_video`): the clips are YUV4MPEG2 files, one
240-fps clip each, and nothing else is on disk — no PNG tree, no blurry frames, no lists.

The windows are make_sharp_window_list's (BIN_dataset.py): frame index k of a clip plays the part of the file number k + 1, so a
stream of n frames gives the windows and keys a folder of 00001.png .. n.png gives.  A frame is named by the pseudo-path
`<clip.y4m>/<NNNNN>.png`, which keeps window_slots, frame_number and the cache's index as they are.  The blurry inputs are
synthesised from the sharp frames (`blur_window`, required), so the only loader is the device one (device_cache.py): the arena
(VideoFrameCache) is filled from the payloads by ops.yuv_to_bgr (libbinclip.so), nothing of a frame is converted on the host, and
every batch is the one ops.gather_windows_blur launch of the folder path (ops.gather_windows_exposed with `blur_gamma`).

With the dataset option `device_cache_format: yuv` the arena keeps the payloads as they are (YuvFrameCache: half the bytes at 4:2:0, a
fill without a kernel, clips of different sizes side by side) and each batch's crops are decoded first, by one ops.yuv_crops_to_bgr
launch (libbincrop.so) into a mini-arena that the same gather launch then reads (plan_crop_batch, YuvFrameCache.crop_batch)."""
import math
import os
import queue
import random
import threading

import numpy as np
import torch
import torch.utils.data as data

from .. import ops, video
from ..options.options import device_cache_format as cache_format
from .BIN_dataset import BLUR_FIRST_CENTRE, BLUR_STEP, NUM_WIN_PER_BUNCH, blur_half_max, exposure_options, parse_blur_window
from .device_cache import CHUNK_BYTES, N_BLUR, N_SLOTS, DeviceFrameCache

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
        self.cache_format = cache_format(opt)
        self.clips = {}                                      # file -> (header, number of frames, (chroma, matrix, range))
        first = None
        for f in clip_files(opt["dataroot_video"]):
            header, n = video.clip_info(f)
            if first is None:
                first = (f, header)
            elif self.cache_format == "yuv" and header.chroma != first[1].chroma:    # a YUV arena: the sizes travel per frame
                raise ValueError(f"mode BIN_video: the clips differ in chroma: {first[0]} is {first[1].chroma}, {f} is {header.chroma}")
            elif self.cache_format != "yuv" and \
                    (header.width, header.height, header.chroma) != (first[1].width, first[1].height, first[1].chroma):
                raise ValueError(f"mode BIN_video: the clips differ: {first[0]} is {first[1].width}x{first[1].height} {first[1].chroma}, "
                                 f"{f} is {header.width}x{header.height} {header.chroma}")
            self.clips[f] = (header, n, video.resolve_format(header, matrix, rng))
        self.frame_size = (first[1].height, first[1].width)  # the first clip's; with device_cache_format: yuv the others may differ
        _, ch, cw = self.input_frame_size
        for f, (header, _, _) in self.clips.items():
            if ch > header.height or cw > header.width:
                raise ValueError(f"mode BIN_video: LQ_size asks for a {cw}x{ch} crop of {header.width}x{header.height} frames ({f})")
        self.all_paths, _ = make_clip_window_list([(f, n) for f, (_, n, _) in self.clips.items()], blur_window=self.blur_window)

    def __len__(self):
        return len(self.all_paths)

    def __getitem__(self, index):
        raise ValueError(NO_HOST_LOADER)

    def make_device_cache(self, device, max_gb=64):
        """The arena DeviceWindowLoader serves this dataset from: BGR frames, or the payloads themselves (`device_cache_format: yuv`)."""
        return (YuvFrameCache if self.cache_format == "yuv" else VideoFrameCache)(self, device, max_gb)


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
        chunks = [(clip, skip, n, frame_bytes, stride) for clip, _, skip, _, n in plan]
        per = max(_chunk_frames(n, stride) for *_, n in plan)
        with torch.cuda.device(self.device):
            dev = [torch.empty((per, stride), dtype=torch.uint8, device=self.device) for _ in range(2)]

            def convert(b, rows, i, at, m):
                """Each chunk is uploaded and converted by one launch straight into its arena slice."""
                _, fmt, _, start, _ = plan[i]
                dev[b][:m].copy_(rows, non_blocking=True)
                ops.yuv_to_bgr(dev[b][:m], h, w, fmt, out=self.frames[start + at:start + at + m])
            _stream_clips(chunks, self.device, convert)


def plan_crop_batch(table, frame_offset, frame_h, frame_w, frame_format, clip_ranges):
    """What YuvFrameCache.crop_batch decodes for a batch and how the batch's table reads the result; host arithmetic on numpy arrays.
    `table`: window_table's rows with h (int [n, 17 + 4] or [n, 17 + 6]), ids being arena ids; `frame_*`: per arena id the payload's
    byte offset, the frame's H and W and its format index; `clip_ranges`: int [clips, 2].  Per sample the span of arena ids from its
    first blurry centre - h to its last + h (every slot of a window lies inside it) is decoded at the sample's (y0, x0), the spans
    packed one after the other in table order.  Returns (rows, table, ranges):
      rows   int64 [frames, 6], ops.yuv_crops_to_bgr's table: frame k of the mini-arena;
      table  the input with the ids made local to the mini-arena, y0 = x0 = 0, flip, h and the keys kept;
      ranges int64 [n, 2], each sample's [start, end) block of the mini-arena, which plays the part of its clip.
    Raises ValueError when a span leaves the arena or its clip."""
    tab = np.asarray(table)
    if tab.ndim != 2 or tab.shape[0] < 1 or tab.shape[1] not in (N_SLOTS + 4, N_SLOTS + 6):
        raise ValueError(f"plan_crop_batch: table must be [n, {N_SLOTS} + 4] or [n, {N_SLOTS} + 6], got {tab.shape}")
    ids, y0, x0, half = tab[:, :N_SLOTS].astype(np.int64), tab[:, N_SLOTS], tab[:, N_SLOTS + 1], tab[:, N_SLOTS + 3].astype(np.int64)
    lo = np.minimum(ids[:, :N_BLUR].min(axis=1) - half, ids.min(axis=1))
    hi = np.maximum(ids[:, :N_BLUR].max(axis=1) + half, ids.max(axis=1))
    cr = np.asarray(clip_ranges, dtype=np.int64).reshape(-1, 2)
    cr = cr[np.argsort(cr[:, 0])]
    clip = np.searchsorted(cr[:, 0], lo, side="right") - 1   # the clip that holds the first frame of the span
    if half.min() < 0 or lo.min() < 0 or hi.max() >= len(frame_offset) or (clip < 0).any() or (hi >= cr[np.maximum(clip, 0), 1]).any():
        raise ValueError("plan_crop_batch: a sample's span, first blurry centre - h .. last + h, leaves the arena or crosses a clip boundary")
    count = hi - lo + 1
    end = np.cumsum(count)
    start = end - count
    fid = np.repeat(lo - start, count) + np.arange(end[-1])  # the arena id behind each frame of the mini-arena
    rows = np.stack([np.asarray(frame_offset, dtype=np.int64)[fid], np.asarray(frame_h, dtype=np.int64)[fid],
                     np.asarray(frame_w, dtype=np.int64)[fid], np.repeat(y0, count).astype(np.int64),
                     np.repeat(x0, count).astype(np.int64), np.asarray(frame_format, dtype=np.int64)[fid]], axis=1)
    local = tab.copy()
    local[:, :N_SLOTS] = ids - (lo - start)[:, None]
    local[:, N_SLOTS:N_SLOTS + 2] = 0
    return rows, local, np.stack([start, end], axis=1)


class YuvFrameCache(DeviceFrameCache):
    """The device frame cache of a VideoClipDataset kept as it arrives (`device_cache_format: yuv`): one flat uint8 arena that holds the
    Y4M payloads of the frames VideoFrameCache would hold, under the same arena ids (`paths`, `index`, `clip_ranges`), each at its
    clip's stride (the frame bytes rounded up to 16).  At 4:2:0 that is half the bytes of the BGR arena, and a frame's size and format
    are per-frame facts (`frame_offset`, `frame_h`, `frame_w`, `frame_format`, host arrays by arena id), so the clips may differ in
    size, matrix and range.  The fill is the reader thread and the two page-locked buffers of VideoFrameCache with one upload per
    chunk straight into the arena: no kernel runs.  Each batch's crops are decoded by one ops.yuv_crops_to_bgr launch (crop_batch) into
    a mini-arena on which ops.gather_windows_blur / ops.gather_windows_exposed run as they are.  Raises ValueError before allocating
    anything when the arena would exceed `max_gb` (10^9 bytes)."""

    def __init__(self, dataset, device, max_gb=64):
        half = blur_half_max(dataset.blur_window)
        spans = self._index_spans(dataset.all_paths, half)
        if not self.paths:
            raise ValueError("DeviceFrameCache: the window list is empty")
        n = len(self.paths)
        self.chroma = next(iter(dataset.clips.values()))[2][0]
        self.frame_offset, self.frame_h, self.frame_w, self.frame_format = (np.empty(n, dtype=np.int64) for _ in range(4))
        chunks, at = [], 0
        for (clip, (lo, _)), (start, end) in zip(spans.items(), self.clip_ranges):
            header, _, fmt = dataset.clips[clip]
            frame_bytes = ops.yuv_frame_bytes(header.height, header.width, fmt[0])[0]
            stride = -(-frame_bytes // STAGING_ALIGN) * STAGING_ALIGN
            self.frame_offset[start:end] = at + stride * np.arange(end - start)
            self.frame_h[start:end], self.frame_w[start:end] = header.height, header.width
            self.frame_format[start:end] = ops.yuv_format_index(fmt)
            # (clip, 0-based index of its first cached frame, frames, frame bytes, stride), and where its first payload goes
            chunks.append(((clip, lo - half - 1, int(end - start), frame_bytes, stride), at))
            at += stride * int(end - start)
        self.nbytes = at
        if self.nbytes > max_gb * 1e9:
            raise ValueError(f"DeviceFrameCache: {n} YUV {self.chroma} frames need {self.nbytes / 1e9:.2f} GB ({self.nbytes} bytes), "
                             f"more than device_cache_max_gb = {max_gb}")
        self.device = torch.device(device)
        self.arena = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        self._mini = None                                    # crop_batch's buffer
        self._span_max = (N_BLUR - 1) * BLUR_STEP + 1 + 2 * half   # frames from a window's first blurry centre - h to its last + h

        def upload(b, rows, i, first, m):
            """Each chunk is one upload straight into the arena, pad bytes and all (they are never read)."""
            (_, _, _, _, stride), base = chunks[i]
            self.arena[base + first * stride:base + (first + m) * stride].view(m, stride).copy_(rows, non_blocking=True)
        _stream_clips([c for c, _ in chunks], self.device, upload)

    def src_size(self, window):
        """(H, W) of the clip the window is cut from: what its crop offsets are drawn against."""
        k = self.index[window[0][0]]
        return int(self.frame_h[k]), int(self.frame_w[k])

    def crop_batch(self, table, crop):
        """One decode launch for the batch `table` (window_table's rows with h): returns (mini-arena uint8 [frames, ch, cw, 3], the
        table remapped onto it, one [start, end) range per sample), the arguments of ops.gather_windows_blur / _exposed."""
        ch, cw = (int(v) for v in crop)
        rows, local, ranges = plan_crop_batch(table, self.frame_offset, self.frame_h, self.frame_w, self.frame_format, self.clip_ranges)
        need = len(local) * self._span_max                   # what a batch of this many samples can ask for: allocated once per loader
        if self._mini is None or self._mini.shape[0] < need or tuple(self._mini.shape[1:3]) != (ch, cw):
            self._mini = torch.empty((need, ch, cw, 3), dtype=torch.uint8, device=self.device)
        mini = ops.yuv_crops_to_bgr(self.arena, rows, (ch, cw), self.chroma, out=self._mini[:len(rows)])
        return mini, local, ranges


def _chunk_frames(n, stride):
    """Frames per chunk of a clip of n cached frames at `stride` bytes each: what a page-locked buffer of CHUNK_BYTES holds."""
    return max(1, min(n, CHUNK_BYTES // stride))


def _stream_clips(chunks, device, consume):
    """The payloads of `chunks`, (clip, frames to skip, frames to take, frame bytes, staging stride) per clip in arena order, through two
    page-locked buffers in turn: a reader thread reads the next chunk while `consume(buffer index, rows, clip index, first frame of the
    chunk, frames)` enqueues the upload of this one on the current stream of `device` (`rows`: page-locked uint8 [frames, stride], a
    payload at the start of each row; the rest of a row is whatever the buffer held).  Returns once everything enqueued has finished."""
    size = max(_chunk_frames(n, stride) * stride for _, _, n, _, stride in chunks)
    host = [torch.empty(size, dtype=torch.uint8, pin_memory=True) for _ in range(2)]
    free, filled = queue.Queue(), queue.Queue()

    def read():
        """Every chunk of every clip in arena order: (buffer, clip index, first frame, frames), then None; an exception goes to the
        consumer."""
        try:
            for i, (clip, skip, n, frame_bytes, stride) in enumerate(chunks):
                scratch = bytearray(frame_bytes)
                per = _chunk_frames(n, stride)
                with video.Y4MReader(clip) as rd:
                    for _ in range(skip):                    # the frames before the first exposure: read and dropped
                        if not rd.readinto(scratch):
                            raise ValueError(f"{clip} ends at frame {rd.index}")
                    for at in range(0, n, per):
                        b = free.get()
                        if b is None:
                            return
                        m = min(per, n - at)
                        rows = host[b].numpy()[:m * stride].reshape(m, stride)
                        for j in range(m):
                            if not rd.readinto(rows[j, :frame_bytes]):
                                raise ValueError(f"{clip} ends at frame {rd.index}: {skip + n} were counted")
                        filled.put((b, i, at, m))
            filled.put(None)
        except BaseException as e:                           # noqa: B902 (handed over, raised by the consumer)
            filled.put(e)

    free.put(0)
    free.put(1)
    reader = threading.Thread(target=read, name="clip-reader", daemon=True)
    reader.start()
    try:
        with torch.cuda.device(device):
            last = None                                      # (buffer, event behind its upload) of the previous chunk
            while True:
                item = filled.get()
                if item is None:
                    break
                if isinstance(item, BaseException):
                    raise item
                b, i, at, m = item
                stride = chunks[i][4]
                consume(b, host[b][:m * stride].view(m, stride), i, at, m)
                done = torch.cuda.Event()
                done.record()
                if last is not None:                         # the previous chunk has left its page-locked buffer: read into it again
                    last[1].synchronize()
                    free.put(last[0])
                last = (b, done)
            torch.cuda.current_stream().synchronize()
    finally:
        free.put(None)
        free.put(None)
        reader.join()
