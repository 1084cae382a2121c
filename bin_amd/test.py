"""Evaluate / run bin_stage4 over folders of blurry frames: the reference's test.py (with --gt_path: PSNR/SSIM of the
interpolated and deblurred frames against the sharp ground truth) and demo.py (without) in one entry point.

    python -m bin_amd.test --netName bin_stage4 --input_path DATA/test_blur --gt_path DATA/test \\
        --output_path OUT --opt bin_amd/options/bin_stage4_adobe240.yml [--time_step 0.5]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m bin_amd.test ... --launcher pytorch
    DECODER ... -f yuv4mpegpipe - | python -m bin_amd.test --input_video - --output_video - --opt ... | ENCODER ...

With --input_video / --output_video the frames are those of one Y4M stream (bin_amd/video.py) instead of PNG files: same windows,
same outputs, written in display order at twice the frame rate (run_video below; one rank).  --factor 4 | 8
chains passes on the fp32 outputs for four or eight times the frame rate (the same run_video: bin_amd/chain.py has the window loop
of every factor).  --output_rate N[:D] writes any frame rate up to eight times the input's: the frames of the factor's stream,
resampled on the device (bin_amd/rate.py; --resample blend | nearest).  --gt_video GT.y4m scores every written frame against the
sharp stream at the output rate or a whole multiple of it, per plane, on the device (bin_amd/score.py; --gt_offset, --score_log).

What the reference does per input frame `index` of a clip (test.py:236-402) and this keeps:
  * the six blurry frames index + [-2..3], clamped to the clip (test.py:257-261, 333);
  * replicate padding to the next multiple of 128, or 32 px per side when already one (test.py:348-366);
  * outputs Ft_p[13] -> <num+8>.png (the interpolated frame), Ft_p[8] -> <num+4>.png and, except for the last
    window, Ft_p[12] -> <num+12>.png (the deblurred frames), `num` being the frame's own file number
    (test.py:286-293, 380-402); files that already exist are not recomputed;
  * tensor -> image: clamp [0,1], x255, round, RGB->BGR uint8 (util.py:113-137), done on the device.
What is different: PNG decode/encode and the metrics run on a thread pool beside the
GPU work instead of in line; decoded frames and their padded device copies are cached across the 5-of-6 overlap of
consecutive windows; stage-1 RDN results are reused across consecutive windows (exact); and with --launcher
pytorch the flattened (clip, frame) window list is sharded contiguously over the ranks, per-rank metric sums being
combined with one all-reduce at the end."""
import argparse
import logging
import os
import queue
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import harness, ops
from .data import util as data_util
from .models import create_model
from .options import options as option
from .utils import dist_util, util
from .utils.util import AverageMeter

OUT_KEYS = (13, 8, 12)         # interpolated, first deblurred, second deblurred (test.py:380-382)
METRICS = ("interp_psnr", "interp_ssim", "interp_err", "deblur_psnr", "deblur_ssim", "blurry_psnr", "blurry_ssim",
           "interp_ssim_sk", "deblur_ssim_sk", "blurry_ssim_sk")      # *_sk: test.py's SSIM (util.compare_ssim), --metrics device


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--netName", type=str, default="bin_stage4")
    p.add_argument("--input_path", type=str, default=None, help="folder of clips (folders of PNG frames)")
    p.add_argument("--gt_path", type=str, default=None, help="sharp frames; omit for demo mode (no metrics)")
    p.add_argument("--output_path", type=str, default=None)
    p.add_argument("--input_video", type=str, default=None, help="a Y4M file, or - for stdin: instead of --input_path / --output_path")
    p.add_argument("--output_video", type=str, default=None, help="the Y4M file to write at twice the frame rate, or - for stdout")
    p.add_argument("--yuv_matrix", choices=["auto", "bt601", "bt709"], default="auto",
                   help="auto: bt709 when W >= 1280 or H > 576, else bt601")
    p.add_argument("--yuv_range", choices=["auto", "limited", "full"], default="auto",
                   help="auto: the stream's XCOLORRANGE tag, else limited")
    p.add_argument("--scene_cut", type=float, default=None, metavar="T",
                   help="--input_video: detect scene cuts (luma histogram distance >= T, bin_amd/scene.py) and interpolate within "
                        "scenes only; off by default")
    p.add_argument("--scene_cut_min_mad", type=float, default=0.0, metavar="M",
                   help="--scene_cut: a cut also needs a mean absolute luma difference >= M")
    p.add_argument("--factor", type=int, choices=[2, 4, 8], default=2,
                   help="--input_video: the output's frame rate over the input's; 4 and 8 chain passes on the fp32 outputs "
                        "(bin_amd/chain.py), every second frame of a factor's stream being the stream of half the factor")
    p.add_argument("--output_rate", type=str, default=None, metavar="N[:D]",
                   help="--input_video: the output's absolute frame rate, up to 8 times the input's (bin_amd/rate.py): the frames are "
                        "laid on the stream of the smallest factor that reaches it (--factor is then a lower bound on that grid)")
    p.add_argument("--resample", choices=["blend", "nearest"], default=None,
                   help="--output_rate: an output frame between two frames of the dense stream is their fp32 mix (blend, the default) "
                        "or the nearer one of them (nearest)")
    p.add_argument("--gt_video", type=str, default=None,
                   help="--input_video: a Y4M ground truth at the output's frame rate or a whole multiple s of it; written frame m is "
                        "scored against its frame s m + --gt_offset, per plane, on the device (bin_amd/score.py)")
    p.add_argument("--gt_offset", type=int, default=0, metavar="K", help="--gt_video: the ground-truth frame of output frame 0")
    p.add_argument("--score_log", type=str, default=None, metavar="FILE",
                   help="--gt_video: one tab-separated row per scored output frame (indices, class, the six sums, the two SSIMs)")
    p.add_argument("--gpu_id", type=str, default=None)
    p.add_argument("--time_step", type=float, default=0.5)
    p.add_argument("--opt", type=str, required=True, help="Path to option YAML file.")
    p.add_argument("--launcher", choices=["none", "pytorch"], default="none")
    p.add_argument("--precision", choices=["f16", "f16x3"], default=None)
    p.add_argument("--io_threads", type=int, default=8)
    p.add_argument("--batch", type=int, default=1, help="windows per forward (small frames: 8 fills the chip; no "
                   "cross-window stage-1 reuse when > 1)")
    p.add_argument("--no_reuse", action="store_true", help="recompute the stage-1 calls shared by consecutive windows")
    p.add_argument("--self_ensemble", type=str, default=None, metavar="G",
                   help="test-time self-ensemble over a group of the letters h (flip W), v (flip H), t (reverse time), or flipx4 "
                        "(= hv) / x8 (= hvt): every image is the mean of the 2^k oriented forwards (bin_amd/ensemble.py)")
    p.add_argument("--backend", default=None, help="torch.distributed backend for --launcher pytorch (default: nccl = "
                   "RCCL on a GPU box; gloo lets several ranks share one device)")
    p.add_argument("--manifest", action="store_true", help="each rank also writes written.rank<R>.txt under the result "
                   "folder: the files IT saved (shard-ownership audit)")
    p.add_argument("--ssim", action="store_true", help="--metrics host: also compute SSIM (numpy, seconds per 720p frame)")
    p.add_argument("--metrics", choices=["host", "device"], default="host",
                   help="where the scores are computed: host = numpy, as before; device = binhip_image_score on a stream of the "
                   "writer thread, PSNR bit-identical, SSIM always on, plus the *_ssim_sk keys (test.py's skimage SSIM)")
    args = p.parse_args(argv)
    if args.input_video is None and args.output_video is None and (args.input_path is None or args.output_path is None):
        p.error("the following arguments are required: --input_path, --output_path (or --input_video, --output_video)")
    check_args(args)
    return args


def check_args(args):
    """The folder run takes --input_path and --output_path; the video run --input_video and --output_video, and neither a ground
    truth nor several ranks.  Anything else is refused here: before the options are read or the model is built."""
    video = args.input_video is not None or args.output_video is not None
    folder = args.input_path is not None or args.output_path is not None
    if not video and (getattr(args, "scene_cut", None) is not None or getattr(args, "scene_cut_min_mad", 0.0)):
        raise ValueError("--scene_cut / --scene_cut_min_mad: scene cuts are looked for in a video only (--input_video)")
    if not video and getattr(args, "factor", 2) != 2:
        raise ValueError("--factor: passes are chained on a video only (--input_video)")
    if not video and (getattr(args, "output_rate", None) is not None or getattr(args, "resample", None) is not None):
        raise ValueError("--output_rate / --resample: a frame rate is resampled on a video only (--input_video)")
    if getattr(args, "output_rate", None) is None and getattr(args, "resample", None) is not None:
        raise ValueError("--resample goes with --output_rate")
    if getattr(args, "output_rate", None) is not None:
        from . import rate
        n, d = rate.parse_rate(args.output_rate)        # (malformed: ValueError)
        if n > 2 ** 31 - 1 or d > 2 ** 31 - 1:
            raise ValueError(f"--output_rate: {args.output_rate} does not fit a Y4M header")
        if args.input_video not in (None, "-") and os.path.isfile(args.input_video):
            from . import video                             # a file's header can be looked at now (a pipe's: run_video, once it is read)
            with open(args.input_video, "rb") as f:
                rate.Grid(video.parse_header(f.readline(video.MAX_LINE)).rate, (n, d), getattr(args, "factor", 2))
    if getattr(args, "scene_cut", None) is None and getattr(args, "scene_cut_min_mad", 0.0):
        raise ValueError("--scene_cut_min_mad goes with --scene_cut")
    gt_video, score_log, gt_offset = getattr(args, "gt_video", None), getattr(args, "score_log", None), getattr(args, "gt_offset", 0)
    if args.input_video is None and (gt_video is not None or score_log is not None):
        raise ValueError("--gt_video / --score_log: a ground-truth stream scores a video only (--input_video)")
    if score_log is not None and gt_video is None:
        raise ValueError("--score_log goes with --gt_video")
    if gt_video is None and gt_offset:
        raise ValueError("--gt_offset goes with --gt_video")
    if gt_video is not None:
        from . import score
        score.check_offset(gt_offset)
        if gt_video == "-" and args.input_video == "-":
            raise ValueError("--gt_video - together with --input_video -: stdin carries one stream")
        if all(v not in (None, "-") and os.path.isfile(v) for v in (args.input_video, gt_video)):
            from . import rate, video                       # two files: their headers can be compared now (a pipe's: run_video)
            with open(args.input_video, "rb") as f, open(gt_video, "rb") as g:
                header, gt_header = (video.parse_header(x.readline(video.MAX_LINE)) for x in (f, g))
            written = header.multiplied(getattr(args, "factor", 2))
            if getattr(args, "output_rate", None) is not None:
                written = header.at_rate(rate.Grid(header.rate, rate.parse_rate(args.output_rate), getattr(args, "factor", 2)).out_rate)
            score.align(written, gt_header, gt_offset)
    if video and folder:
        raise ValueError("give either --input_path / --output_path or --input_video / --output_video, not both kinds")
    if video:
        if args.input_video is None or args.output_video is None:
            raise ValueError("--input_video and --output_video go together")
        if args.gt_path is not None:
            raise ValueError("--gt_path: scoring a video is not supported (--input_video)")
        if args.launcher == "pytorch":
            raise ValueError("--launcher pytorch: a video is not sharded across ranks (--input_video)")


def list_windows(input_path):
    """[(clip, frame names, index)] for every window of every clip, in the reference's order."""
    wins = []
    for clip in sorted(os.listdir(input_path)):
        frames = sorted(f for f in os.listdir(os.path.join(input_path, clip)) if data_util.is_image_file(f))
        wins += [(clip, frames, i) for i in range(len(frames) - 1)]
    return wins


def output_names(frames, index):
    """(interp, first deblur, second deblur or None) file names of window `index` (test.py:286-293, 311-312, 394)."""
    num = int(frames[index][:-4])
    name = lambda n: str(n).zfill(5) + ".png"
    return name(num + 8), name(num + 4), (name(num + 12) if index < len(frames) - 2 else None)


class _Sums:
    """Thread-safe per-clip / total metric accumulators.  Values are kept per scored image (`tag`: its file name) and summed in
    name order, so the sums do not depend on the order in which the writer threads finish."""

    def __init__(self):
        self.lock = threading.Lock()
        self.values = {}                              # (clip, key) -> {tag: value}

    def add(self, clip, key, value, tag):
        with self.lock:
            self.values.setdefault((clip, key), {})[tag] = float(value)

    def _sum(self, clips):
        out = {k: [0.0, 0] for k in METRICS}
        for (clip, key), d in sorted(self.values.items()):
            if clip in clips:
                for _, v in sorted(d.items()):
                    out[key][0] += v
                    out[key][1] += 1
        return out

    @property
    def total(self):
        return self._sum({c for c, _ in self.values})

    @property
    def clips(self):
        return {c: self._sum({c}) for c in sorted({c for c, _ in self.values})}


def _score(sums, clip, kind, img_bgr, gt_path, want_ssim, tag):
    if gt_path is None or not os.path.exists(gt_path):
        return
    gt = data_util.imread_u8(gt_path)[:, :, :3]
    sums.add(clip, kind + "_psnr", util.calculate_psnr(img_bgr, gt), tag)
    if kind == "interp":
        sums.add(clip, "interp_err", np.mean(np.abs(img_bgr.astype(np.float64) - gt.astype(np.float64))), tag)
    if want_ssim:
        sums.add(clip, kind + "_ssim", util.calculate_ssim(img_bgr, gt), tag)


class _DeviceScorer:
    """--metrics device: scores an image against its GT with ops.image_scores on a stream of the calling writer thread (one per
    thread), never on the network's stream.  The GT is decoded on the thread as before; both images are uploaded from host
    memory on that stream and 32 bytes per image come back."""

    def __init__(self, dev):
        self.dev, self.local = dev, threading.local()

    def __call__(self, sums, clip, kind, img_bgr, gt_path, tag):
        if gt_path is None or not os.path.exists(gt_path):
            return
        gt = data_util.imread_u8(gt_path)[:, :, :3]
        if gt.shape != img_bgr.shape:
            raise ValueError(f"{gt_path}: GT shape {gt.shape} != output shape {img_bgr.shape}")
        with torch.cuda.device(self.dev):
            stream = getattr(self.local, "stream", None)
            if stream is None:
                stream = self.local.stream = torch.cuda.Stream(device=self.dev)
            with torch.cuda.stream(stream):
                a = torch.from_numpy(np.ascontiguousarray(img_bgr)).to(self.dev, non_blocking=True)
                b = torch.from_numpy(np.ascontiguousarray(gt)).to(self.dev, non_blocking=True)
                row = ops.image_scores(a, b).cpu().numpy()[0]
        r = util.score_row(row, img_bgr.size)
        sums.add(clip, kind + "_psnr", r["psnr"], tag)
        if kind == "interp":
            sums.add(clip, "interp_err", r["mae"], tag)
        sums.add(clip, kind + "_ssim", r["ssim"], tag)
        sums.add(clip, kind + "_ssim_sk", r["ssim_sk"], tag)


class _Uploader:
    """page-locked uint8 buffer -> device tensor on the upload stream, the compute stream waiting on the event: the launching
    thread never blocks in a copy.  A buffer goes back through `release` once its upload has finished."""

    def __init__(self, dev, stream, release):
        self.dev, self.stream, self.release, self.in_flight = dev, stream, release, []

    def __call__(self, buf):
        with torch.cuda.stream(self.stream):
            g = buf.to(self.dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        torch.cuda.current_stream(self.dev).wait_event(ev)
        g.record_stream(torch.cuda.current_stream(self.dev))
        self.in_flight.append((ev, buf))
        while self.in_flight and self.in_flight[0][0].query():
            self.release(self.in_flight.pop(0)[1])
        return g


def main(argv=None, stats=None):
    """`stats` (optional dict, filled on rank 0): windows run, wall seconds incl. all IO, net + glue seconds per window —
    what bench.py's `harness` leg reports."""
    args = parse_args(argv)
    opt = option.parse(args.opt, is_train=False)
    if args.launcher == "pytorch":
        import torch.distributed as dist
        local = int(os.environ.get("LOCAL_RANK", "0"))
        torch.cuda.set_device(local)
        if not dist.is_initialized():
            dist.init_process_group(args.backend or dist_util.default_backend())
        rank, world = dist.get_rank(), dist.get_world_size()
        opt["gpu_ids"] = [local]
    else:
        rank, world = 0, 1
        if args.gpu_id is not None:
            torch.cuda.set_device(int(args.gpu_id))
            opt["gpu_ids"] = [int(args.gpu_id)]
    opt["dist"] = False                      # inference needs no gradient sync; ranks only share the window list
    if args.precision:
        opt["network_G"]["precision"] = args.precision
    opt = option.dict_to_nonedict(opt)

    n_out = round(1 / args.time_step)
    assert n_out == 2, "bin_stage4 interpolates the middle frame (time_step 0.5), as the reference asserts"
    if args.input_video is not None:
        return run_video(args, opt, stats)
    result_root = os.path.join(args.output_path, f"{n_out * 30}fps_test_results", opt["name"])
    os.makedirs(result_root, exist_ok=True)
    if rank == 0:
        util.setup_logger("base", result_root, "test", screen=True, tofile=True)
    log = logging.getLogger("base")

    # Ramp (round 5): the window list is known before the network exists, so the decoder pool starts on the FIRST windows'
    # frames now and works while the model is constructed and its weights are laid out (into plain host arrays: the
    # page-locked staging buffers need the device context, which the main thread is about to create).
    windows = list_windows(args.input_path)
    begin, end = harness.shard_windows(len(windows), rank, world)
    pool = ThreadPoolExecutor(max_workers=max(2, args.io_threads))
    strip_pool = ThreadPoolExecutor(max_workers=max(4, args.io_threads))       # leaf tasks only (they never wait): no deadlock
    early = {}
    if begin < end:
        clip0, frames0, index0 = windows[begin]
        for ahead in range(0, 3):
            if begin + ahead < end and windows[begin + ahead][0] == clip0:
                # (the window's OWN index: list_windows need not hand out consecutive indices — advisor r05)
                for fid in harness.window_frame_ids(windows[begin + ahead][2], len(frames0)):
                    if (clip0, fid) not in early:
                        early[(clip0, fid)] = pool.submit(data_util.imread_u8, os.path.join(args.input_path, clip0, frames0[fid]))

    # ... and so do the page-locked buffers of the pipeline (a dozen decode staging images, ten 3-image output buffers):
    # hipHostMalloc costs 1-3 ms apiece, which the first ten windows used to pay in line
    stage_pool, stage_lock, pinned = [], threading.Lock(), []

    first_early = next(iter(early.values()), None)

    def preallocate():
        # best effort on a daemon thread: a failure here (unreadable first frame, no page-locked memory left) must be SAID — the
        # pipeline then allocates its buffers in line as before round 5 — not die silently with the thread (advisor r05)
        try:
            if first_early is None:
                return
            first = first_early.result()
            if first.ndim != 3 or first.shape[2] != 3:
                return
            for _ in range(12):
                buf = torch.empty(first.shape, dtype=torch.uint8, pin_memory=True)
                with stage_lock:
                    stage_pool.append(buf)
            for _ in range(10):
                pinned.append(torch.empty((3,) + tuple(first.shape), dtype=torch.uint8, pin_memory=True))
        except Exception as e:
            logging.getLogger("base").warning("bin_amd.test: pre-allocation of the page-locked buffers skipped (%s: %s)",
                                              type(e).__name__, e)
    prealloc = threading.Thread(target=preallocate, daemon=True)
    if torch.cuda.is_available():
        prealloc.start()

    model = create_model(opt)
    netG = model.netG
    netG.eval()
    dev = next(netG.parameters()).device
    net = harness.WindowRunner(netG, 1, not args.no_reuse, args.batch, args.self_ensemble)
    if net.ens[0] is not None:
        log.info("self-ensemble: group %s, M = %d forwards per window", net.ens[0].group, net.ens[0].M)
    log.info("In Data: %s | model: %s | parameters: %d | ranks: %d | stage-1 reuse: %s", args.input_path,
             opt["path"]["pretrain_model_G"], sum(p.numel() for p in netG.parameters() if p.requires_grad), world, net.reuse)

    sums = _Sums()
    device_score = _DeviceScorer(dev) if args.metrics == "device" else None

    def score(clip, kind, img_bgr, gt_path, tag):
        if device_score is not None:
            device_score(sums, clip, kind, img_bgr, gt_path, tag)
        else:
            _score(sums, clip, kind, img_bgr, gt_path, args.ssim, tag)
    copy_stream = torch.cuda.Stream(device=dev)
    decoded, frames_dev, pending = {}, {}, []
    geom = None                                        # (h, w, pads) of the current clip
    claimed = set()                                    # (`pinned`: recycled page-locked output buffers, pre-allocated above)
    cur_clip, timer = None, AverageMeter()

    # Decoded frames reach the device WITHOUT ever blocking the launching thread (round 4): a copy from pageable memory is
    # stream-ordered but host-synchronous — the host sat in it until the previous window's kernels had drained, and the GPU
    # then idled for the ~5 ms the host needs to queue the next window (steady state 0.90 of the in-HBM rate).  Now the decoder
    # thread leaves the image in a recycled page-locked buffer and the upload runs on its own stream behind an event.
    upload_stream = torch.cuda.Stream(device=dev)
    if prealloc.ident is not None:                     # (started)
        prealloc.join()

    def decode(path, ready=None):                      # (worker thread)
        img = data_util.imread_u8(path) if ready is None else ready.result()
        src = torch.from_numpy(img)
        with stage_lock:
            buf = next((b for b in stage_pool if b.shape == src.shape), None)
            if buf is not None:
                stage_pool.remove(buf)
        if buf is None:
            buf = torch.empty(src.shape, dtype=torch.uint8, pin_memory=True)
        buf.copy_(src)
        return buf

    def release(buf):
        with stage_lock:
            stage_pool.append(buf)
    upload = _Uploader(dev, upload_stream, release)

    def want(clip, frames, fid):                       # async decode, at most once per frame
        key = (clip, fid)
        if key not in decoded:
            decoded[key] = pool.submit(decode, os.path.join(args.input_path, clip, frames[fid]), early.pop(key, None))
        return decoded[key]

    def finish(job):
        """(worker thread) ONE output image of a window: wait for its D2H copy, encode + write it, score it.  One task per
        image (round 5; before: the window's three images in one task) — in steady state the pool is busy either way, but
        the LAST window's three encodes now run side by side instead of one after the other (the drain at the end of a clip)."""
        clip, name, mine, kind, img, done, blurry_path = job
        done.synchronize()
        img = img.numpy()
        if mine:
            if name.lower().endswith(".png") and img.ndim == 3 and img.shape[2] == 3:
                # DEFLATE in four bands on their own small pool (round 5): the last window of a clip waits for one band, not
                # for a whole image (util.png_bytes_striped; same pixels for any PNG reader)
                util.save_png_striped(img, os.path.join(result_root, clip, name), pool=strip_pool, strips=4)
            else:
                util.save_img(img, os.path.join(result_root, clip, name))
            with written_lock:
                written.append(os.path.join(clip, name))
        if mine or kind == "interp":               # the reference scores a deblurred frame when it writes it
            score(clip, kind, img, args.gt_path and os.path.join(args.gt_path, clip, name), name)
        if blurry_path is not None and args.gt_path:
            score(clip, "blurry", data_util.imread_u8(blurry_path)[:, :, :3], os.path.join(args.gt_path, clip, name), name)

    written, written_lock = [], threading.Lock()       # files THIS rank saved (--manifest)
    stamps = []                                        # host time at which each window's work had been queued
    group = []                                         # windows of one clip waiting to go through the net together

    def flush():
        """One forward for the windows in `group` (batched along N when there are several), then hand each window's
        three u8 images to the writer pool through a copy stream."""
        if not group:
            return
        t0 = time.time()
        (h, w), (l, r, t, b) = geom[:2], geom[2]
        results = net.run(1, [(ids, six) for _, _, _, six, _, ids in group], OUT_KEYS)
        for (clip, names, owned, _, blurry_path, _), Ft_p in zip(group, results):
            outs = torch.stack([ops.frame_to_u8(Ft_p[k], t, l, h, w) for k in OUT_KEYS])
            ready = torch.cuda.Event()
            ready.record()
            host = pinned.pop() if pinned and pinned[-1].shape == outs.shape else torch.empty(
                outs.shape, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ready)
                host.copy_(outs, non_blocking=True)
                outs.record_stream(copy_stream)
                done = torch.cuda.Event()
                done.record()
            jobs = [pool.submit(finish, (clip, name, mine, kind, host[k], done, blurry_path if k == 0 else None))
                    for k, (name, mine, kind) in enumerate(zip(names, owned, ("interp", "deblur", "deblur"))) if name is not None]
            pending.append((jobs, host))
        while len(pending) > 8 + len(group):             # bound host memory; surfaces worker exceptions
            jobs, buf = pending.pop(0)
            for job in jobs:
                job.result()
            pinned.append(buf)
        timer.update((time.time() - t0) / len(group), len(group))
        stamps.extend([time.time()] * len(group))
        group.clear()

    t_all = time.time()
    with torch.no_grad():
        for wi in range(begin, end):
            clip, frames, index = windows[wi]
            if clip != cur_clip:
                flush()
                cur_clip = clip
                decoded.clear(); frames_dev.clear()
                net.new_scene()          # the memos, the oriented frames and the per-orientation memos belong to the clip
                os.makedirs(os.path.join(result_root, clip), exist_ok=True)
            if wi == begin + 3:
                early.clear()            # the early decodes belong to the first three windows; whatever was not taken is dropped
            names = output_names(frames, index)
            clip_dir = os.path.join(result_root, clip)
            # who writes what follows from the GLOBAL window index alone, as in the serial reference loop: <num+12>
            # belongs to the window that reaches it first (its Ft_p[12]); the next window's Ft_p[8] has the same name
            # and is dropped — so a window writes its first deblurred frame only when it opens the clip.  Decided
            # without looking at the file system, two ranks on either side of a shard boundary can never both write
            # one file (the existence check below only skips work a previous run already finished).
            owned = [True, index == 0, names[2] is not None]
            owned = [mine and (clip, n) not in claimed and not os.path.exists(os.path.join(clip_dir, n))
                     for n, mine in zip(names, owned)]
            claimed.update((clip, n) for n, mine in zip(names, owned) if mine)
            if not any(owned) and not args.gt_path:
                continue
            ids = harness.window_frame_ids(index, len(frames))
            for ahead in range(1, 3 + args.batch):       # keep the decoders a few windows ahead of the GPU
                if wi + ahead < end and windows[wi + ahead][0] == clip:
                    for fid in harness.window_frame_ids(index + ahead, len(frames)):
                        want(clip, frames, fid)
            six = []
            for fid in ids:
                if fid not in frames_dev:
                    img = want(clip, frames, fid).result()
                    if img.shape[2] != 3:
                        raise RuntimeError(f"{clip}/{frames[fid]}: expected a 3-channel image")
                    geom = (img.shape[0], img.shape[1], util.pad_sizes(img.shape[0], img.shape[1]))
                    frames_dev[fid] = ops.u8_to_frame(upload(img), geom[2])
                six.append(frames_dev[fid])
            for fid in [f for f in frames_dev if f < min(ids)]:      # the windows in `group` hold their own references
                del frames_dev[fid]
                decoded.pop((clip, fid), None)
            group.append((clip, names, owned, six, os.path.join(args.input_path, clip, frames[ids[3]]), ids))
            if len(group) >= args.batch:
                flush()
        flush()
        t_loop = time.time()
        torch.cuda.current_stream(dev).synchronize()
        t_gpu = time.time()
        for jobs, _ in pending:
            for job in jobs:
                job.result()
    torch.cuda.synchronize()
    ops.check_status(dev)                 # a frame that left the fp16 storage range is an error, not a result
    wall = time.time() - t_all
    timeline = {"first_window_queued_s": round(stamps[0] - t_all, 4) if stamps else None,
                "all_windows_queued_s": round(t_loop - t_all, 4), "gpu_done_s": round(t_gpu - t_all, 4), "files_done_s": round(wall, 4)}
    pool.shutdown()
    strip_pool.shutdown()
    if args.manifest:
        with open(os.path.join(result_root, f"written.rank{rank}.txt"), "w") as f:
            f.write("".join(sorted(w + "\n" for w in written)))

    # ---- combine the ranks' sums (one small all-reduce) and report like test.py:466-502
    total = sums.total
    vec = torch.tensor([v for k in METRICS for v in total[k]] + [end - begin, wall], dtype=torch.float64)
    if world > 1:
        import torch.distributed as dist
        if dist.get_backend() != "gloo":      # nccl reduces device tensors; gloo takes the host vector as it is
            vec = vec.to(dev)
        wall_t = vec[-1:].clone()
        dist.all_reduce(vec, op=dist.ReduceOp.SUM)
        dist.all_reduce(wall_t, op=dist.ReduceOp.MAX)
        vec[-1] = wall_t[0]
        vec = vec.cpu()
    if rank == 0:
        tot = {k: (vec[2 * i].item() / max(vec[2 * i + 1].item(), 1)) for i, k in enumerate(METRICS)}
        counted = {k for i, k in enumerate(METRICS) if vec[2 * i + 1].item() > 0}
        n_win, wall = int(vec[-2].item()), vec[-1].item()
        if world == 1:
            for clip, d in sums.clips.items():
                log.info("clip %s: " % clip + " ".join(f"{k} {d[k][0] / max(d[k][1], 1):.4f}" for k in METRICS if d[k][1]))
        # the keys of the host scores are always listed (as the reference does); the *_sk keys only when they were scored
        log.info("Avg. testset " + " ".join(f"{k} {tot[k]:.4f}" for k in METRICS if k in counted or not k.endswith("_sk")))
        log.info("windows: %d  wall: %.2f s  -> %.2f interpolated frames/s (IO included); net+glue per window %.4f s",
                 n_win, wall, n_win / max(wall, 1e-9), timer.avg)
        if stats is not None:
            stats.update(windows=n_win, wall=wall, net_s_per_window=timer.avg, stamps=[t - t_all for t in stamps], timeline=timeline,
                         metrics={k: tot[k] for k in METRICS if k in counted})
    return 0


class _VideoFeed:
    """The input side of the video runner, chain.run_stream's feed.  A reader thread fills recycled page-locked payload buffers (it starts with the
    object: ahead of the model's construction, as the folder runner's decoders do); `attach(dev)` creates the upload stream once the
    device is known; `read_to(i)` uploads frames behind an event and unpacks them with ops.yuv_to_frame into `frames_dev` until
    frame i is on the device or the stream has ended (`n_frames`).  With --scene_cut, ops.luma_stats runs on the upload stream
    right behind each upload, its 264-byte record comes back through a page-locked buffer and an event of that stream, and
    `resolve_cuts()` decides every frame read so far into `cuts` (log lines name output frame `factor` x the input frame)."""

    def __init__(self, args, reader, fmt, pads, factor, log):
        self.args, self.reader, self.fmt, self.pads, self.factor, self.log = args, reader, fmt, pads, factor, log
        self.h, self.w, self.nbytes = reader.header.height, reader.header.width, reader.header.frame_bytes
        self.free_in, self.filled = queue.Queue(), queue.Queue()
        for _ in range(12):
            self.free_in.put(None)                     # allocated on first use by the reader thread
        self.frames_dev = {}
        self.n_read, self.n_frames = 0, None           # frames uploaded so far; the stream's length once its end was read
        self.scene_on = args.scene_cut is not None
        self.out_frame = lambda c: factor * c          # the output frame a cut at input frame c falls on (run_video: --output_rate)
        self.cuts, self.n_dup = [], 0                  # cut positions found so far; frames equal to the one before
        self.rec_pending, self.rec_free, self.rec_prev = {}, [], None   # frame -> (page-locked record, event); spare buffers; (sad, hist) of the frame before
        self.prev_payload, self.n_resolved = None, 0   # kept alive until the next frame's statistics are queued; frames decided so far
        threading.Thread(target=self._read_frames, daemon=True).start()

    def _read_frames(self):                            # (reader thread)
        try:
            while True:
                buf = self.free_in.get()
                if buf is None:
                    buf = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
                if not self.reader.readinto(buf.numpy()):
                    break
                self.filled.put(buf)
            self.filled.put(None)
        except BaseException as e:                     # handed to the main thread, which raises it
            self.filled.put(e)

    def attach(self, dev):
        self.upload_stream = torch.cuda.Stream(device=dev)
        self.upload = _Uploader(dev, self.upload_stream, self.free_in.put)   # finished uploads hand their buffer back to the reader

    def _queue_stats(self, i, g):
        """Frame i's statistics on the upload stream, behind its upload; the record goes to page-locked memory behind an event."""
        h, w = self.h, self.w
        with torch.cuda.stream(self.upload_stream):
            rec = ops.luma_stats(g[:h * w], None if self.prev_payload is None else self.prev_payload[:h * w], h, w)
            host = self.rec_free.pop() if self.rec_free else torch.empty(ops.LUMA_RECORD_BYTES, dtype=torch.uint8, pin_memory=True)
            host.copy_(rec, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.rec_pending[i] = (host, ev)
        self.prev_payload = g

    def resolve_cuts(self):
        """Decide every frame whose statistics were queued (waits on the upload stream's events only)."""
        from . import scene
        h, w, args = self.h, self.w, self.args
        while self.n_resolved < self.n_read:
            host, ev = self.rec_pending.pop(self.n_resolved)
            ev.synchronize()
            rec = ops.read_luma_record(host)
            self.rec_free.append(host)
            if self.n_resolved > 0:
                self.n_dup += scene.is_duplicate(rec)
                if scene.is_cut(self.rec_prev, rec, h, w, args.scene_cut, args.scene_cut_min_mad):
                    self.cuts.append(self.n_resolved)
                    self.log.info("scene cut at input frame %d (output frame %d): distance %.4f, mean |dY| %.3f", self.n_resolved,
                                  self.out_frame(self.n_resolved), scene.distance(self.rec_prev[1], rec[1], h, w), rec[0] / float(h * w))
            self.rec_prev = rec
            self.n_resolved += 1

    def read_to(self, i):
        """Take frames from the reader until frame `i` is on the device or the stream has ended."""
        while self.n_frames is None and self.n_read <= i:
            item = self.filled.get()
            if item is None:
                self.n_frames = self.n_read
            elif isinstance(item, BaseException):
                raise item
            else:
                g = self.upload(item)
                if self.scene_on:
                    self._queue_stats(self.n_read, g)
                self.frames_dev[self.n_read] = ops.yuv_to_frame(g, self.h, self.w, self.fmt, self.pads)
                self.n_read += 1


class _GtFeed:
    """The ground-truth side of a scored video run (--gt_video), modelled on _VideoFeed.  A reader thread reads the stream in order
    and hands over the frames offset, offset + s, offset + 2 s, ...: the frames the stride skips are read into the same recycled
    page-locked buffer and go nowhere, and the thread never reads past the frame it hands over next.  The buffers are few and the
    queue is bounded, so the ground truth never runs ahead of the output by more than that.  `take()` (main thread) gives the next
    wanted frame as a device payload, uploaded on the upload stream behind an event the compute stream waits on, or None once the
    ground truth has ended; the page-locked buffer goes back to the reader when its upload has finished."""
    BUFFERS = 6

    def __init__(self, reader, stride, offset):
        self.reader, self.stride, self.offset, self.nbytes = reader, stride, offset, reader.header.frame_bytes
        self.free_in, self.filled = queue.Queue(), queue.Queue(maxsize=self.BUFFERS)
        for _ in range(self.BUFFERS):
            self.free_in.put(None)                     # allocated on first use by the reader thread
        self.ended, self.n_taken = False, 0
        threading.Thread(target=self._read_frames, daemon=True).start()

    def _read_frames(self):                            # (reader thread)
        try:
            index, wanted, buf = 0, self.offset, None
            while True:
                if buf is None:
                    buf = self.free_in.get()
                    if buf is None:
                        buf = torch.empty(self.nbytes, dtype=torch.uint8, pin_memory=True)
                if not self.reader.readinto(buf.numpy()):
                    break
                if index == wanted:
                    self.filled.put(buf)
                    buf, wanted = None, wanted + self.stride
                index += 1                             # (a skipped frame: the next read overwrites it)
            self.filled.put(None)
        except BaseException as e:                     # handed to the main thread, which raises it
            self.filled.put(e)

    def attach(self, dev, upload_stream):
        self.upload = _Uploader(dev, upload_stream, self.free_in.put)

    def take(self):
        if self.ended:
            return None
        while True:
            try:
                item = self.filled.get_nowait()
                break
            except queue.Empty:
                if not self.upload.in_flight:          # the reader is at work: wait for it
                    item = self.filled.get()
                    break
                ev, buf = self.upload.in_flight.pop(0)  # it may be waiting for a buffer: the oldest upload's (the upload stream only)
                ev.synchronize()
                self.free_in.put(buf)
        if item is None:
            self.ended = True
            return None
        if isinstance(item, BaseException):
            raise item
        self.n_taken += 1
        return self.upload(item)


class _VideoScorer:
    """_VideoWriter's scorer (--gt_video): called with (pos, row, is_hold) right after output frame `pos` was packed into `row` of
    the staging tensor, so the scored bytes are the bytes that get written.  ops.payload_scores runs on the compute stream against
    the frame _GtFeed hands over, into a slot of a device ring of 64-byte records; `flush` (hand_over's, on the copy stream behind
    the event it waits on anyway) copies the new slots to a page-locked ring allocated once, behind an event, and `collect` reads
    the records whose event has completed (`wait=True`: all of them, at the end of the run).  The compute stream is never
    synchronised for it and nothing is allocated while the stream runs."""
    RING = 256

    def __init__(self, gt, plan, header, dev):
        from . import score
        self.gt, self.plan, self.dev = gt, plan, dev
        self.h, self.w, self.chroma = header.height, header.width, header.chroma
        ch, cw = header.chroma_size
        self.tally = score.Tally(self.h * self.w, ch * cw)
        self.dev_recs = torch.empty((self.RING, ops.PLANE_SCORES_BYTES), dtype=torch.uint8, device=dev)
        self.host_recs = torch.empty((self.RING, ops.PLANE_SCORES_BYTES), dtype=torch.uint8, pin_memory=True)
        self.pending, self.n_scored = [], 0            # [pos, gt index, class, slot, event or None]; records made so far

    def __call__(self, pos, row, is_hold):
        truth = self.gt.take()
        if truth is None:
            self.tally.no_gt()
            return
        if len(self.pending) == self.RING:             # (more frames between two hand-overs than the ring has slots)
            self.flush()
            self.collect(wait=True)
        slot = self.n_scored % self.RING
        ops.payload_scores(row, truth, self.h, self.w, self.chroma, ssim=min(self.h, self.w) >= 7, out=self.dev_recs[slot])
        self.pending.append([pos, self.plan.gt_index(pos), self.plan.frame_class(pos, is_hold), slot, None])
        self.n_scored += 1

    def flush(self):
        """The records made since the last flush -> page-locked memory, on the current stream, which must be behind their kernels."""
        new = [e for e in self.pending if e[4] is None]
        if not new:
            return
        first, count = new[0][3], len(new)             # consecutive slots of the ring: one copy, or two where they wrap
        for lo, hi in ((first, min(first + count, self.RING)), (0, first + count - self.RING)):
            if hi > lo:
                self.host_recs[lo:hi].copy_(self.dev_recs[lo:hi], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        for e in new:
            e[4] = ev

    def collect(self, wait=False):
        if wait:
            self.flush()
        while self.pending and self.pending[0][4] is not None and (wait or self.pending[0][4].query()):
            pos, index, cls, slot, ev = self.pending.pop(0)
            ev.synchronize()
            self.tally.add((pos, index, cls) + ops.read_plane_scores(self.host_recs[slot]))


class _VideoWriter:
    """The output side of the video runner.  `emit` (chain.Chain's) packs each frame with ops.frame_to_yuv straight into a row of a
    [3, frame_bytes] device staging tensor (a hold copies the row before it), `emit_at_rate` (rate.Resampler's) likewise with
    ops.blend_to_yuv where two frames are mixed; `hand_over` sends what was staged to page-locked memory
    on the copy stream and to the ONE writer thread: jobs (page-locked [3, frame_bytes] buffer, rows to write, event after which they
    are complete) are written first in, first out, which is display order; buffers come back through `free_out`.  An error of the
    thread is kept in `error` (it keeps draining, so that the main thread never blocks on a dead writer) and raised by hand_over.
    `scorer` (optional, --gt_video): called with (pos, row, is_hold) right after a row is packed; at every hand_over its new records
    go to page-locked memory on the copy stream (`flush`) and it is asked to `collect` what has completed."""

    def __init__(self, target, out_header, fmt, pads, dev, scorer=None):
        from . import video
        self.header, self.fmt, self.pads, self.dev, self.scorer = out_header, fmt, pads, dev, scorer
        self.copy_stream = torch.cuda.Stream(device=dev)
        self.staged, self.last_row, self.n_written = [], None, 0      # [device staging tensor, rows filled]; the row packed last
        self.to_write, self.free_out, self.error = queue.Queue(maxsize=10), [], []

        def write_frames():
            writer = None
            while True:
                job = self.to_write.get()
                if job is None:
                    break
                if self.error:
                    continue
                try:
                    if writer is None:
                        writer = video.Y4MWriter(target, out_header)
                    host, n, done = job
                    done.synchronize()
                    for k in range(n):
                        writer.write(host[k].numpy())
                    self.free_out.append(host)
                except BaseException as e:
                    self.error.append(e)
            if writer is not None and not self.error:
                writer.close()
        self.thread = threading.Thread(target=write_frames, daemon=True)
        self.thread.start()

    def _next_row(self, pos):
        assert pos == self.n_written + sum(n for _, n in self.staged)          # display order
        if not self.staged or self.staged[-1][1] == 3:
            self.staged.append([torch.empty((3, self.header.frame_bytes), dtype=torch.uint8, device=self.dev), 0])
        outs, n = self.staged[-1]
        self.staged[-1][1] = n + 1
        return outs[n]

    def emit(self, pos, frame):
        from . import chain
        row = self._next_row(pos)
        if frame is chain.HOLD:
            row.copy_(self.last_row)
        else:
            l, r, t, b = self.pads
            ops.frame_to_yuv(frame, t, l, self.header.height, self.header.width, self.fmt, out=row)
        self.last_row = row
        if self.scorer is not None:
            self.scorer(pos, row, frame is chain.HOLD)

    def emit_at_rate(self, m, left, right, w):
        """rate.Resampler's emit (--output_rate): `left` alone, or the mix left + w (right - left) packed in the same launch."""
        row = self._next_row(m)
        l, r, t, b = self.pads
        if right is None:
            ops.frame_to_yuv(left, t, l, self.header.height, self.header.width, self.fmt, out=row)
        else:
            ops.blend_to_yuv(left, right, w, t, l, self.header.height, self.header.width, self.fmt, out=row)
        self.last_row = row
        if self.scorer is not None:
            self.scorer(m, row, False)

    def hand_over(self):
        for outs, n in self.staged:
            ready = torch.cuda.Event()
            ready.record()
            host = self.free_out.pop() if self.free_out else torch.empty(outs.shape, dtype=torch.uint8, pin_memory=True)
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                host[:n].copy_(outs[:n], non_blocking=True)
                outs.record_stream(self.copy_stream)
                done = torch.cuda.Event()
                done.record()
            self.to_write.put((host, n, done))
            self.n_written += n
        if self.scorer is not None and self.staged:
            ready = torch.cuda.Event()
            ready.record()
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(ready)
                self.scorer.flush()
            self.scorer.collect()
        self.staged.clear()
        if self.error:
            raise self.error[0]

    def finish(self):
        self.to_write.put(None)
        self.thread.join()


def run_video(args, opt, stats=None):
    """The folder runner's pipeline over one Y4M stream, at every --factor.  A reader thread fills recycled page-locked payload
    buffers; each frame is uploaded once on the upload stream behind an event and unpacked by ops.yuv_to_frame on the compute stream
    (_VideoFeed); chain.run_stream is the window loop: window i runs once frame i + 3 or the end of the stream has been read (the
    length of a piped stream is not known ahead), inside its scene with --scene_cut, through harness.WindowRunner; its fp32 outputs go
    to chain.Chain, which at --factor 4 | 8 runs the higher passes as their frames appear and emits in display order, so the frames
    resident on the device do not grow with the stream; _VideoWriter packs, copies and writes.  The bytes are
    harness.interpolate_video's at the same factor.  --output_rate: rate.Resampler sits between the Chain and the writer and lays
    the output frames on the dense stream; a frame between two of its frames is their fp32 mix, packed in the same launch
    (ops.blend_to_yuv).  Logging goes to stderr and the log file, never to stdout (--output_video -).
    --scene_cut: ops.luma_stats runs on the upload stream right behind each frame's upload (its inputs are the payloads alone), its
    264-byte record comes back through a page-locked buffer and an event of that stream; the compute stream is never waited on for
    it.  Window i needs the cut flags up to the pair (i + 2, i + 3), frames read_to(i + 3) has taken already.
    --gt_video: _GtFeed reads the ground truth beside the input, _VideoScorer scores every packed row against its frame
    (ops.payload_scores on the compute stream, the upload on the upload stream behind an event); the 64-byte records come back
    through page-locked memory and events and are tallied per class (bin_amd/score.py); the table goes to the log, the rows to
    --score_log and to `stats["scores"]`.  The written bytes do not change with it."""
    from . import chain, rate, score, video
    factor = getattr(args, "factor", 2)
    log_root = os.getcwd() if args.output_video == "-" else os.path.dirname(os.path.abspath(args.output_video))
    os.makedirs(log_root, exist_ok=True)
    util.setup_logger("base", log_root, "test_video", screen=True, tofile=True)
    log = logging.getLogger("base")
    reader = video.Y4MReader(args.input_video)       # (the header is read and checked here: before the model is built)
    header = reader.header
    grid, out_header = None, None
    if getattr(args, "output_rate", None) is not None:   # (a pipe's header is known only now: still before the model is built)
        grid = rate.Grid(header.rate, rate.parse_rate(args.output_rate), factor)
        factor, out_header = grid.F, header.at_rate(grid.out_rate)
    fmt = video.resolve_format(header, args.yuv_matrix, args.yuv_range)
    h, w = header.height, header.width
    pads = util.pad_sizes(h, w)
    written_header = out_header or header.multiplied(factor)
    gt_reader = gt_feed = plan = None
    if getattr(args, "gt_video", None) is not None:      # (refusals: still before the model is built)
        gt_reader = video.Y4MReader(args.gt_video)
        try:
            plan = score.Plan(score.align(written_header, gt_reader.header, args.gt_offset), args.gt_offset, factor, grid is not None)
        except BaseException:
            gt_reader.close()
            reader.close()
            raise
        gt_feed = _GtFeed(gt_reader, plan.stride, plan.offset)
    feed = _VideoFeed(args, reader, fmt, pads, factor, log)
    if grid is not None:
        feed.out_frame = lambda c: -(-c * grid.p // grid.q)         # the first output frame at or after the cut

    model = create_model(opt)
    netG = model.netG
    netG.eval()
    dev = next(netG.parameters()).device
    net = harness.WindowRunner(netG, chain.levels(factor), not args.no_reuse, args.batch, args.self_ensemble, (h, w))
    if net.ens[0] is not None:
        log.info("self-ensemble: group %s, M = %d forwards per window", net.ens[0].group, net.ens[0].M)
    log.info("In video: %s %dx%d C%s F%d:%d -> %s at factor %d | YUV: %s %s | model: %s | stage-1 reuse: %s", args.input_video, w, h,
             header.colorspace or "420", header.rate[0], header.rate[1], args.output_video, factor, fmt[1], fmt[2],
             opt["path"]["pretrain_model_G"], net.reuse)
    mode = getattr(args, "resample", None) or "blend"
    if grid is not None:
        log.info("output rate: F%d:%d, %s: the frames of the factor-%d stream, resample %s", grid.out_rate[0], grid.out_rate[1],
                 grid.describe(), grid.F, mode)
    feed.attach(dev)
    scorer = None
    if gt_feed is not None:
        log.info("ground truth: %s F%d:%d, output frame m against its frame %d m + %d", args.gt_video, gt_reader.header.rate[0],
                 gt_reader.header.rate[1], plan.stride, plan.offset)
        gt_feed.attach(dev, feed.upload_stream)
        scorer = _VideoScorer(gt_feed, plan, written_header, dev)
    out = _VideoWriter(args.output_video, written_header, fmt, pads, dev, scorer)
    emit = out.emit if grid is None else rate.Resampler(grid, out.emit_at_rate, mode).push
    timer, stamps = AverageMeter(), []

    def timed(flush):
        t0 = time.time()
        n = flush()
        out.hand_over()
        if n:
            timer.update((time.time() - t0) / n, n)
            stamps.extend([time.time()] * n)

    t_all = time.time()
    try:
        with torch.no_grad():
            run = chain.run_stream(feed, net, emit, factor, net.batch, timed)
            torch.cuda.current_stream(dev).synchronize()
    finally:
        out.finish()
        reader.close()
        if gt_reader is not None:
            gt_reader.close()
    if out.error:
        raise out.error[0]
    n_frames, cuts = feed.n_frames, feed.cuts
    if n_frames < 2:
        raise ValueError(f"{args.input_video}: a video needs at least 2 frames to interpolate (got {n_frames})")
    torch.cuda.synchronize()
    ops.check_status(dev)                 # a frame that left the fp16 storage range is an error, not a result
    wall = time.time() - t_all
    log.info("frames in: %d  out: %d  factor: %d  windows per pass: %s  wall: %.2f s  -> %.2f output frames/s (IO included); net+glue "
             "per window %.4f s; frames resident in the passes at most %d", n_frames, out.n_written, factor, run["windows_per_pass"], wall,
             out.n_written / max(wall, 1e-9), timer.avg, run["frames_resident_peak"])
    if feed.scene_on:
        log.info("scene cuts: %d at input frames %s; duplicates: %d", len(cuts), ", ".join(str(c) for c in cuts) or "-", feed.n_dup)
    scores = None
    if scorer is not None:
        scorer.collect(wait=True)
        scores = {"rows": sorted(scorer.tally.rows), "summary": scorer.tally.summary(), "stride": plan.stride, "offset": plan.offset}
        for line in score.table(scores["summary"]):
            log.info("%s", line)
        if getattr(args, "score_log", None) is not None:
            score.write_log(args.score_log, scores["rows"])
    if stats is not None:
        stats.update(run, wall=wall, net_s_per_window=timer.avg, stamps=[s - t_all for s in stamps], frames_out=out.n_written,
                     factor=factor)
        if scores is not None:
            stats.update(scores=scores)
        if feed.scene_on:
            stats.update(cuts=list(cuts))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
