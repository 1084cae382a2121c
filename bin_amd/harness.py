"""Evaluation harness pieces of the reference's test.py that touch the hot path: the sliding 6-frame
window rule (test.py:257-261), the padding rule (test.py:348-366), which outputs are consumed
(test.py:380-382) and window-sharded multi-GPU inference (shard by WINDOW index, not by
clip — the 8 Adobe240 clips have 63-418 frames, so per-clip sharding caps the 8-GPU speed-up at 3.1x)."""
import torch

from . import chain
from .utils import util

builtins_range = range                     # (interpolate_video has a parameter called `range`)


def shard_windows(n_windows, rank, world):
    """Contiguous, balanced [begin, end) range of the flattened (clip, frame) window list for `rank`."""
    base, rem = divmod(n_windows, world)
    begin = rank * base + min(rank, rem)
    return begin, begin + base + (1 if rank < rem else 0)


window_frame_ids = chain.window_ids        # (index, n_frames) -> the 6 blurry frames of the window centred on frame `index` (test.py:257-261)


class WindowRunner:
    """The one place that turns "these windows" into generator calls, for the folder runner, interpolate_clip and the video loop
    (chain.run_stream, whose `net` this is).  Every pass (level 1, the pass on the input frames, included) owns its memo dict and,
    with `ensemble`, its SelfEnsemble: both key on the identity of long-lived input tensors, and the passes interleave.
    reuse_stage1 (N3): consecutive windows share 4 of their 5 stage-1 frame pairs, 2 stage-2 calls and 1 stage-3 call; their RDN
    results are reused (exact: same inputs, same kernels), 17 -> 10 RDN calls per window.  batch > 1: the windows of a call go through
    the net as ONE forward along N (per-image arithmetic is unchanged, so the images are bit-identical), and there is no memo.
    `geometry` = (h, w) of the unpadded frame: what `reframe` needs, so only a run with passes above level 1."""

    def __init__(self, netG, levels=1, reuse_stage1=True, batch=1, ensemble=None, geometry=None):
        from .ensemble import SelfEnsemble, parse_group
        inner = netG.module if hasattr(netG, "module") else netG
        self.netG, self.geometry, self.batch = netG, geometry, max(1, int(batch))
        self.reuse = bool(reuse_stage1 and self.batch == 1 and getattr(inner, "reuse_schedule", False))
        self.caches = [{} if self.reuse else None for _ in builtins_range(levels)]
        self.ens = [SelfEnsemble(netG, ensemble) if parse_group(ensemble) else None for _ in builtins_range(levels)]

    def new_scene(self):
        """A scene or a clip begins: nothing memoised belongs to it."""
        for cache, ens in zip(self.caches, self.ens):
            if cache is not None:
                cache.clear()
            if ens is not None:
                ens.reset()

    def run(self, level, jobs, slots):
        """The generator on `jobs` = [(ids, six frames)], windows of pass `level`, batched along N when there are several: one
        {slot: [1,3,H,W] estimate} per window."""
        cache, ens = self.caches[level - 1], self.ens[level - 1]
        if len(jobs) == 1:
            ids, inputs = jobs[0]
            if ens is not None:
                Ft_p = ens.window(ids, inputs, slots=slots, reuse=cache is not None)
            else:
                Ft_p = self.netG(*inputs, stage1_cache=cache) if cache is not None else self.netG(*inputs)
            return [{k: Ft_p[k] for k in slots}]
        inputs = [torch.cat([frames[k] for _, frames in jobs], 0) for k in builtins_range(6)]
        Ft_p = ens(inputs, slots=slots) if ens is not None else self.netG(*inputs)
        return [{k: Ft_p[k][j:j + 1] for k in slots} for j in builtins_range(len(jobs))]

    def forward(self, level, jobs):
        return [out[13] for out in self.run(level, jobs, (13,))]

    def reframe(self, frames):
        from . import _lib, ops
        h, w = self.geometry
        pads = util.pad_sizes(h, w)
        out = []
        for first in builtins_range(0, len(frames), _lib.CHAIN_MAX_ITEMS):
            out += ops.reframe(frames[first:first + _lib.CHAIN_MAX_ITEMS], pads[2], pads[0], h, w, pads)
        return out


@torch.no_grad()
def interpolate_clip(netG, clip, rank=0, world=1, reuse_stage1=True, batch=1, ensemble=None):
    """Run the test.py inner loop over a clip for this rank's share of its T-1 windows.
    `clip`: [T,H,W,3] uint8 BGR (what cv2.imread yields; decoded, padded and re-encoded ON THE DEVICE by the
    u8_to_frame / frame_to_u8 kernels, each padded frame cached because 5 of a window's 6 frames recur in the
    next window) or [T,3,H,W] fp32 RGB in [0,1].  Returns {window index: (interp, deblur_first, deblur_second)}
    as cropped HWC BGR uint8 images — what test.py writes with cv2.imwrite (test.py:380-402).
    reuse_stage1, batch: WindowRunner's.  A small frame does not fill the chip (a 320x320 window is 50 tiles per launch on 256
    CUs): 8 windows per forward give 2.5x the windows/s at 256x256 and 1.75x at 448x256 (tools/bench_small.py).  Windows are
    independent (the net re-zeros its LSTM state per call).
    ensemble: a self-ensemble group (bin_amd/ensemble.py: letters of `hvt`, `flipx4`, `x8`); every image is then the mean of the
    M = 2^k oriented forwards, the flips and the merge being two HIP launches.  With reuse_stage1 every orientation keeps its own
    oriented frames and memo, so the 17 -> 10 RDN calls per window hold in each.  None / "" / "none": off."""
    from . import ops
    dev = next(netG.parameters()).device
    is_u8 = clip.dtype == torch.uint8
    if is_u8:
        T, h, w, _ = clip.shape
    else:
        T, _, h, w = clip.shape
    pads = util.pad_sizes(h, w)
    l, r, t, b = pads
    begin, end = shard_windows(T - 1, rank, world)
    cache = {}

    def frame(i):
        if i not in cache:
            if is_u8:
                cache[i] = ops.u8_to_frame(clip[i].to(dev), pads)
            else:
                cache[i] = util.replicate_pad(clip[i:i + 1].to(dev), pads)
        return cache[i]

    net = WindowRunner(netG, 1, reuse_stage1, batch, ensemble)
    out = {}
    for first in range(begin, end, net.batch):
        idx = list(range(first, min(first + net.batch, end)))
        ids = [window_frame_ids(i, T) for i in idx]
        for k in [k for k in cache if k < min(ids[0])]:  # the frames no later window names
            del cache[k]
        outs = net.run(1, [(six, [frame(i) for i in six]) for six in ids], (13, 8, 12))
        for i, Ft_p in zip(idx, outs):
            out[i] = tuple(ops.frame_to_u8(Ft_p[k], t, l, h, w).cpu().numpy() for k in (13, 8, 12))
        ops.check_status(dev)             # the .cpu() above synchronised: a saturated fp16 plane is an error, not an image
    return out


class _MemoryFeed:
    """chain.run_stream's feed over a stream that is all there: the length and the cuts are known from the start, `frames_dev` is
    filled frame by frame as the loop asks (ops.yuv_to_frame) and emptied by the loop."""

    def __init__(self, payloads, header, fmt, pads, dev, cuts):
        self.payloads, self.geometry, self.dev = payloads, (header.height, header.width, fmt, pads), dev
        self.n_frames, self.cuts, self.scene_on = payloads.shape[0], cuts, bool(cuts)
        self.frames_dev, self.n_read = {}, 0

    def read_to(self, i):
        from . import ops
        while self.n_read <= min(i, self.n_frames - 1):
            self.frames_dev[self.n_read] = ops.yuv_to_frame(self.payloads[self.n_read].to(self.dev).contiguous(), *self.geometry)
            self.n_read += 1

    def resolve_cuts(self):
        pass


@torch.no_grad()
def interpolate_video(netG, payloads, header, matrix="auto", range="auto", reuse_stage1=True, batch=1, gt=None, gt_offset=0, gt_stride=1,
                      ensemble=None, rate=None, resample="blend", factor=2, scene_cut=None):
    """The window loop of the video runner (chain.run_stream) over the frames of a Y4M stream held in memory.  `payloads`:
    [T, frame_bytes] uint8 (host or device), the frames of `header` (bin_amd/video.py).  Returns the [factor (T-1), frame_bytes] uint8
    device tensor of the output payloads in display order; at factor 2 D0, I0, D1, I1, ..., D(T-2), I(T-2): exactly the frames the
    folder runner writes for a one-clip folder, in name order — window 0 yields Ft_p[8], Ft_p[13], Ft_p[12], a middle window Ft_p[13],
    Ft_p[12], the last one Ft_p[13].  YUV -> padded frame and frame -> YUV are the kernels of libbinyuv.so (ops.yuv_to_frame /
    ops.frame_to_yuv), the padded frames cached across the 5-of-6 overlap.  matrix / range: video.resolve_format.  reuse_stage1,
    batch, ensemble: as in interpolate_clip.
    scene_cut: None = the stream is one clip.  A number is the threshold of `detect_cuts`, an iterable of ints the cut positions
    themselves (c: frames c-1 and c are of different scenes).  The windows then stay inside their scene (chain.level1_plan): every
    scene comes out as if it ran alone, plus its last deblurred frame, and the frames up to the next scene are that frame, held.
    Same length, same layout.
    factor: 2, 4 or 8: above 2 the passes of bin_amd/chain.py on the fp32 outputs, which never leave the device; every second
    payload is the output at factor / 2.
    rate: None, or the absolute output frame rate as (N, D) or a Fraction (bin_amd/rate.py): the result is then the [M, frame_bytes]
    stream at that rate, up to 8 times the header's, laid on the dense stream of the smallest factor F >= max(rate / input rate,
    factor); an output frame between two dense frames is their mix in fp32, converted in the same launch (ops.blend_to_yuv), and never
    a mix across a cut.  resample: "blend", or "nearest" for the nearer dense frame instead (ties go to the earlier one).
    gt: None, or the [Tg, frame_bytes] uint8 payloads (host or device) of a ground-truth stream of the same header whose frame
    gt_stride m + gt_offset is the truth of output frame m (bin_amd/score.py).  Every output payload is then scored against it as the
    bytes it was packed to, on the device, right after it is packed (ops.payload_scores), and the call returns (out, rows): one
    score.py row per output frame that has a ground-truth frame, after one download of all records.  `out` is the same bytes."""
    from . import ops, scene, video
    from . import rate as rate_
    from . import score as score_
    chain.levels(factor)
    if gt is not None:
        if gt.dim() != 2 or gt.dtype != torch.uint8 or gt.shape[1] != header.frame_bytes:
            raise ValueError(f"gt must be uint8 [Tg, {header.frame_bytes}] for this header (got {gt.dtype} {tuple(gt.shape)})")
        score_.check_offset(gt_offset)
    if resample not in rate_.MODES:
        raise ValueError(f"resample must be one of {rate_.MODES} (got {resample!r})")
    grid = None
    if rate is not None:
        grid = rate_.Grid(header.rate, rate, factor)
        factor = grid.F
    k = chain.levels(factor)
    T = payloads.shape[0]
    if T < 2:
        raise ValueError(f"interpolate_video needs at least 2 frames (got {T})")
    fmt = video.resolve_format(header, matrix, range)
    h, w = header.height, header.width
    if payloads.dim() != 2 or payloads.dtype != torch.uint8 or payloads.shape[1] != header.frame_bytes:
        raise ValueError(f"payloads must be uint8 [T, {header.frame_bytes}] for this header (got {payloads.dtype} {tuple(payloads.shape)})")
    dev = next(netG.parameters()).device
    if scene_cut is None:
        cuts = []
    elif isinstance(scene_cut, (int, float)):
        cuts = detect_cuts(payloads, header, float(scene_cut), device=dev)
    else:
        cuts = scene.check_cuts(scene_cut, T)
    pads = util.pad_sizes(h, w)
    l, r, t, b = pads
    n_out = factor * (T - 1) if grid is None else grid.frames(T)
    out = torch.empty((n_out, header.frame_bytes), dtype=torch.uint8, device=dev)
    written = []
    plan = records = None
    if gt is not None:
        plan = score_.Plan(gt_stride, gt_offset, factor, grid is not None)
        records = torch.empty((n_out, ops.PLANE_SCORES_BYTES), dtype=torch.uint8, device=dev)
    scored = []                                        # (output frame, its class) of every frame that has a ground truth

    def score(pos, is_hold):                           # (right after out[pos] is packed: the scored bytes are the returned bytes)
        if plan is not None and plan.gt_index(pos) < gt.shape[0]:
            truth = gt[plan.gt_index(pos)].to(dev).contiguous()
            ops.payload_scores(out[pos], truth, h, w, header.chroma, ssim=min(h, w) >= 7, out=records[pos])
            scored.append((pos, plan.frame_class(pos, is_hold)))

    def emit(pos, f):
        if f is chain.HOLD:
            out[pos].copy_(out[pos - 1])
        else:
            ops.frame_to_yuv(f, t, l, h, w, fmt, out=out[pos])
        written.append(pos)
        score(pos, f is chain.HOLD)

    def emit_at_rate(m, left, right, weight):
        if right is None:
            ops.frame_to_yuv(left, t, l, h, w, fmt, out=out[m])
        else:
            ops.blend_to_yuv(left, right, weight, t, l, h, w, fmt, out=out[m])
        written.append(m)
        score(m, False)

    def checked(flush):
        flush()
        ops.check_status(dev)             # (synchronises, as the image download of interpolate_clip does at this point)

    net = WindowRunner(netG, k, reuse_stage1, batch, ensemble, (h, w))
    sink = emit if grid is None else rate_.Resampler(grid, emit_at_rate, resample).push
    chain.run_stream(_MemoryFeed(payloads, header, fmt, pads, dev, cuts), net, sink, factor, net.batch, checked)
    assert written == list(builtins_range(n_out))               # display order
    if gt is None:
        return out
    host = records.cpu()
    return out, [(m, plan.gt_index(m), cls) + ops.read_plane_scores(host[m]) for m, cls in scored]


def luma_records(payloads, header, device=None):
    """[(sad, hist)] of the T frames of a stream (ops.luma_stats over the Y planes, frame 0 against nothing): one launch per frame
    into one [T, 264] device buffer, one download."""
    from . import ops
    h, w = header.height, header.width
    if payloads.dim() != 2 or payloads.dtype != torch.uint8 or payloads.shape[1] != header.frame_bytes:
        raise ValueError(f"payloads must be uint8 [T, {header.frame_bytes}] for this header (got {payloads.dtype} {tuple(payloads.shape)})")
    if not payloads.is_cuda:
        payloads = payloads.to(device if device is not None else "cuda")
    payloads = payloads.contiguous()
    T = payloads.shape[0]
    recs = torch.empty((T, ops.LUMA_RECORD_BYTES), dtype=torch.uint8, device=payloads.device)
    for i in builtins_range(T):
        ops.luma_stats(payloads[i, :h * w], payloads[i - 1, :h * w] if i else None, h, w, out=recs[i])
    host = recs.cpu()
    return [ops.read_luma_record(host[i]) for i in builtins_range(T)]


def detect_cuts(payloads, header, threshold, min_mad=0.0, device=None):
    """The cut positions of a stream: every i in 1 .. T-1 whose frame opens a scene by scene.is_cut on the luma statistics the
    kernel of libbinscene.so measures.  `payloads`: [T, frame_bytes] uint8, host or device (a host stream goes to `device`, default the current one)."""
    from . import scene
    recs = luma_records(payloads, header, device)
    h, w = header.height, header.width
    return [i for i in builtins_range(1, len(recs)) if scene.is_cut(recs[i - 1], recs[i], h, w, threshold, min_mad)]


class GraphedNet:
    """hipGraph replay of the 6-frame forward for one input shape (launch-bound regime: a 256x256 demo window is ~1150
    kernel launches of a few microseconds each, so the host, not the GPU, sets the pace when they are issued one by one).
    The library allocates nothing and never syncs, which is what makes its launch sequences capturable.

    multi_stream=False: the whole serial forward is ONE graph.
    multi_stream=True : every RDN call (67 launches) and ConvLSTM cell is its own graph, captured on the stream the
    3-stream schedule runs it on; a replayed forward is 23 graph launches whose cross-stream dependencies stay eager
    events.  (One graph over all three streams is not possible on this stack: hipStreamEndCapture crashes once two
    captured streams depend on each other in both directions — tools/probe_graph.py.)
    `__call__` copies the new frames into the static input buffers and replays; outputs are the static output tensors
    of the capture (overwritten by the next replay)."""

    def __init__(self, netG, example_frames, warmup=2, multi_stream=False):
        self.net = netG
        self.multi_stream = multi_stream
        self.static_in = [f.detach().clone().contiguous().float() for f in example_frames]
        self.inner = inner = netG.module if hasattr(netG, "module") else netG
        saved_streams = getattr(inner, "n_streams", None)
        if not multi_stream:
            inner.n_streams = 1
        elif inner.resolved_streams() < 2:
            raise RuntimeError("GraphedNet(multi_stream=True) needs the multi-stream inference schedule (n_streams > 1)")
        self._ns = inner.resolved_streams()
        try:
            self._capture(netG, warmup)
        finally:
            inner.n_streams = saved_streams

    def _capture(self, netG, warmup):
        with torch.no_grad():
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(warmup):                  # relayouts, LDS attributes, workspaces: before capture
                    netG(*self.static_in)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            from .rdn_plan import release_workspaces
            release_workspaces(side)                     # the warm-up stream dies here: do not keep its workspace
            if self.multi_stream:
                self.inner._graph_mode = "capture"
                try:
                    self.static_out = netG(*self.static_in)
                finally:
                    self.inner._graph_mode = None
                self.call_graphs = self.inner._call_graphs
                self.inner._call_graphs = None
                torch.cuda.synchronize()
            else:
                self.graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph):
                    self.static_out = netG(*self.static_in)

    @torch.no_grad()
    def __call__(self, *frames):
        for dst, src in zip(self.static_in, frames):
            dst.copy_(src, non_blocking=True)
        if not self.multi_stream:
            self.graph.replay()
            return self.static_out
        inner = self.inner
        saved = inner.n_streams
        inner.n_streams = self._ns                       # the stream assignment the per-call graphs were captured with
        inner._graph_mode, inner._call_graphs = "replay", self.call_graphs
        try:
            return netG_call(self.net, self.static_in)
        finally:
            inner._graph_mode, inner._call_graphs = None, None
            inner.n_streams = saved


def netG_call(netG, frames):
    return netG(*frames)
