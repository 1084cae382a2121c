"""Case table of the chained interpolation passes (bin_amd/chain.py, include/binchain.h): the definition restated by brute force on
stub frames that carry a rational timestamp, the stub feed and runner the CPU tests hand to chain.run_stream, and the shapes of the reframe kernel
the GPU tests run.  Host side only."""
import itertools
from fractions import Fraction

FACTORS = (2, 4, 8)
LENGTHS = tuple(range(2, 10))                      # T of the scheduler tests
HOLD = "hold"


# ------------------------------------------------------------------------------------------------ the definition, by brute force
def window_ids(j, n):
    return [min(max(j + d, 0), n - 1) for d in (-2, -1, 0, 1, 2, 3)]


def scene_levels(n, k, t0=0):
    """A scene of n input frames that starts at time t0: ([S1, ..., Sk] as lists of timestamps, {level p >= 2: [window ids]})."""
    seq = [Fraction(t0) + Fraction(i, 2) for i in range(2 * (n - 1) + 1)]
    out, ids = [seq], {}
    for p in range(2, k + 1):
        prev, nxt, ids[p] = out[-1], [], []
        for j in range(len(prev) - 1):
            w = window_ids(j, len(prev))
            ids[p].append(w)
            nxt += [prev[j], (prev[w[2]] + prev[w[3]]) / 2]
        out.append(nxt + [prev[-1]])
    return out, ids


def segments(T, cuts):
    edges = [0] + sorted(cuts) + [T]
    return list(zip(edges[:-1], edges[1:]))


def expected_stream(T, cuts, F):
    """[timestamp or HOLD] per output position of a T-frame stream, every scene run alone."""
    k = F.bit_length() - 1
    out = []
    for s, e in segments(T, cuts):
        assert len(out) == min(F * s, F * (T - 1))
        last = scene_levels(e - s, k, s)[0][-1]
        if e == T:
            out += last[:-1]
        else:
            out += last + [HOLD] * (F - 1)
    assert len(out) == F * (T - 1)
    return out


def expected_level1_ids(T, cuts):
    """The six input frame ids of every level-1 forward, in order: the scenes alone, ids shifted by the scene's start."""
    out = []
    for s, e in segments(T, cuts):
        n = e - s
        if n == 1 and e < T:
            out.append([s] * 6)
        out += [[s + i for i in window_ids(j, n)] for j in range(n - 1)]
    return out


def all_cut_sets(T):
    return [c for r in range(T) for c in itertools.combinations(range(1, T), r)]


# ------------------------------------------------------------------------------------------------ the stub driver
class Stub:
    """A frame: a timestamp, whether it is a reframed copy, and of what; a level-1 frame's `src` is (window, Ft_p slot)."""

    def __init__(self, t, of=None, src=None):
        self.t, self.of, self.src = Fraction(t), of, src


class StubFeed:
    """The feed of chain.run_stream over T stub frames.  `live`: nothing is known ahead, as on a pipe: read_to reads no further than
    asked, the length is learnt by reading past the last frame, and `cuts` knows a cut once both frames of its pair were read and
    raises when asked about a frame that was not.  Otherwise everything is known from the start, as in harness.interpolate_video."""

    def __init__(self, T, cuts=(), live=False, log=None):
        self.T, self.all_cuts, self.live, self.log = T, sorted(cuts), live, [] if log is None else log
        self.frames_dev, self.n_read, self.n_frames = {}, 0, None if live else T
        self.scene_on, self.n_resolved, self.cuts = bool(cuts) or live, 0 if live else T, self
        self.asked = []                                 # the argument of every read_to

    def read_to(self, i):
        self.asked.append(i)
        self.log.append(("read", i))
        while self.n_read <= i and self.n_read < self.T:
            self.frames_dev[self.n_read] = Stub(self.n_read)
            self.n_read += 1
        if self.n_read <= i:
            self.n_frames = self.T                      # read past the last frame

    def resolve_cuts(self):
        self.n_resolved = self.n_read if self.live else self.T

    def __contains__(self, i):                          # `cuts`
        if i >= self.n_resolved:
            raise AssertionError(f"asked whether frame {i} opens a scene with {self.n_resolved} frames decided")
        return i in self.all_cuts

    def __iter__(self):
        return iter([c for c in self.all_cuts if c < self.n_resolved])


class StubRun:
    """chain.run_stream, the loop that ships, over a StubFeed and this stub runner.  `step`: level-1 frames per Chain.push (None: all
    of a window's at once, as the loop pushes them).  Records everything the tests look at; in `log`: ("read", i) per read_to(i), ("scene",) per new_scene,
    ("run", [ids, ...]) per level-1 forward, ("push", level-1 frames so far), ("forward", level, ids) per window of a pass above,
    ("end",) per scene."""

    def __init__(self, T, F, cuts=(), batch=1, step=None, live=False):
        from bin_amd import chain
        self.T, self.F, self.emitted, self.reframed, self.log, self.level1_ids = T, F, [], [], [], []
        self.sources = []                               # per output position: the `src` of the frame emitted there (None: a hold, a pass's frame)
        self.seen = {}                                  # (level, sequence id) -> the objects handed over for it
        self.pushed, self.keep = 0, []                  # (every stub stays alive: ids are unique for the whole run)
        self.batch, self.feed, self.flushes = batch, StubFeed(T, cuts, live, self.log), []
        run = self

        class Recording(chain.Chain):                   # the loop's own Chain, with its pushes split into `step`s and logged
            def __init__(self, *args, **kwargs):
                super().__init__(*args, **kwargs)
                run.chain = self

            def push(self, frames):
                for first in range(0, len(frames), step or len(frames)):
                    part = frames[first:first + (step or len(frames))]
                    run.pushed += len(part)
                    run.log.append(("push", run.pushed))
                    super().push(part)

            def end(self, final):
                run.log.append(("end",))
                super().end(final)

        def around(flush):
            self.flushes.append(flush())

        shipped, chain.Chain = chain.Chain, Recording
        try:
            self.stats = chain.run_stream(self.feed, self, self.emit, F, batch, around)
        finally:
            chain.Chain = shipped

    def new_scene(self):
        self.log.append(("scene",))

    def run(self, level, jobs, slots):
        assert level == 1 and 1 <= len(jobs) <= self.batch and tuple(slots) == (13, 8, 12)
        for ids, frames in jobs:
            assert [f.t for f in frames] == ids, "the six frames are the feed's frames of the six ids"
        self.log.append(("run", [ids for ids, _ in jobs]))
        self.level1_ids += [ids for ids, _ in jobs]
        out = [{8: Stub(ids[2], src=(ids[2], 8)), 13: Stub(Fraction(ids[2] + ids[3], 2), src=(ids[2], 13)), 12: Stub(ids[3], src=(ids[2], 12))}
               for ids, _ in jobs]
        self.keep += [f for o in out for f in o.values()]
        return out

    def forward(self, level, jobs):
        assert level >= 2 and 1 <= len(jobs) <= self.chain.batch
        out = []
        for ids, frames in jobs:
            assert all(f.of is not None for f in frames), "the inputs of a pass are reframed frames"
            self.log.append(("forward", level, ids))
            for i, f in zip(ids, frames):
                self.seen.setdefault((len([x for x in self.log if x == ("scene",)]), level, i), set()).add(id(f))
            out.append(Stub((frames[2].t + frames[3].t) / 2))
        self.keep += out
        return out

    def reframe(self, frames):
        assert all(f.of is None for f in frames), "a reframed frame is never reframed again"
        self.reframed += [id(f) for f in frames]
        out = [Stub(f.t, of=f) for f in frames]
        self.keep += out
        return out

    def emit(self, pos, frame):
        assert pos == len(self.emitted), "display order"
        self.emitted.append(HOLD if frame is None else frame.t)
        self.sources.append(None if frame is None else frame.src)


# ------------------------------------------------------------------------------------------------ the reframe kernel's shapes (GPU)
# (name, planes, Hs, Ws, top, left, h, w, (pad_left, pad_right, pad_top, pad_bottom), takes the 16-byte path when the pointers allow)
REFRAME_SHAPES = (
    ("one pixel", 1, 1, 1, 0, 0, 1, 1, (0, 0, 0, 0), False),
    ("one pixel of a frame, padded", 3, 5, 7, 2, 3, 1, 1, (2, 1, 1, 3), False),
    ("odd sizes", 3, 37, 53, 3, 5, 29, 41, (7, 5, 2, 9), False),
    ("the 24x40 frame", 3, 128, 128, 52, 44, 24, 40, (44, 44, 52, 52), True),
    ("the 33x47 frame", 3, 128, 128, 47, 40, 33, 47, (40, 41, 47, 48), False),
    ("aligned widths, crop offset 2", 3, 64, 64, 1, 2, 16, 32, (4, 4, 1, 0), False),
    ("aligned widths, pad_left 3", 3, 64, 64, 1, 4, 16, 32, (3, 5, 0, 1), False),
    ("aligned, no pad on the left and top", 2, 40, 48, 8, 8, 30, 36, (0, 12, 0, 5), True),
    ("aligned, no pad on the right and bottom", 2, 40, 48, 0, 12, 30, 36, (8, 0, 3, 0), True),
    ("aligned, no pads, the whole source", 6, 24, 64, 0, 0, 24, 64, (0, 0, 0, 0), True),
    ("more than one block per item", 3, 200, 320, 4, 8, 180, 300, (8, 12, 10, 2), True),
)
SPECIALS = (float("nan"), float("inf"), float("-inf"), -0.0, 0.0, 1.0, -1e-30, 1.0000001, 2.5, -3.0, 1e38, -1e38)


# ------------------------------------------------------------------------------------------------ the clips (GPU)
def clip_header(h, w, chroma):
    return b"YUV4MPEG2 W%d H%d F30:1 Ip A1:1 C%s XCOLORRANGE=FULL\n" % (w, h, b"444" if chroma == 444 else b"420jpeg")


def clip(h, w, chroma, T):
    """A smooth moving pattern (in gamut): [T, frame_bytes] uint8 payloads of an h x w stream, numpy."""
    import numpy as np
    ch, cw = (h, w) if chroma == 444 else ((h + 1) // 2, (w + 1) // 2)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ch, 0:cw]
    frames = []
    for k in range(T):
        Y = 110 + 70 * np.sin(0.31 * (xx + 2 * k)) * np.cos(0.23 * yy) + 8 * ((xx // 5 + yy // 4 + k) % 2)
        U = 128 + 30 * np.sin(0.4 * (cx - k) * (20.0 / cw))
        V = 128 + 30 * np.cos(0.35 * (cy + k) * (12.0 / ch))
        frames.append(np.concatenate([np.rint(p).astype(np.uint8).reshape(-1) for p in (Y, U, V)]))
    return np.stack(frames)
