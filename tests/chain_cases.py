"""Case table of the chained interpolation passes (bin_amd/chain.py, include/binchain.h): the definition restated by brute force on
stub frames that carry a rational timestamp, the stub driver of chain.Chain the CPU tests run, and the shapes of the reframe kernel
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
    """A frame: a timestamp, whether it is a reframed copy, and of what."""

    def __init__(self, t, of=None):
        self.t, self.of = Fraction(t), of


class StubRun:
    """chain.Chain over stub frames, level 1 driven by chain.level1_plan as the runners drive it.  `step`: level-1 frames per push
    (None: all of a window's at once).  Records everything the tests look at."""

    def __init__(self, T, F, cuts=(), batch=1, step=None):
        from bin_amd import chain
        self.T, self.F, self.emitted, self.reframed, self.log, self.level1_ids = T, F, [], [], [], []
        self.seen = {}                                  # (level, sequence id) -> the objects handed over for it
        self.pushed, self.keep = 0, []                  # (every stub stays alive: ids are unique for the whole run)
        self.chain = chain.Chain(F, self.forward, self.reframe, self.emit, batch=batch, new_scene=lambda: self.log.append(("scene",)))
        for s, e in segments(T, cuts):
            begun = False
            for i in range(s, min(e, T - 1)):
                ids, slots, last = chain.level1_plan(i, s, e)
                if not begun:
                    self.chain.begin(s)
                    begun = True
                if ids is None:
                    continue
                self.level1_ids.append(ids)
                t = {8: ids[2], 13: Fraction(ids[2] + ids[3], 2), 12: ids[3]}
                frames = [Stub(t[slot]) for slot in slots]
                self.keep += frames
                for first in range(0, len(frames), step or len(frames)):
                    part = frames[first:first + (step or len(frames))]
                    self.pushed += len(part)
                    self.log.append(("push", self.pushed))
                    self.chain.push(part)
            if begun:
                self.log.append(("end",))
                self.chain.end(final=e == T)

    def forward(self, level, jobs):
        assert 1 <= len(jobs) <= self.chain.batch
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
