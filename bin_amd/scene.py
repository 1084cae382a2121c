"""Scene cuts in a video stream: the decision on the luma statistics of libbinscene.so (ops.luma_stats, include/binscene.h) and the
plan that keeps the sliding 6-frame window inside one scene.  Host side only, pure Python / numpy: nothing here touches a device.

A record is (sad, hist): the sum of |Y - Y of the frame before| over the luma plane and the 64-bin histogram of Y >> 2
(ops.read_luma_record).  Frames i-1 and i are in different scenes (a cut at position i) when the histograms lie far apart and the
planes differ enough:

    distance = sum |hist_a - hist_b| / (2 h w)  in [0, 1]      (the total variation distance of the two luma distributions)
    cut      = distance >= threshold  and  sad / (h w) >= min_mad  and  sad != 0

The output keeps the length and layout of a run without cuts: 2 (T - 1) payloads, position 2i = D_i (frame i deblurred), position
2i + 1 = I_i (the frame between i and i + 1), so frame timing does not depend on the option.  `plan` gives, per window, the six
frame ids (clamped to the window's scene: the reference's end-of-clip rule, applied at scene ends) and what it contributes; across
a cut there is no midpoint, I_i is D_i held."""
import numpy as np

HOLD = None                                # plan()'s slot of a held frame: the payload emitted just before, once more


def distance(hist_a, hist_b, h, w):
    """sum |hist_a - hist_b| / (2 h w), in float64 from the integer counts."""
    a, b = np.asarray(hist_a, dtype=np.int64), np.asarray(hist_b, dtype=np.int64)
    return float(np.abs(a - b).sum()) / (2.0 * h * w)


def is_cut(rec_prev, rec_cur, h, w, threshold, min_mad=0.0):
    """Whether the frame of `rec_cur` opens a scene.  rec_*: (sad, hist); rec_cur's sad is the one against rec_prev's frame.  A
    frame with sad == 0 repeats the frame before it (`is_duplicate`) and is never a cut."""
    sad = int(rec_cur[0])
    if sad == 0:
        return False
    return distance(rec_prev[1], rec_cur[1], h, w) >= threshold and sad / float(h * w) >= min_mad


def is_duplicate(rec_cur):
    return int(rec_cur[0]) == 0


def check_cuts(cuts, T):
    """The sorted list of distinct cut positions; ValueError when one lies outside 1 .. T-1 (T = None: no upper end yet)."""
    out = sorted({int(c) for c in cuts})
    if out and (out[0] < 1 or (T is not None and out[-1] > T - 1)):
        raise ValueError(f"scene cuts lie in 1 .. T-1 = {None if T is None else T - 1} (got {out})")
    return out


def segments(T, cuts):
    """The maximal runs [s, e) of frames 0 .. T-1 that no cut divides.  cuts: positions c in 1 .. T-1, c meaning that frames c-1
    and c belong to different scenes."""
    edges = [0] + check_cuts(cuts, T) + [T]
    return [(s, e) for s, e in zip(edges[:-1], edges[1:])]


def plan(i, s, e, T):
    """Window i (0 <= i <= T-2) of a T-frame stream, frame i lying in the scene [s, e): (ids, outputs).  ids: the six frame ids of
    the forward, or None when none is run.  outputs: ((position, slot), ...) in display order, slot being the Ft_p slot of that
    forward or HOLD (the payload emitted just before this one, again).  T may be None while the stream's end is unknown; it then
    must lie beyond i + 2."""
    if not (0 <= s <= i < e) or (T is not None and (e > T or i > T - 2)):
        raise ValueError(f"plan: window {i} of scene [{s}, {e}) in {T} frames")
    if i + 1 < e:
        ids = [min(max(i + d, s), e - 1) for d in (-2, -1, 0, 1, 2, 3)]
        out = ((2 * i, 8),) if i == s else ()
        out += ((2 * i + 1, 13),)
        if T is None or i + 1 <= T - 2:
            out += ((2 * i + 2, 12),)
        return ids, out
    # a cut follows frame i: no midpoint across it
    if i > s:
        return None, ((2 * i + 1, HOLD),)              # D_i came from window i-1's slot 12
    return [s] * 6, ((2 * i, 8), (2 * i + 1, HOLD))     # a one-frame scene


def scene_of(i, cuts, T):
    """The scene [s, e) of frame i."""
    for s, e in segments(T, cuts):
        if s <= i < e:
            return s, e
    raise ValueError(f"frame {i} of {T}")
