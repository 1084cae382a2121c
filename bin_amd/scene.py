"""Scene cuts in a video stream: the decision on the luma statistics of libbinscene.so (ops.luma_stats, include/binscene.h) and the
scenes a set of cuts divides a stream into.  Host side only, pure Python / numpy: nothing here touches a device.

A record is (sad, hist): the sum of |Y - Y of the frame before| over the luma plane and the 64-bin histogram of Y >> 2
(ops.read_luma_record).  Frames i-1 and i are in different scenes (a cut at position i) when the histograms lie far apart and the
planes differ enough:

    distance = sum |hist_a - hist_b| / (2 h w)  in [0, 1]      (the total variation distance of the two luma distributions)
    cut      = distance >= threshold  and  sad / (h w) >= min_mad  and  sad != 0

The output keeps the length and layout of a run without cuts: 2 (T - 1) payloads, position 2i = D_i (frame i deblurred), position
2i + 1 = I_i (the frame between i and i + 1), so frame timing does not depend on the option.  The sliding 6-frame window stays
inside one scene (chain.level1_plan: the six frame ids clamped to the window's scene, the reference's end-of-clip rule applied at
scene ends); across a cut there is no midpoint, I_i is D_i held."""
import numpy as np


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
