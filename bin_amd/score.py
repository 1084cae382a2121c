"""Scoring a video run against a ground-truth stream (`--gt_video`, harness.interpolate_video's `gt=`): which ground-truth frame an
output frame is scored against, which class of frame it is, the tally of the per-frame records and the log file.  Host side only:
nothing here touches a device; the records are the tuples ops.read_plane_scores gives for what ops.payload_scores measured on the
written bytes (include/binscore.h).

Alignment (the Adobe240 protocol on a stream): the input is a blurry stream at rate R, the ground truth the sharp stream at the
output rate or at a whole multiple s of it; output frame m is scored against ground-truth frame s m + offset.  One 240 fps sharp
file then serves factor 2 (s = 4), factor 4 (s = 2) and factor 8 (s = 1) of a 30 fps input; with --output_rate the same rule holds
against the written header's rate.  The rates are compared as exact fractions.

Classes, by the frame's phase m % F in the factor-F stream: phase 0 is `deblurred`, F/2 `interp_L1` (the first pass's midpoints),
odd multiples of F/4 `interp_L2`, the rest at F = 8 `interp_L3`; a frame emitted as chain.HOLD is `held` and counts in no other
class.  With --output_rate there is one class, `all`.

A row is (output index, ground-truth index, class, sse_y, sse_u, sse_v, sad_y, sad_u, sad_v, ssim_g11, ssim_u7)."""
import math
from fractions import Fraction

from .utils.util import psnr_from_mse

CLASSES = ("deblurred", "interp_L1", "interp_L2", "interp_L3", "held", "all")
OVERALL = "overall"
LOG_COLUMNS = ("out", "gt", "class", "sse_y", "sse_u", "sse_v", "sad_y", "sad_u", "sad_v", "ssim_g11", "ssim_u7")


def stride(gt_rate, out_rate):
    """s of a ground truth at gt_rate = (n, d) for an output at out_rate: their ratio as exact fractions, a positive integer.
    ValueError (naming both rates) otherwise."""
    ratio = Fraction(*gt_rate) / Fraction(*out_rate)
    if ratio.denominator != 1 or ratio < 1:
        raise ValueError(f"--gt_video: the ground truth's frame rate {gt_rate[0]}:{gt_rate[1]} is not a whole multiple of the output's "
                         f"{out_rate[0]}:{out_rate[1]} (ratio {ratio})")
    return int(ratio)


def check_offset(offset):
    if type(offset) is not int or offset < 0:
        raise ValueError(f"--gt_offset: the first ground-truth frame is a non-negative integer (got {offset!r})")
    return offset


def align(out_header, gt_header, offset=0):
    """The stride s of `gt_header`'s stream under `out_header`'s (the header that is written), after the checks that the two can be
    compared at all: one width, height and chroma family, the same XCOLORRANGE where both carry one, a non-negative offset."""
    check_offset(offset)
    for what, a, b in (("width", out_header.width, gt_header.width), ("height", out_header.height, gt_header.height),
                       ("chroma", out_header.chroma, gt_header.chroma)):
        if a != b:
            raise ValueError(f"--gt_video: the ground truth's {what} {b} is not the output's {a}")
    if out_header.full_range is not None and gt_header.full_range is not None and out_header.full_range != gt_header.full_range:
        name = {True: "FULL", False: "LIMITED"}
        raise ValueError(f"--gt_video: the ground truth's XCOLORRANGE={name[gt_header.full_range]} is not the output's "
                         f"XCOLORRANGE={name[out_header.full_range]}")
    return stride(gt_header.rate, out_header.rate)


def frame_class(m, factor, is_hold=False, at_rate=False):
    """The class of output frame m of a factor-`factor` stream (module docstring)."""
    if at_rate:
        return "all"
    if is_hold:
        return "held"
    if factor not in (2, 4, 8):
        raise ValueError(f"factor must be one of (2, 4, 8) (got {factor!r})")
    phase = m % factor
    if phase == 0:
        return "deblurred"
    if 2 * phase == factor:
        return "interp_L1"
    if (4 * phase) % factor == 0:
        return "interp_L2"
    return "interp_L3"


class Plan:
    """What a scorer needs to know about output frame m: the ground-truth frame it is scored against and its class."""

    def __init__(self, stride, offset, factor, at_rate=False):
        if type(stride) is not int or stride < 1:
            raise ValueError(f"the ground truth's stride is a positive integer (got {stride!r})")
        self.stride, self.offset, self.factor, self.at_rate = stride, check_offset(offset), factor, bool(at_rate)

    def gt_index(self, m):
        return self.stride * m + self.offset

    def frame_class(self, m, is_hold=False):
        return frame_class(m, self.factor, is_hold, self.at_rate)


def _mean(values):
    values = [v for v in values if not math.isnan(v)]
    return math.fsum(values) / len(values) if values else float("nan")


class Tally:
    """The rows of a run, per class and overall.  `ny`, `nc`: samples of the Y plane and of one chroma plane.  Pooled PSNRs come from
    the summed integer SSEs (Python integers, one division), so they are exact and do not depend on the order of the rows; the
    means are math.fsum's, which does not either."""

    def __init__(self, ny, nc):
        self.ny, self.nc, self.rows, self.unscored = int(ny), int(nc), [], 0

    def add(self, row):
        self.rows.append(tuple(row))

    def no_gt(self, n=1):
        """Output frames whose ground-truth index lies past the end of the ground truth: counted, not scored."""
        self.unscored += n

    def _summary(self, rows):
        n = len(rows)
        out = {"n": n}
        if not n:
            return out
        sse = [sum(r[3 + p] for r in rows) for p in range(3)]
        out["psnr_y"] = psnr_from_mse(sse[0] / (n * self.ny))
        out["psnr_u"] = psnr_from_mse(sse[1] / (n * self.nc))
        out["psnr_v"] = psnr_from_mse(sse[2] / (n * self.nc))
        out["psnr_yuv"] = psnr_from_mse(sum(sse) / (n * (self.ny + 2 * self.nc)))
        per_frame = [psnr_from_mse(r[3] / self.ny) for r in rows if r[3] != 0]
        out["n_identical"] = n - len(per_frame)              # frames equal to their ground truth in Y: infinite PSNR, left out
        out["mean_psnr_y"] = _mean(per_frame)
        out["ssim_g11"] = _mean([r[9] for r in rows])
        out["ssim_u7"] = _mean([r[10] for r in rows])
        return out

    def summary(self):
        """{class: {...}} for every class that has rows, "overall" (held frames included) and "unscored" (a count)."""
        rows = sorted(self.rows)
        out = {c: self._summary([r for r in rows if r[2] == c]) for c in CLASSES if any(r[2] == c for r in rows)}
        out[OVERALL] = self._summary(rows)
        out["unscored"] = self.unscored
        return out


def table(summary):
    """The per-class table as log lines."""
    lines = ["%-10s %6s %9s %9s %9s %9s %12s %6s %9s %9s" % ("class", "n", "psnr_y", "psnr_u", "psnr_v", "psnr_yuv", "mean_psnr_y",
                                                              "ident", "ssim_g11", "ssim_u7")]
    for name in CLASSES + (OVERALL,):
        s = summary.get(name)
        if not s or not s["n"]:
            continue
        lines.append("%-10s %6d %9.4f %9.4f %9.4f %9.4f %12.4f %6d %9.6f %9.6f" % (
            name, s["n"], s["psnr_y"], s["psnr_u"], s["psnr_v"], s["psnr_yuv"], s["mean_psnr_y"], s["n_identical"], s["ssim_g11"],
            s["ssim_u7"]))
    if summary.get("unscored"):
        lines.append(f"{summary['unscored']} output frames lie past the end of the ground truth and were not scored")
    return lines


def write_log(path, rows):
    """One tab-separated row per scored output frame under a header line; floats as repr, so a reader gets the same doubles."""
    with open(path, "w") as f:
        f.write("\t".join(LOG_COLUMNS) + "\n")
        for r in sorted(rows):
            f.write("\t".join([str(r[0]), str(r[1]), r[2]] + [str(int(v)) for v in r[3:9]] + [repr(float(v)) for v in r[9:11]]) + "\n")


def read_log(path):
    """The rows write_log wrote."""
    with open(path) as f:
        lines = f.read().splitlines()
    if not lines or tuple(lines[0].split("\t")) != LOG_COLUMNS:
        raise ValueError(f"{path}: not a score log")
    rows = []
    for ln in lines[1:]:
        c = ln.split("\t")
        rows.append((int(c[0]), int(c[1]), c[2]) + tuple(int(v) for v in c[3:9]) + (float(c[9]), float(c[10])))
    return rows
