"""Output at any frame rate (`--output_rate N[:D]`, harness.interpolate_video's `rate=`): the time grid that lays the output frames
on the dense stream of bin_amd/chain.py, and the resampler between Chain's `emit` and the YUV packer.  Host side only, pure Python:
nothing here touches a device; the frames are whatever the caller hands over (device tensors in the runners, stubs in the CPU
tests).  All arithmetic is in Python integers, so a long stream does not drift.

The input rate is n:d (the Y4M header's), the requested output rate N:D, their ratio rho = (N d)/(D n) = p/q in lowest terms,
0 < rho <= 8.  The dense stream has F frames per input frame, F the smallest of 2, 4, 8 with F >= max(rho, factor): `factor` is a
lower bound on the grid.  Output frame m sits at the dense coordinate

    x_m = m F q / p,    left neighbour a_m = (m F q) // p,    weight of the right neighbour w_m = ((m F q) mod p) / p in [0, 1),

and a stream of T input frames, whose dense stream is the positions 0 .. F(T-1)-1 that Chain emits, gives the
M = ((F(T-1) - 1) p) // (F q) + 1 output frames with x_m <= F(T-1) - 1.  For rho = F that is the dense stream itself.

`Resampler` takes Chain's (position, frame | HOLD) calls and emits (m, left, right, w) as soon as position ceil(x_m) has arrived:
`right` is None and w 0 where the output is one frame alone, otherwise the output is left + w (right - left) (ops.blend_to_yuv).
It holds at most two dense frames.  A hold IS the last real frame (the same object), and a mix never crosses a cut: in the dense
stream a real frame that follows a HOLD opens a scene, and only such a frame does (Chain emits F-1 >= 1 holds after every scene a
cut ends and none elsewhere), so where `right` opens a scene the output is `left` alone: the cut falls on the first output frame at
or after it and stays a hard cut.  mode "nearest" never mixes: `left` when w <= 1/2 (ties go left) or `right` opens a scene, else
`right`."""

HOLD = None                                # Chain's emit() frame of a held position (chain.HOLD)
FACTORS = (2, 4, 8)                        # chain.FACTORS
MAX_RATIO = 8                              # rho above this is refused: the densest grid there is
MODES = ("blend", "nearest")


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def rate_pair(rate, what="rate"):
    """(N, D), positive ints as written (not reduced), of a frame rate given as (N, D), as an int or as a Fraction.  ValueError for
    anything else: floats, bools, zero and negative rates."""
    if isinstance(rate, (tuple, list)):
        if len(rate) != 2:
            raise ValueError(f"{what}: a frame rate is N or (N, D) (got {rate!r})")
        n, d = rate
    elif not isinstance(rate, bool) and hasattr(rate, "numerator") and hasattr(rate, "denominator"):
        n, d = rate.numerator, rate.denominator
    else:
        raise ValueError(f"{what}: a frame rate is N, (N, D) or a Fraction (got {rate!r})")
    if type(n) is not int or type(d) is not int or n < 1 or d < 1:
        raise ValueError(f"{what}: a frame rate is a ratio of two positive integers (got {rate!r})")
    return n, d


def parse_rate(text):
    """(N, D) of the command line's `N[:D]`; ValueError names what is malformed."""
    n, sep, d = str(text).partition(":")
    if not n.isdigit() or (sep and not d.isdigit()):
        raise ValueError(f"--output_rate: {text!r} is not a frame rate N[:D] of positive integers")
    return rate_pair((int(n), int(d) if sep else 1), "--output_rate")


class Grid:
    """The output frames of a stream at `out_rate` on the dense stream of an input at `in_rate`: p, q (rho = p/q in lowest terms)
    and the dense factor F.  ValueError when rho > 8, when a rate is not one and when `factor` is none of 2, 4, 8."""

    def __init__(self, in_rate, out_rate, factor=2):
        n, d = rate_pair(in_rate, "input rate")
        N, D = rate_pair(out_rate, "output rate")
        if type(factor) is not int or factor not in FACTORS:
            raise ValueError(f"factor must be one of {FACTORS} (got {factor!r})")
        p, q = N * d, D * n
        g = _gcd(p, q)
        self.p, self.q = p // g, q // g
        if self.p > MAX_RATIO * self.q:
            raise ValueError(f"output rate {N}:{D} is {self.p}/{self.q} times the input rate {n}:{d}: at most {MAX_RATIO} times is "
                             f"supported")
        self.F = next(F for F in FACTORS if F * self.q >= self.p and F >= factor)
        self.in_rate, self.out_rate = (n, d), (N, D)

    def at(self, m):
        """(a_m, r_m): output frame m has the dense left neighbour a_m and the weight r_m / p of the frame after it."""
        return divmod(m * self.F * self.q, self.p)

    def weight(self, m):
        """w_m as the float nearest to r_m / p (what the kernel is given)."""
        return self.at(m)[1] / self.p

    def frames(self, n_frames):
        """M of a stream of n_frames >= 2 input frames: the outputs on the dense positions 0 .. F (n_frames - 1) - 1."""
        if n_frames < 2:
            raise ValueError(f"a stream needs at least 2 frames (got {n_frames})")
        return ((self.F * (n_frames - 1) - 1) * self.p) // (self.F * self.q) + 1

    def describe(self):
        return f"rho {self.p}/{self.q}, F {self.F}"


class Resampler:
    """Between chain.Chain's `emit` and the packer.  `push(position, frame | HOLD)` is Chain's emit; `emit(m, left, right, w)` is
    called once per output frame, in order, as soon as the dense position ceil(x_m) has arrived; `right` is None and w 0 where
    the output is `left` alone (no mix is launched).  `m` is the number of outputs so far."""

    def __init__(self, grid, emit, mode="blend"):
        if mode not in MODES:
            raise ValueError(f"resample must be one of {MODES} (got {mode!r})")
        self.grid, self.emit, self.mode = grid, emit, mode
        self.m, self.position = 0, -1
        self.before, self.last = None, None         # the dense frames at position - 1 and position: all that is held
        self.held, self.opens = False, False        # `last` is a hold; `last` opens a scene

    def push(self, position, frame):
        if position != self.position + 1:
            raise RuntimeError(f"Resampler.push: position {position} after {self.position}")
        if frame is HOLD:
            if self.last is None:
                raise RuntimeError("Resampler.push: a hold with nothing to hold")
            frame, self.opens, self.held = self.last, False, True
        else:
            self.opens, self.held = self.held, False
        self.before, self.last, self.position = self.last, frame, position
        while True:
            a, r = self.grid.at(self.m)
            if a + (r > 0) > position:
                return
            if r == 0:
                out = (self.last, None, 0)
            elif self.opens or self.before is self.last:
                out = (self.before, None, 0)        # never across a cut; a held frame between two copies of itself
            elif self.mode == "nearest":
                out = (self.before if 2 * r <= self.grid.p else self.last, None, 0)
            else:
                out = (self.before, self.last, r / self.grid.p)
            self.emit(self.m, *out)
            self.m += 1
