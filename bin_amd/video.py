"""YUV4MPEG2 (Y4M) streams: the header, a sequential reader and a writer.  Raw planar 8-bit YUV is what every decoder and encoder
speaks through a pipe, so `python -m bin_amd.test --input_video - --output_video -` sits between two of them; the colour
conversion, the chroma resampling, the padding and the crop are the two kernels of libbinyuv.so (ops.yuv_to_frame /
ops.frame_to_yuv, include/binyuv.h), nothing of a frame is touched on the host.

Supported: progressive 8-bit 4:2:0 (`C420jpeg`, `C420mpeg2`, `C420paldv`, `C420`, or no C tag) and 4:4:4 (`C444`).  The three 4:2:0
sitings are converted alike (chroma is replicated up and box-averaged down, which is an exact round trip); the tag passes through.
Interlaced streams, 4:2:2, mono and bit depths above 8 are refused by name."""
import sys
from dataclasses import dataclass, field, replace

MAGIC = b"YUV4MPEG2"
FRAME = b"FRAME"
CHROMA_420 = ("420jpeg", "420mpeg2", "420paldv", "420")
MAX_LINE = 4096                      # a header or FRAME line longer than this is not Y4M


@dataclass(frozen=True)
class Y4MHeader:
    """The stream header: W, H, the frame rate F as n:d, I (interlacing), A (pixel aspect), C (colour space; None = absent = 4:2:0) and
    the X tags verbatim (without the X)."""
    width: int
    height: int
    rate: tuple = (30, 1)
    interlace: str = None
    aspect: str = None
    colorspace: str = None
    extra: tuple = field(default_factory=tuple)

    @property
    def chroma(self):
        return 444 if self.colorspace == "444" else 420

    @property
    def full_range(self):
        """True / False from XCOLORRANGE=FULL / LIMITED, None when the stream does not say."""
        for x in self.extra:
            if x.upper().startswith("COLORRANGE="):
                return {"FULL": True, "LIMITED": False}.get(x.split("=", 1)[1].upper())
        return None

    @property
    def chroma_size(self):
        if self.chroma == 444:
            return self.height, self.width
        return (self.height + 1) // 2, (self.width + 1) // 2

    @property
    def frame_bytes(self):
        ch, cw = self.chroma_size
        return self.width * self.height + 2 * ch * cw

    def doubled(self):
        """The header of the interpolated stream: F = 2n:d, everything else unchanged."""
        return replace(self, rate=(2 * self.rate[0], self.rate[1]))

    def multiplied(self, f):
        """The header of a stream interpolated to f times the frame rate (--factor): F = f n:d, everything else unchanged."""
        if type(f) is not int or f < 1:
            raise ValueError(f"a frame rate is multiplied by a positive integer (got {f!r})")
        return replace(self, rate=(f * self.rate[0], self.rate[1]))

    def at_rate(self, rate):
        """The header of a stream resampled to the absolute frame rate `rate` (--output_rate; (N, D), N or a Fraction): F = N:D as
        written, not reduced any further; everything else unchanged."""
        from .rate import rate_pair
        return replace(self, rate=rate_pair(rate, "output rate"))

    def line(self):
        tags = [f"W{self.width}", f"H{self.height}", f"F{self.rate[0]}:{self.rate[1]}"]
        if self.interlace is not None:
            tags.append("I" + self.interlace)
        if self.aspect is not None:
            tags.append("A" + self.aspect)
        if self.colorspace is not None:
            tags.append("C" + self.colorspace)
        tags += ["X" + x for x in self.extra]
        return MAGIC + b" " + " ".join(tags).encode("ascii") + b"\n"


def parse_header(line):
    """The Y4MHeader of a header line (bytes or str, with or without its newline).  ValueError names what is refused."""
    if isinstance(line, bytes):
        line = line.decode("ascii", errors="replace")
    parts = line.rstrip("\n").split(" ")
    if parts[0] != MAGIC.decode():
        raise ValueError(f"not a YUV4MPEG2 stream (starts with {parts[0][:16]!r})")
    w = h = None
    rate, interlace, aspect, cs, extra = (30, 1), None, None, None, []
    for tag in (p for p in parts[1:] if p):
        key, val = tag[0], tag[1:]
        if key == "W":
            w = int(val)
        elif key == "H":
            h = int(val)
        elif key == "F":
            n, _, d = val.partition(":")
            rate = (int(n), int(d or 1))
        elif key == "I":
            if val in ("t", "b", "m"):
                raise ValueError(f"Y4M tag I{val}: interlaced streams are not supported")
            if val not in ("p", "?"):
                raise ValueError(f"Y4M tag I{val}: unknown interlacing")
            interlace = val
        elif key == "A":
            aspect = val
        elif key == "C":
            if val.startswith("422"):
                raise ValueError(f"Y4M tag C{val}: 4:2:2 is not supported")
            if val.startswith("mono"):
                raise ValueError(f"Y4M tag C{val}: mono is not supported")
            if val not in CHROMA_420 + ("444",):
                what = "bit depths above 8 are" if "p" in val[3:] and val[:3] in ("420", "444") else "this colour space is"
                raise ValueError(f"Y4M tag C{val}: {what} not supported")
            cs = val
        elif key == "X":
            extra.append(val)
        else:
            raise ValueError(f"Y4M tag {tag}: unknown header tag")
    if w is None or h is None or w < 1 or h < 1:
        raise ValueError("Y4M header without a positive W and H")
    if rate[0] < 1 or rate[1] < 1:
        raise ValueError(f"Y4M tag F{rate[0]}:{rate[1]}: not a frame rate")
    return Y4MHeader(w, h, rate, interlace, aspect, cs, tuple(extra))


def _open(target, mode):
    """(binary file object, whether this module opened it) of a path, a file object or `-`."""
    if target == "-":
        return (sys.stdin.buffer if "r" in mode else sys.stdout.buffer), False
    if isinstance(target, (str, bytes)) or hasattr(target, "__fspath__"):
        return open(target, mode), True
    return target, False


class Y4MReader:
    """Sequential reader of a path, a binary file object or `-` (stdin).  It never seeks and never reads past what it yields: a line
    is read byte by byte, a payload by its length, so it works on a pipe and leaves the stream at the next frame."""

    def __init__(self, source):
        self.f, self._mine = _open(source, "rb")
        self.index = 0
        first = self._line()
        if first is None:
            raise ValueError("empty Y4M stream")
        self.header = parse_header(first)

    def _line(self):
        out = bytearray()
        while True:
            c = self.f.read(1)
            if not c:
                if out:
                    raise ValueError(f"Y4M stream ends inside a line ({bytes(out[:16])!r}...)")
                return None
            if c == b"\n":
                return bytes(out)
            out += c
            if len(out) > MAX_LINE:
                raise ValueError("Y4M line of more than %d bytes" % MAX_LINE)

    def readinto(self, buf):
        """The next frame's payload into `buf` (a writable buffer of frame_bytes bytes).  False at the end of the stream."""
        line = self._line()
        if line is None:
            return False
        if line != FRAME and not line.startswith(FRAME + b" "):   # (a FRAME line may carry parameters)
            raise ValueError(f"Y4M frame {self.index}: expected a FRAME line, found {line[:16]!r}")
        view = memoryview(buf).cast("B")
        if len(view) != self.header.frame_bytes:
            raise ValueError(f"buffer of {len(view)} bytes for frames of {self.header.frame_bytes}")
        got = 0
        while got < len(view):                                    # a pipe returns short reads
            n = self.f.readinto(view[got:]) if hasattr(self.f, "readinto") else self._copy(view, got)
            if not n:
                raise ValueError(f"Y4M frame {self.index} is truncated: {got} of {len(view)} bytes")
            got += n
        self.index += 1
        return True

    def _copy(self, view, got):
        chunk = self.f.read(len(view) - got)
        view[got:got + len(chunk)] = chunk
        return len(chunk)

    def __iter__(self):
        while True:
            buf = bytearray(self.header.frame_bytes)
            if not self.readinto(buf):
                return
            yield buf

    def close(self):
        if self._mine:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Y4MWriter:
    """Writer to a path, a binary file object or `-` (stdout): the header line once, then `FRAME` and the payload per frame."""

    def __init__(self, target, header):
        self.f, self._mine = _open(target, "wb")
        self.header = header
        self.index = 0
        self.f.write(header.line())

    def write(self, payload):
        view = memoryview(payload).cast("B")
        if len(view) != self.header.frame_bytes:
            raise ValueError(f"Y4M frame {self.index}: payload of {len(view)} bytes for frames of {self.header.frame_bytes}")
        self.f.write(FRAME + b"\n")
        self.f.write(view)
        self.index += 1

    def close(self):
        self.f.flush()
        if self._mine:
            self.f.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def clip_info(path):
    """(Y4MHeader, number of frames) of a clip in a seekable file (a path or a seekable binary file object), without reading a payload.
    From the file size when every frame is a bare `FRAME` line and its payload (the size fits and FRAME stands at the first and at the
    last computed offset); otherwise by walking the FRAME lines with seeks.  ValueError names a trailing partial frame; `-` and
    objects that cannot seek are refused."""
    if isinstance(path, (str, bytes)) and path in ("-", b"-"):
        raise ValueError("clip_info needs a seekable file: `-` (a pipe) cannot be measured without reading it")
    f, mine = _open(path, "rb")
    try:
        if not (hasattr(f, "seekable") and f.seekable()):
            raise ValueError(f"clip_info needs a seekable file (got {f!r})")
        f.seek(0)
        rd = Y4MReader(f)
        header, start, size = rd.header, f.tell(), f.seek(0, 2)
        step = len(FRAME) + 1 + header.frame_bytes

        def bare(at):
            f.seek(at)
            return f.read(len(FRAME) + 1) == FRAME + b"\n"
        n, rest = divmod(size - start, step)
        if rest == 0 and (n == 0 or (bare(start) and bare(start + (n - 1) * step))):
            return header, n
        n, at = 0, start
        while at < size:
            f.seek(at)
            try:
                line = rd._line()
            except ValueError as e:
                raise ValueError(f"Y4M frame {n} is truncated: {e}") from None
            if line != FRAME and not line.startswith(FRAME + b" "):
                raise ValueError(f"Y4M frame {n}: expected a FRAME line, found {line[:16]!r}")
            at = f.tell() + header.frame_bytes
            if at > size:
                raise ValueError(f"Y4M frame {n} is truncated: {size - f.tell()} of {header.frame_bytes} bytes")
            n += 1
        return header, n
    finally:
        if mine:
            f.close()


def resolve_format(header, matrix="auto", range="auto"):
    """(chroma, matrix, range) of a stream for ops.yuv_to_frame / ops.frame_to_yuv.  matrix "auto": bt709 when W >= 1280 or H > 576,
    else bt601; range "auto": the header's XCOLORRANGE, else limited."""
    if matrix == "auto":
        matrix = "bt709" if (header.width >= 1280 or header.height > 576) else "bt601"
    if range == "auto":
        range = "full" if header.full_range else "limited"
    if matrix not in ("bt601", "bt709"):
        raise ValueError(f"unknown YUV matrix {matrix!r} (auto, bt601, bt709)")
    if range not in ("limited", "full"):
        raise ValueError(f"unknown YUV range {range!r} (auto, limited, full)")
    return header.chroma, matrix, range
