"""The domain of libbinhip.so's C ABI as ONE table (a plain helper module, imported by name): for every entry point of
include/binhip.h, what a valid call looks like and what the entry point refuses before it launches.

  BASELINES   id -> Baseline: `build(ctx)` returns the ctypes argument list of a VALID call at the smallest shape the entry point
              supports, one baseline per mode whose required pointers differ (nterms 1 / 3, each epilogue, with / without state,
              store_o3, ...).  Every device pointer comes from `ctx.p(name, nbytes)`: `nbytes` is how many bytes the callee may touch
              there, the contract tests/test_gpu_abi_baselines.py holds the kernels to with guard bands around exactly that size.
  MUTATIONS   (baseline id, {name: value}, expected code, reason): the baseline with those names overridden (a pointer name -> 0 is a
              NULL pointer, `images[1]` an entry of a pointer array) must return exactly `code`.
  LIMITS      (baseline id, last accepted override, first refused override, code, reason): both sides of a numeric limit.
  WORKSPACES  (baseline id, query entry point, its arguments, the size argument's name, geometries the call refuses): the query is
              non-zero for the baseline and 0 for every refused geometry, `bytes - 1` is BINHIP_E_WORKSPACE, `bytes` is accepted.

tests/test_cpu_abi_domain.py runs all of it on a machine without a GPU, where an ACCEPTED call cannot launch: validation passes, the
launch finds no device and the call returns a positive hipError_t.  Only the baselines ever run on a GPU.  Limits are named through
bin_amd/_lib.py's mirrors of the header's #defines, so a changed limit moves its rows."""
import collections
import ctypes as C

from bin_amd import _lib as L

E_ARG, E_SHAPE, E_WS = -1, -2, -3

# the four entry points that take nothing that can be wrong (tests/test_cpu_abi_domain.py holds this list literally)
EXEMPT = ("binhip_version", "binhip_device_cus", "binhip_charbonnier_partials", "binhip_profiler_destroy")

NHW_LIMIT = 1 << 26            # N H W of a convolution stays below it (plane < 2 GiB, include/binhip.h BinConvDesc)
LAYOUT_MAX_THREADS = (1 << 32) - 256     # layout entry points: one thread per output slot / element (include/binhip.h, "Launch limit")
TOP = {"N": 3, "H": 2731, "W": 8191}     # N H W = 2^26 - 1
MAX_IMAGES = 5                 # frames averaged by a FINAL epilogue / packed by binhip_pack_inputs
MAX_Y_CPG = 128                # binhip_conv2d_bwd_data: chunks per output group
SCORE_MAX_HW = 65535           # binhip_image_score / binhip_frame_score: H, W and (image score) n
GATHER_MAX_SLOTS = 32          # binhip_gather_windows: n_slots
GATHER_MAX_ITEMS = (1 << 31) - 1
PROF_MAX_LAUNCHES = 16384      # binhip_profiler_create
G11, U7 = 11, 7                # the two SSIM windows

Baseline = collections.namedtuple("Baseline", "id entry build accept cpu")
Mutation = collections.namedtuple("Mutation", "base over code why")
Limit = collections.namedtuple("Limit", "base ok bad code why")
Workspace = collections.namedtuple("Workspace", "base query qargs size_name refused")

BASELINES, MUTATIONS, LIMITS, WORKSPACES = collections.OrderedDict(), [], [], []


def lib():
    return L.lib()


class Ctx:
    """One materialisation of a baseline.  `over`: the mutation; `alloc(name, nbytes, fill)` -> the address of a buffer of `nbytes`
    (fill: 0 = zero bytes, a float = that fp32 value everywhere)."""

    def __init__(self, over, alloc):
        self.over, self.alloc, self.used, self.sizes, self.keep, self.after = dict(over), alloc, set(), {}, [], []

    def v(self, name, default):
        if name in self.over:
            self.used.add(name)
            return self.over[name]
        return default

    def p(self, name, nbytes, fill=0):
        """A required device pointer: the callee may touch `nbytes` bytes there."""
        if name in self.over:
            self.used.add(name)
            return self.over[name]
        self.sizes[name] = int(nbytes)
        return self.alloc(name, int(nbytes), fill)

    def null(self, name):
        """A pointer this mode does not pass."""
        return self.v(name, 0)

    def ptrs(self, name, n, nbytes, fill=0, absent=()):
        """A HOST array of `n` device pointers (NULL for the whole array: {name: 0}; entries in `absent` are NULL in the baseline)."""
        if self.v(name, 1) == 0:
            return None
        n = n if 0 <= n <= 64 else 1
        arr = (C.c_void_p * max(n, 1))()
        for i in range(n):
            arr[i] = self.null(f"{name}[{i}]") if i in absent else self.p(f"{name}[{i}]", nbytes, fill)
        self.keep.append(arr)
        return arr


def dummy_alloc():
    """Distinct, non-null, 256-byte aligned addresses that are never dereferenced."""
    count = [0]

    def alloc(name, nbytes, fill):
        count[0] += 1
        return count[0] << 36
    return alloc


def launched(rv, gpu):
    """What an accepted call returns: 0 on a GPU; without one, validation passed and the launch found no device (a hipError_t > 0)."""
    return rv == 0 if gpu else rv > 0


def baseline(entry, mode="", accept=launched, cpu=True):
    def deco(fn):
        bid = entry[len("binhip_"):] + ("/" + mode if mode else "")
        assert bid not in BASELINES, bid
        BASELINES[bid] = Baseline(bid, entry, fn, accept, cpu)
        return fn
    return deco


def mut(base, over, code, why):
    assert base in BASELINES, base
    MUTATIONS.append(Mutation(base, over, code, why))


def nulls(base, names, why, code=E_ARG):
    for n in names:
        mut(base, {n: 0}, code, why)


def dims(base, names, why, code=E_SHAPE, values=(0, -1)):
    for n in names:
        for v in values:
            mut(base, {n: v}, code, why)


def limit(base, ok, bad, code, why):
    assert base in BASELINES, base
    LIMITS.append(Limit(base, ok, bad, code, why))


def chunks(c):
    return (c + 15) // 16


def r32(c):
    return (c + 31) // 32 * 32


def plane(N, H, W):
    return N * H * W * 32              # bytes of one fp16 [N][H][W][16] chunk plane


def wbytes(rows_pad, cin_chunks, ks):
    return lib().binhip_weights_bytes(rows_pad, cin_chunks, ks)


def shape_of(c, default):
    s = L.BinRdnShape()
    s.G0, s.D, s.C, s.G = c.v("shape", default)
    return s


# ================================================================================================== host queries
@baseline("binhip_conv_cout_block", accept=lambda rv, gpu: rv == 32)
def _(c):
    return [c.v("ksize", 3), c.v("cout_pad", 32), c.v("nterms", 1)]


for _v in (0, -32, 48):
    mut("conv_cout_block", {"cout_pad": _v}, -1, "binhip_conv.hip bh_conv_cout_block: cout_pad is a positive multiple of 32, else -1")


@baseline("binhip_weights_bytes", accept=lambda rv, gpu: rv == 32 * 2 * 9 * 32)
def _(c):
    return [c.v("cout_pad", 32), c.v("cin_chunks", 2), c.v("ksize", 3)]


dims("weights_bytes", ("cout_pad", "cin_chunks", "ksize"), "binhip.h binhip_weights_bytes: 0 when an argument is not positive", code=0)


@baseline("binhip_dgrad_rows_pad", accept=lambda rv, gpu: rv == 224)
def _(c):
    return [c.v("ksize", 1), c.v("cin", 224)]


dims("dgrad_rows_pad", ("cin",), "binhip.h binhip_dgrad_rows_pad: 0 for cin <= 0", code=0, values=(0, -1, -100))


# ================================================================================================== binhip_conv2d_fwd
P_, S_, F_, X_ = L.EPI_PLANES, L.EPI_SHUFFLE, L.EPI_FINAL, L.EPI_FINAL_SUBPIX
CONV_MODES = {
    "planes-nt1": dict(ks=3, cc=1, cout=32, cp=32, nt=1, epi=P_, relu=1),
    "planes-nt3": dict(ks=3, cc=1, cout=32, cp=32, nt=3, epi=P_, relu=1),
    "planes-res-nt3": dict(ks=3, cc=1, cout=32, cp=32, nt=3, epi=P_, res=True),
    "planes-k1-nt1": dict(ks=1, cc=2, cout=20, cp=32, nt=1, epi=P_),
    "planes-k5-half-nt3": dict(ks=5, cc=2, cout=32, cp=32, nt=3, epi=P_, reserved=L.CONV_HALF_LAST_CHUNK),
    "shuffle-nt1": dict(ks=3, cc=2, cout=256, cp=256, nt=1, epi=S_),
    "shuffle-nt3": dict(ks=3, cc=2, cout=256, cp=256, nt=3, epi=S_),
    "final-nt1": dict(ks=3, cc=4, cout=3, cp=32, nt=1, epi=F_, nimg=2),
    "final-nt3": dict(ks=3, cc=4, cout=3, cp=32, nt=3, epi=F_, nimg=2),
    "final-noimg-nt1": dict(ks=3, cc=4, cout=3, cp=32, nt=1, epi=F_, nimg=0),
    "subpix-nt1": dict(ks=5, cc=2, cout=12, cp=32, nt=1, epi=X_, nimg=2),
    "subpix-nt3": dict(ks=5, cc=2, cout=12, cp=32, nt=3, epi=X_, nimg=2),
    "subpix-fold-nt3": dict(ks=5, cc=2, cout=12, cp=32, nt=3, epi=X_, nimg=2, reserved=L.CONV_UPNET_FOLD),
}


def _conv_fwd(m):
    def build(c):
        N, H, W = c.v("N", 1), c.v("H", 2), c.v("W", 2)
        ks, cc, cout, cp = c.v("ksize", m["ks"]), c.v("cin_chunks", m["cc"]), c.v("cout", m["cout"]), c.v("cout_pad", m["cp"])
        nt, epi = c.v("nterms", m["nt"]), c.v("epilogue", m["epi"])
        d = L.BinConvDesc()
        d.N, d.H, d.W, d.ksize, d.cin_chunks, d.cout, d.cout_pad, d.nterms, d.epilogue = N, H, W, ks, cc, cout, cp, nt, epi
        d.relu, d.x_cpg, d.x_group_stride = c.v("relu", m.get("relu", 0)), c.v("x_cpg", 0), c.v("x_group_stride", 0)
        d.n_images = nimg = c.v("n_images", m.get("nimg", 0))
        d.reserved = c.v("reserved", m.get("reserved", 0))
        d.status = c.p("status", 4)
        lo = m["nt"] == 3
        fold = m.get("reserved", 0) & L.CONV_UPNET_FOLD
        px = plane(N, H, W)
        x_hi = c.p("x_hi", cc * px)
        x_lo = c.p("x_lo", cc * px) if lo else c.null("x_lo")
        wb = cc * 5 * 4 * 32 * 16 * 2 if fold else wbytes(cp, cc, ks)          # (the folded slab: binhip.h BINHIP_PLAN_UPNET_FOLD)
        w_hi = c.p("w_hi", wb)
        w_lo = c.p("w_lo", wb) if lo else c.null("w_lo")
        bias = c.p("bias", cp * 4)
        res = m.get("res")
        res_hi = c.p("res_hi", chunks(cout) * px) if res else c.null("res_hi")
        res_lo = c.p("res_lo", chunks(cout) * px) if res and lo else c.null("res_lo")
        y_hi = y_lo = y_f32 = 0
        images = None
        if m["epi"] in (P_, S_):
            yb = chunks(cout) * px if m["epi"] == P_ else chunks(cout // 4) * 4 * px
            y_hi = c.p("y_hi", yb)
            y_lo = c.p("y_lo", yb) if lo else c.null("y_lo")
        else:
            fb = N * cout * H * W * 4                     # FINAL [N, cout, H, W]; FINAL_SUBPIX [N, cout / 4, 2H, 2W]: the same bytes
            y_f32 = c.p("y_f32", fb)
            if m.get("nimg") or "n_images" in c.over or "images" in c.over:
                images = c.ptrs("images", nimg, fb)
        return [None if c.v("d", 1) == 0 else C.byref(d), x_hi, x_lo, w_hi, w_lo, bias, res_hi, res_lo, y_hi, y_lo, y_f32, images, None]
    return build


for _mode, _m in CONV_MODES.items():
    baseline("binhip_conv2d_fwd", _mode)(_conv_fwd(_m))

_B = "conv2d_fwd/planes-nt1"
_PREP = "binhip_conv.hip bh_prepare_conv"
nulls(_B, ("d", "x_hi", "w_hi", "bias", "y_hi"), "binhip.h: every pointer of the call's mode is required")
nulls("conv2d_fwd/planes-nt3", ("x_lo", "w_lo", "y_lo"), "binhip.h nterms 3: the lo planes are read / stored by every x3 kernel")
nulls("conv2d_fwd/planes-res-nt3", ("res_lo",), "conv epilogue reads r_lo wherever has_res under nterms 3")
nulls("conv2d_fwd/shuffle-nt3", ("y_hi", "y_lo"), "SHUFFLE stores chunk planes")
for _b in ("conv2d_fwd/final-nt1", "conv2d_fwd/final-nt3", "conv2d_fwd/subpix-nt1", "conv2d_fwd/subpix-nt3", "conv2d_fwd/subpix-fold-nt3"):
    nulls(_b, ("y_f32",), "the FINAL epilogues store fp32 NCHW")
    nulls(_b, ("images", "images[0]", "images[1]"),
          "binhip_conv_common.h: both FINAL epilogues read a.img[t][idx] for every t < nimg (conv_x3_kernel<5, FINAL_SUBPIX> too)")
    limit(_b, {"n_images": MAX_IMAGES}, {"n_images": MAX_IMAGES + 1}, E_ARG, "ConvKArgs.img holds 5 frames")
    mut(_b, {"n_images": -1}, E_ARG, "binhip.h BinConvDesc.n_images: 0 .. 5")
dims(_B, ("N", "H", "W", "cin_chunks", "cout"), _PREP + ": every dimension is positive")
dims(_B, ("cout_pad",), "weight rows: a positive multiple of 32 that holds cout")
mut(_B, {"cout_pad": 48, "cout": 32}, E_SHAPE, "bh_conv_cout_block: cout_pad % 32")
mut(_B, {"cout": 48, "cout_pad": 32}, E_SHAPE, "och_limit comes from cout, the weights have cout_pad rows: cout <= cout_pad")
limit(_B, {"cout": 32}, {"cout": 33}, E_SHAPE, "cout <= cout_pad")
for _v in (0, 2, 7, -1):
    mut(_B, {"ksize": _v}, E_SHAPE, "binhip.h BinConvDesc.ksize: 1, 3 or 5 (bh_dispatch_conv has no other row)")
for _v in (0, 2, 4, -1):
    mut(_B, {"nterms": _v}, E_ARG, "binhip.h BinConvDesc.nterms: 1 or 3")
for _v in (3, 5, -1, 8):
    mut(_B, {"epilogue": _v}, E_ARG, "binhip.h BINHIP_EPI_*: 0, 1, 2, 4")
for _v in (4, 8, 1 << 30, -1):
    mut(_B, {"reserved": _v}, E_ARG, "binhip.h BinConvDesc.reserved: an undefined bit")
mut(_B, {"reserved": L.CONV_HALF_LAST_CHUNK}, E_ARG, "BINHIP_CONV_HALF_LAST_CHUNK with ksize != 5")
mut(_B, {"reserved": L.CONV_UPNET_FOLD}, E_ARG, "BINHIP_CONV_UPNET_FOLD outside FINAL_SUBPIX")
mut("conv2d_fwd/subpix-nt1", {"reserved": L.CONV_UPNET_FOLD}, E_ARG, "BINHIP_CONV_UPNET_FOLD with nterms 1")
mut("conv2d_fwd/shuffle-nt1", {"cout": 254}, E_SHAPE, "PixelShuffle(2): cout % 4")
mut("conv2d_fwd/shuffle-nt1", {"ksize": 1}, E_SHAPE, "bh_dispatch_conv: SHUFFLE exists for 3x3 only")
limit("conv2d_fwd/final-nt1", {"cout": 4}, {"cout": 5}, E_ARG, "binhip.h BINHIP_EPI_FINAL: cout <= 4")
for _b in ("conv2d_fwd/subpix-nt1", "conv2d_fwd/subpix-nt3"):
    for _v in (6, 16):
        mut(_b, {"cout": _v}, E_ARG, "binhip.h BINHIP_EPI_FINAL_SUBPIX: cout = 4 c', c' <= 3")
    mut(_b, {"ksize": 3}, E_SHAPE, "the fused UPNet is 5x5")
    mut(_b, {"cout_pad": 64}, E_SHAPE, "the fused UPNet has one 32-row block")
# x_cpg <= 0 is one group (binhip.h BinConvDesc.x_cpg), the stride is then ignored; a grouped input steps forward
limit(_B, {"x_cpg": -3, "x_group_stride": -64}, {"x_cpg": 1, "x_group_stride": -64}, E_SHAPE,
      "binhip.h BinConvDesc.x_cpg: <= 0 one group (stride ignored); > 0 needs x_group_stride >= 0 (conv_chunk_base steps forward)")
limit(_B, {"x_cpg": 1, "x_group_stride": 0}, {"x_cpg": 1, "x_group_stride": -1}, E_SHAPE, "x_group_stride >= 0 for a grouped input")
limit(_B, {"N": 3, "H": 2731, "W": 8191}, {"N": 1, "H": 8192, "W": 8192}, E_SHAPE, "N H W < 2^26 (3 * 2731 * 8191 = 2^26 - 1)")

# ================================================================================================== binhip_conv2d_bwd_data
BWD_DATA_MODES = {
    "plain-nt1": dict(nt=1),
    "plain-nt3": dict(nt=3),
    "res-acc-mask-nt3": dict(nt=3, res=1, acc=True, mask=1),
    "res-acc-mask-nt1": dict(nt=1, res=1, acc=True, mask=1),
    "grouped-nt1": dict(nt=1, y_cpg=1),
    "unshuf-nt1": dict(nt=1, unshuf=2),
}


def _bwd_data(m):
    def build(c):
        N, H, W = c.v("N", 1), c.v("H", 2), c.v("W", 2)
        ks, cc, cout, cp = c.v("ksize", 3), c.v("cin_chunks", 1), c.v("cout", 32), c.v("cout_pad", 32)
        nt = c.v("nterms", m["nt"])
        d = L.BinConvDesc()
        d.N, d.H, d.W, d.ksize, d.cin_chunks, d.cout, d.cout_pad, d.nterms = N, H, W, ks, cc, cout, cp, nt
        d.epilogue, d.reserved = c.v("epilogue", P_), c.v("reserved", m.get("unshuf", 0))
        d.status = c.p("status", 4)
        lo = m["nt"] == 3
        px = plane(N, H, W)
        och = chunks(cout)
        y_cpg = c.v("y_cpg", m.get("y_cpg", 0))
        stride = c.v("y_group_stride", 2 * px // 2 if m.get("y_cpg") else 0)      # elements: two planes per group, one of them used
        if m.get("y_cpg"):
            ybytes = (och - 1) * 2 * px + px                                       # och groups of one chunk, 2 planes apart
        elif m.get("unshuf"):
            ybytes = 4 * m["unshuf"] * plane(N, H // 2, W // 2)                    # 4 * y_unshuf planes at H/2 x W/2
        else:
            ybytes = och * px

        def pair(name, nbytes, on):
            return (c.p(name + "_hi", nbytes) if on else c.null(name + "_hi"),
                    c.p(name + "_lo", nbytes) if on and lo else c.null(name + "_lo"))
        gy = pair("gy", cc * px, True)
        wt = pair("wt", wbytes(cp, cc, ks), True)
        res = pair("res", m.get("res", 0) * px, m.get("res"))
        acc = pair("acc", ybytes, m.get("acc"))
        mask_hi = c.p("mask_hi", och * px) if m.get("mask") is not None else c.null("mask_hi")
        gx = pair("gx", ybytes, True)
        return [None if c.v("d", 1) == 0 else C.byref(d), gy[0], gy[1], wt[0], wt[1], c.p("zero_bias", cp * 4), res[0], res[1],
                c.v("res_chunks", m.get("res", 0)), acc[0], acc[1], mask_hi, c.v("mask_from", m.get("mask", 0)), y_cpg, stride, gx[0], gx[1],
                None]
    return build


for _mode, _m in BWD_DATA_MODES.items():
    baseline("binhip_conv2d_bwd_data", _mode)(_bwd_data(_m))

_B = "conv2d_bwd_data/plain-nt1"
nulls(_B, ("d", "gy_hi", "wt_hi", "zero_bias", "gx_hi"), "binhip.h binhip_conv2d_bwd_data: required pointers")
nulls("conv2d_bwd_data/plain-nt3", ("gy_lo", "wt_lo", "gx_lo"), "nterms 3: lo planes")
nulls("conv2d_bwd_data/res-acc-mask-nt3", ("res_lo", "acc_lo"), "nterms 3: a residual / accumulator comes as a hi/lo pair")
for _v in (S_, F_, X_, -1):
    mut(_B, {"epilogue": _v}, E_ARG, "backward-data stores chunk planes: epilogue must be BINHIP_EPI_PLANES")
mut(_B, {"reserved": -1}, E_ARG, "binhip.h BinConvDesc.reserved: y_unshuf is a plane count, negative is BINHIP_E_ARG")
dims(_B, ("N", "H", "W", "cin_chunks", "cout"), _PREP + ": every dimension is positive")
mut(_B, {"cout": 48, "cout_pad": 32}, E_SHAPE, "cout <= cout_pad (rows_pad of binhip_weights_relayout_dgrad)")
for _v in (0, 2):
    mut(_B, {"nterms": _v}, E_ARG, "nterms: 1 or 3")
limit(_B, {"y_cpg": MAX_Y_CPG, "y_group_stride": 64}, {"y_cpg": MAX_Y_CPG + 1, "y_group_stride": 64}, E_SHAPE,
      "y_cpg_inv = ceil(2^20 / y_cpg) divides exactly for y_cpg <= 128 only (binhip_conv_common.h)")
limit(_B, {"y_cpg": -2, "y_group_stride": -64}, {"y_cpg": 1, "y_group_stride": -64}, E_SHAPE,
      "binhip.h: y_cpg <= 0 one group (stride ignored); a grouped output steps forward: y_group_stride >= 0")
limit("conv2d_bwd_data/grouped-nt1", {"y_group_stride": 0}, {"y_group_stride": -1}, E_SHAPE, "y_group_stride >= 0")
_U = "conv2d_bwd_data/unshuf-nt1"
mut(_U, {"H": 3}, E_SHAPE, "y_unshuf: inverse PixelShuffle(2) needs H even")
mut(_U, {"W": 3}, E_SHAPE, "y_unshuf: inverse PixelShuffle(2) needs W even")
mut(_U, {"y_cpg": 1, "y_group_stride": 64}, E_SHAPE, "y_unshuf with a grouped output")
limit(_U, {"reserved": 2}, {"reserved": 1}, E_SHAPE, "binhip.h: 16 * y_unshuf >= cout (cout 32)")
# res_chunks / mask_from against the output chunk count: defined for every value (binhip.h binhip_conv2d_bwd_data)
_R = "conv2d_bwd_data/res-acc-mask-nt1"
for _v in (0, -1, 2, 1000):
    limit(_R, {"res_chunks": _v}, None, 0, "binhip.h: res_chunks <= 0 or beyond the output chunks = every chunk (only chunks < och_limit load)")
for _v in (-1, 0, 2, 1000):
    limit(_R, {"mask_from": _v}, None, 0, "binhip.h: mask_from <= 0 = every chunk, beyond the output chunks = none")
limit(_B, {"N": 3, "H": 2731, "W": 8191}, {"N": 1, "H": 8192, "W": 8192}, E_SHAPE, "N H W < 2^26")


# ================================================================================================== binhip_conv2d_bwd_weight
def _wgrad_q(c, m):
    return [c.v("ksize", m["ks"]), c.v("N", 1), c.v("H", 2), c.v("W", 2), c.v("cin_chunks", m["cc"]), c.v("cout", m["cout"])]


def _bwd_weight(m):
    def build(c):
        ks, N, H, W, cc, cout = _wgrad_q(c, m)
        nt = c.v("nterms", m["nt"])
        cin = c.v("cin", m["cin"])
        d = L.BinConvDesc()
        d.N, d.H, d.W, d.ksize, d.cin_chunks, d.cout, d.cout_pad, d.nterms = N, H, W, ks, cc, cout, r32(max(cout, 1)), nt
        d.x_cpg, d.x_group_stride = c.v("x_cpg", 0), c.v("x_group_stride", 0)
        lo = m["nt"] == 3
        px = plane(N, H, W)
        ws = lib().binhip_wgrad_workspace_bytes(ks, N, H, W, cc, cout)
        return [None if c.v("d", 1) == 0 else C.byref(d), c.p("x_hi", cc * px), c.p("x_lo", cc * px) if lo else c.null("x_lo"),
                c.p("gy_hi", chunks(cout) * px), c.p("gy_lo", chunks(cout) * px) if lo else c.null("gy_lo"),
                c.p("inv_scale", 4, 1.0) if m.get("inv") else c.null("inv_scale"), c.p("workspace", ws), c.v("workspace_bytes", ws),
                c.p("dw_oihw", cout * cin * ks * ks * 4), c.p("dbias", cout * 4) if m.get("db", True) else c.null("dbias"),
                cin, c.v("shuffle_perm", m.get("shuffle", 0)), c.v("accumulate", m.get("acc", 0)), None]
    return build


WGRAD_MODES = {
    "k3-nt1": dict(ks=3, cc=1, cout=32, cin=16, nt=1, inv=True),
    "k3-nt3": dict(ks=3, cc=1, cout=32, cin=16, nt=3, inv=True, acc=1),
    "k3-shuffle-nodb-nt1": dict(ks=3, cc=1, cout=32, cin=12, nt=1, shuffle=1, db=False),
    "k1-nt1": dict(ks=1, cc=2, cout=32, cin=32, nt=1),
    "k1-wide-nt3": dict(ks=1, cc=1, cout=128, cin=16, nt=3),
    "k5-nt1": dict(ks=5, cc=2, cout=32, cin=24, nt=1),
}
for _mode, _m in WGRAD_MODES.items():
    baseline("binhip_conv2d_bwd_weight", _mode)(_bwd_weight(_m))
    WORKSPACES.append(Workspace("conv2d_bwd_weight/" + _mode, "binhip_wgrad_workspace_bytes", (lambda c, m=_m: _wgrad_q(c, m)),
                                "workspace_bytes", [{"N": 0}, {"H": 0}, {"W": -1}, {"cin_chunks": 0}, {"cout": 0}, {"ksize": 2}]))


@baseline("binhip_wgrad_workspace_bytes", accept=lambda rv, gpu: rv > 0)
def _(c):
    return _wgrad_q(c, WGRAD_MODES["k3-nt1"])


dims("wgrad_workspace_bytes", ("N", "H", "W", "cin_chunks", "cout"), "binhip_wgrad.hip check_shape: 0 for a geometry the call refuses", code=0)
for _v in (0, 2, 4, 7):
    mut("wgrad_workspace_bytes", {"ksize": _v}, 0, "ksize: 1, 3 or 5")

_B = "conv2d_bwd_weight/k3-nt1"
_WG = "binhip_wgrad.hip bh_wgrad_partials"
nulls(_B, ("d", "x_hi", "gy_hi", "workspace", "dw_oihw"), _WG + ": required pointers (inv_scale and dbias may be NULL)")
nulls("conv2d_bwd_weight/k3-nt3", ("x_lo", "gy_lo"), "nterms 3: lo planes")
dims(_B, ("N", "H", "W", "cin_chunks", "cout"), "check_shape: every dimension is positive")
for _v in (0, 2, 4):
    mut(_B, {"ksize": _v}, E_SHAPE, "ksize: 1, 3 or 5")
for _v in (0, 2):
    mut(_B, {"nterms": _v}, E_ARG, "nterms: 1 or 3")
dims(_B, ("cin",), "cin: 1 .. 16 cin_chunks")
limit(_B, {"cin": 16}, {"cin": 17}, E_SHAPE, "cin <= 16 cin_chunks: dw rows beyond the planes do not exist")
mut(_B, {"shuffle_perm": 1, "cout": 30}, E_SHAPE, "shuffle_perm: PixelShuffle(2) row order needs cout % 4 == 0")
limit(_B, {"x_cpg": -3, "x_group_stride": -64}, {"x_cpg": 1, "x_group_stride": -64}, E_SHAPE,
      "binhip.h BinConvDesc.x_cpg: <= 0 one group; a grouped input steps forward (wg_x_plane)")
limit(_B, {"N": 3, "H": 2731, "W": 8191}, {"N": 1, "H": 8192, "W": 8192}, E_SHAPE, "N H W < 2^26")


# ================================================================================================== weight relayouts
def _relayout(m, dgrad):
    def build(c):
        cout, cin, ks = c.v("cout", m["cout"]), c.v("cin", m["cin"]), c.v("ksize", m["ks"])
        rows, cc, cb = c.v("rows_pad", m["rows"]), c.v("cin_chunks", m["cc"]), c.v("cout_block", m["cb"])
        sh = c.v("shuffle_perm", m.get("shuffle", 0))
        w = c.p("w_oihw", cout * cin * ks * ks * 4)
        w_hi = c.p("w_hi", wbytes(rows, cc, ks))
        w_lo = c.p("w_lo", wbytes(rows, cc, ks)) if m.get("lo") else c.null("w_lo")
        bias_out = c.p("bias_out", rows * 4)
        if dgrad:
            return [w, cout, cin, ks, rows, cc, cb, sh, w_hi, w_lo, bias_out, None]
        bias = c.p("bias", cout * 4) if m.get("bias") else c.null("bias")
        return [w, bias, cout, cin, ks, rows, cc, cb, sh, w_hi, w_lo, bias_out, None]
    return build


RELAYOUT_MODES = {
    "hi": dict(cout=20, cin=12, ks=3, rows=32, cc=1, cb=32),
    "hi-lo-bias": dict(cout=32, cin=16, ks=1, rows=32, cc=1, cb=32, lo=True, bias=True),
    "shuffle-k5": dict(cout=64, cin=16, ks=5, rows=64, cc=1, cb=32, lo=True, bias=True, shuffle=1),
}
DGRAD_MODES = {
    "hi": dict(cout=20, cin=12, ks=3, rows=32, cc=2, cb=32),
    "hi-lo-shuffle": dict(cout=32, cin=40, ks=3, rows=64, cc=2, cb=64, lo=True, shuffle=1),
}
for _mode, _m in RELAYOUT_MODES.items():
    baseline("binhip_weights_relayout", _mode)(_relayout(_m, False))
for _mode, _m in DGRAD_MODES.items():
    baseline("binhip_weights_relayout_dgrad", _mode)(_relayout(_m, True))
_RC = "binhip_relayout.hip relayout_check"
for _B in ("weights_relayout/hi", "weights_relayout_dgrad/hi"):
    nulls(_B, ("w_oihw", "w_hi", "bias_out"), _RC + ": required pointers (bias and w_lo may be NULL)")
    dims(_B, ("cout", "cin", "cin_chunks", "rows_pad", "cout_block"), _RC + ": every dimension is positive")
    for _v in (0, 2, 4, -1):
        mut(_B, {"ksize": _v}, E_SHAPE, "ksize: 1, 3 or 5 (the layouts the convolution kernels read)")
    mut(_B, {"rows_pad": 48, "cout_block": 48}, E_SHAPE, "rows_pad % 32")
    mut(_B, {"cout_block": 40}, E_SHAPE, "cout_block: a multiple of 32 that divides rows_pad")
    mut(_B, {"rows_pad": 64, "cout_block": 48}, E_SHAPE, "cout_block divides rows_pad")
limit("weights_relayout/hi", {"cout": 32}, {"cout": 33}, E_SHAPE, "cout <= cout_pad: rows beyond the plane")
limit("weights_relayout/hi", {"cin": 16}, {"cin": 17}, E_SHAPE, "cin <= 16 cin_chunks")
limit("weights_relayout_dgrad/hi", {"cin": 32}, {"cin": 33}, E_SHAPE, "dgrad rows = cin <= rows_pad")
limit("weights_relayout_dgrad/hi", {"cout": 32}, {"cout": 33}, E_SHAPE, "dgrad K = cout <= 16 cin_chunks")
mut("weights_relayout/hi", {"shuffle_perm": 1, "cout": 20}, E_SHAPE, "shuffle_perm: cout == cout_pad (20 != 32)")
mut("weights_relayout/shuffle-k5", {"cout": 62}, E_SHAPE, "shuffle_perm: cout % 4 and cout == cout_pad")
mut("weights_relayout_dgrad/hi-lo-shuffle", {"cout": 30}, E_SHAPE, "shuffle_perm: cout % 4")


def _gather_build(group, nt_lo):
    def build(c):
        g = c.v("group", group)
        rows, cc = (96 if group == 0 else 32), 2 * (4 - group)
        if c.v("w_oihw4", 1) == 0:
            w4 = None
        else:
            w4 = (C.c_void_p * 4)()
            for k in range(4):      # conv k of bin_stage4's block: [32][96 + 32 k][3][3] fp32; entries below `group` may be NULL
                w4[k] = c.null(f"w_oihw4[{k}]") if k < group else c.p(f"w_oihw4[{k}]", 32 * (96 + 32 * k) * 9 * 4)
            c.keep.append(w4)
        return [w4, g, c.v("cout_block", 32), c.p("w_hi", wbytes(rows, cc, 3)), c.p("w_lo", wbytes(rows, cc, 3)) if nt_lo else c.null("w_lo"),
                c.p("bias_out", rows * 4), None]
    return build


baseline("binhip_weights_relayout_rdb_gather", "group0-hi-lo")(_gather_build(0, True))
baseline("binhip_weights_relayout_rdb_gather", "group3-hi")(_gather_build(3, False))
_B = "weights_relayout_rdb_gather/group0-hi-lo"
nulls(_B, ("w_oihw4", "w_hi", "bias_out"), "required pointers")
nulls(_B, tuple(f"w_oihw4[{k}]" for k in range(4)), "fetch_gather reads w[conv] of every conv >= group")
nulls("weights_relayout_rdb_gather/group3-hi", ("w_oihw4[3]",), "fetch_gather reads w[conv] of every conv >= group")
limit(_B, {"group": 0}, {"group": -1}, E_ARG, "binhip.h: group 0 .. 3")
mut("weights_relayout_rdb_gather/group3-hi", {"group": 4}, E_ARG, "binhip.h: group 0 .. 3")
mut("weights_relayout_rdb_gather/group3-hi", {"group": 7}, E_ARG, "binhip.h: group 0 .. 3")
dims(_B, ("cout_block",), "cout_block: a multiple of 32 that divides the rows")
mut(_B, {"cout_block": 64}, E_SHAPE, "cout_block divides the 96 rows")


def _item(c, i, kind):
    """One BinRelayoutItem of the batch baseline: FWD, DGRAD, and group 1 of a (32, -, 2, 32) block in gather form."""
    it = L.BinRelayoutItem()
    pre = f"items[{i}]."
    kind_v = c.v(pre + "kind", kind)
    if kind == L.RELAYOUT_RDB_GATHER:
        G0, Cc, G, g = 32, 2, 32, 1
        it.shape.G0, it.shape.C, it.shape.G = c.v(pre + "shape.G0", G0), c.v(pre + "shape.C", Cc), c.v(pre + "shape.G", G)
        for k in range(Cc):
            it.w[k] = c.null(pre + f"w[{k}]") if k < g and k > 0 else c.p(pre + f"w[{k}]", G * (G0 + G * k) * 9 * 4)
        rows, cc, ks, cout, cin = G, (Cc - g) * G // 16, 3, G, G0 + G * g
        it.shuffle_or_group = c.v(pre + "shuffle_or_group", g)
    else:
        cout, cin, ks = (20, 12, 3) if kind == L.RELAYOUT_FWD else (32, 40, 1)
        rows, cc = (32, 1) if kind == L.RELAYOUT_FWD else (64, 2)
        it.w[0] = c.p(pre + "w[0]", cout * cin * ks * ks * 4)
        it.bias = c.p(pre + "bias", cout * 4) if kind == L.RELAYOUT_FWD else 0
        it.shuffle_or_group = c.v(pre + "shuffle_or_group", 0)
    rows, cc, ks = c.v(pre + "rows_pad", rows), c.v(pre + "cin_chunks", cc), c.v(pre + "ksize", ks)
    it.w_hi, it.w_lo, it.bias_out = c.p(pre + "w_hi", wbytes(rows, cc, ks)), c.p(pre + "w_lo", wbytes(rows, cc, ks)), c.p(pre + "bias_out", rows * 4)
    it.kind, it.cout, it.cin, it.ksize, it.rows_pad, it.cin_chunks = kind_v, c.v(pre + "cout", cout), c.v(pre + "cin", cin), ks, rows, cc
    it.cout_block = c.v(pre + "cout_block", 32)
    return it


@baseline("binhip_weights_relayout_batch")
def _(c):
    n = c.v("n", 3)
    if c.v("items", 1) == 0:
        return [None, n, None]
    arr = (L.BinRelayoutItem * 3)(*[_item(c, i, k) for i, k in enumerate((L.RELAYOUT_FWD, L.RELAYOUT_DGRAD, L.RELAYOUT_RDB_GATHER))])
    return [arr, n, None]


_B = "weights_relayout_batch"
nulls(_B, ("items",), "binhip_weights_relayout_batch: items")
dims(_B, ("n",), "n >= 1", code=E_ARG)
for _i in range(3):
    nulls(_B, tuple(f"items[{_i}].{f}" for f in ("w[0]", "w_hi", "bias_out")), _RC + ": an item names w[0], w_hi and bias_out whatever its kind")
    for _v in (3, -1):
        mut(_B, {f"items[{_i}].kind": _v}, E_ARG, "binhip.h BINHIP_RELAYOUT_*: 0, 1, 2")
nulls(_B, ("items[2].w[1]",), "RDB_GATHER: w[k] for every conv k >= group")
limit(_B, {"items[2].shuffle_or_group": 1}, {"items[2].shuffle_or_group": 2}, E_ARG, "RDB_GATHER: group < C")
mut(_B, {"items[2].shuffle_or_group": -1}, E_ARG, "RDB_GATHER: group >= 0")
mut(_B, {"items[2].shape.C": L.RDN_MAX_CONVS + 1}, E_SHAPE, "RDB_GATHER: C <= BINHIP_RDN_MAX_CONVS (BinRelayoutItem.w holds C pointers)")
mut(_B, {"items[2].shape.G": 48}, E_SHAPE, "RDB_GATHER: G % 32")
mut(_B, {"items[2].shape.G0": 48}, E_SHAPE, "RDB_GATHER: G0 % 32")
mut(_B, {"items[2].rows_pad": 64}, E_SHAPE, "RDB_GATHER: rows_pad = G for group >= 1")
mut(_B, {"items[2].cin_chunks": 4}, E_SHAPE, "RDB_GATHER: cin_chunks = (C - group) G / 16")
mut(_B, {"items[2].ksize": 1}, E_SHAPE, "RDB_GATHER: 3x3")
mut(_B, {"items[0].ksize": 2}, E_SHAPE, "ksize: 1, 3 or 5")
mut(_B, {"items[1].cout_block": 48}, E_SHAPE, "cout_block % 32")


# ================================================================================================== layout glue
def _nchw(scaled, lo):
    def build(c):
        N, Cn, H, W = c.v("N", 1), c.v("C", 3), c.v("H", 2), c.v("W", 3)
        yb = chunks(Cn) * plane(N, H, W)
        a = [c.p("x", N * Cn * H * W * 4), N, Cn, H, W]
        if scaled:
            a.append(c.p("scale", 8, 1.0))
        return a + [c.p("y_hi", yb), c.p("y_lo", yb) if lo else c.null("y_lo"), c.p("status", 4), None]
    return build


for _lo in (False, True):
    baseline("binhip_nchw_to_planes", "hi-lo" if _lo else "hi")(_nchw(False, _lo))
    baseline("binhip_nchw_to_planes_scaled", "hi-lo" if _lo else "hi")(_nchw(True, _lo))
nulls("nchw_to_planes/hi", ("x", "y_hi"), "binhip_layout.hip: x and y_hi (y_lo, status may be NULL)")
nulls("nchw_to_planes_scaled/hi", ("x", "y_hi", "scale"), "binhip_layout.hip: x, y_hi and scale")
dims("nchw_to_planes/hi", ("N", "C", "H", "W"), "every dimension is positive")
dims("nchw_to_planes_scaled/hi", ("N", "C", "H", "W"), "every dimension is positive")
for _b in ("nchw_to_planes/hi", "nchw_to_planes_scaled/hi-lo"):      # chunks * (2^26 - 1) * 2 slots: 31 chunks fit, 32 make 2^32 - 64
    limit(_b, dict(TOP, C=31 * 16), dict(TOP, C=31 * 16 + 1), E_SHAPE, "one thread per 16-byte slot: at most 2^32 - 256 (launch limit)")


def _planes_to_nchw(lo):
    def build(c):
        N, Cn, H, W = c.v("N", 1), c.v("C", 20), c.v("H", 3), c.v("W", 2)
        xb = chunks(Cn) * plane(N, H, W)
        return [c.p("x_hi", xb), c.p("x_lo", xb) if lo else c.null("x_lo"), N, Cn, H, W, c.p("y", N * Cn * H * W * 4), None]
    return build


baseline("binhip_planes_to_nchw", "hi")(_planes_to_nchw(False))
baseline("binhip_planes_to_nchw", "hi-lo")(_planes_to_nchw(True))
nulls("planes_to_nchw/hi", ("x_hi", "y"), "x_hi and y")
dims("planes_to_nchw/hi", ("N", "C", "H", "W"), "every dimension is positive")
limit("planes_to_nchw/hi-lo", dict(TOP, C=63), dict(TOP, C=64), E_SHAPE, "one thread per element: 64 * (2^26 - 1) = 2^32 - 64 > 2^32 - 256")


@baseline("binhip_pixel_unshuffle_f32")
def _(c):
    N, Cn, H, W, r = c.v("N", 1), c.v("C", 3), c.v("H", 4), c.v("W", 6), c.v("r", 2)
    return [c.p("x", N * Cn * H * W * 4), N, Cn, H, W, r, c.p("y", N * Cn * H * W * 4), None]


nulls("pixel_unshuffle_f32", ("x", "y"), "x and y")
dims("pixel_unshuffle_f32", ("N", "C", "H", "W", "r"), "every dimension and r are positive")
mut("pixel_unshuffle_f32", {"H": 5}, E_SHAPE, "H % r")
mut("pixel_unshuffle_f32", {"W": 7}, E_SHAPE, "W % r")
mut("pixel_unshuffle_f32", {"r": 4}, E_SHAPE, "H % r (4 % 4 == 0 but 6 % 4 != 0)")
limit("pixel_unshuffle_f32", dict(TOP, C=63, r=1), dict(TOP, C=64, r=1), E_SHAPE, "one thread per element: at most 2^32 - 256 (launch limit)")


def _pack(n, lo):
    def build(c):
        nimg, N, H, W = c.v("n_images", n), c.v("N", 1), c.v("H", 2), c.v("W", 4)
        yb = chunks(12 * n) * plane(N, H // 2, W // 2)
        return [c.ptrs("images", nimg, N * 3 * H * W * 4), nimg, N, H, W, c.p("y_hi", yb), c.p("y_lo", yb) if lo else c.null("y_lo"),
                c.p("status", 4), None]
    return build


baseline("binhip_pack_inputs", "2-hi")(_pack(2, False))
baseline("binhip_pack_inputs", "5-hi-lo")(_pack(5, True))
nulls("pack_inputs/2-hi", ("images", "y_hi", "images[0]", "images[1]"), "pack_inputs_kernel reads a.img[im] of every frame")
nulls("pack_inputs/5-hi-lo", tuple(f"images[{i}]" for i in range(5)), "pack_inputs_kernel reads a.img[im] of every frame")
dims("pack_inputs/2-hi", ("n_images", "N", "H", "W"), "every dimension is positive")
mut("pack_inputs/2-hi", {"H": 3}, E_SHAPE, "pixel_reshuffle(2): H even")
mut("pack_inputs/2-hi", {"W": 5}, E_SHAPE, "pixel_reshuffle(2): W even")
limit("pack_inputs/5-hi-lo", {"n_images": MAX_IMAGES}, {"n_images": MAX_IMAGES + 1}, E_SHAPE, "PackArgs.img holds 5 frames")
# 4 chunks * N * H/2 * W/2 * 2 slots = 2 N H W: the limit sits at N H W = 2^31 - 128, far above the 2^26 of the convolutions behind it
limit("pack_inputs/5-hi-lo", {"N": 1, "H": 65536, "W": 32766}, {"N": 1, "H": 65536, "W": 32768}, E_SHAPE,
      "one thread per 16-byte slot: at most 2^32 - 256 (launch limit)")


@baseline("binhip_u8_to_frame")
def _(c):
    H, W = c.v("H", 2), c.v("W", 3)
    pl, pr, pt, pb = c.v("pad_left", 1), c.v("pad_right", 2), c.v("pad_top", 0), c.v("pad_bottom", 1)
    return [c.p("bgr_hwc", H * W * 3), H, W, pl, pr, pt, pb, c.p("out_chw", 3 * (H + pt + pb) * (W + pl + pr) * 4), None]


nulls("u8_to_frame", ("bgr_hwc", "out_chw"), "both pointers")
dims("u8_to_frame", ("H", "W"), "H, W positive")
for _n in ("pad_left", "pad_right", "pad_top", "pad_bottom"):
    limit("u8_to_frame", {_n: 0}, {_n: -1}, E_SHAPE, "pads are >= 0")


@baseline("binhip_frame_to_u8")
def _(c):
    Hp, Wp, top, left, H, W = c.v("Hp", 4), c.v("Wp", 5), c.v("top", 1), c.v("left", 2), c.v("H", 3), c.v("W", 3)
    return [c.p("chw", 3 * Hp * Wp * 4), Hp, Wp, top, left, H, W, c.p("bgr_hwc", H * W * 3), None]


nulls("frame_to_u8", ("chw", "bgr_hwc"), "both pointers")
dims("frame_to_u8", ("H", "W"), "H, W positive")
limit("frame_to_u8", {"top": 0}, {"top": -1}, E_SHAPE, "top >= 0")
limit("frame_to_u8", {"left": 0}, {"left": -1}, E_SHAPE, "left >= 0")
limit("frame_to_u8", {"top": 1, "H": 3, "Hp": 4}, {"top": 2, "H": 3, "Hp": 4}, E_SHAPE, "top + H <= Hp: the crop lies inside the frame")
limit("frame_to_u8", {"left": 2, "W": 3, "Wp": 5}, {"left": 3, "W": 3, "Wp": 5}, E_SHAPE, "left + W <= Wp")


def _unshuffle(lo):
    def build(c):
        N, H, W, n = c.v("N", 1), c.v("H", 1), c.v("W", 2), c.v("nchunks", 1)
        xb = n * plane(N, 2 * H, 2 * W)
        return [c.p("x_hi", xb), c.p("x_lo", xb) if lo else c.null("x_lo"), N, H, W, n, c.p("y_hi", xb), c.p("y_lo", xb) if lo else c.null("y_lo"), None]
    return build


baseline("binhip_unshuffle_planes", "hi")(_unshuffle(False))
baseline("binhip_unshuffle_planes", "hi-lo")(_unshuffle(True))
nulls("unshuffle_planes/hi", ("x_hi", "y_hi"), "x_hi and y_hi")
nulls("unshuffle_planes/hi-lo", ("x_lo", "y_lo"), "x_lo and y_lo come together")
dims("unshuffle_planes/hi", ("N", "H", "W", "nchunks"), "every dimension is positive")
limit("unshuffle_planes/hi-lo", dict(TOP, nchunks=7), dict(TOP, nchunks=8), E_SHAPE, "4 nchunks N H W 2 slots: 64 * (2^26 - 1) > 2^32 - 256 (launch limit)")


def _unpack(n, full):
    def build(c):
        nimg, N, H, W = c.v("n_images", n), c.v("N", 1), c.v("H", 2), c.v("W", 4)
        gb = chunks(12 * n) * plane(N, H // 2, W // 2)
        fb = N * 3 * H * W * 4
        return [c.p("gx0_hi", gb) if full else c.null("gx0_hi"), c.p("gx0_lo", gb) if full else c.null("gx0_lo"), c.p("gout", fb),
                c.p("scale", 8, 1.0) if full else c.null("scale"), nimg, N, H, W, c.ptrs("outs", nimg, fb, absent=() if full else (1,)), None]
    return build


baseline("binhip_unpack_input_grads", "3-full")(_unpack(3, True))
baseline("binhip_unpack_input_grads", "2-skip-only")(_unpack(2, False))
nulls("unpack_input_grads/3-full", ("gout", "outs"), "gout and outs (gx0, scale and single outs[i] may be NULL: binhip.h)")
dims("unpack_input_grads/3-full", ("n_images", "N", "H", "W"), "every dimension is positive")
mut("unpack_input_grads/3-full", {"H": 3}, E_SHAPE, "H even")
mut("unpack_input_grads/3-full", {"W": 5}, E_SHAPE, "W even")
limit("unpack_input_grads/3-full", {"n_images": MAX_IMAGES}, {"n_images": MAX_IMAGES + 1}, E_SHAPE, "UnpackArgs.out holds 5 frames")
limit("unpack_input_grads/3-full", {"N": 1, "H": 32768, "W": 43690}, {"N": 1, "H": 32768, "W": 43692}, E_SHAPE,
      "one thread per element of one frame, 3 N H W: at most 2^32 - 256 (launch limit)")


# ================================================================================================== ConvLSTM
def _lstm_fwd(state):
    def build(c):
        N, H, W = c.v("N", 1), c.v("H", 2), c.v("W", 3)
        fb = N * 3 * H * W * 4
        return [c.p("x", fb), c.p("c_prev", fb) if state else c.null("c_prev"), c.p("h_prev", fb) if state else c.null("h_prev"),
                c.p("w", 12 * 6 * 9 * 4), c.p("b", 12 * 4), 1.0, N, H, W, c.p("c_new", fb), c.p("h_new", fb), None]
    return build


baseline("binhip_convlstm_fwd", "state")(_lstm_fwd(True))
baseline("binhip_convlstm_fwd", "zero-state")(_lstm_fwd(False))
nulls("convlstm_fwd/state", ("x", "w", "b", "h_new"), "x, w, b and h_new (c_new may be NULL: binhip.h)")
nulls("convlstm_fwd/state", ("c_prev", "h_prev"), "binhip.h: c_prev / h_prev both present or both absent")
mut("convlstm_fwd/zero-state", {"c_prev": 1 << 40}, E_ARG, "c_prev / h_prev both present or both absent")
mut("convlstm_fwd/zero-state", {"h_prev": 1 << 40}, E_ARG, "c_prev / h_prev both present or both absent")
dims("convlstm_fwd/state", ("N", "H", "W"), "every dimension is positive")


def _gates_fwd(state):
    def build(c):
        N, hid, H, W = c.v("N", 1), c.v("hidden", 2), c.v("H", 2), c.v("W", 3)
        fb = N * hid * H * W * 4
        return [c.p("gates", 4 * fb), c.p("c_prev", fb) if state else c.null("c_prev"), 1.0, N, hid, H, W, c.p("c_new", fb), c.p("h_new", fb), None]
    return build


baseline("binhip_lstm_gates_fwd", "state")(_gates_fwd(True))
baseline("binhip_lstm_gates_fwd", "zero-state")(_gates_fwd(False))
nulls("lstm_gates_fwd/state", ("gates", "c_new", "h_new"), "lstm_gates_fwd_kernel stores both outputs")
dims("lstm_gates_fwd/state", ("N", "hidden", "H", "W"), "every dimension is positive")


def _gates_bwd(gh, gc, cprev):
    def build(c):
        N, hid, H, W = c.v("N", 1), c.v("hidden", 2), c.v("H", 2), c.v("W", 3)
        fb = N * hid * H * W * 4
        return [c.p("gates", 4 * fb), c.p("c_prev", fb) if cprev else c.null("c_prev"), c.p("g_h", fb) if gh else c.null("g_h"),
                c.p("g_c", fb) if gc else c.null("g_c"), 1.0, N, hid, H, W, c.p("g_gates", 4 * fb), c.p("g_cprev", fb) if cprev else c.null("g_cprev"),
                None]
    return build


baseline("binhip_lstm_gates_bwd", "gh-gc-state")(_gates_bwd(True, True, True))
baseline("binhip_lstm_gates_bwd", "gh")(_gates_bwd(True, False, False))
baseline("binhip_lstm_gates_bwd", "gc")(_gates_bwd(False, True, False))
nulls("lstm_gates_bwd/gh-gc-state", ("gates", "g_gates"), "gates and g_gates")
nulls("lstm_gates_bwd/gh", ("g_h",), "binhip.h: g_h and g_c not both NULL")
nulls("lstm_gates_bwd/gc", ("g_c",), "binhip.h: g_h and g_c not both NULL")
dims("lstm_gates_bwd/gh-gc-state", ("N", "hidden", "H", "W"), "every dimension is positive")


def _lstm_q(c):
    return [c.v("N", 1), c.v("H", 2), c.v("W", 3)]


@baseline("binhip_convlstm_bwd_workspace_bytes", accept=lambda rv, gpu: rv > 0)
def _(c):
    return _lstm_q(c)


dims("convlstm_bwd_workspace_bytes", ("N", "H", "W"), "0 for a geometry the call refuses", code=0)


def _lstm_bwd(state, gh, gc, outs):
    def build(c):
        N, H, W = _lstm_q(c)
        fb = N * 3 * H * W * 4
        ws = lib().binhip_convlstm_bwd_workspace_bytes(N, H, W)

        def opt(name, nbytes, on):
            return c.p(name, nbytes) if on else c.null(name)
        return [c.p("x", fb), opt("c_prev", fb, state), opt("h_prev", fb, state), c.p("w", 648 * 4), c.p("b", 48), 1.0, N, H, W,
                opt("g_h", fb, gh), opt("g_c", fb, gc), c.p("workspace", ws), c.v("workspace_bytes", ws), opt("gx", fb, outs),
                opt("g_hprev", fb, outs and state), opt("g_cprev", fb, outs and state), opt("dw", 648 * 4, outs), opt("db", 48, outs), None]
    return build


baseline("binhip_convlstm_bwd", "state-all")(_lstm_bwd(True, True, True, True))
baseline("binhip_convlstm_bwd", "zero-state-gh")(_lstm_bwd(False, True, False, True))
baseline("binhip_convlstm_bwd", "gc-no-outputs")(_lstm_bwd(False, False, True, False))
nulls("convlstm_bwd/state-all", ("x", "w", "b", "workspace"), "x, w, b and workspace (any output may be NULL: binhip.h)")
nulls("convlstm_bwd/state-all", ("c_prev", "h_prev"), "c_prev / h_prev both present or both absent")
nulls("convlstm_bwd/zero-state-gh", ("g_h",), "g_h and g_c not both NULL")
nulls("convlstm_bwd/gc-no-outputs", ("g_c",), "g_h and g_c not both NULL")
dims("convlstm_bwd/state-all", ("N", "H", "W"), "every dimension is positive")
for _b in ("convlstm_bwd/state-all", "convlstm_bwd/zero-state-gh"):
    WORKSPACES.append(Workspace(_b, "binhip_convlstm_bwd_workspace_bytes", _lstm_q, "workspace_bytes", [{"N": 0}, {"H": -1}, {"W": 0}]))


# ================================================================================================== losses
def _partials(numel, terms=1):
    return terms * lib().binhip_charbonnier_partials(numel) * 4


def _loss_fwd(kinded):
    def build(c):
        n = c.v("numel", 7)
        a = [c.p("x", n * 4), c.p("y", n * 4), n, 1e-6, c.p("partials", _partials(n)), c.p("loss", 4), None]
        return ([c.v("kind", kinded)] + a) if kinded is not None else a
    return build


def _loss_bwd(kinded, gx, gy):
    def build(c):
        n = c.v("numel", 7)
        a = [c.p("x", n * 4), c.p("y", n * 4), n, 1e-6, c.p("gloss", 4, 1.0), c.p("gx", n * 4) if gx else c.null("gx"),
             c.p("gy", n * 4) if gy else c.null("gy"), None]
        return ([c.v("kind", kinded)] + a) if kinded is not None else a
    return build


baseline("binhip_charbonnier_fwd")(_loss_fwd(None))
baseline("binhip_charbonnier_bwd", "gx-gy")(_loss_bwd(None, True, True))
baseline("binhip_charbonnier_bwd", "gy")(_loss_bwd(None, False, True))
for _k, _nm in ((L.LOSS_CHARBONNIER, "cb"), (L.LOSS_L1_SUM, "l1"), (L.LOSS_L2_SUM, "l2")):
    baseline("binhip_pixel_loss_fwd", _nm)(_loss_fwd(_k))
    baseline("binhip_pixel_loss_bwd", _nm + "-gx")(_loss_bwd(_k, True, False))
for _b in ("charbonnier_fwd", "pixel_loss_fwd/cb"):
    nulls(_b, ("x", "y", "partials", "loss"), "binhip_loss.hip: every pointer")
    dims(_b, ("numel",), "numel >= 1")
for _b in ("charbonnier_bwd/gx-gy", "pixel_loss_bwd/cb-gx"):
    nulls(_b, ("x", "y", "gloss"), "x, y and gloss")
    dims(_b, ("numel",), "numel >= 1")
nulls("charbonnier_bwd/gy", ("gy",), "binhip.h: gx and gy not both NULL")
nulls("pixel_loss_bwd/l1-gx", ("gx",), "binhip.h: gx and gy not both NULL")
for _b in ("pixel_loss_fwd/cb", "pixel_loss_bwd/cb-gx"):
    limit(_b, {"kind": L.LOSS_L2_SUM}, {"kind": L.LOSS_L2_SUM + 1}, E_ARG, "binhip.h BINHIP_LOSS_*: 0, 1, 2")
    mut(_b, {"kind": -1}, E_ARG, "binhip.h BINHIP_LOSS_*: 0, 1, 2")


def _terms(c, T, numel):
    t = L.BinLossTerms()
    t.n_terms = nt = c.v("n_terms", T)
    for i in range(T):
        t.x[i], t.y[i] = c.p(f"t.x[{i}]", numel * 4), c.p(f"t.y[{i}]", numel * 4)
    return t, nt


def _multi_fwd(T):
    def build(c):
        n = c.v("numel", 5)
        t, nt = _terms(c, T, n)
        return [c.v("kind", L.LOSS_CHARBONNIER), None if c.v("t", 1) == 0 else C.byref(t), n, 1e-6, c.p("partials", _partials(n, T)),
                c.p("terms", T * 4), c.p("loss", 4), None]
    return build


def _multi_bwd(T, K):
    def build(c):
        n = c.v("numel", 5)
        t, nt = _terms(c, T, n)
        g = L.BinLossGrads()
        g.n_out = c.v("n_out", K)
        for k in range(K):
            g.out[k] = c.p(f"g.out[{k}]", n * 4)
            g.term_a[k], g.sign_a[k] = c.v(f"g.term_a[{k}]", k % T), 1.0
            g.term_b[k], g.sign_b[k] = c.v(f"g.term_b[{k}]", (k + 1) % T if k % 2 else -1), -1.0
        return [c.v("kind", L.LOSS_L2_SUM), None if c.v("t", 1) == 0 else C.byref(t), n, 1e-6, c.p("gloss", 4, 1.0),
                None if c.v("g", 1) == 0 else C.byref(g), None]
    return build


baseline("binhip_multi_loss_fwd", "2")(_multi_fwd(2))
baseline("binhip_multi_loss_fwd", "max")(_multi_fwd(L.LOSS_MAX_TERMS))
baseline("binhip_multi_loss_bwd", "2x3")(_multi_bwd(2, 3))
baseline("binhip_multi_loss_bwd", "max")(_multi_bwd(L.LOSS_MAX_TERMS, L.LOSS_MAX_TERMS))
nulls("multi_loss_fwd/2", ("t", "partials", "terms", "loss", "t.x[0]", "t.x[1]", "t.y[0]", "t.y[1]"), "multi_loss_partial_kernel reads x[t], y[t] of every term")
nulls("multi_loss_fwd/max", tuple(f"t.{s}[{i}]" for s in "xy" for i in (0, L.LOSS_MAX_TERMS - 1)), "every term's x and y")
dims("multi_loss_fwd/2", ("numel",), "numel >= 1")
dims("multi_loss_fwd/2", ("n_terms",), "n_terms: 1 .. BINHIP_LOSS_MAX_TERMS", code=E_ARG)
limit("multi_loss_fwd/max", {"n_terms": L.LOSS_MAX_TERMS}, {"n_terms": L.LOSS_MAX_TERMS + 1}, E_ARG, "BinLossTerms holds BINHIP_LOSS_MAX_TERMS pairs")
limit("multi_loss_fwd/2", {"kind": L.LOSS_L2_SUM}, {"kind": L.LOSS_L2_SUM + 1}, E_ARG, "BINHIP_LOSS_*: 0, 1, 2")
_B = "multi_loss_bwd/2x3"
nulls(_B, ("t", "g", "gloss", "g.out[0]", "g.out[1]", "g.out[2]"), "multi_loss_bwd_kernel stores out[k] of every k < n_out")
nulls(_B, ("t.x[0]", "t.y[1]"), "multi_loss_bwd_kernel reads t.x[term], t.y[term]: every term's pair is required, as in the forward")
dims(_B, ("numel",), "numel >= 1")
dims(_B, ("n_terms", "n_out"), "1 .. BINHIP_LOSS_MAX_TERMS", code=E_ARG)
limit("multi_loss_bwd/max", {"n_terms": L.LOSS_MAX_TERMS}, {"n_terms": L.LOSS_MAX_TERMS + 1}, E_ARG, "BinLossTerms holds BINHIP_LOSS_MAX_TERMS pairs")
limit("multi_loss_bwd/max", {"n_out": L.LOSS_MAX_TERMS}, {"n_out": L.LOSS_MAX_TERMS + 1}, E_ARG, "BinLossGrads holds BINHIP_LOSS_MAX_TERMS outputs")
limit(_B, {"g.term_a[2]": 1}, {"g.term_a[2]": 2}, E_ARG, "term_a < n_terms (n_terms 2): t.x[term_a] is read")
limit(_B, {"g.term_b[1]": 1}, {"g.term_b[1]": 2}, E_ARG, "term_b < n_terms (n_terms 2)")
limit(_B, {"g.term_a[0]": 0}, {"g.term_a[0]": -1}, E_ARG, "term_a >= 0")
limit(_B, {"g.term_b[0]": -7}, None, 0, "binhip.h BinLossGrads: a negative term_b = one term only")
limit(_B, {"kind": L.LOSS_L2_SUM}, {"kind": L.LOSS_L2_SUM + 1}, E_ARG, "BINHIP_LOSS_*: 0, 1, 2")


@baseline("binhip_grad_scale")
def _(c):
    n = c.v("numel", 9)
    return [c.p("g", n * 4, 1.0), n, c.v("target", 16.0), c.p("partials", _partials(n)), c.p("scale_out", 8), None]


nulls("grad_scale", ("g", "partials", "scale_out"), "every pointer")
dims("grad_scale", ("numel",), "numel >= 1")
for _v in (0.0, -1.0, float("nan")):
    mut("grad_scale", {"target": _v}, E_SHAPE, "target > 0 (a NaN is not)")


# ================================================================================================== fused dense-block tail
def _tail(nt, store):
    def build(c):
        N, H, W = c.v("N", 1), c.v("H", 2), c.v("W", 2)
        ntv = c.v("nterms", nt)
        lo = nt == 3
        px = plane(N, H, W)
        so = c.v("store_o3", store)

        def pair(name, nbytes):
            return c.p(name + "_hi", nbytes), (c.p(name + "_lo", nbytes) if lo else c.null(name + "_lo"))
        blk = pair("blk", (14 if store else 12) * px)          # planes 12, 13 are touched (written) with store_o3 only
        wc = pair("wc", wbytes(32, 12, 3))
        bc = c.p("bias_c", 32 * 4)
        wl = pair("wl", wbytes(96, 14, 1))
        bl = c.p("bias_l", 96 * 4)
        y = pair("y", 6 * px)
        return [N, H, W, ntv, blk[0], blk[1], wc[0], wc[1], bc, wl[0], wl[1], bl, y[0], y[1], so, c.p("status", 4), None]
    return build


for _nt in (1, 3):
    for _s in (0, 1):
        baseline("binhip_rdb_tail_fwd", f"nt{_nt}-o3{_s}")(_tail(_nt, _s))
nulls("rdb_tail_fwd/nt1-o30", ("blk_hi", "wc_hi", "wl_hi", "bias_c", "bias_l", "y_hi"), "binhip_fused.hip: required pointers")
nulls("rdb_tail_fwd/nt3-o31", ("blk_lo", "wc_lo", "wl_lo", "y_lo"), "nterms 3: lo planes")
dims("rdb_tail_fwd/nt1-o30", ("N", "H", "W"), "every dimension is positive")
for _v in (0, 2):
    mut("rdb_tail_fwd/nt1-o30", {"nterms": _v}, E_ARG, "nterms: 1 or 3")
limit("rdb_tail_fwd/nt1-o30", {"N": 3, "H": 2731, "W": 8191}, {"N": 1, "H": 8192, "W": 8192}, E_SHAPE, "N H W < 2^26")

# ================================================================================================== RDN plans
SMALL = (32, 1, 1, 32)
STAGE4 = (0, 0, 0, 0)            # all zero = bin_stage4's (96, 12, 4, 32)
# the BinRdnShape values bin_amd.rdn_plan.check_shape refuses
BAD_SHAPES = ((48, 6, 4, 32), (16, 6, 4, 32), (288, 6, 4, 32), (64, 6, 4, 16), (64, 6, 4, 160), (64, 6, 4, 0), (64, 6, 0, 32),
              (64, 6, L.RDN_MAX_CONVS + 1, 32), (64, 0, 4, 32), (64, 21, 4, 32), (64, -1, 4, 32), (0, 6, 4, 32))


def resolved(shape):
    return (96, 12, 4, 32) if tuple(shape) == (0, 0, 0, 0) else tuple(shape)


def rdn_layers(shape, n_inputs):
    """(cout, cin, ksize) of the 2 + D (C + 1) + 4 layers in plan order (binhip.h BinRdnShape)."""
    G0, D, Cc, G = resolved(shape)
    ly = [(G0, 12 * n_inputs, 5), (G0, G0, 3)]
    for _ in range(D):
        ly += [(G, G0 + k * G, 3) for k in range(Cc)] + [(G0, G0 + Cc * G, 1)]
    return ly + [(G0, D * G0, 1), (G0, G0, 3), (256, G0, 3), (3, 64, 3)]


def _frame_q(c, nt, shape):
    sh = shape_of(c, shape)
    c.keep.append(sh)
    return [c.v("N", 1), c.v("H", 4), c.v("W", 4), c.v("n_inputs", 2), c.v("nterms", nt), None if c.v("shape_ptr", 1) == 0 else C.byref(sh)]


def _rdn_fwd(nt, shape, flags=0, fused=False, fold=False):
    def build(c):
        N, H, W, nin, ntv, shp = _frame_q(c, nt, shape)
        p = L.BinRdnPlan()
        p.N, p.H, p.W, p.n_inputs, p.nterms, p.reserved = N, H, W, nin, ntv, c.v("reserved", flags)
        p.shape.G0, p.shape.D, p.shape.C, p.shape.G = c.v("shape", shape)
        G0 = resolved(shape)[0]
        layers = rdn_layers(shape, 2)
        for i, (cout, cin, ks) in enumerate(layers):
            wb = wbytes(r32(cout), chunks(cin), ks)
            p.w_hi[i] = c.p(f"w_hi[{i}]", wb)
            p.w_lo[i] = c.p(f"w_lo[{i}]", wb) if nt == 3 else 0
            p.bias[i] = c.p(f"bias[{i}]", r32(cout) * 4)
        n = len(layers)
        if fused:           # slots L, L + 1 of BINHIP_PLAN_FUSED_UPNET
            wb = (G0 // 16) * 5 * 4 * 32 * 16 * 2 if fold else wbytes(32, G0 // 16, 5)
            p.w_hi[n], p.bias[n] = c.p(f"w_hi[{n}]", wb), c.p(f"bias[{n}]", 32 * 4)
            p.w_lo[n] = c.p(f"w_lo[{n}]", wb) if nt == 3 else 0
            p.w_hi[n + 1], p.bias[n + 1] = c.p(f"w_hi[{n + 1}]", 9 * 12 * 25 * G0 * 4), c.p(f"bias[{n + 1}]", 9 * 12 * 4)
        p.status = c.p("status", 4)
        ws = lib().binhip_rdn_workspace_bytes(N, H, W, nin, ntv, shp)
        fb = N * 3 * H * W * 4
        return [None if c.v("plan", 1) == 0 else C.byref(p), c.ptrs("inputs", nin if nin in (2, 3, 5) else 2, fb), c.p("out", fb),
                c.p("workspace", ws), c.v("workspace_bytes", ws), None]
    return build


_F = L
RDN_FWD_MODES = {
    "small-nt1": (1, SMALL, dict()),
    "small-nt3": (3, SMALL, dict()),
    "small-keep-nt3": (3, SMALL, dict(flags=_F.PLAN_KEEP_ACTS)),
    "small-fused-nt1": (1, SMALL, dict(flags=_F.PLAN_FUSED_UPNET, fused=True)),
    "small-fused-train-nt3": (3, SMALL, dict(flags=_F.PLAN_KEEP_ACTS | _F.PLAN_FUSED_UPNET | _F.PLAN_FUSED_UPNET_TRAIN, fused=True)),
    "small-fold-nt3": (3, SMALL, dict(flags=_F.PLAN_FUSED_UPNET | _F.PLAN_UPNET_FOLD, fused=True, fold=True)),
    "stage4-keep-nt1": (1, STAGE4, dict(flags=_F.PLAN_KEEP_ACTS)),
    "stage4-nofuse-nt3": (3, STAGE4, dict(flags=_F.PLAN_NO_FUSE)),
    "stage4-nt3": (3, STAGE4, dict()),
}
for _mode, (_nt, _shape, _kw) in RDN_FWD_MODES.items():
    baseline("binhip_rdn_forward", _mode)(_rdn_fwd(_nt, _shape, **_kw))
    WORKSPACES.append(Workspace("rdn_forward/" + _mode, "binhip_rdn_workspace_bytes", (lambda c, nt=_nt, s=_shape: _frame_q(c, nt, s)),
                                "workspace_bytes", [{"H": 5}, {"W": 6 + 1}, {"N": 0}, {"n_inputs": 4}, {"shape": (48, 6, 4, 32)}]))

_PLAN_FLAGS = (_F.PLAN_KEEP_ACTS | _F.PLAN_NO_FUSE | _F.PLAN_RDB3 | _F.PLAN_FUSED_UPNET | _F.PLAN_FUSED_UPNET_TRAIN | _F.PLAN_UPNET_FOLD)
_B = "rdn_forward/small-nt1"
nulls(_B, ("plan", "inputs", "out", "workspace", "inputs[0]", "inputs[1]"), "binhip_plan.hip binhip_rdn_forward: required pointers, every input frame")
for _i in range(len(rdn_layers(SMALL, 2))):
    nulls(_B, (f"w_hi[{_i}]", f"bias[{_i}]"), "BinRdnPlan: w_hi / bias of every layer the shape has")
    nulls("rdn_forward/small-nt3", (f"w_lo[{_i}]",), "BinRdnPlan: w_lo of every layer under nterms 3")
for _i in (0, 33, 65):
    nulls("rdn_forward/stage4-nt3", (f"w_hi[{_i}]", f"w_lo[{_i}]", f"bias[{_i}]"), "BinRdnPlan: bin_stage4 has 66 layers")
dims(_B, ("N", "H", "W"), "frames_ok: positive")
mut(_B, {"H": 5}, E_SHAPE, "BinRdnPlan: H even")
mut(_B, {"W": 7}, E_SHAPE, "BinRdnPlan: W even")
for _v in (0, 1, 4, 6, -1):
    mut(_B, {"n_inputs": _v}, E_SHAPE, "BinRdnPlan.n_inputs: 2, 3 or 5")
for _v in (0, 2, -1):
    mut(_B, {"nterms": _v}, E_ARG, "nterms: 1 or 3")
for _s in BAD_SHAPES:
    mut(_B, {"shape": _s}, E_SHAPE, "binhip.h BinRdnShape / rdn_plan.check_shape refuses it")
for _v in (64, 128, 1 << 30, -1 & ~_PLAN_FLAGS):
    mut(_B, {"reserved": _v}, E_ARG, "BinRdnPlan.reserved: an undefined BINHIP_PLAN_* bit")
mut(_B, {"reserved": _F.PLAN_FUSED_UPNET | _F.PLAN_UPNET_FOLD}, E_ARG, "BINHIP_PLAN_UPNET_FOLD with nterms 1")
mut("rdn_forward/small-fold-nt3", {"reserved": _F.PLAN_UPNET_FOLD}, E_ARG, "BINHIP_PLAN_UPNET_FOLD without _FUSED_UPNET")
mut("rdn_forward/small-fold-nt3", {"reserved": _F.PLAN_FUSED_UPNET | _F.PLAN_UPNET_FOLD | _F.PLAN_KEEP_ACTS}, E_ARG, "BINHIP_PLAN_UPNET_FOLD with KEEP_ACTS")
limit("rdn_forward/small-nt3", {"reserved": _PLAN_FLAGS & ~(_F.PLAN_UPNET_FOLD | _F.PLAN_KEEP_ACTS)},
      {"reserved": (_PLAN_FLAGS & ~(_F.PLAN_UPNET_FOLD | _F.PLAN_KEEP_ACTS)) | (_PLAN_FLAGS + 1)}, E_ARG,
      "every defined flag that may be combined is accepted; the next bit is not")
limit(_B, {"N": 1, "H": 8192, "W": 8190}, {"N": 1, "H": 8192, "W": 8192}, E_SHAPE, "N H W < 2^26: UPNet.2 runs at full resolution")
_n = len(rdn_layers(SMALL, 2))
for _s in (f"w_hi[{_n}]", f"bias[{_n}]", f"w_hi[{_n + 1}]", f"bias[{_n + 1}]"):
    limit("rdn_forward/small-fused-nt1", {_s: 0}, None, 0,
          "binhip.h BINHIP_PLAN_FUSED_UPNET: a NULL slot L / L + 1 pointer = the two-layer form runs (its slots are always required)")
nulls("rdn_forward/small-fused-nt1", (f"w_hi[{_n - 2}]", f"bias[{_n - 1}]"), "UPNet.0 / UPNet.2 slots are required with BINHIP_PLAN_FUSED_UPNET too")


@baseline("binhip_rdn_workspace_bytes", "small-nt1", accept=lambda rv, gpu: rv > 0)
def _(c):
    return _frame_q(c, 1, SMALL)


@baseline("binhip_rdn_workspace_bytes", "default-shape-nt3", accept=lambda rv, gpu: rv > 0)
def _(c):
    return _frame_q(c, 3, STAGE4)[:5] + [None]


@baseline("binhip_rdn_backward_workspace_bytes", "small-nt1", accept=lambda rv, gpu: rv > 0)
def _(c):
    return _frame_q(c, 1, SMALL)


def _layout(words):
    def build(c):
        q = _frame_q(c, 3, SMALL)
        n_out = c.v("n_out", words)
        out = None if c.v("out", 1) == 0 else (C.c_int64 * max(words, 1))()
        c.keep.append(out)
        return q + [out, n_out]
    return build


baseline("binhip_rdn_workspace_layout", accept=lambda rv, gpu: rv == 0)(_layout(L.RDN_LAYOUT_WORDS))
baseline("binhip_rdn_backward_workspace_layout", accept=lambda rv, gpu: rv == 0)(_layout(L.RDN_BWD_LAYOUT_WORDS))
for _b, _code in (("rdn_workspace_bytes/small-nt1", 0), ("rdn_backward_workspace_bytes/small-nt1", 0), ("rdn_workspace_layout", E_SHAPE),
                  ("rdn_backward_workspace_layout", E_SHAPE)):
    dims(_b, ("N", "H", "W"), "frames_ok: positive", code=_code)
    mut(_b, {"H": 5}, _code, "H even")
    mut(_b, {"W": 7}, _code, "W even")
    for _v in (0, 4, 6):
        mut(_b, {"n_inputs": _v}, _code, "n_inputs: 2, 3 or 5")
    for _s in BAD_SHAPES:
        mut(_b, {"shape": _s}, _code, "rdn_plan.check_shape refuses it")
    limit(_b, {"N": 1, "H": 8192, "W": 8190}, {"N": 1, "H": 8192, "W": 8192}, _code, "N H W < 2^26")
nulls("rdn_workspace_layout", ("out",), "out")
nulls("rdn_backward_workspace_layout", ("out",), "out")
limit("rdn_workspace_layout", {"n_out": L.RDN_LAYOUT_WORDS}, {"n_out": L.RDN_LAYOUT_WORDS - 1}, E_ARG, "out holds BINHIP_RDN_LAYOUT_WORDS words")
limit("rdn_backward_workspace_layout", {"n_out": L.RDN_BWD_LAYOUT_WORDS}, {"n_out": L.RDN_BWD_LAYOUT_WORDS - 1}, E_ARG,
      "out holds BINHIP_RDN_BWD_LAYOUT_WORDS words")


def _rdn_bwd(nt, shape, flags=0, fused=False):
    def build(c):
        N, H, W, nin, ntv, shp = _frame_q(c, nt, shape)
        G0, D, Cc, G = resolved(shape)
        fl = c.v("reserved", flags)
        p = L.BinRdnBwdPlan()
        p.N, p.H, p.W, p.n_inputs, p.nterms, p.reserved = N, H, W, nin, ntv, fl
        p.shape.G0, p.shape.D, p.shape.C, p.shape.G = c.v("shape", shape)
        layers = rdn_layers(shape, 2)
        lo = nt == 3
        i = 0

        def slot(i, rows, cc, ks, dwb, dbb):
            wb = wbytes(rows, cc, ks)
            p.wt_hi[i] = c.p(f"wt_hi[{i}]", wb)
            p.wt_lo[i] = c.p(f"wt_lo[{i}]", wb) if lo else 0
            p.dw[i], p.db[i] = c.p(f"dw[{i}]", dwb), c.p(f"db[{i}]", dbb)
        for i, (cout, cin, ks) in enumerate(layers):
            k = (i - 2) % (Cc + 1)
            if 2 <= i < 2 + D * (Cc + 1) and k < Cc:           # conv k of a dense block: its slot holds gather group k
                rows, cc = (G0 if k == 0 else G), (Cc - k) * G // 16
            else:
                rows, cc = lib().binhip_dgrad_rows_pad(ks, cin), chunks(cout)
            slot(i, rows, cc, ks, cout * cin * ks * ks * 4, cout * 4)
        n = len(layers)
        if fused:           # BINHIP_BWD_FUSED_UPNET: slots L, L + 1
            slot(n, r32(G0), 1, 5, 12 * G0 * 25 * 4, 12 * 4)
            p.wt_hi[n + 1] = c.p(f"wt_hi[{n + 1}]", 9 * 12 * 25 * G0 * 4)
            p.dw[n + 1], p.db[n + 1] = c.p(f"dw[{n + 1}]", N * 9 * 12 * 25 * G0 * 4), c.p(f"db[{n + 1}]", N * 9 * 12 * 4)
        p.zero_bias = c.p("zero_bias", max(D * G0, G0 + Cc * G, 256) * 4)
        fb = N * 3 * H * W * 4
        for k in range(2):
            p.gin[k] = c.p(f"gin[{k}]", fb) if k == 0 else 0      # gin[i] may be NULL: frame 1 needs no gradient
        p.status = c.p("status", 4)
        nt_saved = 3 if flags & L.BWD_SAVED_X3 else ntv
        sb = lib().binhip_rdn_workspace_bytes(N, H, W, nin, nt_saved, shp)
        ws = lib().binhip_rdn_backward_workspace_bytes(N, H, W, nin, ntv, shp)
        return [None if c.v("plan", 1) == 0 else C.byref(p), c.p("saved", sb), c.v("saved_bytes", sb), c.p("gout", fb, 1.0),
                c.p("workspace", ws), c.v("workspace_bytes", ws), None]
    return build


RDN_BWD_MODES = {
    "small-nt1": (1, SMALL, dict()),
    "small-nt3": (3, SMALL, dict()),
    "small-savedx3-acc-nt1": (1, SMALL, dict(flags=L.BWD_SAVED_X3 | L.BWD_ACCUMULATE)),
    "small-fused-nt3": (3, SMALL, dict(flags=L.BWD_FUSED_UPNET, fused=True)),
    "stage4-nt1": (1, STAGE4, dict()),
}
for _mode, (_nt, _shape, _kw) in RDN_BWD_MODES.items():
    baseline("binhip_rdn_backward", _mode)(_rdn_bwd(_nt, _shape, **_kw))
    WORKSPACES.append(Workspace("rdn_backward/" + _mode, "binhip_rdn_backward_workspace_bytes",
                                (lambda c, nt=_nt, s=_shape: _frame_q(c, nt, s)), "workspace_bytes",
                                [{"H": 5}, {"W": 7}, {"N": 0}, {"n_inputs": 4}, {"shape": (48, 6, 4, 32)}]))
_B = "rdn_backward/small-nt1"
nulls(_B, ("plan", "saved", "gout", "workspace", "zero_bias"), "binhip_plan.hip binhip_rdn_backward: required pointers")
for _i in range(len(rdn_layers(SMALL, 2))):
    nulls(_B, (f"wt_hi[{_i}]", f"dw[{_i}]", f"db[{_i}]"), "BinRdnBwdPlan: wt_hi / dw / db of every layer the shape has")
    nulls("rdn_backward/small-nt3", (f"wt_lo[{_i}]",), "BinRdnBwdPlan: wt_lo of every layer under nterms 3")
_n = len(rdn_layers(SMALL, 2))
nulls("rdn_backward/small-fused-nt3", (f"wt_hi[{_n}]", f"wt_lo[{_n}]", f"wt_hi[{_n + 1}]", f"dw[{_n}]", f"db[{_n}]", f"dw[{_n + 1}]", f"db[{_n + 1}]"),
      "BINHIP_BWD_FUSED_UPNET: slots L and L + 1")
for _i in (0, 65):
    nulls("rdn_backward/stage4-nt1", (f"wt_hi[{_i}]", f"dw[{_i}]", f"db[{_i}]"), "bin_stage4 has 66 layers")
dims(_B, ("N", "H", "W"), "frames_ok: positive")
mut(_B, {"H": 5}, E_SHAPE, "H even")
mut(_B, {"W": 7}, E_SHAPE, "W even")
for _v in (0, 4, 6):
    mut(_B, {"n_inputs": _v}, E_SHAPE, "n_inputs: 2, 3 or 5")
for _v in (0, 2):
    mut(_B, {"nterms": _v}, E_ARG, "nterms: 1 or 3")
for _s in BAD_SHAPES:
    mut(_B, {"shape": _s}, E_SHAPE, "rdn_plan.check_shape refuses it")
for _v in (8, 16, 1 << 20, -8):
    mut(_B, {"reserved": _v}, E_ARG, "BinRdnBwdPlan.reserved: an undefined BINHIP_BWD_* bit")
mut("rdn_backward/small-nt3", {"reserved": L.BWD_SAVED_X3}, E_ARG, "BINHIP_BWD_SAVED_X3 is for an nterms 1 backward")
limit(_B, {"reserved": L.BWD_ACCUMULATE}, {"reserved": L.BWD_ACCUMULATE | 8}, E_ARG, "defined flags are accepted, the next bit is not")
mut(_B, {"saved_bytes": 255}, E_WS, "saved_bytes < binhip_rdn_workspace_bytes of the forward")
mut("rdn_backward/small-savedx3-acc-nt1", {"saved_bytes": lambda: lib().binhip_rdn_workspace_bytes(1, 4, 4, 2, 1, C.byref(L.BinRdnShape(*SMALL)))},
    E_WS, "BINHIP_BWD_SAVED_X3: `saved` has the nterms 3 size")
limit(_B, {"N": 1, "H": 8192, "W": 8190}, {"N": 1, "H": 8192, "W": 8192}, E_SHAPE, "N H W < 2^26")


# ================================================================================================== scores
def _taps(c, flags):
    if c.v("g11_taps", 1) == 0 or not (flags & L.SCORE_SSIM_G11):
        return None
    t = (C.c_double * G11)(*([1.0 / G11] * G11))
    c.keep.append(t)
    return t


def _score_q(c, H, W, flags, n=2):
    return [c.v("n", n), c.v("H", H), c.v("W", W), c.v("flags", flags)]


def _image_score(H, W, flags):
    def build(c):
        n, Hh, Ww, fl = _score_q(c, H, W, flags)
        ws = lib().binhip_image_score_workspace_bytes(n, Hh, Ww, fl)
        return [c.p("a", n * Hh * Ww * 3), c.p("b", n * Hh * Ww * 3), n, Hh, Ww, fl, _taps(c, flags), c.p("ws", ws), c.v("ws_bytes", ws),
                c.p("out", n * 32), None]
    return build


def _frame_score(H, W, flags):
    def build(c):
        n, Hh, Ww, fl = _score_q(c, H, W, flags)
        ws = lib().binhip_frame_score_workspace_bytes(n, Hh, Ww, fl)
        fb = 3 * Hh * Ww * 4
        return [c.ptrs("x", n, fb), c.ptrs("y", n, fb), n, Hh, Ww, fl, _taps(c, flags), c.p("ws", ws), c.v("ws_bytes", ws), c.p("out", n * 32), None]
    return build


_BOTH = L.SCORE_SSIM_G11 | L.SCORE_SSIM_U7
for _e, _mk in (("image_score", _image_score), ("frame_score", _frame_score)):
    baseline("binhip_" + _e, "psnr")(_mk(1, 1, 0))
    baseline("binhip_" + _e, "ssim")(_mk(G11, G11, _BOTH))
    baseline("binhip_" + _e + "_workspace_bytes", accept=lambda rv, gpu: rv > 0)(lambda c: _score_q(c, G11, G11, _BOTH))
    _B, _S, _Q = _e + "/psnr", _e + "/ssim", _e + "_workspace_bytes"
    nulls(_B, ("ws", "out"), "ws and out")
    nulls(_S, ("g11_taps",), "g11_taps with BINHIP_SCORE_SSIM_G11")
    dims(_B, ("n", "H", "W"), "score_shape: positive")
    dims(_Q, ("n", "H", "W"), "0 for a geometry the call refuses", code=0)
    for _v in (4, 8, -1):
        mut(_B, {"flags": _v}, E_ARG, "an undefined BINHIP_SCORE_* flag")
        mut(_Q, {"flags": _v}, 0, "an undefined BINHIP_SCORE_* flag")
    for _d in ("H", "W"):
        limit(_B, {_d: SCORE_MAX_HW}, {_d: SCORE_MAX_HW + 1}, E_SHAPE, "H, W <= 65535 (grid and 16-bit tile coordinates)")
        limit(_S, {_d: G11, "flags": L.SCORE_SSIM_G11}, {_d: G11 - 1, "flags": L.SCORE_SSIM_G11}, E_SHAPE, "the 11x11 window needs H, W >= 11")
        limit(_S, {_d: U7, "flags": L.SCORE_SSIM_U7}, {_d: U7 - 1, "flags": L.SCORE_SSIM_U7}, E_SHAPE, "the 7x7 window needs H, W >= 7")
        limit(_Q, {_d: G11}, {_d: G11 - 1}, 0, "the 11x11 window needs H, W >= 11")
    for _b in (_B, _S):
        WORKSPACES.append(Workspace(_b, "binhip_" + _Q, (lambda c, b=_b: _score_q(c, *((1, 1, 0) if b.endswith("psnr") else (G11, G11, _BOTH)))),
                                    "ws_bytes", [{"n": 0}, {"H": 0}, {"W": SCORE_MAX_HW + 1}, {"flags": 4}]))
nulls("image_score/psnr", ("a", "b"), "a and b")
limit("image_score/psnr", {"n": SCORE_MAX_HW}, {"n": SCORE_MAX_HW + 1}, E_SHAPE, "n <= 65535 (grid z)")
nulls("frame_score/psnr", ("x", "y", "x[0]", "x[1]", "y[0]", "y[1]"), "binhip.h binhip_frame_score: a null array or a null element")
limit("frame_score/psnr", {"n": L.SCORE_MAX_PAIRS}, {"n": L.SCORE_MAX_PAIRS + 1}, E_SHAPE, "FramePairs holds BINHIP_SCORE_MAX_PAIRS pairs")
limit("frame_score_workspace_bytes", {"n": L.SCORE_MAX_PAIRS}, {"n": L.SCORE_MAX_PAIRS + 1}, 0, "BINHIP_SCORE_MAX_PAIRS")


# ================================================================================================== training batches
def _gather(blur):
    def build(c):
        nf, H, W, n, ns = c.v("n_frames", 3), c.v("H", 3), c.v("W", 5), c.v("n", 2), c.v("n_slots", 2)
        ch, cw = c.v("ch", 2), c.v("cw", 3)
        a = [c.p("frames", nf * H * W * 3), nf, H, W, c.p("table", n * (ns + (4 if blur else 3)) * 4), n, ns]
        if blur:
            a.append(c.v("n_blur", 1))
        return a + [ch, cw, c.p("out", ns * n * 3 * ch * cw * 4), None]
    return build


baseline("binhip_gather_windows")(_gather(False))
baseline("binhip_gather_windows_blur")(_gather(True))
for _B in ("gather_windows", "gather_windows_blur"):
    nulls(_B, ("frames", "table", "out"), "binhip.h: BINHIP_E_ARG for a null pointer")
    dims(_B, ("n_frames", "H", "W", "n", "n_slots", "ch", "cw"), "binhip.h: BINHIP_E_SHAPE for a non-positive size")
    limit(_B, {"n_slots": GATHER_MAX_SLOTS}, {"n_slots": GATHER_MAX_SLOTS + 1}, E_SHAPE, "n_slots: 1 .. 32")
    limit(_B, {"ch": 3, "H": 3}, {"ch": 4, "H": 3}, E_SHAPE, "ch <= H: the crop lies inside the frame")
    limit(_B, {"cw": 5, "W": 5}, {"cw": 6, "W": 5}, E_SHAPE, "cw <= W")
    _nb = {"n_blur": 0} if _B.endswith("blur") else {}
    limit(_B, dict(_nb, n_slots=1, n=1, ch=GATHER_MAX_ITEMS, H=GATHER_MAX_ITEMS, cw=1, W=1),
          dict(_nb, n_slots=1, n=2, ch=1 << 30, H=1 << 30, cw=1, W=1), E_SHAPE, "at most 2^31 - 1 four-pixel output quads")
limit("gather_windows_blur", {"n_blur": 2}, {"n_blur": 3}, E_SHAPE, "n_blur <= n_slots (2)")
limit("gather_windows_blur", {"n_blur": 0}, {"n_blur": -1}, E_SHAPE, "n_blur >= 0")


# ================================================================================================== profiler
@baseline("binhip_profiler_create")
def _(c):
    h = C.c_void_p(0)
    c.keep.append(h)
    c.after.append(lambda: h.value and lib().binhip_profiler_destroy(h))
    return [c.v("ksize", 3), c.v("cout_pad", 32), c.v("epilogue", 0), c.v("max_launches", 2), None if c.v("out", 1) == 0 else C.byref(h)]


nulls("profiler_create", ("out",), "out")
dims("profiler_create", ("max_launches",), "max_launches >= 1", code=E_ARG)
limit("profiler_create", {"max_launches": PROF_MAX_LAUNCHES}, {"max_launches": PROF_MAX_LAUNCHES + 1}, E_ARG, "binhip.h: at most 16384 pairs")


# a live handle exists only where hipEventCreate succeeds: the baseline runs on a GPU only, its refusal everywhere
@baseline("binhip_profiler_read", cpu=False)
def _(c):
    if c.v("p", 1) == 0:
        return [None, None, None]
    h = C.c_void_p(0)
    assert lib().binhip_profiler_create(3, 32, 0, 2, C.byref(h)) == 0
    ms, n = C.c_double(-1.0), C.c_int(-1)
    c.keep += [h, ms, n]
    c.after.append(lambda: lib().binhip_profiler_destroy(h))
    return [h, C.byref(ms), C.byref(n)]


nulls("profiler_read", ("p",), "p")


def materialise(base, over, alloc):
    """(entry point, argument list, ctx) of baseline `base` under the override `over` (values may be callables, resolved here)."""
    b = BASELINES[base]
    over = {k: (v() if callable(v) else v) for k, v in over.items()}
    ctx = Ctx(over, alloc)
    args = b.build(ctx)
    unused = set(over) - ctx.used
    assert not unused, f"{base}: the baseline never looked at {sorted(unused)}"
    assert len(args) == len(L._SIGNATURES[b.entry][1]), f"{base}: {len(args)} arguments, {b.entry} takes {len(L._SIGNATURES[b.entry][1])}"
    return b.entry, args, ctx


def call(base, over, alloc):
    entry, args, ctx = materialise(base, over, alloc)
    try:
        return getattr(lib(), entry)(*args), ctx
    finally:
        for f in ctx.after:
            f()
