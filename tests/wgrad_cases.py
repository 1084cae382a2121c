"""Case table, work-split geometry, operand families and float64 references of the weight-gradient kernels (binhip_wgrad.hip), shared
by tests/test_gpu_wgrad.py and tests/test_cpu_wgrad_cases.py.

geometry() restates wg_geom() / w1_plan() of binhip_wgrad.hip: which kernel or template variant a shape runs, how many workgroup groups
there are, and how the pixel tiles are dealt to the PB workgroups of a group (workgroup pb walks tiles pb, pb + PB, ... through a
two-stage LDS ring).  tests/test_cpu_wgrad_cases.py holds it to binhip_wgrad_workspace_bytes(), which is a function of the same
quantities.  Every case is in the table BECAUSE of a property of that split at 256 CUs and carries the property as a predicate; the GPU
test asserts the predicate with the CU count of its device, so on another device the case fails instead of passing without running what it
is there for.

Operand families
  A  integers: X and gY uniform in -3 .. 3, output channel co of gY times MULT[co] (1, 2 or 5: two channels that are mixed up differ).
     Every product and partial sum is an integer below 2^24, exact in fp16, in the MFMA and in fp32, in any order: both precisions must
     return the float64 reference bit for bit.  Condition (no tolerance): the same backward of |X| and |gY| stays below 2^24.
  B  split-exact: a + b * 2^-11 with a in {+-1, +-2}, b in {-1, 0, 1}, about 90 % of gY zero.  hi = a and lo = b * 2^-11 exactly, so the
     three products xh*gh + xl*gh + xh*gl of the f16x3 form are all live, all multiples of 2^-11 (the lo*lo term the form drops is the
     only multiple of 2^-22).  Condition: 2^11 * sum|terms| < 2^24.  The reference is that definition in float64 on the stored planes.
     (|a| = 1 with b of the opposite sign is left out: 1 - 2^-11 is itself an fp16 number, so there hi would not be a.)
  C  white noise against float64, at the suite's TOL_BWD.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

W1_NW, W1_NCOT = 8, 3                  # binhip_wgrad.hip: waves of the streaming 1x1 kernel, its 32-wide output tiles (cout <= 96)
LDS_LIMIT = 160 * 1024
DEFAULT_CUS = 256                      # what the library assumes without a device (cus() in binhip_wgrad.hip)

Geometry = namedtuple("Geometry", "kernel groups ntiles PB tiles_min tiles_max mapping workspace_bytes "
                                  "cin_chunks ncp ncot ndyg ntap tiles_x tiles_y cgroups ppg clipped")


def chunks(c):
    return (c + 15) // 16


def w1_plan(ncp):
    """w1_plan(): (ppw, tr, cgroups, ppg) of the streaming 1x1 kernel for ncp input-channel pairs."""
    ppw = 1 if ncp <= W1_NW else 2
    cap = W1_NW * ppw
    cgroups = (ncp + cap - 1) // cap
    ppg = (ncp + cgroups - 1) // cgroups
    slots = 2 * (2 * W1_NCOT + 2 * ppg)
    tr = 2 if (ppw == 1 and 2 * slots * 2 * 1024 <= LDS_LIMIT) else 1
    return ppw, tr, cgroups, ppg


def geometry(ks, N, H, W, cin, cout, cus=DEFAULT_CUS):
    """wg_geom() in Python.  kernel: "3x3" (wgrad3x3_xrow_kernel), "5x5" (wgrad_mfma_kernel<5,1,NT>), "1x1_generic"
    (wgrad_mfma_kernel<1,1,NT>, cout > 96) or "w1<PPW,TR>" (wgrad1x1_kernel<NT,PPW,TR>).  groups: workgroups that walk the same tiles
    (blockIdx.y of the streaming kernel).  tiles_min / tiles_max: tiles of the least / most loaded workgroup = rounds of its LDS ring.
    mapping: wg_block()'s "xcd" (PB % 8 == 0) or "plain" unpacking of the workgroup id, "grid" for the streaming kernel's 2-D grid.
    clipped: PB was limited by the tile count."""
    cus = cus if cus > 0 else DEFAULT_CUS
    cc = chunks(cin)
    ncp, ncot = (cc + 1) // 2, (cout + 31) // 32
    tiles_x = (W + 31) // 32
    if ks == 1 and cout <= 32 * W1_NCOT:
        ppw, tr, cgroups, ppg = w1_plan(ncp)
        kernel, groups, mapping = "w1<%d,%d>" % (ppw, tr), cgroups, "grid"
        ndyg, ntap = 1, 1
        tiles_y = (H + tr - 1) // tr
        ntiles = tiles_x * tiles_y * N
        want = max(cus // cgroups, 1)
        PB = min(want, ntiles)
        partial = ncp * ncot * PB * 1024
    else:
        kernel = {1: "1x1_generic", 3: "3x3", 5: "5x5"}[ks]
        tr = 1 if ks == 5 else ks
        ndyg, ntap = ks // tr, tr * ks
        cgroups, ppg = 1, 0
        tiles_y = (H + 7) // 8
        ntiles = tiles_x * tiles_y * N
        groups = ncp * ncot * ndyg
        want = max(cus // groups, 1)
        PB = min(want, ntiles)
        if PB >= 8:
            PB &= ~7
        mapping = "xcd" if PB % 8 == 0 else "plain"
        partial = groups * PB * ntap * 1024
    bias = ncot * PB * 32
    return Geometry(kernel, groups, ntiles, PB, ntiles // PB, (ntiles + PB - 1) // PB, mapping, (partial + bias) * 4 + 256,
                    cc, ncp, ncot, ndyg, ntap, tiles_x, tiles_y, cgroups, ppg, want > ntiles)


# property name -> predicate on (case, geometry)
PROPERTIES = {
    "3x3": lambda c, g: g.kernel == "3x3",
    "5x5": lambda c, g: g.kernel == "5x5",
    "1x1_generic": lambda c, g: g.kernel == "1x1_generic",
    "w1<1,2>": lambda c, g: g.kernel == "w1<1,2>",
    "w1<1,1>": lambda c, g: g.kernel == "w1<1,1>",
    "w1<2,1>": lambda c, g: g.kernel == "w1<2,1>",
    "rounds>=3": lambda c, g: g.tiles_max >= 3 and g.tiles_min >= 2,          # stage parity over an odd and an even tile count follows
    "rounds>=6": lambda c, g: g.tiles_min >= 6,                               # from uneven; rounds>=6 holds both in every workgroup
    "uneven": lambda c, g: g.tiles_min != g.tiles_max,
    "plain_mapping": lambda c, g: g.mapping == "plain" and g.PB > 1,
    "xcd_mapping": lambda c, g: g.mapping == "xcd",
    "pb_clipped": lambda c, g: g.clipped,
    "one_tile": lambda c, g: g.ntiles == 1 and g.PB == 1,
    "odd_chunks": lambda c, g: g.cin_chunks % 2 == 1,
    "ragged_cout": lambda c, g: c.cout % 32 != 0,
    "ragged_cin": lambda c, g: c.cin % 16 != 0,
    "column_groups=2": lambda c, g: g.cgroups == 2,
    "column_groups=3": lambda c, g: g.cgroups == 3,
    "odd_ppg": lambda c, g: g.ppg % 2 == 1 and g.kernel == "w1<2,1>",          # a wave with one live and one idle channel pair
    "ragged_tiles": lambda c, g: c.W % 32 != 0,                                 # tiles that hang over the right edge
    "images>=3": lambda c, g: c.N >= 3,
}

Case = namedtuple("Case", "tag ks N H W cin cout props")


def _c(tag, shape, props):
    return Case(tag, *shape, tuple(props.split()))


# (ks, N, H, W, cin, cout); the first 17 are the smallest shapes with their properties at 256 CUs, the last five are the shapes of
# test_wgrad_1x1_ragged / test_wgrad_3x3_shapes whose property no other row has
CASES = (
    _c("3x3_pb40_3or4", (3, 4, 64, 128, 192, 32), "3x3 rounds>=3 uneven xcd_mapping images>=3"),
    _c("3x3_up0", (3, 2, 40, 96, 96, 256), "3x3 rounds>=3 uneven xcd_mapping"),
    _c("3x3_224_256_plain", (3, 1, 24, 70, 224, 256), "3x3 plain_mapping rounds>=3 uneven ragged_tiles"),
    _c("3x3_48_images", (3, 48, 9, 33, 96, 32), "3x3 rounds>=3 uneven ragged_tiles images>=3 xcd_mapping"),
    _c("3x3_cout3", (3, 3, 17, 40, 64, 3), "3x3 ragged_cout pb_clipped uneven ragged_tiles"),
    _c("3x3_one_tile", (3, 1, 5, 7, 40, 35), "3x3 one_tile odd_chunks ragged_cout ragged_cin"),
    _c("5x5_24", (5, 2, 33, 70, 24, 96), "5x5 uneven ragged_tiles ragged_cin"),
    _c("5x5_36", (5, 2, 33, 70, 36, 96), "5x5 odd_chunks rounds>=3 uneven ragged_tiles ragged_cin"),
    _c("5x5_60", (5, 3, 19, 45, 60, 96), "5x5 rounds>=3 uneven ragged_tiles ragged_cin images>=3"),
    _c("5x5_fused_upnet", (5, 4, 40, 130, 96, 12), "5x5 rounds>=6 uneven ragged_cout images>=3"),
    _c("5x5_one_pixel", (5, 1, 1, 1, 24, 96), "5x5 one_tile"),
    _c("w1_p1t2_rounds", (1, 4, 64, 200, 224, 96), "w1<1,2> rounds>=3 uneven images>=3"),
    _c("w1_p1t1_rounds", (1, 4, 33, 200, 256, 96), "w1<1,1> rounds>=3 uneven images>=3"),
    _c("w1_p1t1_clipped", (1, 2, 19, 45, 256, 96), "w1<1,1> pb_clipped ragged_tiles"),
    _c("w1_p2t1_gff0", (1, 3, 40, 130, 1152, 96), "w1<2,1> column_groups=3 rounds>=6 uneven images>=3"),
    _c("g1_128", (1, 2, 33, 70, 96, 128), "1x1_generic xcd_mapping uneven ragged_tiles"),
    _c("g1_224_256_plain", (1, 1, 19, 45, 224, 256), "1x1_generic plain_mapping uneven ragged_tiles"),
    _c("w1_cout35", (1, 1, 5, 7, 40, 35), "w1<1,2> ragged_cout odd_chunks ragged_cin pb_clipped"),
    _c("w1_one_chunk", (1, 1, 8, 32, 16, 96), "w1<1,2> odd_chunks pb_clipped"),
    _c("w1_p2t1_600_64", (1, 1, 33, 70, 600, 64), "w1<2,1> column_groups=2 ragged_cin pb_clipped ragged_tiles"),
    _c("w1_p2t1_odd_ppg", (1, 3, 6, 40, 272, 96), "w1<2,1> odd_ppg pb_clipped images>=3"),
    _c("3x3_one_chunk", (3, 1, 40, 33, 16, 32), "3x3 odd_chunks pb_clipped uneven"),
)
BY_TAG = {c.tag: c for c in CASES}
TAGS = tuple(c.tag for c in CASES)

# family B: the tiny shapes plus one shape of two or more rounds per kernel and variant
SPLIT_TAGS = ("3x3_one_tile", "5x5_one_pixel", "w1_cout35", "w1_one_chunk", "3x3_up0", "5x5_36", "w1_p1t2_rounds", "w1_p1t1_rounds",
              "w1_p2t1_gff0", "g1_128")
# one case of several rounds per kernel for accumulate / inv_scale; cout 256 for shuffle_perm; more than six input chunks (or the fused
# UPNet's exactly six) for x_cpg = 6; N > 1 for the sum over single images
ARG_TAGS = ("3x3_up0", "5x5_36", "w1_p1t1_rounds", "g1_128")
SHUFFLE_TAGS = ("3x3_up0", "3x3_224_256_plain", "g1_224_256_plain")
GROUP_TAGS = ("3x3_224_256_plain", "5x5_fused_upnet", "w1_p1t1_rounds", "w1_p2t1_gff0", "g1_224_256_plain")
IMAGE_SUM_TAGS = ("3x3_pb40_3or4", "5x5_fused_upnet", "w1_p1t1_rounds", "g1_128")

MULTS = (1, 2, 5)
EXACT_LIMIT = float(1 << 24)


def check_properties(case, cus):
    """Assert every property the case is in the table for, at `cus` compute units; returns the geometry."""
    g = geometry(case.ks, case.N, case.H, case.W, case.cin, case.cout, cus)
    for p in case.props:
        assert PROPERTIES[p](case, g), f"{case.tag}: property '{p}' does not hold at {cus} CUs: {g}"
    return g


def _gen(case, salt):
    return torch.Generator().manual_seed(1000003 * salt + 7919 * TAGS.index(case.tag) + case.cin + 31 * case.cout)


def channel_mults(cout):
    """MULT[co] = MULTS[co % 3]: neighbours, channels 16 apart (a chunk), 32 apart (an output tile) and 64 apart all differ."""
    return torch.tensor(MULTS, dtype=torch.float32)[torch.arange(cout) % 3]


def family_a(case):
    """(X, gY) fp32 NCHW of small integers."""
    gen = _gen(case, 1)
    x = torch.randint(-3, 4, (case.N, case.cin, case.H, case.W), generator=gen).float()
    gy = torch.randint(-3, 4, (case.N, case.cout, case.H, case.W), generator=gen).float()
    return x, gy * channel_mults(case.cout).view(1, -1, 1, 1)


def split_density(case):
    """Share of nonzero gY in family B: about 10 %, less where 10 % of the pixels times the largest term (4 + 2 * 2^-10) would come near
    2^13 = 2^24 / 2^11."""
    return min(0.10, 1400.0 / (case.N * case.H * case.W))


def _split_values(shape, gen):
    a = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, shape, generator=gen)]
    b = torch.randint(-1, 2, shape, generator=gen).float()
    b = torch.where((a.abs() == 1) & (b * a < 0), -b, b)          # 1 - 2^-11 is an fp16 number: keep b on a's side there
    return a, b


def family_b(case):
    """(X, gY, (xa, xb, ga, gb)) with X = xa + xb * 2^-11 and gY = ga + gb * 2^-11 (fp32 holds both exactly)."""
    gen = _gen(case, 2)
    xa, xb = _split_values((case.N, case.cin, case.H, case.W), gen)
    ga, gb = _split_values((case.N, case.cout, case.H, case.W), gen)
    keep = (torch.rand(ga.shape, generator=gen) < split_density(case)).float()
    ga, gb = ga * keep, gb * keep
    return xa + xb * 2.0 ** -11, ga + gb * 2.0 ** -11, (xa, xb, ga, gb)


def family_c(case):
    gen = _gen(case, 3)
    return (torch.randn(case.N, case.cin, case.H, case.W, generator=gen),
            torch.randn(case.N, case.cout, case.H, case.W, generator=gen))


def split16(x):
    """The stored split of the chunk planes: hi = fp16(x), lo = fp16(x - hi) (include/binhip.h), as fp32 tensors."""
    hi = x.half().float()
    return hi, (x - hi).half().float()


def reference(x, gy, ks, dtype=torch.float64):
    """(dW, db): autograd of F.conv2d(padding = ks // 2) in `dtype`."""
    cout, cin = gy.shape[1], x.shape[1]
    w = torch.zeros(cout, cin, ks, ks, dtype=dtype, requires_grad=True)
    b = torch.zeros(cout, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype), w, b, padding=ks // 2).backward(gy.to(dtype))
    return w.grad, b.grad


def split_reference(xh, xl, gh, gl, ks, nterms):
    """The kernels' definition on stored planes, in float64: dW = sum xh*gh + xl*gh + xh*gl (by linearity two backwards), db = sum gh + gl;
    nterms = 1: the hi planes alone."""
    if nterms == 1:
        return reference(xh, gh, ks)
    dw1, db1 = reference(xh.double() + xl.double(), gh, ks)
    dw2, db2 = reference(xh, gl, ks)
    return dw1 + dw2, db1 + db2


def planes_to_nchw(p, channels):
    """A chunk-plane tensor [chunks, N, H, W, 16] (any device) as NCHW fp32 on the CPU."""
    c, n, h, w, _ = p.shape
    return p.permute(1, 0, 4, 2, 3).reshape(n, c * 16, h, w)[:, :channels].float().cpu()


@functools.lru_cache(maxsize=None)
def reference_a(tag):
    """float64 (dW, db) of family A; cached per case and never modified by a test."""
    c = BY_TAG[tag]
    x, gy = family_a(c)
    return reference(x, gy, c.ks)


@functools.lru_cache(maxsize=None)
def reference_c(tag):
    c = BY_TAG[tag]
    x, gy = family_c(c)
    return reference(x, gy, c.ks)


def white_noise_bits(case, nterms):
    """{"dw", "db"}: sha256 of the bytes of the library's dW and db on family C (needs a GPU).  What tests/golden/make_wgrad_bits.py
    records and test_wgrad_white_noise_bits_are_the_recorded_ones recomputes."""
    import hashlib
    from bin_amd import ops
    x, gy = family_c(case)
    dw, db = ops.conv2d_bwd_weight(ops.nchw_to_planes(x.cuda(), nterms), ops.nchw_to_planes(gy.cuda(), nterms), case.cout, case.cin,
                                   case.ks, nterms)
    return {"dw": hashlib.sha256(dw.cpu().numpy().tobytes()).hexdigest(), "db": hashlib.sha256(db.cpu().numpy().tobytes()).hexdigest()}


def shuffle_rows(t):
    """The `cq` permutation of shuffle_perm: row co of the plain result lands at (co % cq) * 4 + co // cq, cq = cout / 4."""
    cout = t.shape[0]
    cq = cout // 4
    co = torch.arange(cout)
    out = torch.empty_like(t)
    out[(co % cq) * 4 + co // cq] = t
    return out
