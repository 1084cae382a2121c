"""CPU: the weight-gradient case table (tests/wgrad_cases.py) — its Python geometry against the library's own workspace size, every
case's property at 256 CUs, the exactness conditions of the integer and split-exact operand families, and the return codes of
binhip_conv2d_bwd_weight that are decided before any device work."""
import ctypes as C

import pytest
import torch

import wgrad_cases as wc


def _cus(lib):
    n = lib.binhip_device_cus()
    return n if n > 0 else wc.DEFAULT_CUS          # cus() of binhip_wgrad.hip


def test_geometry_matches_the_library_workspace_size():
    """geometry().workspace_bytes == binhip_wgrad_workspace_bytes for every case and over ks 1 / 3 / 5 x cin 16 .. 1152 x cout 3 .. 256 x
    frames, plus one-row frames of PB - 1, PB, PB + 1, 2 PB + 1 tiles: the size is (groups * PB * taps * 1024 + co tiles * PB * 32) floats,
    so kernel choice, groups and PB (clip and rounding to 8 included) are all in it."""
    from bin_amd import _lib as L
    lib = L.lib()
    cus = _cus(lib)
    for c in wc.CASES:
        g = wc.geometry(c.ks, c.N, c.H, c.W, c.cin, c.cout, cus)
        assert lib.binhip_wgrad_workspace_bytes(c.ks, c.N, c.H, c.W, wc.chunks(c.cin), c.cout) == g.workspace_bytes, c.tag
    cins = (16, 24, 36, 40, 60, 96, 128, 192, 224, 225, 240, 256, 257, 272, 512, 600, 1152)
    couts = (3, 12, 32, 35, 64, 96, 97, 128, 160, 256)
    frames = [(n, h, w) for n in (1, 3) for h in (1, 8, 9, 33) for w in (1, 32, 33, 200)]
    checked = 0
    for ks in (1, 3, 5):
        for cin in cins:
            for cout in couts:
                want = max(cus // wc.geometry(ks, 1, 1, 1, cin, cout, cus).groups, 1)
                around = [(1, 1, 32 * t) for t in (want - 1, want, want + 1, 2 * want + 1, 7, 8, 9) if t >= 1]
                for n, h, w in frames + around:
                    g = wc.geometry(ks, n, h, w, cin, cout, cus)
                    got = lib.binhip_wgrad_workspace_bytes(ks, n, h, w, wc.chunks(cin), cout)
                    assert got == g.workspace_bytes, (ks, n, h, w, cin, cout, got, g)
                    checked += 1
    assert checked > 15000


def test_geometry_kernel_choice_and_tile_split():
    """The variant thresholds of w1_plan() (one pair per wave and two rows up to 7 pairs, one row at 8, two pairs per wave from 9, a new
    column group every 16 pairs), use_w1()'s cout <= 96, and the tile split: min / max tiles per workgroup sum to the tile count."""
    assert [wc.geometry(1, 1, 8, 32, cin, 96).kernel for cin in (16, 224, 225, 256, 257, 512, 513, 1152)] == \
        ["w1<1,2>", "w1<1,2>", "w1<1,1>", "w1<1,1>", "w1<2,1>", "w1<2,1>", "w1<2,1>", "w1<2,1>"]
    assert [wc.geometry(1, 1, 8, 32, cin, 96).cgroups for cin in (256, 512, 513, 1024, 1025, 1152)] == [1, 1, 2, 2, 3, 3]
    assert wc.geometry(1, 1, 8, 32, 96, 96).kernel == "w1<1,2>" and wc.geometry(1, 1, 8, 32, 96, 97).kernel == "1x1_generic"
    assert wc.geometry(3, 1, 8, 32, 96, 96).kernel == "3x3" and wc.geometry(5, 1, 8, 32, 96, 96).kernel == "5x5"
    for c in wc.CASES:
        g = wc.geometry(c.ks, c.N, c.H, c.W, c.cin, c.cout)
        per_wg = [len(range(pb, g.ntiles, g.PB)) for pb in range(g.PB)]
        assert sum(per_wg) == g.ntiles and min(per_wg) == g.tiles_min and max(per_wg) == g.tiles_max, c.tag
        assert 1 <= g.PB <= g.ntiles and g.PB * g.groups <= max(wc.DEFAULT_CUS, g.groups)


@pytest.mark.parametrize("tag", wc.TAGS)
def test_case_properties_hold_at_256_cus(tag):
    wc.check_properties(wc.BY_TAG[tag], 256)


def test_case_table_covers_every_kernel_variant_and_property():
    """Every property of the table is carried by some case; every kernel and variant has a case of three or more rounds (the generic 1x1's
    tiles per workgroup reach two: its groups = pairs x co tiles exceed 11 at every cout > 96) and the listed tags exist."""
    used = {p for c in wc.CASES for p in c.props}
    assert used == set(wc.PROPERTIES), set(wc.PROPERTIES) ^ used
    for kernel in ("3x3", "5x5", "w1<1,2>", "w1<1,1>", "w1<2,1>"):
        assert any(kernel in c.props and ("rounds>=3" in c.props or "rounds>=6" in c.props) for c in wc.CASES), kernel
    assert any("1x1_generic" in c.props and "uneven" in c.props for c in wc.CASES)
    for kernel in ("3x3", "1x1_generic"):
        assert any(kernel in c.props and "plain_mapping" in c.props for c in wc.CASES), kernel
    for tags in (wc.SPLIT_TAGS, wc.ARG_TAGS, wc.SHUFFLE_TAGS, wc.GROUP_TAGS, wc.IMAGE_SUM_TAGS):
        assert set(tags) <= set(wc.TAGS) and len(set(tags)) == len(tags)
    assert all(wc.BY_TAG[t].cout % 4 == 0 for t in wc.SHUFFLE_TAGS) and all(wc.BY_TAG[t].N > 1 for t in wc.IMAGE_SUM_TAGS)
    assert len(wc.CASES) == 22


@pytest.mark.parametrize("tag", wc.TAGS)
def test_family_a_is_exact_in_any_order(tag):
    """Integers: sum |x| |g| (the same backward of the absolute values) < 2^24 for every output, so every fp32 partial sum is an exact
    integer in any order; and float32 autograd on the CPU returns the float64 reference exactly."""
    c = wc.BY_TAG[tag]
    x, gy = wc.family_a(c)
    assert torch.equal(x, x.round()) and torch.equal(gy, gy.round()) and float(x.abs().max()) <= 3 and float(gy.abs().max()) <= 15
    assert torch.equal(x.half().float(), x) and torch.equal(gy.half().float(), gy)
    m = wc.channel_mults(c.cout)
    assert set(m.tolist()) <= {1.0, 2.0, 5.0} and all(bool((m[k:] != m[:-k]).all()) for k in (1, 16, 32, 64) if k < c.cout)
    aw, ab = wc.reference(x.abs(), gy.abs(), c.ks)
    assert float(aw.max()) < wc.EXACT_LIMIT and float(ab.max()) < wc.EXACT_LIMIT
    dw, db = wc.reference_a(tag)
    dw32, db32 = wc.reference(x, gy, c.ks, torch.float32)
    assert torch.equal(dw32.double(), dw) and torch.equal(db32.double(), db)
    assert torch.equal(dw, dw.round()) and float(dw.abs().max()) > 0


@pytest.mark.parametrize("tag", wc.SPLIT_TAGS)
def test_family_b_splits_exactly_and_is_exact_in_any_order(tag):
    """a + b 2^-11 is stored as hi = a, lo = b 2^-11; the three live products are multiples of 2^-11 with 2^11 sum|terms| < 2^24 for every
    output, so the fp32 sums are exact in any order; about 90 % of gY is zero and all three products occur."""
    c = wc.BY_TAG[tag]
    x, gy, (xa, xb, ga, gb) = wc.family_b(c)
    xh, xl = wc.split16(x)
    gh, gl = wc.split16(gy)
    assert torch.equal(xh, xa) and torch.equal(xl, xb * 2.0 ** -11) and torch.equal(gh, ga) and torch.equal(gl, gb * 2.0 ** -11)
    zero = float((gy == 0).float().mean())
    assert 0.85 <= zero <= 0.99, zero
    if c.N * c.H * c.W > 16:
        assert bool((xl != 0).any()) and bool((gl != 0).any()) and bool((xl < 0).any()) and bool((xl > 0).any())
    aw, ab = wc.split_reference(xh.abs(), xl.abs(), gh.abs(), gl.abs(), c.ks, 3)
    assert 2.0 ** 11 * float(aw.max()) < wc.EXACT_LIMIT and 2.0 ** 11 * float(ab.max()) < wc.EXACT_LIMIT, float(aw.max())
    dw, db = wc.split_reference(xh, xl, gh, gl, c.ks, 3)
    assert torch.equal(dw * 2.0 ** 11, (dw * 2.0 ** 11).round()) and torch.equal(dw.float().double(), dw)
    assert torch.equal(db.float().double(), db)
    dw1, db1 = wc.split_reference(xh, xl, gh, gl, c.ks, 1)
    assert torch.equal(dw1, dw1.round()) and torch.equal(dw1, wc.reference(xa, ga, c.ks)[0])
    if c.N * c.H * c.W > 16:
        assert not torch.equal(dw, dw1), "the lo products contribute"


def test_shuffle_rows_is_the_pixel_shuffle_permutation():
    t = torch.arange(12.0).view(12, 1)
    assert wc.shuffle_rows(t).view(-1).tolist() == [0, 3, 6, 9, 1, 4, 7, 10, 2, 5, 8, 11]


# ------------------------------------------------------------------------------------------------ return codes without device work
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


def _call(lib, n=1, h=8, w=32, ks=3, cin_chunks=2, cout=32, nterms=1, cin=32, shuffle=0, ws_bytes=None, null=(), desc=True):
    """binhip_conv2d_bwd_weight with host dummies for every pointer: each call here is rejected before a kernel is launched."""
    from bin_amd import _lib as L
    d = L.BinConvDesc()
    d.N, d.H, d.W, d.ksize, d.cin_chunks, d.cout, d.nterms = n, h, w, ks, cin_chunks, cout, nterms
    dummy = (C.c_char * 64)()
    p = {k: C.cast(dummy, C.c_void_p) for k in ("x_hi", "x_lo", "gy_hi", "gy_lo", "ws", "dw", "db")}
    for k in null:
        p[k] = C.c_void_p(0)
    if ws_bytes is None:
        ws_bytes = lib.binhip_wgrad_workspace_bytes(ks, n, h, w, cin_chunks, cout) - 1
    return lib.binhip_conv2d_bwd_weight(C.byref(d) if desc else None, p["x_hi"], p["x_lo"], p["gy_hi"], p["gy_lo"], None, p["ws"],
                                        ws_bytes, p["dw"], p["db"], cin, shuffle, 0, None)


def test_bwd_weight_return_codes_before_any_launch():
    from bin_amd import _lib as L
    lib = L.lib()
    assert lib.binhip_wgrad_workspace_bytes(3, 1, 8, 32, 2, 32) > 256
    for c in wc.CASES:                                            # a workspace one byte short, for every kernel and variant
        for nterms in (1, 3):
            assert _call(lib, c.N, c.H, c.W, c.ks, wc.chunks(c.cin), c.cout, nterms, c.cin) == E_WORKSPACE, c.tag
    assert _call(lib, ws_bytes=0) == E_WORKSPACE
    assert _call(lib, n=64, h=1024, w=1024, ws_bytes=0) == E_SHAPE                  # N H W = 2^26
    assert _call(lib, n=1, h=1, w=(1 << 26) - 1, ws_bytes=0) == E_WORKSPACE          # one below: past the shape checks
    for ks in (7, 2, 0, -3):                                      # no workspace size for a kernel size the library does not have
        assert _call(lib, ks=ks, ws_bytes=1 << 30) == E_SHAPE, ks
        assert lib.binhip_wgrad_workspace_bytes(ks, 1, 8, 32, 2, 32) == 0, ks
    assert _call(lib, cin=33) == E_SHAPE and _call(lib, cin=0) == E_SHAPE           # cin > 16 cin_chunks; no channels
    assert _call(lib, cin=32) == E_WORKSPACE and _call(lib, cin=17) == E_WORKSPACE
    assert _call(lib, cout=34, shuffle=1) == E_SHAPE and _call(lib, cout=36, shuffle=1) == E_WORKSPACE
    for bad in (dict(n=0), dict(h=0), dict(w=-1), dict(cin_chunks=0), dict(cout=0)):
        assert _call(lib, ws_bytes=1 << 20, **bad) == E_SHAPE, bad
    assert _call(lib, nterms=2) == E_ARG and _call(lib, nterms=0) == E_ARG
    assert _call(lib, desc=False) == E_ARG
    for name in ("x_hi", "gy_hi", "ws", "dw"):
        assert _call(lib, null=(name,)) == E_ARG, name
    for name in ("x_lo", "gy_lo"):
        assert _call(lib, nterms=3, null=(name,)) == E_ARG, name
        assert _call(lib, nterms=1, null=(name,)) == E_WORKSPACE, name            # the lo planes are not needed at nterms = 1
    assert _call(lib, null=("db",)) == E_WORKSPACE                                 # db is optional


def test_wrapper_checks_out_before_any_launch():
    """ops.conv2d_bwd_weight: accumulate needs something to add to, and `out` must be device fp32 of the right shapes."""
    from bin_amd import ops
    x = ops.CP(torch.zeros(2, 1, 8, 32, 16, dtype=torch.float16), None, 32)
    gy = ops.CP(torch.zeros(2, 1, 8, 32, 16, dtype=torch.float16), None, 32)
    ws = torch.zeros(wc.geometry(3, 1, 8, 32, 32, 32).workspace_bytes, dtype=torch.uint8)
    with pytest.raises(ValueError, match="needs out"):
        ops.conv2d_bwd_weight(x, gy, 32, 32, 3, 1, accumulate=True, workspace=ws)
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
        ops.conv2d_bwd_weight(x, gy, 32, 32, 3, 1, out=(torch.zeros(32, 32, 3, 3), torch.zeros(32)), workspace=ws)
