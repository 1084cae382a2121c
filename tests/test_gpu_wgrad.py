"""-m gpu: weight-gradient kernels (3x3 X-row, 5x5, 1x1 streaming, the batched reduction) and the conv backward-data/weight fixtures, against the reference's autograd outputs and float64; and, over the case table of tests/wgrad_cases.py, exact integer and split-exact probes that both precisions must
return bit for bit ("Weight-gradient kernels")."""
import functools
import hashlib
import json
import os
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden
import wgrad_cases as wc

pytestmark = pytest.mark.gpu


CONVS_BWD = {
    "k2_sfe1_24": ("model1.SFENet1", 5), "k2_sfe1_36": ("model2.SFENet1", 5), "k2_sfe1_60": ("model3.SFENet1", 5),
    "k3_sfe2": ("model1.SFENet2", 3),
    "k4_rdbconv0": ("model1.RDBs.0.convs.0.conv.0", 3), "k4_rdbconv1": ("model1.RDBs.0.convs.1.conv.0", 3),
    "k4_rdbconv2": ("model1.RDBs.0.convs.2.conv.0", 3), "k4_rdbconv3": ("model1.RDBs.0.convs.3.conv.0", 3),
    "k5_lff": ("model1.RDBs.0.LFF", 1), "k6_gff0": ("model1.GFF.0", 1), "k8_up0": ("model1.UPNet.0", 3),
    "k9_up2": ("model1.UPNet.2", 3),
}


TOL_BWD = {1: 3e-3, 3: 3e-5}


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("key", sorted(CONVS_BWD))
def test_conv_dgrad_wgrad_golden(key, nterms, canon_gpu):
    """dX, dW, db of every live conv shape vs the reference autograd (g1_convs)."""
    from bin_amd import ops
    g = load_golden("g1_convs")
    wname, ks = CONVS_BWD[key]
    w = canon_gpu[wname + ".weight"]
    cout, cin = w.shape[0], w.shape[1]
    x = torch.from_numpy(g[key + ".x"]).cuda()
    gy = torch.from_numpy(g[key + ".gy"]).cuda()
    gyp = ops.nchw_to_planes(gy, nterms)
    gx = ops.planes_to_nchw(ops.conv2d_bwd_data(gyp, ops.DgradWeights(w, nterms)), cin)
    assert _rel(gx, torch.from_numpy(g[key + ".gx"]).cuda()) <= TOL_BWD[nterms], "dgrad"
    dw, db = ops.conv2d_bwd_weight(ops.nchw_to_planes(x, nterms), gyp, cout, cin, ks, nterms)
    assert _rel(dw, torch.from_numpy(g[key + ".gw"]).cuda()) <= TOL_BWD[nterms], "wgrad"
    assert _rel(db, torch.from_numpy(g[key + ".gb"]).cuda()) <= TOL_BWD[nterms], "dbias"


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 19, 45), (1, 8, 32)])
def test_wgrad_ragged(nterms, shape):
    from bin_amd import ops
    n, h, w = shape
    gen = torch.Generator().manual_seed(h * 100 + w)
    x = torch.randn(n, 40, h, w, generator=gen, dtype=torch.float64)
    gy = torch.randn(n, 35, h, w, generator=gen, dtype=torch.float64)
    wt = torch.zeros(35, 40, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(35, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, wt, b, padding=1).backward(gy)
    dw, db = ops.conv2d_bwd_weight(ops.nchw_to_planes(x.float().cuda(), nterms),
                                   ops.nchw_to_planes(gy.float().cuda(), nterms), 35, 40, 3, nterms)
    assert _rel(dw.cpu().double(), wt.grad) <= TOL_BWD[nterms]
    assert _rel(db.cpu().double(), b.grad) <= TOL_BWD[nterms]


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("cfg", [(2, 33, 70, 192, 32), (1, 16, 32, 96, 96), (3, 17, 40, 224, 35), (1, 40, 33, 16, 32),
                                 (2, 64, 64, 160, 32), (1, 130, 31, 128, 64)])
def test_wgrad_3x3_shapes(nterms, cfg):
    """the 3x3 weight-gradient kernel (eight waves, two LDS stages) over 1-7 channel pairs, 1-3 output tiles, tiles that hang
    over the right / bottom edge, more workgroups than tiles, several images (reference: autograd of F.conv2d(padding=1),
    RDN.py:141,187-207).  The same shapes validated the rolling-row experiment of the tuning build."""
    from bin_amd import ops
    n, h, w, cin, cout = cfg
    gen = torch.Generator().manual_seed(h * 1000 + w + cin)
    x = torch.randn(n, cin, h, w, generator=gen, dtype=torch.float64)
    gy = torch.randn(n, cout, h, w, generator=gen, dtype=torch.float64)
    wt = torch.zeros(cout, cin, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, wt, b, padding=1).backward(gy)
    xp, gp = ops.nchw_to_planes(x.float().cuda(), nterms), ops.nchw_to_planes(gy.float().cuda(), nterms)
    dw, db = ops.conv2d_bwd_weight(xp, gp, cout, cin, 3, nterms)
    assert _rel(dw.cpu().double(), wt.grad) <= TOL_BWD[nterms]
    assert _rel(db.cpu().double(), b.grad) <= TOL_BWD[nterms]
    dw2, db2 = ops.conv2d_bwd_weight(xp, gp, cout, cin, 3, nterms)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "fixed summation order"


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("cfg", [(1, 5, 7, 40, 35), (2, 19, 45, 224, 96), (1, 8, 32, 16, 96), (1, 33, 70, 600, 64),
                                 (3, 6, 40, 272, 96), (1, 130, 64, 1152, 96)])
def test_wgrad_1x1_ragged(nterms, cfg):
    """the streaming 1x1 kernel: one / two channel pairs per wave, 1-3 workgroup columns, odd chunk counts, strips that hang
    over the right and bottom edges, more workgroups than strips (reference: autograd of F.conv2d, RDN.py:141,162)."""
    from bin_amd import ops
    n, h, w, cin, cout = cfg
    gen = torch.Generator().manual_seed(h * 100 + w + cin)
    x = torch.randn(n, cin, h, w, generator=gen, dtype=torch.float64)
    gy = torch.randn(n, cout, h, w, generator=gen, dtype=torch.float64)
    wt = torch.zeros(cout, cin, 1, 1, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(cout, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.conv2d(x, wt, b).backward(gy)
    dw, db = ops.conv2d_bwd_weight(ops.nchw_to_planes(x.float().cuda(), nterms),
                                   ops.nchw_to_planes(gy.float().cuda(), nterms), cout, cin, 1, nterms)
    assert _rel(dw.cpu().double(), wt.grad) <= TOL_BWD[nterms]
    assert _rel(db.cpu().double(), b.grad) <= TOL_BWD[nterms]
    dw2, db2 = ops.conv2d_bwd_weight(ops.nchw_to_planes(x.float().cuda(), nterms),
                                     ops.nchw_to_planes(gy.float().cuda(), nterms), cout, cin, 1, nterms)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "fixed summation order"


# ------------------------------------------------------------------------------------------------ the case table (tests/wgrad_cases.py)
# Exact probes: operands whose products and partial sums are exact in fp16, in the MFMA and in fp32 (families A and B), so both precisions
# must return the float64 reference BIT FOR BIT whatever the summation order; no tolerance anywhere but in the white-noise family C, which
# keeps TOL_BWD.  Every test asserts the case's work-split property with the CU count of the device it runs on.
SENTINEL = -7.25e7
GUARD = 61                                # floats of sentinel on either side of dw / db: the views start off a 16-byte boundary


def _case(tag):
    """(case, geometry on this device) with every property of the case asserted, and the library's workspace size held to geometry()."""
    from bin_amd import _lib as L
    lib = L.lib()
    c = wc.BY_TAG[tag]
    g = wc.check_properties(c, lib.binhip_device_cus())
    assert lib.binhip_wgrad_workspace_bytes(c.ks, c.N, c.H, c.W, wc.chunks(c.cin), c.cout) == g.workspace_bytes
    return c, g


def _planes(t, nterms):
    from bin_amd import ops
    return ops.nchw_to_planes(t.cuda(), nterms)


def _exact(got, ref, what):
    """torch.equal against the float64 reference, with the count and size of the differences in the message."""
    got = got.detach().cpu().double()
    if not torch.equal(got, ref):
        bad = got != ref                                          # a NaN differs from everything
        diff = (got - ref)[bad]
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} differ, largest |difference| {float(diff.abs().max())}, "
                             f"first at {tuple(bad.nonzero()[0].tolist())}: got {float(got[bad][0])}, reference {float(ref[bad][0])}")


def _guarded(shape):
    """(view, whole buffer): a contiguous fp32 view of `shape` with GUARD sentinel floats on either side."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf[GUARD:GUARD + n].view(shape), buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _nan_workspace(g, extra=0):
    """A caller's workspace of exactly the needed size (+ extra), every byte of it a NaN pattern, 16 bytes into its allocation."""
    ws = torch.full((g.workspace_bytes // 4 + 8 + (extra + 3) // 4,), float("nan"), dtype=torch.float32, device="cuda").view(torch.uint8)
    return ws[16:16 + g.workspace_bytes + extra]


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.TAGS)
def test_wgrad_integer_probe_is_bit_exact(tag, nterms):
    """Family A over the whole table: dW and db are the float64 reference's integers, bit for bit, in both precisions."""
    from bin_amd import ops
    c, g = _case(tag)
    x, gy = wc.family_a(c)
    dw, db = ops.conv2d_bwd_weight(_planes(x, nterms), _planes(gy, nterms), c.cout, c.cin, c.ks, nterms)
    rw, rb = wc.reference_a(tag)
    _exact(dw, rw, f"{tag} dW ({g.kernel}, PB {g.PB}, {g.tiles_min}-{g.tiles_max} tiles per workgroup)")
    _exact(db, rb, f"{tag} db")


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.SPLIT_TAGS)
def test_wgrad_split_exact_probe_is_bit_exact(tag, nterms):
    """Family B: the stored planes are hi = a, lo = b 2^-11, and the result is sum xh gh + xl gh + xh gl of those planes exactly (at
    nterms = 1 the pure-hi part, an integer)."""
    from bin_amd import ops
    c, g = _case(tag)
    x, gy, (xa, xb, ga, gb) = wc.family_b(c)
    xp, gp = _planes(x, nterms), _planes(gy, nterms)
    xh, gh = wc.planes_to_nchw(xp.hi, c.cin), wc.planes_to_nchw(gp.hi, c.cout)
    assert torch.equal(xh, xa) and torch.equal(gh, ga), "hi planes"
    if nterms == 3:
        xl, gl = wc.planes_to_nchw(xp.lo, c.cin), wc.planes_to_nchw(gp.lo, c.cout)
        assert torch.equal(xl, xb * 2.0 ** -11) and torch.equal(gl, gb * 2.0 ** -11), "lo planes"
    else:
        xl = gl = None
    rw, rb = wc.split_reference(xh, xl, gh, gl, c.ks, nterms)
    dw, db = ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms)
    _exact(dw, rw, f"{tag} dW ({g.kernel})")
    _exact(db, rb, f"{tag} db")


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.ARG_TAGS)
def test_wgrad_accumulate_and_inv_scale_are_exact(tag, nterms):
    """accumulate = 1 onto integer-filled dW / db gives the integer sum; inv_scale = 2^-3 and 2^5 scale the integers exactly."""
    from bin_amd import ops
    c, _ = _case(tag)
    x, gy = wc.family_a(c)
    xp, gp = _planes(x, nterms), _planes(gy, nterms)
    rw, rb = wc.reference_a(tag)
    gen = torch.Generator().manual_seed(77)
    dw0 = torch.randint(-1000, 1001, rw.shape, generator=gen).float()
    db0 = torch.randint(-1000, 1001, rb.shape, generator=gen).float()
    dw, db = dw0.clone().cuda(), db0.clone().cuda()
    out = ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms, accumulate=True, out=(dw, db))
    assert out[0] is dw and out[1] is db
    _exact(dw, rw + dw0.double(), f"{tag} accumulated dW")
    _exact(db, rb + db0.double(), f"{tag} accumulated db")
    for scale in (2.0 ** -3, 2.0 ** 5):
        sc = torch.tensor([scale, 1.0 / scale], dtype=torch.float32, device="cuda")
        sw, sb = ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms, inv_scale=sc[:1])
        _exact(sw, rw * scale, f"{tag} dW x {scale}")
        _exact(sb, rb * scale, f"{tag} db x {scale}")
    ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms, inv_scale=sc[:1], accumulate=True, out=(dw, db))
    _exact(dw, rw * 33 + dw0.double(), f"{tag} dW accumulated twice, the second time x 32")
    _exact(db, rb * 33 + db0.double(), f"{tag} db accumulated twice")


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.SHUFFLE_TAGS)
def test_wgrad_shuffle_perm_is_the_row_permutation(tag, nterms):
    """shuffle_perm at cout 256: row co of the plain result lands at row (co % 64) * 4 + co // 64 (UPNet.0's PixelShuffle order)."""
    from bin_amd import ops
    c, _ = _case(tag)
    x, gy = wc.family_a(c)
    dw, db = ops.conv2d_bwd_weight(_planes(x, nterms), _planes(gy, nterms), c.cout, c.cin, c.ks, nterms, shuffle=True)
    rw, rb = wc.reference_a(tag)
    _exact(dw, wc.shuffle_rows(rw), f"{tag} shuffled dW")
    _exact(db, wc.shuffle_rows(rb), f"{tag} shuffled db")


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.GROUP_TAGS)
def test_wgrad_grouped_input_planes(tag, nterms):
    """x_cpg = 6 with a group stride of 14 planes (GFF.0 reads planes 0 - 5 of each block buffer): input chunk i is plane
    14 (i // 6) + i % 6 of a buffer whose other planes hold 1000.0.  Equal to the call on the gathered planes, and to the reference."""
    from bin_amd import ops
    c, _ = _case(tag)
    x, gy = wc.family_a(c)
    xp, gp = _planes(x, nterms), _planes(gy, nterms)
    cc = wc.chunks(c.cin)
    ngroups = (cc + 5) // 6
    big_hi = torch.full((14 * ngroups,) + tuple(xp.hi.shape[1:]), 1000.0, dtype=torch.float16, device="cuda")
    big_lo = torch.full_like(big_hi, 1000.0) if nterms == 3 else None
    for i in range(cc):
        big_hi[14 * (i // 6) + i % 6] = xp.hi[i]
        if nterms == 3:
            big_lo[14 * (i // 6) + i % 6] = xp.lo[i]
    plane = xp.hi[0].numel()
    dw, db = ops.conv2d_bwd_weight(ops.CP(big_hi, big_lo, c.cin), gp, c.cout, c.cin, c.ks, nterms, x_cpg=6, x_group_stride=14 * plane)
    pw, pb = ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms)
    assert torch.equal(dw, pw) and torch.equal(db, pb), "grouped planes != gathered planes"
    rw, rb = wc.reference_a(tag)
    _exact(dw, rw, f"{tag} dW from grouped planes")
    _exact(db, rb, f"{tag} db from grouped planes")


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.TAGS)
def test_wgrad_relies_on_no_memory_contents(tag, nterms):
    """A caller's workspace full of NaN (and 16 bytes off its allocation), dW / db as views inside buffers of a sentinel: after a
    non-accumulating call the results are exact and every sentinel stands, whatever cout leaves of the last 32- or 64-wide tile (35, 3,
    12).  A workspace one byte short is refused and writes nothing."""
    from bin_amd import ops
    c, g = _case(tag)
    x, gy = wc.family_a(c)
    xp, gp = _planes(x, nterms), _planes(gy, nterms)
    dw, dw_buf = _guarded((c.cout, c.cin, c.ks, c.ks))
    db, db_buf = _guarded((c.cout,))
    with pytest.raises(RuntimeError, match="workspace too small"):
        ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms, out=(dw, db), workspace=_nan_workspace(g, -1))
    assert bool((dw_buf == SENTINEL).all()) and bool((db_buf == SENTINEL).all())
    ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms, out=(dw, db), workspace=_nan_workspace(g))
    rw, rb = wc.reference_a(tag)
    _exact(dw, rw, f"{tag} dW with a NaN workspace")
    _exact(db, rb, f"{tag} db with a NaN workspace")
    assert _guards_intact(dw_buf) and _guards_intact(db_buf), "sentinel around dW / db overwritten"


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.IMAGE_SUM_TAGS)
def test_wgrad_batch_equals_the_sum_of_its_images(tag, nterms):
    """The N-image call equals the exact sum of its N single-image calls (which split their tiles differently: another PB, other
    rounds), accumulated by the kernel itself into one buffer."""
    from bin_amd import ops
    c, _ = _case(tag)
    x, gy = wc.family_a(c)
    dw, db = ops.conv2d_bwd_weight(_planes(x, nterms), _planes(gy, nterms), c.cout, c.cin, c.ks, nterms)
    sw, sb = torch.zeros_like(dw), torch.zeros_like(db)
    for i in range(c.N):
        ops.conv2d_bwd_weight(_planes(x[i:i + 1], nterms), _planes(gy[i:i + 1], nterms), c.cout, c.cin, c.ks, nterms, accumulate=True,
                              out=(sw, sb))
    assert torch.equal(dw, sw) and torch.equal(db, sb)
    rw, rb = wc.reference_a(tag)
    _exact(sw, rw, f"{tag} dW summed over single images")


_ratios = {}


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.TAGS)
def test_wgrad_white_noise_vs_float64(tag, nterms):
    """Family C over the whole table against float64 at TOL_BWD; two calls give the same bits (fixed summation order).  Prints the
    largest error-to-bar ratio so far per kernel and precision."""
    from bin_amd import ops
    c, g = _case(tag)
    x, gy = wc.family_c(c)
    xp, gp = _planes(x, nterms), _planes(gy, nterms)
    dw, db = ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms)
    rw, rb = wc.reference_c(tag)
    ew, eb = _rel(dw.cpu().double(), rw), _rel(db.cpu().double(), rb)
    key = (g.kernel, nterms)
    _ratios[key] = max(_ratios.get(key, 0.0), ew / TOL_BWD[nterms], eb / TOL_BWD[nterms])
    print(f"wgrad family C {tag} nterms={nterms} {g.kernel}: dW {ew:.3g} db {eb:.3g} bar {TOL_BWD[nterms]:g}; "
          f"largest error / bar of {g.kernel} so far {_ratios[key]:.3f}")
    assert ew <= TOL_BWD[nterms] and eb <= TOL_BWD[nterms]
    dw2, db2 = ops.conv2d_bwd_weight(xp, gp, c.cout, c.cin, c.ks, nterms)
    assert torch.equal(dw, dw2) and torch.equal(db, db2), "fixed summation order"


@functools.lru_cache(maxsize=None)
def _recorded_bits():
    with open(os.path.join(GOLDEN, "wgrad_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("tag", wc.TAGS)
def test_wgrad_white_noise_bits_are_the_recorded_ones(tag, nterms):
    """Families A and B are exact in any summation order; this holds the order itself: dW and db of family C are, bit for bit, what
    tests/golden/make_wgrad_bits.py recorded from the commit named in tests/golden/wgrad_bits.json.  PB and with it the order depend on
    the CU count, so on a device with another CU count than the fixture's the test fails and says so."""
    from bin_amd import _lib as L
    rec = _recorded_bits()
    cus = L.lib().binhip_device_cus()
    assert cus == rec["cus"], (f"tests/golden/wgrad_bits.json was recorded on a device of {rec['cus']} CUs, this one has {cus}: another "
                               f"pixel-block split, another summation order; record the fixture anew for this device")
    key = f"{tag}/{nterms}"
    assert key in rec["bits"], f"{key} is not in the fixture (left out as not reproducible: {rec['left_out']})"
    got = wc.white_noise_bits(wc.BY_TAG[tag], nterms)
    assert got == rec["bits"][key], f"{key}: the bits differ from those recorded from {rec['recorded_from']}"


# ------------------------------------------------------------------------------------------------ live wgrad timing
def test_backward_profiler_times_the_weight_gradient_launches():
    import ctypes
    from bin_amd import _lib as L
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict, synthetic_frames
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    net = net.cuda().train()
    frames = [f.cuda() for f in synthetic_frames(3, 1, 64, 64, 6)]
    lib = L.lib()
    handle = ctypes.c_void_p(0)
    L.check(lib.binhip_profiler_create(3, 32, L.PROF_WGRAD, 512, ctypes.byref(handle)), "profiler_create")
    try:
        net.set_profiler(handle, backward=True)
        loss = sum((o * o).mean() for o in net(*frames))
        loss.backward()
        torch.cuda.synchronize()
        net.set_profiler(None, backward=True)
        ms, n = ctypes.c_double(0), ctypes.c_int(0)
        L.check(lib.binhip_profiler_read(handle, ctypes.byref(ms), ctypes.byref(n)), "profiler_read")
        assert n.value == 4 * 12 * 4                      # four RDN calls x 12 dense blocks x 4 convs (3x3, 32 outputs)
        assert 0.0 < ms.value < 1e4
    finally:
        lib.binhip_profiler_destroy(handle)
