"""CPU: the folded main launch of the fused UPNet (BINHIP_PLAN_UPNET_FOLD) is a pure re-indexing of the 5x5 form.
`rdn_plan.folded_upnet_weights` maps the interior operator to the slab [chunk][t = 0..4][b = 0..3][32 rows][16 channels]; here that
slab is applied in float64 exactly as the kernel walks it: 16 x 32 tiles of matrix positions, a wave per position pair (Y, Y + 1), the
five input rows Y - 2 + t and four columns X - 2 + b out of a zero-padded patch, rows 0-11 of the product stored as the shifted 2 x 2
blocks of position Y and rows 16-27 as those of Y + 1, nothing on the full-resolution border ring (upnet_ring_kernel owns it) or outside
the image."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bin_amd.rdn_plan import folded_upnet_planes, folded_upnet_weights, fused_upnet_weights

G0 = 32
SHAPES = [(1, 1), (2, 3), (5, 16), (16, 5), (17, 33)]
TH, TW = 16, 32


@pytest.fixture(scope="module")
def operator():
    g = torch.Generator().manual_seed(0)
    w0, b0 = torch.randn(256, G0, 3, 3, generator=g).double() * 0.1, torch.randn(256, generator=g).double() * 0.1
    w2, b2 = torch.randn(3, 64, 3, 3, generator=g).double() * 0.1, torch.randn(3, generator=g).double()
    W, B = fused_upnet_weights(w0, b0, w2, b2)
    return W[4], B[4]


def folded_main_launch(x, slab, bias):
    """What the folded kernel stores: (out [N, 3, 2H, 2W], NaN where it stores nothing; count of stores per pixel)."""
    n, g0, H, W = x.shape
    ty, tx = -(-H // TH), -(-W // TW)
    out = np.full((n, 3, 2 * H, 2 * W), np.nan)
    count = np.zeros((3, 2 * H, 2 * W), dtype=np.int64)
    xc = x.reshape(n, g0 // 16, 16, H, W)
    for t_y in range(ty):
        for t_x in range(tx):
            y0, x0 = t_y * TH, t_x * TW
            # the patch image: TH + 4 rows x TW + 4 columns around the tile, 2 of halo, zero outside the image
            patch = np.zeros((n, g0 // 16, 16, TH + 4, TW + 4))
            ys, xs = np.arange(y0 - 2, y0 + TH + 2), np.arange(x0 - 2, x0 + TW + 2)
            oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
            iy, ix = np.nonzero(oky)[0][:, None], np.nonzero(okx)[0][None, :]
            patch[:, :, :, iy, ix] = xc[:, :, :, ys[oky][:, None], xs[okx][None, :]]
            for wave in range(TH // 2):
                acc = np.zeros((n, 32, TW))                               # one accumulator tile: 32 rows x 32 positions
                for b in range(4):
                    for t in range(5):
                        frag = patch[:, :, :, 2 * wave + t, b:b + TW]     # [n, chunk, channel, position]
                        acc += np.einsum("cmk,nckp->nmp", slab[:, t, b], frag)
                for r in range(2):
                    Y = y0 + 2 * wave + r
                    for m in range(12):
                        c, i, j = m >> 2, (m >> 1) & 1, m & 1
                        R = 2 * Y - i
                        if not 1 <= R <= 2 * H - 2:
                            continue
                        C = 2 * (x0 + np.arange(TW)) - j
                        ok = (C >= 1) & (C <= 2 * W - 2)
                        out[:, c, R, C[ok]] = acc[:, 16 * r + m][:, ok] + bias[m]
                        count[c, R, C[ok]] += 1
    return out, count


@pytest.mark.parametrize("hw", SHAPES)
def test_folded_slab_equals_the_5x5_operator_off_the_ring(hw, operator):
    W4, B4 = operator
    H, W = hw
    g = torch.Generator().manual_seed(1 + H * 64 + W)
    # both sides add the same 16 x G0 float64 products per pixel in different orders: a few ulps of the result.  The bar is absolute, so
    # the inputs keep |out| below 4 (ulp 4.4e-16 .. 8.9e-16): 1e-14 is then at least 11 ulps, far below any mis-indexed tap (~1e-2)
    x = torch.randn(2, G0, H, W, generator=g).double() * 0.1
    ref = F.pixel_shuffle(F.conv2d(x, W4, B4, padding=2), 2).numpy()
    slab = folded_upnet_weights(W4)
    assert tuple(slab.shape) == (G0 // 16, 5, 4, 32, 16)
    out, count = folded_main_launch(x.numpy(), slab.numpy(), B4.numpy())
    ring = np.ones((2 * H, 2 * W), dtype=bool)
    ring[1:-1, 1:-1] = False
    # every full-resolution pixel exactly once: the ring by upnet_ring_kernel (one workgroup per ring pixel), the rest by the main launch
    assert np.array_equal(count + ring, np.ones_like(count))
    assert np.isnan(out[:, :, ring]).all()
    if (~ring).any():
        err = np.abs(out[:, :, ~ring] - ref[:, :, ~ring]).max()
        print(f"{H} x {W}: folded vs 5x5 max-abs {err:.2e}, |out| {np.abs(ref).max():.2f}")
        assert err <= 1e-14 and np.abs(ref).max() < 4.0


def test_folded_slab_is_a_selection_of_the_operator(operator):
    """No arithmetic: rows 12-15 / 28-31, t = 4 of the first position and t = 0 of the second are zero, every other entry is one of the
    operator's, and each non-zero operator entry appears exactly twice (once per position of the pair)."""
    W4, _ = operator
    slab = folded_upnet_weights(W4)
    assert float(slab[:, :, :, 12:16].abs().max()) == 0.0 and float(slab[:, :, :, 28:32].abs().max()) == 0.0
    assert float(slab[:, 4, :, 0:12].abs().max()) == 0.0 and float(slab[:, 0, :, 16:28].abs().max()) == 0.0
    assert torch.equal(slab[:, 0:4, :, 0:12], slab[:, 1:5, :, 16:28])
    nz = W4[W4 != 0]
    assert torch.equal(torch.sort(slab[slab != 0]).values, torch.sort(torch.cat((nz, nz))).values)
    assert int((W4 != 0).sum()) == 12 * G0 * 16                        # the operator's own zeros: 4 x 4 taps of 25 per channel


def test_folded_planes_match_the_relayout_rounding_and_swizzle(operator):
    """hi = fp16(w), lo = fp16(w - hi) of the fp32-rounded slab; rows 8-15 and 24-31 carry their two 8-channel slots swapped."""
    W4, _ = operator
    slab = folded_upnet_weights(W4)
    hi, lo = folded_upnet_planes(slab)
    hi, lo = hi.view(G0 // 16, 20, 32, 2, 8), lo.view(G0 // 16, 20, 32, 2, 8)
    w = slab.float().view(G0 // 16, 20, 32, 2, 8)
    for row in (0, 7, 8, 11, 16, 23, 24, 27):
        s = (row >> 3) & 1
        for slot in range(2):
            want = w[:, :, row, slot ^ s]
            assert torch.equal(hi[:, :, row, slot], want.half())
            assert torch.equal(lo[:, :, row, slot], (want - want.half().float()).half())
    assert float((hi.float() + lo.float()).abs().max()) > 0
