"""CPU: util.compare_ssim (the reference test.py's SSIM, skimage compare_ssim(multichannel=True) restated) and the argument checks of
the device scoring entry points (binhip_image_score*), which return before any HIP call."""
import ctypes as C

import numpy as np
import pytest

from bin_amd import _lib as L
from bin_amd.utils import util


def _closed_form_7x7(x, y):
    """SSIM of one 7x7 window from plain sums: means over 49, variances and covariance over 48."""
    x, y = x.astype(np.float64).ravel(), y.astype(np.float64).ravel()
    mx, my = x.sum() / 49, y.sum() / 49
    vx = ((x - mx) ** 2).sum() / 48
    vy = ((y - my) ** 2).sum() / 48
    vxy = ((x - mx) * (y - my)).sum() / 48
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    return ((2 * mx * my + c1) * (2 * vxy + c2)) / ((mx * mx + my * my + c1) * (vx + vy + c2))


def test_compare_ssim_of_one_window_is_the_closed_form():
    g = np.random.default_rng(1)
    a = g.integers(0, 256, (7, 7, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) + g.integers(-40, 41, (7, 7, 3)), 0, 255).astype(np.uint8)
    per = [_closed_form_7x7(a[..., c], b[..., c]) for c in range(3)]
    assert util.compare_ssim(a[..., 0], b[..., 0]) == pytest.approx(per[0], rel=0, abs=1e-13)
    assert util.compare_ssim(a, b) == pytest.approx(sum(per) / 3, rel=0, abs=1e-13)


def test_compare_ssim_identity_channels_and_size():
    g = np.random.default_rng(2)
    a = g.integers(0, 256, (19, 23, 3), dtype=np.uint8)
    b = g.integers(0, 256, (19, 23, 3), dtype=np.uint8)
    assert util.compare_ssim(a, a) == 1.0
    assert util.compare_ssim(np.full((9, 9, 3), 77, np.uint8), np.full((9, 9, 3), 77, np.uint8)) == 1.0
    per = [util.compare_ssim(a[..., c], b[..., c]) for c in range(3)]
    assert util.compare_ssim(a, b) == pytest.approx(np.mean(per), rel=0, abs=1e-15)
    assert -1.0 <= util.compare_ssim(a, b) < 0.5
    for shape in ((6, 30, 3), (30, 6, 3), (6, 6)):
        with pytest.raises(ValueError):
            util.compare_ssim(np.zeros(shape, np.uint8), np.zeros(shape, np.uint8))
    with pytest.raises(ValueError):
        util.compare_ssim(a, b[:-1])


def test_compare_ssim_matches_a_uniform_filter_restatement():
    ndimage = pytest.importorskip("scipy.ndimage")
    g = np.random.default_rng(3)
    a = g.integers(0, 256, (40, 57, 3), dtype=np.uint8)
    b = np.clip(a.astype(int) + g.integers(-60, 61, a.shape), 0, 255).astype(np.uint8)

    def sk(x, y):
        x, y = x.astype(np.float64), y.astype(np.float64)
        f = lambda z: ndimage.uniform_filter(z, size=7)
        ux, uy = f(x), f(y)
        vx, vy, vxy = (49 / 48) * (f(x * x) - ux * ux), (49 / 48) * (f(y * y) - uy * uy), (49 / 48) * (f(x * y) - ux * uy)
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
        return s[3:-3, 3:-3].mean()
    for x, y in ((a, b), (a, g.integers(0, 256, a.shape, dtype=np.uint8))):
        want = np.mean([sk(x[..., c], y[..., c]) for c in range(3)])
        assert abs(util.compare_ssim(x, y) - want) <= 1e-12


def test_score_row_uses_the_host_psnr_expression():
    g = np.random.default_rng(4)
    a = g.integers(0, 256, (12, 17, 3), dtype=np.uint8)
    b = g.integers(0, 256, (12, 17, 3), dtype=np.uint8)
    d = a.astype(np.int64) - b.astype(np.int64)
    r = util.score_row(np.array([(d * d).sum(), np.abs(d).sum(), 0.5, 0.25], dtype=np.float64), a.size)
    assert r["psnr"] == util.calculate_psnr(a, b)
    assert r["mae"] == np.mean(np.abs(a.astype(np.float64) - b.astype(np.float64)))
    assert (r["ssim"], r["ssim_sk"]) == (0.5, 0.25)
    assert util.score_row(np.zeros(4), a.size)["psnr"] == float("inf") == util.calculate_psnr(a, a)
    k = util._gauss_taps()
    assert np.array_equal(np.outer(k, k), util._gauss_window()) and k.shape == (11,)


def test_image_score_entry_points_validate_before_any_hip_call():
    lib = L.lib()
    G, U = L.SCORE_SSIM_G11, L.SCORE_SSIM_U7
    taps = (C.c_double * 11)(*util._gauss_taps())
    p = C.c_void_p(64)                                # never dereferenced: every call below fails its checks first
    need = lib.binhip_image_score_workspace_bytes(2, 20, 30, G | U)
    assert need > 0 and need % 64 == 0
    assert lib.binhip_image_score_workspace_bytes(2, 20, 30, 0) == need
    call = lambda a=p, b=p, n=2, h=20, w=30, flags=G | U, t=taps, ws=p, nb=need, out=p: \
        lib.binhip_image_score(a, b, n, h, w, flags, t, ws, nb, out, None)
    E_ARG, E_SHAPE, E_WS = -1, -2, -3
    assert call(a=None) == E_ARG and call(b=None) == E_ARG and call(ws=None) == E_ARG and call(out=None) == E_ARG
    assert call(t=None) == E_ARG
    assert call(flags=4) == E_ARG and call(flags=G | 8) == E_ARG
    assert call(h=10) == E_SHAPE and call(w=10) == E_SHAPE
    assert call(h=6, flags=U) == E_SHAPE and call(w=6, flags=U) == E_SHAPE
    assert call(n=0) == E_SHAPE and call(h=0, flags=0) == E_SHAPE and call(w=-1, flags=0) == E_SHAPE
    assert call(nb=need - 1) == E_WS and call(nb=0) == E_WS
    # the workspace query gives 0 for what the call would refuse
    for args in ((0, 20, 30, G), (2, 10, 30, G), (2, 20, 10, G), (2, 6, 30, U), (2, 20, 30, 4), (2, -1, 30, 0)):
        assert lib.binhip_image_score_workspace_bytes(*args) == 0, args
    assert lib.binhip_image_score_workspace_bytes(1, 7, 7, U) > 0
    assert lib.binhip_image_score_workspace_bytes(1, 1, 1, 0) > 0


def test_image_scores_has_no_cpu_path():
    import torch
    from bin_amd import ops
    a = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.image_scores(a, a)


def test_harness_metrics_option():
    from bin_amd import test as run_test
    base = ["--input_path", "x", "--output_path", "y", "--opt", "z"]
    assert run_test.parse_args(base).metrics == "host"
    assert run_test.parse_args(base + ["--metrics", "device"]).metrics == "device"
    with pytest.raises(SystemExit):
        run_test.parse_args(base + ["--metrics", "gpu"])
    assert run_test.METRICS[:7] == ("interp_psnr", "interp_ssim", "interp_err", "deblur_psnr", "deblur_ssim", "blurry_psnr",
                                    "blurry_ssim")
    assert run_test.METRICS[7:] == ("interp_ssim_sk", "deblur_ssim_sk", "blurry_ssim_sk")
    s = run_test._Sums()
    for tag, v in (("b", 0.1), ("a", 0.2), ("c", 0.7)):
        s.add("c0", "interp_psnr", v, tag)
    s.add("c1", "interp_psnr", 1.0, "a")
    assert s.total["interp_psnr"] == [((0.2 + 0.1) + 0.7) + 1.0, 4]
    assert s.clips["c0"]["interp_psnr"][1] == 3 and s.clips["c1"]["interp_ssim_sk"] == [0.0, 0]
