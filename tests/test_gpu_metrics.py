"""-m gpu: image scores on the device (binhip_image_score through ops.image_scores) against the host metrics — exact sums, so PSNR and
MAE to the bit; both SSIM definitions to 1e-9 — and bin_amd.test --metrics device against --metrics host --ssim on a tiny tree."""
import os
import threading

import numpy as np
import pytest
import torch

from bin_amd import ops
from bin_amd.utils import util

pytestmark = pytest.mark.gpu

SHAPES = [(7, 7), (11, 11), (12, 300), (73, 101), (352, 640), (720, 1280)]
KINDS = ("identical", "mild", "independent", "constant", "saturated")


def _pair(kind, h, w, seed):
    g = np.random.default_rng(seed)
    a = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "identical":
        return a, a.copy()
    if kind == "mild":
        return a, np.clip(a.astype(np.int16) + g.integers(-6, 7, a.shape), 0, 255).astype(np.uint8)
    if kind == "independent":
        return a, g.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "constant":                                            # sigma = 0 everywhere
        return np.full((h, w, 3), 37, np.uint8), np.full((h, w, 3), 219, np.uint8)
    a[: h // 2] = 255                                                 # saturated 0 / 255 regions against each other
    b = a.copy()
    b[: h // 2, : w // 2] = 0
    b[h // 2:, w // 3:] = 255
    return a, b


def _check_row(row, a, b, host_ssim=True):
    d = a.astype(np.int64) - b.astype(np.int64)
    assert row[0] == float((d * d).sum()) and row[1] == float(np.abs(d).sum())
    r = util.score_row(row, a.size)
    assert r["psnr"] == util.calculate_psnr(a, b)                                  # bit for bit (inf included)
    assert r["mae"] == np.mean(np.abs(a.astype(np.float64) - b.astype(np.float64)))
    if min(a.shape[:2]) < 11:
        assert np.isnan(row[2])
    elif host_ssim:
        assert abs(row[2] - util.calculate_ssim(a, b)) <= 1e-9
    if host_ssim:
        assert abs(row[3] - util.compare_ssim(a, b)) <= 1e-9


@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_scores_match_the_host_metrics(h, w):
    big = h * w >= 720 * 1280
    pairs = [_pair(k, h, w, 100 + i) for i, k in enumerate(KINDS)]
    rows = []
    for k, (a, b) in zip(KINDS, pairs):
        row = ops.image_scores(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()).cpu().numpy()
        assert row.shape == (1, 4) and row.dtype == np.float64
        # host calculate_ssim takes seconds per 720p pair: there it runs on two pairs, the sums on all five
        _check_row(row[0], a, b, host_ssim=not big or k in ("mild", "saturated"))
        rows.append(row[0])
    # n = 3 in one call: each row the bits of its n = 1 call
    sel = [1, 2, 4]
    A = torch.from_numpy(np.stack([pairs[i][0] for i in sel])).cuda()
    B = torch.from_numpy(np.stack([pairs[i][1] for i in sel])).cuda()
    got = ops.image_scores(A, B).cpu().numpy()
    assert got.shape == (3, 4)
    for j, i in enumerate(sel):
        assert np.array_equal(got[j], rows[i], equal_nan=True)
    assert np.array_equal(ops.image_scores(A, B, ssim=False).cpu().numpy()[:, :2], got[:, :2])
    assert np.isnan(ops.image_scores(A, B, ssim=False).cpu().numpy()[:, 2:]).all()
    if (h, w) == (11, 11) or (h, w) == (73, 101):
        assert rows[0][0] == 0 and rows[0][2] == 1.0 and rows[0][3] == 1.0                    # identical images


def test_scores_are_deterministic_and_stream_safe():
    h, w = 352, 640
    pairs = [_pair(k, h, w, 7 + i) for i, k in enumerate(("mild", "independent", "saturated", "mild"))]
    A = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    B = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    ref = ops.image_scores(A, B).cpu()
    for _ in range(3):
        assert torch.equal(ops.image_scores(A, B).cpu(), ref)
    results, errors = {}, []
    start = threading.Barrier(4)

    def work(i):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                a, b = A[i:i + 1].clone(), B[i:i + 1].clone()
                start.wait()
                outs = [ops.image_scores(a, b) for _ in range(8)]
                results[i] = [o.cpu() for o in outs]
        except Exception as e:                                            # surfaced below
            errors.append(e)
    threads = [threading.Thread(target=work, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(4):
        for o in results[i]:
            assert torch.equal(o[0], ref[i])


def test_scores_reject_cpu_tensors_and_bad_shapes():
    a = torch.zeros((16, 16, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError):
        ops.image_scores(a, a.cuda())
    with pytest.raises(RuntimeError):
        ops.image_scores(torch.zeros((6, 16, 3), dtype=torch.uint8).cuda(), torch.zeros((6, 16, 3), dtype=torch.uint8).cuda())
    with pytest.raises(ValueError):
        ops.image_scores(a.cuda(), a.cuda().float())
    with pytest.raises(ValueError):
        ops.image_scores(torch.zeros((16, 16, 4), dtype=torch.uint8).cuda(), torch.zeros((16, 16, 4), dtype=torch.uint8).cuda())


def test_folder_evaluation_device_metrics_match_host(tmp_path):
    from test_gpu_harness import _blur_tree, _yml
    from bin_amd import harness
    from bin_amd import test as run_test
    from bin_amd.data import util as du
    from bin_amd.weights import reference_state_dict
    clips = (("c0", 0, 4), ("c1", 40, 3))
    root = _blur_tree(str(tmp_path / "data"), clips=clips, hw=(40, 56))
    weights = str(tmp_path / "w.pth")
    torch.save(reference_state_dict(0), weights)
    runs = {}
    for mode, extra in (("device", ["--metrics", "device"]), ("host", ["--metrics", "host", "--ssim"])):
        out = str(tmp_path / mode)
        stats = {}
        assert run_test.main(["--input_path", os.path.join(root, "test_blur"), "--gt_path", os.path.join(root, "test"),
                              "--output_path", out, "--opt", _yml(tmp_path, weights), "--precision", "f16",
                              "--io_threads", "4"] + extra, stats=stats) == 0
        res = os.path.join(out, "60fps_test_results", "adobe_stage4")
        log = open(os.path.join(res, [f for f in os.listdir(res) if f.endswith(".log")][0])).read()
        runs[mode] = (res, stats["metrics"], log)
    (res_d, m_d, log_d), (res_h, m_h, log_h) = runs["device"], runs["host"]
    for clip, _, _ in clips:
        names = sorted(os.listdir(os.path.join(res_h, clip)))
        assert names == sorted(os.listdir(os.path.join(res_d, clip)))
        for f in names:
            assert np.array_equal(du.imread_u8(os.path.join(res_d, clip, f)), du.imread_u8(os.path.join(res_h, clip, f)))
    host_keys = {"interp_psnr", "interp_ssim", "interp_err", "deblur_psnr", "deblur_ssim", "blurry_psnr", "blurry_ssim"}
    sk = {"interp_ssim_sk", "deblur_ssim_sk", "blurry_ssim_sk"}
    assert set(m_h) == host_keys and set(m_d) == host_keys | sk
    for k in ("interp_psnr", "deblur_psnr", "blurry_psnr", "interp_err"):
        assert m_d[k] == m_h[k], k
    for k in ("interp_ssim", "deblur_ssim", "blurry_ssim"):
        assert abs(m_d[k] - m_h[k]) <= 1e-9, k
    assert "_sk" not in log_h and "interp_ssim_sk" in log_d and "Avg. testset" in log_d
    # the *_sk means recomputed on the host from the written frames, the blurry inputs and the GT
    vals = {k: [] for k in sk}
    for clip, first, n in clips:
        gt = lambda k: du.imread_u8(os.path.join(root, "test", clip, f"{k:05d}.png"))
        blur = lambda k: du.imread_u8(os.path.join(root, "test_blur", clip, f"{k:05d}.png"))
        out = lambda k: du.imread_u8(os.path.join(res_d, clip, f"{k:05d}.png"))
        for i in range(n - 1):
            num = first + 8 * i
            vals["interp_ssim_sk"].append(util.compare_ssim(out(num + 8), gt(num + 8)))
            vals["blurry_ssim_sk"].append(util.compare_ssim(blur(num + 8), gt(num + 8)))
            if i == 0:
                vals["deblur_ssim_sk"].append(util.compare_ssim(out(num + 4), gt(num + 4)))
            if i < n - 2:
                vals["deblur_ssim_sk"].append(util.compare_ssim(out(num + 12), gt(num + 12)))
    assert harness.window_frame_ids(0, 4)[3] == 1                        # the blurry input scored is the window's frame index + 1
    for k in sk:
        assert abs(m_d[k] - float(np.mean(vals[k]))) <= 1e-9, k
