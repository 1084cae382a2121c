"""Cost of scoring on the device (binhip_image_score, `python -m bin_amd.test --metrics device`) against the host metrics.

Writes a synthetic clip and its GT tree (PNG) at each size, then prints one JSON line per measurement:
  * kernel: ops.image_scores time per image pair, all four fields, by hipEvents (median of --reps calls after a warm-up);
  * folder: the bin_amd.test rate (windows / wall s, IO included; each run into a fresh output folder after a warm-up run) for
    no GT, GT with host PSNR only (the default), GT with --metrics device and GT with host --ssim (on the first --ssim_frames
    frames only: seconds per frame).  Host and device runs alternate --repeat times on the same box.
usage: python tools/bench_metrics.py [--sizes 720x1280,352x640] [--frames 25] [--repeat 2] [--kernel_only]"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _write_tree(root, h, w, n_frames):
    import numpy as np
    from PIL import Image
    g = np.random.Generator(np.random.PCG64(5))
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    noise = g.normal(0, 2.0, (h, w, 3)).astype(np.float32)

    def frame(t):
        img = np.stack([127 + 100 * np.sin((xx + 9 * t) / 37.0 + c) * np.cos((yy - 5 * t) / 53.0 - c) for c in range(3)], -1)
        return (img + np.roll(noise, int(7 * t), axis=1)).clip(0, 255).astype(np.uint8)
    for sub in ("test_blur", "test"):
        os.makedirs(os.path.join(root, sub, "clip0"))
    for k in range(n_frames):
        Image.fromarray(frame(k)).save(os.path.join(root, "test_blur", "clip0", f"{8 * k:05d}.png"), compress_level=1)
    for idx in range(0, 8 * n_frames + 8, 4):                   # sharp frames at the +4 / +8 offsets the outputs are named by
        Image.fromarray(frame(idx / 8.0 + 0.1)).save(os.path.join(root, "test", "clip0", f"{idx:05d}.png"), compress_level=1)


def kernel_time(h, w, reps):
    import numpy as np
    import torch
    from bin_amd import ops
    g = np.random.default_rng(1)
    a = torch.from_numpy(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    b = torch.from_numpy(g.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    for _ in range(10):
        ops.image_scores(a, b)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.image_scores(a, b)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"what": "kernel", "size": f"{h}x{w}", "ms_per_pair_median": round(statistics.median(ms), 4),
            "ms_min": round(min(ms), 4), "reps": reps, "note": "ops.image_scores: tile + final launch and two int64->float64 copies, hipEvents"}


def folder_rate(root, tag, extra, frames_dir, yml):
    from bin_amd import test as run_test
    stats = {}
    out = os.path.join(root, "out_" + tag)
    rc = run_test.main(["--input_path", frames_dir, "--output_path", out, "--opt", yml, "--io_threads", "12"] + extra, stats=stats)
    shutil.rmtree(out, ignore_errors=True)
    assert rc == 0
    return stats["windows"] / stats["wall"], stats.get("metrics", {})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="720x1280,352x640")
    ap.add_argument("--frames", type=int, default=25)
    ap.add_argument("--ssim_frames", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--kernel_only", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_metrics needs a GPU"
    import bench
    sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
    for h, w in sizes:
        print(json.dumps(kernel_time(h, w, args.reps)), flush=True)
    if args.kernel_only:
        return
    for h, w in sizes:
        root = tempfile.mkdtemp(prefix="bin_amd_metrics_")
        try:
            _write_tree(root, h, w, args.frames)
            small = os.path.join(root, "ssim_subset")                         # the first frames only, for host --ssim
            os.makedirs(os.path.join(small, "clip0"))
            for f in sorted(os.listdir(os.path.join(root, "test_blur", "clip0")))[:args.ssim_frames]:
                shutil.copy(os.path.join(root, "test_blur", "clip0", f), os.path.join(small, "clip0", f))
            yml = os.path.join(root, "o.yml")
            with open(yml, "w") as f:
                f.write(bench.HARNESS_YML.format(tmp=root))
            blur, gt = os.path.join(root, "test_blur"), ["--gt_path", os.path.join(root, "test")]
            configs = {"no_gt": (blur, []), "gt_host_psnr": (blur, gt), "gt_device": (blur, gt + ["--metrics", "device"])}
            folder_rate(root, "warm", [], blur, yml)
            rates = {k: [] for k in configs}
            for _ in range(args.repeat):                                         # alternating on the same box
                for k, (d, extra) in configs.items():
                    r, m = folder_rate(root, k, extra, d, yml)
                    rates[k].append(r)
            r_ssim, _ = folder_rate(root, "gt_host_ssim", gt + ["--ssim"], small, yml)
            for k, v in rates.items():
                print(json.dumps({"what": "folder", "size": f"{h}x{w}", "config": k, "windows_per_s": [round(x, 3) for x in v],
                                  "median": round(statistics.median(v), 3), "frames": args.frames}), flush=True)
            print(json.dumps({"what": "folder", "size": f"{h}x{w}", "config": "gt_host_ssim", "windows_per_s": [round(r_ssim, 3)],
                              "median": round(r_ssim, 3), "frames": args.ssim_frames}), flush=True)
            ratio = statistics.median(rates["gt_device"]) / statistics.median(rates["gt_host_psnr"])
            print(json.dumps({"what": "ratio", "size": f"{h}x{w}", "device_over_host_psnr": round(ratio, 4)}), flush=True)
        finally:
            shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
