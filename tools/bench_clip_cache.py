"""Measure the fill of the device frame cache from a Y4M clip (dataset mode BIN_video) on one MI355X and write
profiles/clip_cache.md:

  * the arena fill from one 80-frame 640x352 4:2:0 clip (VideoFrameCache) against the fill DeviceFrameCache makes from the PNG tree
    of the same frames: wall time and host CPU seconds (all threads of the process), alternating, medians;
  * binclip_yuv_to_bgr per launch (hipEvents on the compute stream around blocks of launches) against its HBM bound, counted as
    payload bytes read plus arena bytes written;
  * the training step fed by each loader, which should be the same step;
  * the kernels' registers, from hipcc -Rpass-analysis=kernel-resource-usage.

    python tools/bench_clip_cache.py [--out profiles/clip_cache.md]"""
import argparse
import os
import random
import re
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import numpy as np  # noqa: E402

N_FRAMES, H, W = 80, 352, 640
FMT = (420, "bt601", "limited")
BLUR = [7, 11, 15]
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12          # bytes/s: the specification, and what a float4 copy reaches on this part


def write_inputs(root):
    """One clip of moving gradients plus noise (PNG-compressible, as footage is), and the PNG tree of its frames."""
    import torch
    from PIL import Image
    from bin_amd import ops, video
    g = np.random.Generator(np.random.PCG64(1))
    header = video.parse_header(b"YUV4MPEG2 W%d H%d F240:1 Ip A1:1 C420jpeg" % (W, H))
    yy, xx = np.mgrid[0:H, 0:W]
    os.makedirs(os.path.join(root, "clips"))
    payloads = np.empty((N_FRAMES, header.frame_bytes), np.uint8)
    with video.Y4MWriter(os.path.join(root, "clips", "clipA.y4m"), header) as wr:
        for k in range(N_FRAMES):
            luma = ((xx + 2 * yy + 3 * k) % 256 + g.integers(-6, 7, (H, W))).clip(0, 255).astype(np.uint8)
            chroma = [((xx[::2, ::2] * s + 5 * k) % 256).astype(np.uint8) for s in (1, 2)]
            payloads[k] = np.concatenate([luma.reshape(-1)] + [c.reshape(-1) for c in chroma])
            wr.write(payloads[k])
    frames = ops.yuv_to_bgr(torch.from_numpy(payloads).cuda(), H, W, FMT).cpu().numpy()
    os.makedirs(os.path.join(root, "tree", "train", "clipA"))
    for k in range(N_FRAMES):
        Image.fromarray(np.ascontiguousarray(frames[k][:, :, ::-1])).save(os.path.join(root, "tree", "train", "clipA", f"{k + 1:05d}.png"))
    return payloads, frames


def datasets(root, crop):
    from bin_amd.data import create_dataset
    common = {"name": "train", "LQ_size": list(crop), "phase": "train", "blur_window": BLUR, "batch_size": 3, "n_workers": 0, "device_cache": True}
    random.seed(0)
    clip = create_dataset(dict(common, mode="BIN_video", dataroot_video=os.path.join(root, "clips")))
    random.seed(0)
    tree = os.path.join(root, "tree")
    folder = create_dataset(dict(common, mode="BIN", dataroot_GT=tree, dataroot_LQ=tree, data_type="img"))
    return clip, folder


def fills(clip_ds, folder_ds, rounds):
    """{name: [(wall s, host CPU s)]}: each round builds both caches once, alternating; one untimed round first."""
    import torch
    from bin_amd.data.BIN_dataset import blur_half_max
    from bin_amd.data.device_cache import DeviceFrameCache
    build = {"Y4M clip": lambda: clip_ds.make_device_cache("cuda"),
             "PNG tree": lambda: DeviceFrameCache(folder_ds.all_paths, "cuda", blur_half=blur_half_max(folder_ds.blur_window))}
    out, arenas = {k: [] for k in build}, {}
    for r in range(rounds + 1):
        for name, fn in build.items():
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            cache = fn()
            torch.cuda.synchronize()
            if r:
                out[name].append((time.perf_counter() - w0, time.process_time() - c0))
            arenas[name] = cache.frames
    assert torch.equal(arenas["Y4M clip"], arenas["PNG tree"]), "the two fills give the same arena"
    return out, tuple(arenas["Y4M clip"].shape)


def kernel(payloads, copies, pairs=30, per=20):
    """Device us per launch of one ops.yuv_to_bgr over `copies` x 71 staged frames: median, min, max of `pairs` event pairs."""
    import torch
    from bin_amd import ops
    fb = payloads.shape[1]
    stride = -(-fb // 16) * 16
    host = np.zeros((71 * copies, stride), np.uint8)
    host[:, :fb] = np.tile(payloads[9:80], (copies, 1))
    src = torch.from_numpy(host).cuda()
    out = torch.empty((71 * copies, H, W, 3), dtype=torch.uint8, device="cuda")
    for _ in range(5):
        ops.yuv_to_bgr(src, H, W, FMT, out=out)
    us = []
    for _ in range(pairs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(per):
            ops.yuv_to_bgr(src, H, W, FMT, out=out)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / per)
    nbytes = 71 * copies * (fb + H * W * 3)
    return {"frames": 71 * copies, "bytes": nbytes, "us": (min(us), statistics.median(us), max(us))}


def steps(clip_ds, folder_ds, rounds, per):
    """Wall ms per training step (8 windows would not fit 3: batch 3 of 256 x 256 crops), fed by each loader in alternating blocks."""
    import bench_common as BC
    import torch
    from bin_amd.data import create_dataloader
    opt = {"dist": False, "gpu_ids": [0]}
    loaders = {"Y4M clip": create_dataloader(clip_ds, clip_ds.opt, opt, None), "PNG tree": create_dataloader(folder_ds, folder_ds.opt, opt, None)}
    model = BC.train_model()
    ms, count, same = {k: [] for k in loaders}, 0, []
    for r in range(rounds + 1):
        batches = {}
        for name, loader in loaders.items():
            random.seed(100 + r)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                batch = next(iter(loader))
                model.feed_data(batch)
                count += 1
                model.optimize_parameters(count)
            torch.cuda.synchronize()
            if r:
                ms[name].append((time.perf_counter() - t0) * 1e3 / per)
            batches[name] = batch
        same.append(all(torch.equal(batches["Y4M clip"][k], batches["PNG tree"][k]) for k in ("LQs", "GTenh", "GTinp")))
    return ms, all(same)


def resources():
    """[(kernel, VGPRs, VGPR spills, scratch, waves/SIMD)] of binclip.hip."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                              "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(REPO, "bin_amd", "csrc", "binclip.hip"),
                              "-o", os.path.join(tmp, "binclip.o")], capture_output=True, text=True, check=True)
    rows = []
    for block in run.stderr.split("Function Name: ")[1:]:
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        vec, c420 = re.match(r"_Z17yuv_to_bgr_kernelILb([01])ELb([01])E", block).groups()
        rows.append((f"yuv_to_bgr_kernel<{'dwords' if vec == '1' else 'bytes'}, {'4:2:0' if c420 == '1' else '4:4:4'}>",
                     num(" VGPRs"), num("VGPRs Spill"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]")))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "clip_cache.md"))
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_clip_cache needs a GPU"
    med = lambda v: statistics.median(v)
    with tempfile.TemporaryDirectory() as root:
        payloads, _ = write_inputs(root)
        clip_ds, folder_ds = datasets(root, (3, 256, 256))
        fill, shape = fills(clip_ds, folder_ds, args.rounds)
        kern = [kernel(payloads, c) for c in (1, 8)]
        step_ms, same = steps(clip_ds, folder_ds, 3, 4)
    regs = resources()
    L = ["# Filling the device frame cache from a Y4M clip", "",
         "Written by `tools/bench_clip_cache.py` on one MI355X.  Clocks are the driver's default power management, not pinned; every",
         "comparison alternates its sides in one process, after an untimed pass of both.  Figures of one run; compare within the run only.", "",
         f"Run: {time.strftime('%Y-%m-%d %H:%M:%S', time.gmtime())} UTC, {torch.cuda.get_device_name(0)}, {os.cpu_count()} host CPUs visible "
         f"(the PNG fill decodes on {min(16, os.cpu_count() or 1)} threads).", "",
         f"## The arena fill: one {N_FRAMES}-frame {W}x{H} 4:2:0 clip, `blur_window: {BLUR}`", "",
         f"Both fills give the same arena, uint8 {list(shape)} ({shape[0] * H * W * 3 / 1e6:.1f} MB), compared byte for byte in the run.  The clip is",
         "a moving gradient with noise; its PNGs are written at Pillow's default compression.  Wall time from the constructor call to a device",
         "synchronise; host CPU seconds are `time.process_time()`, all threads.", "",
         "| fill | wall ms per fill (min .. median .. max) | host CPU s per fill (median) |", "|---|---|---|"]
    for name, rows in fill.items():
        wall, cpu = [1e3 * r[0] for r in rows], [r[1] for r in rows]
        L.append(f"| {name} | {min(wall):.1f} .. {med(wall):.1f} .. {max(wall):.1f} | {med(cpu):.3f} |")
    a, b = med([r[0] for r in fill["Y4M clip"]]), med([r[0] for r in fill["PNG tree"]])
    ca, cb = med([r[1] for r in fill["Y4M clip"]]), med([r[1] for r in fill["PNG tree"]])
    L += ["", f"Y4M / PNG: wall {a / b:.3f}, host CPU {ca / cb:.3f} (medians of {args.rounds} fills each).", "",
          "## `binclip_yuv_to_bgr` per launch against its HBM bound", "",
          "Bytes = payload bytes read + arena bytes written (1.5 + 3 per pixel at 4:2:0), staging rows rounded up to 16 bytes (the dword",
          f"path).  The bound is bytes / {HBM_PEAK / 1e12:.1f} TB/s (specification); a float4 copy reaches {HBM_COPY / 1e12:.1f} TB/s on this part.  Device time from",
          "hipEvents on the compute stream around 20 back-to-back launches, 30 such pairs, after 5 warm-up launches.", "",
          "| frames per launch | MB moved | us per launch (min .. median .. max) | bound us | bound / median | TB/s |", "|---|---|---|---|---|---|"]
    for k in kern:
        lo, m, hi = k["us"]
        bound = k["bytes"] / HBM_PEAK * 1e6
        L.append(f"| {k['frames']} | {k['bytes'] / 1e6:.1f} | {lo:.2f} .. {m:.2f} .. {hi:.2f} | {bound:.2f} | {bound / m:.2f} | {k['bytes'] / m / 1e6:.2f} |")
    L += ["", "## The training step fed by each loader", "",
          "`bench.py`'s training model (f16x3, `train.optimizer: hip`), batch 3 of 256x256 crops (the clip has 3 windows); `next(iter(loader))`,",
          "`feed_data`, `optimize_parameters`; wall ms per step over blocks of 4 steps between synchronises, 3 blocks each, alternating.",
          f"Under the same `random` state the two loaders' batches were {'equal' if same else 'NOT equal'} bit for bit in every block.", "",
          "| loader | ms per step (min .. median .. max) |", "|---|---|"]
    for name, v in step_ms.items():
        L.append(f"| {name} | {min(v):.2f} .. {med(v):.2f} .. {max(v):.2f} |")
    L += ["", "## Registers", "", "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `binclip.hip`: no LDS, no scratch.", "",
          "| kernel | VGPRs | VGPR spills | scratch B/lane | waves/SIMD |", "|---|---|---|---|---|"]
    L += [f"| {n} | {v} | {s} | {sc} | {o} |" for n, v, s, sc, o in regs]
    if os.path.exists(args.out):                                 # the reading is written by hand below the figures: keep it
        old = open(args.out).read()
        if "\n## Reading\n" in old:
            L += ["", old[old.index("\n## Reading\n") + 1:].rstrip("\n")]
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
