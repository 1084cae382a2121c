"""Measure the device frame cache kept in YUV (`device_cache_format: yuv`, dataset mode BIN_video) against the BGR one on one MI355X and
write profiles/crop_cache.md:

  * the arena fill of one 160-frame 4:2:0 clip, YuvFrameCache (uploads only) against VideoFrameCache (upload + binclip_yuv_to_bgr):
    wall time and host CPU seconds, alternating, and the bytes each arena takes;
  * a batch of 8 x 256^2 crops, `blur_window` 11 and 33, from 640x352 and 1280x720 frames: the crop decode plus the gather on the YUV
    arena against the gather alone on the BGR arena, device time from event pairs, alternating; the decode kernel's achieved bytes
    per second next to its HBM bound by executed bytes;
  * the training step fed from each cache, interleaved in one process: BGR, YUV, BGR again, so that the difference between the two
    BGR-fed series measures the run-to-run spread the YUV-fed series is read against;
  * the kernels' registers, from hipcc -Rpass-analysis=kernel-resource-usage.

    python tools/bench_crop_cache.py [--out profiles/crop_cache.md]"""
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

N_FRAMES, BATCH, CROP = 160, 8, 256
SIZES = [(352, 640), (720, 1280)]                # (H, W): the recipe's size and the footage's own
WINDOWS = [11, 33]
HBM_PEAK, HBM_COPY = 8.0e12, 6.3e12          # bytes/s: the specification, and what a float4 copy reaches on this part


def write_clip(path, h, w):
    """A clip of moving gradients plus noise at 4:2:0."""
    from bin_amd import video
    g = np.random.Generator(np.random.PCG64(h))
    header = video.parse_header(b"YUV4MPEG2 W%d H%d F240:1 Ip A1:1 C420jpeg" % (w, h))
    yy, xx = np.mgrid[0:h, 0:w]
    noise = g.integers(-6, 7, (h, w))
    with video.Y4MWriter(path, header) as wr:
        for k in range(N_FRAMES):
            luma = ((xx + 2 * yy + 3 * k) % 256 + np.roll(noise, 7 * k, axis=1)).clip(0, 255).astype(np.uint8)
            chroma = [((xx[::2, ::2] * s + 5 * k) % 256).astype(np.uint8) for s in (1, 2)]
            wr.write(np.concatenate([luma.reshape(-1)] + [c.reshape(-1) for c in chroma]))


def dataset(folder, window, fmt):
    from bin_amd.data import create_dataset
    random.seed(0)
    return create_dataset({"name": "train", "mode": "BIN_video", "dataroot_video": folder, "LQ_size": [3, CROP, CROP], "phase": "train",
                           "blur_window": window, "batch_size": BATCH, "n_workers": 0, "device_cache": True, "device_cache_format": fmt})


def fills(folder, rounds):
    """{format: [(wall s, host CPU s)]}, {format: arena bytes}: each round builds both caches once, alternating; one untimed round first."""
    import torch
    sets = {fmt: dataset(folder, 33, fmt) for fmt in ("bgr", "yuv")}
    out, nbytes = {k: [] for k in sets}, {}
    for r in range(rounds + 1):
        for fmt, ds in sets.items():
            torch.cuda.synchronize()
            w0, c0 = time.perf_counter(), time.process_time()
            cache = ds.make_device_cache("cuda")
            torch.cuda.synchronize()
            if r:
                out[fmt].append((time.perf_counter() - w0, time.process_time() - c0))
            nbytes[fmt] = (cache.nbytes, len(cache.paths))
            del cache
    return out, nbytes


def decode_bytes(rows, crop, table_bytes):
    """Bytes one decode launch executes: the luma bytes of every crop, the chroma samples under it (4:2:0), the table, the BGR written."""
    ch, cw = crop
    y0, x0 = rows[:, 3], rows[:, 4]
    c_rows, c_cols = (y0 + ch - 1) // 2 - y0 // 2 + 1, (x0 + cw - 1) // 2 - x0 // 2 + 1
    return int(len(rows) * ch * cw + 2 * (c_rows * c_cols).sum() + table_bytes + len(rows) * ch * cw * 3)


def batches(folder, window, blocks=6, per=5):
    """Device ms per call of the batch assembly from each arena, alternating blocks; the two results compared bit for bit."""
    import bench_common as BC
    import torch
    from bin_amd import ops
    from bin_amd.data.BIN_dataset import draw_window_aug
    from bin_amd.data.device_cache import N_BLUR
    from bin_amd.data.video_dataset import plan_crop_batch
    sets = {fmt: dataset(folder, window, fmt) for fmt in ("bgr", "yuv")}
    bgr, yuv = (sets[fmt].make_device_cache("cuda") for fmt in ("bgr", "yuv"))
    ds = sets["yuv"]
    assert len(ds) >= BATCH, f"{len(ds)} windows"
    random.seed(1)
    windows = ds.all_paths[:BATCH]
    table = yuv.table(windows, [draw_window_aug((3, CROP, CROP), src_size=yuv.src_size(w)) for w in windows], [window // 2] * BATCH)
    crop = (CROP, CROP)
    rows, local, ranges = plan_crop_batch(table, yuv.frame_offset, yuv.frame_h, yuv.frame_w, yuv.frame_format, yuv.clip_ranges)
    calls = {"BGR arena: gather": lambda: ops.gather_windows_blur(bgr.frames, table, crop, N_BLUR, bgr.clip_ranges),
             "YUV arena: decode + gather": lambda: ops.gather_windows_blur(*yuv.crop_batch(table, crop)[:2], crop, N_BLUR, ranges),
             "YUV arena: decode alone": lambda: yuv.crop_batch(table, crop)}
    same = torch.equal(calls["BGR arena: gather"](), calls["YUV arena: decode + gather"]())
    for fn in calls.values():
        for _ in range(3):
            fn()
    dev, host = BC.alternating_blocks(calls, blocks, per)
    return {"dev": dev, "host": host, "same": same, "frames": len(rows), "bytes": decode_bytes(rows, crop, 32 * len(rows)),
            "arena": {"bgr": bgr.nbytes, "yuv": yuv.nbytes}}


def steps(folder, rounds, per):
    """Wall ms per training step fed by a BGR-fed loader, the YUV-fed loader and a second BGR-fed loader, in alternating blocks."""
    import bench_common as BC
    import torch
    from bin_amd.data import create_dataloader
    opt = {"dist": False, "gpu_ids": [0]}
    loaders = {}
    for name, fmt in (("BGR (first)", "bgr"), ("YUV", "yuv"), ("BGR (second)", "bgr")):
        ds = dataset(folder, 11, fmt)
        loaders[name] = create_dataloader(ds, ds.opt, opt, None)
    model = BC.train_model()
    ms, count, same = {k: [] for k in loaders}, 0, []
    for r in range(rounds + 1):
        last = {}
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
            last[name] = batch
        same.append(all(torch.equal(last["YUV"][k], last[n][k]) for k in ("LQs", "GTenh", "GTinp") for n in ("BGR (first)", "BGR (second)")))
    return ms, all(same)


def resources():
    """[(kernel, VGPRs, VGPR spills, scratch, waves/SIMD)] of bincrop.hip."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        run = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                              "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(REPO, "bin_amd", "csrc", "extra", "bincrop.hip"),
                              "-o", os.path.join(tmp, "bincrop.o")], capture_output=True, text=True, check=True)
    rows = []
    for block in run.stderr.split("Function Name: ")[1:]:
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        c420, vec = re.match(r"_Z23yuv_crops_to_bgr_kernelILb([01])ELb([01])E", block).groups()
        rows.append((f"yuv_crops_to_bgr_kernel<{'4:2:0' if c420 == '1' else '4:4:4'}, {'12-byte stores' if vec == '1' else 'byte stores'}>",
                     num(" VGPRs"), num("VGPRs Spill"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]")))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "crop_cache.md"))
    ap.add_argument("--rounds", type=int, default=4)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_crop_cache needs a GPU"
    med = statistics.median
    span = lambda v: f"{min(v):.3f} .. {med(v):.3f} .. {max(v):.3f}"
    fill, batch = {}, {}
    with tempfile.TemporaryDirectory() as root:
        for h, w in SIZES:
            folder = os.path.join(root, f"{w}x{h}")
            os.makedirs(folder)
            write_clip(os.path.join(folder, "clipA.y4m"), h, w)
            fill[(h, w)] = fills(folder, args.rounds)
            for window in WINDOWS:
                batch[(h, w, window)] = batches(folder, window)
        step_ms, same = steps(os.path.join(root, f"{SIZES[0][1]}x{SIZES[0][0]}"), args.rounds, 6)
    regs = resources()
    L = ["# The device frame cache kept in YUV: fill, per-batch decode, training step", "",
         "Written by `tools/bench_crop_cache.py` on one MI355X.  Clocks are the driver's default power management, not pinned; every",
         "comparison alternates its sides in one process, after an untimed pass of each.  Figures of one run; compare within the run only.", "",
         f"Run: {time.strftime('%Y-%m-%d %H:%M:%S', time.gmtime())} UTC, {torch.cuda.get_device_name(0)}.", "",
         f"## The arena fill: one {N_FRAMES}-frame 4:2:0 clip, `blur_window: 33`", "",
         "Wall time from the constructor call to a device synchronise; host CPU seconds are `time.process_time()`, all threads.  The BGR",
         "fill uploads each chunk and converts it with one `binclip_yuv_to_bgr` launch; the YUV fill uploads it into the arena and launches",
         "nothing.", "",
         "| frames | arena | frames cached | arena MB | wall ms per fill (min .. median .. max) | host CPU s per fill (median) |", "|---|---|---|---|---|---|"]
    for (h, w), (rows, nbytes) in fill.items():
        for fmt in ("bgr", "yuv"):
            wall, cpu = [1e3 * r[0] for r in rows[fmt]], [r[1] for r in rows[fmt]]
            L.append(f"| {w}x{h} | {fmt} | {nbytes[fmt][1]} | {nbytes[fmt][0] / 1e6:.1f} | {span(wall)} | {med(cpu):.3f} |")
    L += ["", f"## A batch of {BATCH} x {CROP}x{CROP} crops", "",
          "`gather_windows_blur` on the BGR arena against `yuv_crops_to_bgr` (one launch over every frame of the batch's spans) followed by the",
          "same gather on the decoded crops.  Device ms per call from an event pair around each call with the stream idle before it, 6",
          "alternating blocks of 5 calls; host ms is the time the call takes to return (table planning, checks, the pinned upload).", "",
          "| frames | window | arena | device ms (min .. median .. max) | host ms (median) | same bits |", "|---|---|---|---|---|---|"]
    for (h, w, window), b in batch.items():
        for name in b["dev"]:
            L.append(f"| {w}x{h} | {window} | {name} | {span(b['dev'][name])} | {med(b['host'][name]):.3f} | {'yes' if b['same'] else 'NO'} |")
    L += ["", "### The decode kernel against its HBM bound", "",
          "Executed bytes = the luma bytes of every crop + the chroma samples under it + the 32-byte table rows + the BGR bytes written.  The",
          f"bound is bytes / {HBM_PEAK / 1e12:.1f} TB/s (specification); a float4 copy reaches {HBM_COPY / 1e12:.1f} TB/s on this part.  The time is the device time of",
          "`crop_batch` alone, which also holds the table's upload.", "",
          "| frames | window | frames decoded | MB executed | median us | bound us | bound / median | TB/s |", "|---|---|---|---|---|---|---|---|"]
    for (h, w, window), b in batch.items():
        m = med(b["dev"]["YUV arena: decode alone"]) * 1e3
        bound = b["bytes"] / HBM_PEAK * 1e6
        L.append(f"| {w}x{h} | {window} | {b['frames']} | {b['bytes'] / 1e6:.1f} | {m:.1f} | {bound:.1f} | {bound / m:.2f} | {b['bytes'] / m / 1e6:.2f} |")
    a1, y, a2 = (med(step_ms[k]) for k in ("BGR (first)", "YUV", "BGR (second)"))
    spread, diff = abs(a1 - a2), y - (a1 + a2) / 2
    L += ["", "## The training step fed from each cache", "",
          f"`bench.py`'s training model (f16x3, `train.optimizer: hip`), batch {BATCH} of {CROP}x{CROP} crops from the {SIZES[0][1]}x{SIZES[0][0]} clip,",
          "`blur_window: 11`; `next(iter(loader))`, `feed_data`, `optimize_parameters`; wall ms per step over blocks of 6 steps between",
          f"synchronises, {args.rounds} blocks each after an untimed one, in the order BGR, YUV, BGR.  Under the same `random` state the three loaders'",
          f"batches were {'equal' if same else 'NOT equal'} bit for bit in every block.", "",
          "| loader | ms per step (min .. median .. max) |", "|---|---|"]
    L += [f"| {name} | {span(v)} |" for name, v in step_ms.items()]
    L += ["", f"Run-to-run spread (the two BGR-fed medians against each other): {spread:.3f} ms.  YUV-fed median minus the mean of the two",
          f"BGR-fed medians: {diff:+.3f} ms ({100 * diff / ((a1 + a2) / 2):+.2f} %): "
          f"{'within that spread' if abs(diff) <= spread else 'slower than that spread allows' if diff > 0 else 'faster than that spread explains'}.", "",
          "## Registers", "", "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `bincrop.hip`: no LDS, no scratch.", "",
          "| kernel | VGPRs | VGPR spills | scratch B/lane | waves/SIMD |", "|---|---|---|---|---|"]
    L += [f"| {n} | {v} | {s} | {sc} | {o} |" for n, v, s, sc, o in regs]
    if os.path.exists(args.out):                                 # the reading is written by hand below the figures: keep it
        old = open(args.out).read()
        if "\n## Reading\n" in old:
            L += ["", old[old.index("\n## Reading\n") + 1:].rstrip("\n")]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(L) + "\n")
    print("\n".join(L))


if __name__ == "__main__":
    main()
