"""What frame-rate factors above 2 cost (bin_amd/chain.py over binchain_reframe), measured in ONE process on one MI355X and written to
profiles/frame_rate_factor.md.  Needs no files on disk; prints one JSON line per measurement.

  * kernel   : binchain_reframe straight through the C ABI at the 1280x720 geometry (the 720x1280 crop of a 768x1344 output, padded
    back to 768x1344), 1 and 8 items per launch on the 16-byte path and 1 item on the 4-byte path (both pointers one float off),
    BACK calls between one hipEvent pair after a warm-up, blocks alternating, median and spread, the host's time to issue one call
    beside it; against its byte count (the crop read, the padded frame written) at the specification's 8.0 TB/s, and against a
    plain device copy of as many bytes in the same blocks.
  * video    : one synthetic 720p Y4M clip (--frames) file to file through `bin_amd.test` at --factor 2, 4 and 8, alternating, two
    passes each, the second reported: frames/s in and out with all IO, the windows of every pass and their rate over the run's
    wall time (the passes interleave, so a pass has no wall time of its own), the frames resident in the passes.
  * resources: registers / scratch / occupancy of the kernel, from `hipcc -Rpass-analysis=kernel-resource-usage`.
No figure here is comparable across boxes.
usage: python tools/bench_factor.py [--frames 13] [--precision f16x3] [--samples 40] [--blocks 4] [--md PATH]"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import bench_common as B

H, W = 720, 1280
BACK = 50
HBM_SPEC_TBPS = 8.0
FMT = (420, "bt709", "limited")
FACTORS = (2, 4, 8)


def kernel(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    from bin_amd.utils import util
    lib = L.chainlib()
    l, r, t, b = util.pad_sizes(H, W)
    hp, wp = H + t + b, W + l + r
    n = 3 * hp * wp
    g = torch.Generator(device="cuda").manual_seed(7)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    srcs = [torch.rand(n + 4, device="cuda", generator=g) * 1.5 - 0.25 for _ in range(8)]
    dsts = [torch.empty(n + 4, device="cuda") for _ in range(8)]
    nbytes = 4 * (3 * H * W + n)

    def table(count, off):
        tab = (L.BinChainItem * count)()
        for it, s, d in zip(tab, srcs, dsts):
            it.src, it.dst = s.data_ptr() + 4 * off, d.data_ptr() + 4 * off
        return tab

    def back_to_back(fn):
        def run():
            for _ in range(BACK):
                rc = fn()
            assert rc == 0
        return run

    def call(tab, count):
        return lambda: lib.binchain_reframe(tab, count, 3, hp, wp, t, l, H, W, l, r, t, b, stream())
    copy_src, copy_dst = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda"), torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")

    def copy():
        copy_dst.copy_(copy_src, non_blocking=True)
        return 0
    tabs = {"1 item, 16 B path": (table(1, 0), 1), "8 items, 16 B path": (table(8, 0), 8), "1 item, 4 B path": (table(1, 1), 1)}
    legs = {name: back_to_back(call(tab, count)) for name, (tab, count) in tabs.items()}
    legs["device copy of as many bytes (1 item)"] = back_to_back(copy)
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    dev, host = B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))
    rows = []
    for name, ms in dev.items():
        items = tabs[name][1] if name in tabs else 1
        us = sorted(v / BACK * 1e3 for v in ms)
        med = us[len(us) // 2]
        bound = items * nbytes / (HBM_SPEC_TBPS * 1e12) * 1e6
        rows.append({"what": "kernel", "name": name, "us_min": round(us[0], 2), "us_median": round(med, 2), "us_max": round(us[-1], 2),
                     "host_issue_us": round(sorted(v / BACK * 1e3 for v in host[name])[len(us) // 2], 2), "bytes": items * nbytes,
                     "tb_per_s": round(items * nbytes / (med * 1e-6) / 1e12, 3), "hbm_bound_us": round(bound, 2),
                     "share_of_hbm_bound": round(bound / med, 3), "samples": len(us), "calls_per_event_pair": BACK})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def video_runs(args):
    import numpy as np
    import torch
    import bench
    from bin_amd import ops, video
    from bin_amd import test as run_test
    tmp = tempfile.mkdtemp(prefix="bin_amd_factor_")
    try:
        g = np.random.Generator(np.random.PCG64(1))
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        noise = g.normal(0, 2.0, (H, W, 3)).astype(np.float32)
        header = video.Y4MHeader(W, H, (30, 1), "p", "1:1", "420mpeg2", ("COLORRANGE=LIMITED",))
        src = os.path.join(tmp, "in.y4m")
        with video.Y4MWriter(src, header) as wr:                # (untimed set-up: the clip of tools/bench_video_io.py)
            for k in range(args.frames):
                img = np.stack([127 + 100 * np.sin((xx + 9 * k) / 37.0 + c) * np.cos((yy - 5 * k) / 53.0 - c) for c in range(3)], -1)
                img = (img + np.roll(noise, 7 * k, axis=1)).clip(0, 255).astype(np.uint8)
                bgr = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
                wr.write(ops.frame_to_yuv(ops.u8_to_frame(bgr, (0, 0, 0, 0)), 0, 0, H, W, FMT).cpu().numpy())
        yml = os.path.join(tmp, "o.yml")
        with open(yml, "w") as f:
            f.write(bench.HARNESS_YML.format(tmp=tmp))
        rows = {}
        for rep in range(2):                                    # alternating; the second pass of each is the one reported
            for factor in FACTORS:
                stats = {}
                dst = os.path.join(tmp, f"out{factor}.y4m")
                run_test.main(["--opt", yml, "--precision", args.precision, "--input_video", src, "--output_video", dst,
                               "--factor", str(factor)], stats=stats)
                per_pass = stats.get("windows_per_pass", [stats["windows"]])
                rows[factor] = {"what": "video", "factor": factor, "frames_in": args.frames, "frames_out": stats["frames_out"],
                                "wall_s": round(stats["wall"], 3), "frames_in_per_s": round(args.frames / stats["wall"], 3),
                                "frames_out_per_s": round(stats["frames_out"] / stats["wall"], 3), "windows_per_pass": per_pass,
                                "windows_per_s_per_pass": [round(n / stats["wall"], 3) for n in per_pass],
                                "windows_per_s": round(sum(per_pass) / stats["wall"], 3),
                                "frames_resident_peak": stats.get("frames_resident_peak"), "pass": rep}
        for row in rows.values():
            print(json.dumps(row), flush=True)
        return [rows[f] for f in FACTORS]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def resources():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(B.REPO, "bin_amd", "csrc", "binchain.hip")
    tmp = tempfile.mkdtemp(prefix="bin_amd_factor_")
    try:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "binchain.o")],
                           capture_output=True, text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    row = {"what": "resources", "kernel": "chain_reframe_kernel"}
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs Spill|SGPRs Spill|"
                      r"Occupancy \[waves/SIMD\]): (\S+)", ln)
        if m:
            row[m.group(1).split(" [")[0]] = int(m.group(2))
    print(json.dumps(row), flush=True)
    return row


def _markdown(clock, kern, runs, res, args):
    lines = ["# Frame-rate factors 4 and 8: the chained passes and the hand-off kernel", "",
             "Written by `tools/bench_factor.py`: one process on one MI355X, device events on warmed shapes, the sides of every comparison",
             "alternating.  Figures of one run; compare within the run only (boxes differ by several per cent).", "",
             f"Run: {clock['utc']} UTC, {clock['device']}.", "",
             "## `binchain_reframe` at the 1280x720 geometry (crop of 768x1344, padded back to 768x1344)", "",
             f"Bytes per item: the crop read (3 x 720 x 1280 floats) and the padded frame written (3 x 768 x 1344 floats); the bound is that count at",
             f"the {HBM_SPEC_TBPS} TB/s of the specification.", "",
             "| call | device us per call (min .. median .. max) | host us to issue one | bytes | TB/s at the median | HBM bound us | bound / median |",
             "|---|---|---|---|---|---|---|"]
    for r in kern:
        lines.append(f"| {r['name']} | {r['us_min']} .. {r['us_median']} .. {r['us_max']} | {r['host_issue_us']} | {r['bytes']} | {r['tb_per_s']} | "
                     f"{r['hbm_bound_us']} | {r['share_of_hbm_bound']} |")
    bound = [r["name"] for r in kern if r["host_issue_us"] >= 0.9 * r["us_median"]]
    if bound:
        lines += ["", "The host needs as long to issue a call of " + ", ".join(f"`{n}`" for n in bound) + " as its device figure says: that "
                  "figure is the issue rate, an upper bound of the kernel's time."]
    lines += ["", f"## 720p Y4M file to file, {args.frames} frames, {args.precision}", "",
              "Expected from the definition: (F - 1)(T - 1) forwards instead of T - 1.  The passes interleave, so a pass's windows/s is its",
              "window count over the whole run's wall time.", "",
              "| factor | frames out | wall s | frames/s in | frames/s out | windows per pass | windows/s per pass | windows/s, all passes | frames resident in the passes |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in runs:
        lines.append(f"| {r['factor']} | {r['frames_out']} | {r['wall_s']} | {r['frames_in_per_s']} | {r['frames_out_per_s']} | {r['windows_per_pass']} | "
                     f"{r['windows_per_s_per_pass']} | {r['windows_per_s']} | {r['frames_resident_peak']} |")
    by = {r["factor"]: r for r in runs}
    lines += ["", "Against factor 2 of this run: " + "; ".join(
        f"factor {f}: wall x{by[f]['wall_s'] / by[2]['wall_s']:.2f} for x{sum(by[f]['windows_per_pass']) / sum(by[2]['windows_per_pass']):.2f} the forwards, "
        f"frames/s out x{by[f]['frames_out_per_s'] / by[2]['frames_out_per_s']:.2f}" for f in FACTORS if f != 2) + ".",
              "", "## Registers", "", "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `bin_amd/csrc/binchain.hip`:", "",
              "| kernel | SGPRs | VGPRs | AGPRs | VGPR spills | SGPR spills | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|---|---|",
              f"| {res['kernel']} | {res.get('TotalSGPRs')} | {res.get('VGPRs')} | {res.get('AGPRs')} | {res.get('VGPRs Spill')} | {res.get('SGPRs Spill')} | "
              f"{res.get('ScratchSize')} | {res.get('LDS Size')} | {res.get('Occupancy')} |"]
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=13)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "frame_rate_factor.md"))
    args = ap.parse_args()
    if args.frames < 5:
        ap.error("--frames: at least 5")
    import torch
    assert torch.cuda.is_available(), "bench_factor needs a GPU"
    clock = {"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(clock), flush=True)
    res = resources()
    kern = kernel(args)
    runs = video_runs(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(_markdown(clock, kern, runs, res, args))
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
