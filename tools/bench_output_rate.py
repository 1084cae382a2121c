"""What --output_rate costs (bin_amd/rate.py over binrate_blend_to_yuv), measured on one MI355X and written to
profiles/output_rate.md.  Needs no files on disk; prints one JSON line per measurement.

  * kernel    : ops.blend_to_yuv beside ops.frame_to_yuv at 1280x720 4:2:0 inside the pad_sizes frame (768x1344), with the method
    of tools/bench_video_io.py: BACK calls straight through the C ABI between one hipEvent pair after a warm-up, blocks
    alternating, median and spread, the host's time to issue one call beside it.  Each also as a share of its HBM bound at the 8.0
    TB/s of the specification, counted on the crop: 2 x 12 B read + 1.5 B written per pixel for the mix (23.5 MB), 12 B + 1.5 B
    for frame_to_yuv.
  * end to end: the same synthetic 24 fps 720p clip (--frames, at least 41 = 40 windows) through `python -m bin_amd.test` as a Y4M
    file -> Y4M file, every run a fresh child process: --output_rate 60 (rho 5/2 on the factor-4 stream) and --factor 4 of this
    tree, and --factor 4 of another tree (--parent PATH: a built checkout of the parent commit) when given; alternating, two passes
    each, the second reported.  All three run the same forwards.
  * resources : VGPRs / scratch / LDS of the kernel, from `hipcc -Rpass-analysis=kernel-resource-usage`.
No figure here is comparable across boxes.
usage: python tools/bench_output_rate.py [--frames 41] [--precision f16x3] [--samples 40] [--blocks 4] [--parent PATH] [--md PATH]"""
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
WEIGHT = 0.4
CHILD = ("import json, sys\nfrom bin_amd import test as T\ns = {}\nassert T.main(sys.argv[1:], stats=s) == 0\n"
         "print('STATS ' + json.dumps({k: s[k] for k in ('windows', 'wall', 'net_s_per_window', 'frames_out', 'factor', 'windows_per_pass')}))\n")


def kernel(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    from bin_amd import ops
    from bin_amd.utils import util
    l, r, t, b = util.pad_sizes(H, W)
    hp, wp = H + t + b, W + l + r
    g = torch.Generator(device="cuda").manual_seed(3)
    nbytes, ch, cw = ops.yuv_frame_bytes(H, W, 420)
    fa = torch.rand((1, 3, hp, wp), device="cuda", generator=g) * 1.5 - 0.25
    fb = torch.rand((1, 3, hp, wp), device="cuda", generator=g) * 1.5 - 0.25
    out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fmt = ops.yuv_format(FMT)
    ptr = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    planes = lambda: (ptr(out), ptr(out, H * W), ptr(out, H * W + ch * cw))
    yuv, rate = L.yuvlib(), L.ratelib()
    one = {"blend_to_yuv": lambda: rate.binrate_blend_to_yuv(ptr(fa), ptr(fb), WEIGHT, hp, wp, t, l, H, W, C.byref(fmt), *planes(), stream()),
           "frame_to_yuv": lambda: yuv.binyuv_from_frame(ptr(fa), hp, wp, t, l, H, W, C.byref(fmt), *planes(), stream())}

    def back_to_back(fn):
        def run():
            for _ in range(BACK):
                rc = fn()
            assert rc == 0
        return run
    legs = {k: back_to_back(fn) for k, fn in one.items()}
    for fn in legs.values():
        fn()
        fn()
    one["blend_to_yuv"]()
    torch.cuda.synchronize()
    assert torch.equal(out, ops.blend_to_yuv(fa, fb, WEIGHT, t, l, H, W, FMT))
    dev, host = B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))
    bytes_per_pixel = {"blend_to_yuv": 25.5, "frame_to_yuv": 13.5}
    rows = []
    for name, ms in dev.items():
        us = sorted(v / BACK * 1e3 for v in ms)
        med = us[len(us) // 2]
        host_us = sorted(v / BACK * 1e3 for v in host[name])[len(us) // 2]
        bound_us = bytes_per_pixel[name] * H * W / (HBM_SPEC_TBPS * 1e12) * 1e6
        rows.append({"what": "kernel", "name": name, "us_min": round(us[0], 2), "us_median": round(med, 2), "us_max": round(us[-1], 2),
                     "host_issue_us": round(host_us, 2), "samples": len(us), "calls_per_event_pair": BACK,
                     "megabytes": round(bytes_per_pixel[name] * H * W / 1e6, 2), "hbm_bound_us": round(bound_us, 2),
                     "share_of_hbm_bound": round(bound_us / med, 3)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def end_to_end(args):
    import numpy as np
    import torch
    import bench
    from bin_amd import ops, video
    tmp = tempfile.mkdtemp(prefix="bin_amd_output_rate_")
    try:
        g = np.random.Generator(np.random.PCG64(1))
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        noise = g.normal(0, 2.0, (H, W, 3)).astype(np.float32)
        header = video.Y4MHeader(W, H, (24, 1), "p", "1:1", "420mpeg2", ("COLORRANGE=LIMITED",))
        src = os.path.join(tmp, "in.y4m")
        with video.Y4MWriter(src, header) as wr:                # (untimed set-up)
            for k in range(args.frames):
                img = np.stack([127 + 100 * np.sin((xx + 9 * k) / 37.0 + c) * np.cos((yy - 5 * k) / 53.0 - c) for c in range(3)], -1)
                img = (img + np.roll(noise, 7 * k, axis=1)).clip(0, 255).astype(np.uint8)
                bgr = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
                wr.write(ops.frame_to_yuv(ops.u8_to_frame(bgr, (0, 0, 0, 0)), 0, 0, H, W, FMT).cpu().numpy())
        yml = os.path.join(tmp, "o.yml")
        with open(yml, "w") as f:
            f.write(bench.HARNESS_YML.format(tmp=tmp))
        common = ["--opt", yml, "--precision", args.precision, "--input_video", src]
        runs = {"output_rate_60": (B.REPO, ["--output_rate", "60"]), "factor_4": (B.REPO, ["--factor", "4"])}
        if args.parent:
            runs["factor_4_parent"] = (os.path.abspath(args.parent), ["--factor", "4"])
        rows = {}
        for rep in range(2):                                    # alternating; the second pass of each is the one reported
            for name, (tree, extra) in runs.items():
                dst = os.path.join(tmp, f"{name}{rep}.y4m")
                env = dict(os.environ, PYTHONPATH=tree)
                r = subprocess.run([sys.executable, "-c", CHILD] + common + extra + ["--output_video", dst], cwd=tmp, env=env,
                                   capture_output=True, text=True, timeout=args.leg_timeout)
                if r.returncode != 0:                           # nothing is started after a run that failed
                    raise RuntimeError(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
                stats = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("STATS "))[6:])
                out_header = video.Y4MReader(dst).header
                rows[name] = {"what": "end_to_end", "run": name, "windows": stats["windows"], "forwards_per_pass": stats["windows_per_pass"],
                              "wall_s": round(stats["wall"], 3), "windows_per_s": round(stats["windows"] / stats["wall"], 3),
                              "frames_out": stats["frames_out"], "frames_out_per_s": round(stats["frames_out"] / stats["wall"], 2),
                              "net_and_glue_ms_per_window": round(stats["net_s_per_window"] * 1e3, 2),
                              "rate_out": "%d:%d" % out_header.rate, "pass": rep}
                os.remove(dst)
        for row in rows.values():
            print(json.dumps(row), flush=True)
        return list(rows.values())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def resources():
    """VGPRs, scratch and LDS of every instantiation of the kernel, as the compiler reports them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(B.REPO, "bin_amd", "csrc", "binrate.hip")
    tmp = tempfile.mkdtemp(prefix="bin_amd_output_rate_")
    try:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "binrate.o")],
                           capture_output=True, text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            inst = re.search(r"(blend_\w+?_kernel)ILb(\d)ELb(\d)E", m.group(2))
            cur = {"what": "resources", "kernel": inst.group(1) if inst else m.group(2),
                   "path": ("16 B" if inst.group(2) == "1" else "single float") if inst else "", "chroma": (420 if inst.group(3) == "1" else 444) if inst else ""}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    for row in rows:
        print(json.dumps(row), flush=True)
    return rows


def _markdown(clock, kern, e2e, res, args):
    lines = ["# Output at any frame rate: the mix kernel and the --output_rate path", "",
             "Written by `tools/bench_output_rate.py` on one MI355X: device events on warmed shapes, the two sides of every comparison",
             "alternating.  Figures of one run; compare within the run only (boxes differ by several per cent).", "",
             f"Run: {clock['utc']} UTC, {clock['device']}.", "",
             "## Kernels at 1280x720 4:2:0, the crop of a pad_sizes frame (768x1344 padded)", "",
             "HBM bound at the 8.0 TB/s of the specification, counted on the crop: `blend_to_yuv` reads two fp32 frames and writes 1.5 B",
             "per pixel (25.5 B), `frame_to_yuv` reads one (13.5 B).  Both calls come from the same run, alternating.", "",
             "| call | MB moved | device us per call (min .. median .. max) | host us to issue one | HBM bound us | bound / median |",
             "|---|---|---|---|---|---|"]
    for r in kern:
        lines.append(f"| {r['name']} | {r['megabytes']} | {r['us_min']} .. {r['us_median']} .. {r['us_max']} | {r['host_issue_us']} | {r['hbm_bound_us']} | "
                     f"{r['share_of_hbm_bound']} |")
    med = {r["name"]: r["us_median"] for r in kern}
    bound = [r["name"] for r in kern if r["host_issue_us"] >= 0.9 * r["us_median"]]
    if bound:
        lines += ["", "The host needs as long to issue a call of " + ", ".join(f"`{n}`" for n in bound) + " as its device figure says: "
                  "that figure is the issue rate, an upper bound of the kernel's time (and its share of the bound a lower one)."]
    lines += ["", f"`blend_to_yuv` / `frame_to_yuv` = {med['blend_to_yuv'] / med['frame_to_yuv']:.3f} (medians of {kern[0]['samples']} event pairs "
              f"of {BACK} calls each)."]
    if e2e:
        lines += ["", f"## End to end, 720p, the same {args.frames}-frame 24 fps clip, Y4M file to Y4M file", "",
                  "Every run is a fresh process; two passes each, alternating, the second reported.  All runs perform the same forwards.", "",
                  "| run | output rate | windows | forwards per pass | wall s | windows/s (IO included) | frames written | net + glue ms / window |",
                  "|---|---|---|---|---|---|---|---|"]
        for r in e2e:
            lines.append(f"| {r['run']} | {r['rate_out']} | {r['windows']} | {r['forwards_per_pass']} | {r['wall_s']} | {r['windows_per_s']} | "
                         f"{r['frames_out']} | {r['net_and_glue_ms_per_window']} |")
        by = {r["run"]: r for r in e2e}
        base = by.get("factor_4_parent") or by["factor_4"]
        lines += ["", f"`--output_rate 60` / `--factor 4`{' of the parent commit' if 'factor_4_parent' in by else ''}: windows/s "
                  f"x{by['output_rate_60']['windows_per_s'] / base['windows_per_s']:.3f}."]
        if "factor_4_parent" in by:
            lines[-1] += (f"  `--factor 4` of this tree / of the parent commit: x{by['factor_4']['windows_per_s'] / base['windows_per_s']:.3f}, "
                          "which is the run-to-run spread to read the first figure against.")
    lines += ["", "## Registers", "", "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `bin_amd/csrc/binrate.hip`:", "",
              "| kernel | path | chroma | VGPRs | VGPR spills | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['kernel']} | {r['path']} | {r['chroma']} | {r.get('VGPRs')} | {r.get('VGPRs Spill')} | {r.get('ScratchSize')} | "
                     f"{r.get('LDS Size')} | {r.get('Occupancy')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its --factor 4 runs beside this tree's")
    ap.add_argument("--leg_timeout", type=int, default=240, help="seconds a child run may take")
    ap.add_argument("--no_end_to_end", action="store_true")
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "output_rate.md"))
    args = ap.parse_args()
    if args.frames < 41:
        ap.error("--frames: at least 41 (40 windows)")
    import torch
    assert torch.cuda.is_available(), "bench_output_rate needs a GPU"
    clock = {"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(clock), flush=True)
    res = resources()
    kern = kernel(args)
    e2e = [] if args.no_end_to_end else end_to_end(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(_markdown(clock, kern, e2e, res, args))
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
