"""What the video path costs (bin_amd/video.py over binyuv_to_frame / binyuv_from_frame), measured in ONE process on one MI355X and
written to profiles/video_io.md.  Needs no files on disk; prints one JSON line per measurement.

  * kernels : ops.yuv_to_frame and ops.frame_to_yuv at 1280x720 4:2:0 with the pad_sizes pads (768x1344), against ops.u8_to_frame
    and ops.frame_to_u8 at the same size: BACK calls straight through the C ABI, back to back between one hipEvent pair after a
    warm-up, blocks alternating, median and spread, and the host's time to issue one call beside it.  Each also as a share of
    its HBM bound: 1.5 B read + 12 B written per padded pixel, and the reverse.
  * accuracy: the largest |yuv_to_frame - float64| over the case table of tests/video_cases.py, as a share of the 2^-20 bar.
  * end to end: the same synthetic clip (--frames, at least 41 = 40 windows) as a Y4M file -> Y4M file and as a PNG folder -> PNG
    folder through `bin_amd.test`, alternating, two passes each, the second reported: frames/s with all IO, and the host CPU
    seconds of the pass (time.process_time: every thread of the process).
  * resources: VGPRs / scratch / LDS of the kernels, from `hipcc -Rpass-analysis=kernel-resource-usage`.
The baselines are the PNG path and the u8 glue kernels in this same run; no figure here is comparable across boxes.
usage: python tools/bench_video_io.py [--frames 41] [--precision f16x3] [--samples 40] [--blocks 4] [--md PATH]"""
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

sys.path.insert(0, os.path.join(B.REPO, "tests"))

H, W = 720, 1280
BACK = 50
HBM_SPEC_TBPS = 8.0
FMT = (420, "bt709", "limited")


def kernels(args):
    """The four entry points called straight through the C ABI into preallocated tensors, BACK calls between one hipEvent pair, so
    that neither an allocation nor a wrapper sits between two launches; `host_us` is the time the host needs to issue one call (the
    same loop without the final wait): where it is below the device figure, the device figure is the kernel's."""
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    from bin_amd import ops
    from bin_amd.utils import util
    pads = util.pad_sizes(H, W)
    l, r, t, b = pads
    hp, wp = H + t + b, W + l + r
    g = torch.Generator(device="cuda").manual_seed(3)
    nbytes, ch, cw = ops.yuv_frame_bytes(H, W, 420)
    payload = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    img = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    frame = torch.rand((1, 3, hp, wp), device="cuda", generator=g) * 1.5 - 0.25
    out_frame, out_payload, out_img = torch.empty_like(frame), torch.empty_like(payload), torch.empty_like(img)
    fmt = ops.yuv_format(FMT)
    ptr = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    yuv, hip = L.yuvlib(), L.lib()
    one = {"yuv_to_frame": lambda: yuv.binyuv_to_frame(ptr(payload), ptr(payload, H * W), ptr(payload, H * W + ch * cw), H, W, C.byref(fmt),
                                                      l, r, t, b, ptr(out_frame), stream()),
           "u8_to_frame": lambda: hip.binhip_u8_to_frame(ptr(img), H, W, l, r, t, b, ptr(out_frame), stream()),
           "frame_to_yuv": lambda: yuv.binyuv_from_frame(ptr(frame), hp, wp, t, l, H, W, C.byref(fmt), ptr(out_payload),
                                                         ptr(out_payload, H * W), ptr(out_payload, H * W + ch * cw), stream()),
           "frame_to_u8": lambda: hip.binhip_frame_to_u8(ptr(frame), hp, wp, t, l, H, W, ptr(out_img), stream())}

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
    torch.cuda.synchronize()
    assert torch.equal(out_frame, ops.u8_to_frame(img, pads)) and torch.equal(out_payload, ops.frame_to_yuv(frame, t, l, H, W, FMT))
    dev, host = B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))
    bound_us = 13.5 * hp * wp / (HBM_SPEC_TBPS * 1e12) * 1e6
    rows = []
    for name, ms in dev.items():
        us = sorted(v / BACK * 1e3 for v in ms)
        med = us[len(us) // 2]
        host_us = sorted(v / BACK * 1e3 for v in host[name])[len(us) // 2]
        rows.append({"what": "kernel", "name": name, "us_min": round(us[0], 2), "us_median": round(med, 2), "us_max": round(us[-1], 2),
                     "host_issue_us": round(host_us, 2), "samples": len(us), "calls_per_event_pair": BACK, "hbm_bound_us": round(bound_us, 2),
                     "share_of_hbm_bound": round(bound_us / med, 3)})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def accuracy():
    import numpy as np
    import torch
    import video_cases as VC
    from bin_amd import ops
    worst = (0.0, None)
    for h, w, chroma in VC.CASES:
        for payload in (VC.random_payload(h, w, chroma, 100 * h + w), VC.ramp_payload(h, w, chroma, step=7, start=h)):
            dev = torch.from_numpy(payload).cuda()
            for pads in VC.pads_of(h, w):
                for matrix, rng in VC.MATRIX_RANGE:
                    fmt = (chroma, matrix, rng)
                    got = ops.yuv_to_frame(dev, h, w, fmt, pads).cpu().numpy()[0].astype(np.float64)
                    err = float(np.abs(got - VC.to_frame_ref(payload, h, w, fmt, pads)).max())
                    if err > worst[0]:
                        worst = (err, f"{h}x{w} {chroma} {matrix} {rng} pads {pads}")
    row = {"what": "accuracy", "max_abs_err": worst[0], "bar": VC.TO_FRAME_BAR, "err_over_bar": round(worst[0] / VC.TO_FRAME_BAR, 4),
           "at": worst[1], "cases": len(VC.CASES)}
    print(json.dumps(row), flush=True)
    return row


def end_to_end(args):
    import numpy as np
    import torch
    from PIL import Image
    import bench
    from bin_amd import ops, video
    from bin_amd import test as run_test
    tmp = tempfile.mkdtemp(prefix="bin_amd_video_io_")
    try:
        g = np.random.Generator(np.random.PCG64(1))
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        clip = os.path.join(tmp, "test_blur", "clip0")
        os.makedirs(clip)
        noise = g.normal(0, 2.0, (H, W, 3)).astype(np.float32)
        header = video.Y4MHeader(W, H, (30, 1), "p", "1:1", "420mpeg2", ("COLORRANGE=LIMITED",))
        src = os.path.join(tmp, "in.y4m")
        with video.Y4MWriter(src, header) as wr:                # the same pictures on both sides (untimed set-up)
            for k in range(args.frames):
                img = np.stack([127 + 100 * np.sin((xx + 9 * k) / 37.0 + c) * np.cos((yy - 5 * k) / 53.0 - c) for c in range(3)], -1)
                img = (img + np.roll(noise, 7 * k, axis=1)).clip(0, 255).astype(np.uint8)
                Image.fromarray(img).save(os.path.join(clip, f"{8 * k:05d}.png"), compress_level=1)
                bgr = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
                wr.write(ops.frame_to_yuv(ops.u8_to_frame(bgr, (0, 0, 0, 0)), 0, 0, H, W, FMT).cpu().numpy())
        yml = os.path.join(tmp, "o.yml")
        with open(yml, "w") as f:
            f.write(bench.HARNESS_YML.format(tmp=tmp))
        common = ["--opt", yml, "--precision", args.precision]
        runs = {"png_folder": lambda rep: ["--input_path", os.path.join(tmp, "test_blur"), "--output_path", os.path.join(tmp, f"out{rep}"),
                                           "--io_threads", str(args.io_threads)],
                "y4m_file": lambda rep: ["--input_video", src, "--output_video", os.path.join(tmp, f"out{rep}.y4m")]}
        rows = {}
        for rep in range(2):                                    # alternating; the second pass of each is the one reported
            for name, argv in runs.items():
                stats = {}
                cpu0, t0 = time.process_time(), time.perf_counter()
                run_test.main(common + argv(rep), stats=stats)
                rows[name] = {"what": "end_to_end", "path": name, "windows": stats["windows"], "wall_s": round(stats["wall"], 3),
                              "frames_per_s": round(stats["windows"] / stats["wall"], 3),
                              "host_cpu_s": round(time.process_time() - cpu0, 2), "elapsed_with_model_build_s": round(time.perf_counter() - t0, 2),
                              "net_and_glue_ms_per_window": round(stats["net_s_per_window"] * 1e3, 2), "pass": rep}
        out = video.Y4MReader(os.path.join(tmp, "out1.y4m"))
        rows["y4m_file"]["frames_written"] = sum(1 for _ in out)
        rows["y4m_file"]["bytes_in_per_frame"] = header.frame_bytes
        rows["png_folder"]["frames_written"] = sum(1 for _, _, fs in os.walk(os.path.join(tmp, "out1")) for x in fs if x.endswith(".png"))
        for row in rows.values():
            print(json.dumps(row), flush=True)
        return list(rows.values())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def resources():
    """VGPRs, scratch and LDS of every instantiation of the two kernels, as the compiler reports them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(B.REPO, "bin_amd", "csrc", "binyuv.hip")
    tmp = tempfile.mkdtemp(prefix="bin_amd_video_io_")
    try:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                            "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "binyuv.o")],
                           capture_output=True, text=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    rows, cur = [], None
    for ln in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\S+)", ln)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = m.group(2)
            inst = re.search(r"(yuv_\w+?_kernel)ILb(\d)ELb(\d)E", name)
            cur = {"what": "resources", "kernel": inst.group(1) if inst else name,
                   "path": ("16 B" if inst.group(2) == "1" else "byte") if inst else "", "chroma": (420 if inst.group(3) == "1" else 444) if inst else ""}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    for row in rows:
        print(json.dumps(row), flush=True)
    return rows


def _markdown(clock, kern, acc, e2e, res):
    lines = ["# Video IO: the YUV kernels and the Y4M path", "",
             "Written by `tools/bench_video_io.py`: one process on one MI355X, device events on warmed shapes, the two sides of every",
             "comparison alternating.  Figures of one run; compare within the run only (boxes differ by several per cent).", "",
             f"Run: {clock['utc']} UTC, {clock['device']}.", "",
             "## Kernels at 1280x720 4:2:0, pad_sizes pads (768x1344 padded)", "",
             "HBM bound: 1.5 B read + 12 B written per padded pixel for `yuv_to_frame`, the reverse for `frame_to_yuv`, at the 8.0 TB/s",
             "of the specification (the crop that `frame_to_yuv` reads is smaller than the padded frame, so its true traffic is below the",
             "bound's; the u8 kernels move 3 B where the YUV kernels move 1.5 B).", "",
             "| call | device us per call (min .. median .. max) | host us to issue one | HBM bound us | bound / median |", "|---|---|---|---|---|"]
    for r in kern:
        lines.append(f"| {r['name']} | {r['us_min']} .. {r['us_median']} .. {r['us_max']} | {r['host_issue_us']} | {r['hbm_bound_us']} | "
                     f"{r['share_of_hbm_bound']} |")
    med = {r["name"]: r["us_median"] for r in kern}
    bound = [r["name"] for r in kern if r["host_issue_us"] >= 0.9 * r["us_median"]]
    if bound:
        lines += ["", "The host needs as long to issue a call of " + ", ".join(f"`{n}`" for n in bound) + " as its device figure says: "
                  "that figure is the issue rate, an upper bound of the kernel's time (and its share of the bound a lower one)."]
    lines += ["", f"`yuv_to_frame` / `u8_to_frame` = {med['yuv_to_frame'] / med['u8_to_frame']:.3f}; "
              f"`frame_to_yuv` / `frame_to_u8` = {med['frame_to_yuv'] / med['frame_to_u8']:.3f} (medians of {kern[0]['samples']} event pairs of "
              f"{BACK} calls each).", "",
              "## Accuracy of `yuv_to_frame`", "",
              f"Largest |device - float64| over the case table of `tests/video_cases.py` ({acc['cases']} shapes x 4 pads x 4 formats, random bytes and "
              f"the ramp): {acc['max_abs_err']:.3e} = {acc['err_over_bar']} of the 2^-20 bar, at {acc['at']}.", "",
              "## End to end, 720p, the same clip", "",
              "| path | windows | wall s | frames/s (IO included) | host CPU s | net + glue ms / window | frames written |", "|---|---|---|---|---|---|---|"]
    for r in e2e:
        lines.append(f"| {r['path']} | {r['windows']} | {r['wall_s']} | {r['frames_per_s']} | {r['host_cpu_s']} | {r['net_and_glue_ms_per_window']} | "
                     f"{r['frames_written']} |")
    by = {r["path"]: r for r in e2e}
    if {"png_folder", "y4m_file"} <= set(by):
        lines += ["", f"Y4M / PNG: frames/s x{by['y4m_file']['frames_per_s'] / by['png_folder']['frames_per_s']:.3f}, host CPU seconds "
                  f"x{by['y4m_file']['host_cpu_s'] / max(by['png_folder']['host_cpu_s'], 1e-9):.3f} (second pass of two each, alternating; the CPU seconds "
                  "include building the model, which both paths do alike)."]
    lines += ["", "## Registers", "", "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `bin_amd/csrc/binyuv.hip`:", "",
              "| kernel | path | chroma | VGPRs | VGPR spills | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['kernel']} | {r['path']} | {r['chroma']} | {r.get('VGPRs')} | {r.get('VGPRs Spill')} | {r.get('ScratchSize')} | "
                     f"{r.get('LDS Size')} | {r.get('Occupancy')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--io_threads", type=int, default=12)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "video_io.md"))
    args = ap.parse_args()
    if args.frames < 41:
        ap.error("--frames: at least 41 (40 windows)")
    import torch
    assert torch.cuda.is_available(), "bench_video_io needs a GPU"
    clock = {"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(clock), flush=True)
    res = resources()
    kern = kernels(args)
    acc = accuracy()
    e2e = end_to_end(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(_markdown(clock, kern, acc, e2e, res))
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
