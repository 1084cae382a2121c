"""What --gt_video costs (bin_amd/score.py over binscore_planes), measured on one MI355X and written to profiles/video_score.md.
Needs no files on disk; prints one JSON line per measurement.

  * call      : one binscore_planes call at 1280x720 4:2:0 with both SSIMs (one full-size plane with SSIM, two quarter-size planes
    without) beside binhip_frame_score for one pair at 720x1280 (three full-size planes with SSIM), with the method of
    tools/bench_output_rate.py: BACK calls straight through the C ABI between one hipEvent pair after a warm-up, blocks alternating,
    median and spread, the host's time to issue one call beside it.  --parent_lib PATH: the frame score of another libbinhip.so (the
    parent commit's) in the same run.
  * end to end: the same synthetic 30 fps 720p clip (--frames) through `python -m bin_amd.test` at factor 2 as a Y4M file -> Y4M
    file, with --gt_video (a 60 fps stream of the same size) and without, every run a fresh child process, alternating, --runs
    each after one untimed warm-up pass of both.
  * resources : VGPRs / scratch / LDS of the tile walk in both libraries, from `hipcc -Rpass-analysis=kernel-resource-usage`.
No figure here is comparable across boxes.
usage: python tools/bench_video_score.py [--frames 21] [--runs 3] [--precision f16x3] [--samples 40] [--blocks 4] [--parent_lib PATH]
       [--md PATH]"""
import argparse
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import bench_common as B

H, W = 720, 1280
BACK = 25
FMT = (420, "bt709", "limited")
CHILD = ("import json, sys\nfrom bin_amd import test as T\ns = {}\nassert T.main(sys.argv[1:], stats=s) == 0\n"
         "print('STATS ' + json.dumps({k: s[k] for k in ('windows', 'wall', 'net_s_per_window', 'frames_out')}))\n")


def call(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    from bin_amd import ops
    from bin_amd.utils.util import _gauss_taps
    g = torch.Generator(device="cuda").manual_seed(3)
    nbytes, ch, cw = ops.yuv_frame_bytes(H, W, 420)
    pa = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    pb = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda", generator=g)
    fa, fb = (torch.rand((3, H, W), device="cuda", generator=g) for _ in range(2))
    taps = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    flags = L.PLANE_SSIM_G11 | L.PLANE_SSIM_U7
    score, binhip = L.scorelib(), L.lib()
    ptr = lambda x, off=0: C.c_void_p(x.data_ptr() + off)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    planes = lambda p: (ptr(p), ptr(p, H * W), ptr(p, H * W + ch * cw))
    nb_p, nb_f = score.binscore_workspace_bytes(H, W, 420, flags), binhip.binhip_frame_score_workspace_bytes(1, H, W, flags)
    ws_p, ws_f = (torch.empty(n, dtype=torch.uint8, device="cuda") for n in (nb_p, nb_f))
    rec_p, rec_f = torch.empty(64, dtype=torch.uint8, device="cuda"), torch.empty(4, dtype=torch.int64, device="cuda")
    px, py = (C.c_void_p * 1)(fa.data_ptr()), (C.c_void_p * 1)(fb.data_ptr())
    one = {"binscore_planes": lambda: score.binscore_planes(*planes(pa), *planes(pb), H, W, 420, flags, taps, ptr(ws_p), nb_p, ptr(rec_p), stream()),
           "binhip_frame_score": lambda: binhip.binhip_frame_score(px, py, 1, H, W, flags, taps, ptr(ws_f), nb_f, ptr(rec_f), stream())}
    if args.parent_lib:
        parent = C.CDLL(os.path.abspath(args.parent_lib))
        for name in ("binhip_frame_score", "binhip_frame_score_workspace_bytes"):
            getattr(parent, name).restype, getattr(parent, name).argtypes = L._SIGNATURES[name]
        assert parent.binhip_frame_score_workspace_bytes(1, H, W, flags) == nb_f
        rec_q = torch.empty(4, dtype=torch.int64, device="cuda")
        one["binhip_frame_score (parent)"] = lambda: parent.binhip_frame_score(px, py, 1, H, W, flags, taps, ptr(ws_f), nb_f, ptr(rec_q), stream())

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
    if args.parent_lib:
        assert torch.equal(rec_f, rec_q), "the parent's frame score, bit for bit"
    dev, host = B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))
    rows = []
    for name, ms in dev.items():
        us = sorted(v / BACK * 1e3 for v in ms)
        host_us = sorted(v / BACK * 1e3 for v in host[name])[len(us) // 2]
        rows.append({"what": "call", "name": name, "us_min": round(us[0], 2), "us_median": round(us[len(us) // 2], 2), "us_max": round(us[-1], 2),
                     "host_issue_us": round(host_us, 2), "samples": len(us), "calls_per_event_pair": BACK})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def end_to_end(args):
    import numpy as np
    import torch
    import bench
    from bin_amd import ops, video
    tmp = tempfile.mkdtemp(prefix="bin_amd_video_score_")
    try:
        g = np.random.Generator(np.random.PCG64(1))
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        noise = g.normal(0, 2.0, (H, W, 3)).astype(np.float32)
        header = video.Y4MHeader(W, H, (30, 1), "p", "1:1", "420mpeg2", ("COLORRANGE=LIMITED",))

        def frame(k):                                           # k in half input frames: the ground truth has twice the rate
            img = np.stack([127 + 100 * np.sin((xx + 4.5 * k) / 37.0 + c) * np.cos((yy - 2.5 * k) / 53.0 - c) for c in range(3)], -1)
            img = (img + np.roll(noise, 3 * k, axis=1)).clip(0, 255).astype(np.uint8)
            bgr = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
            return ops.frame_to_yuv(ops.u8_to_frame(bgr, (0, 0, 0, 0)), 0, 0, H, W, FMT).cpu().numpy()
        src, gt = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "gt.y4m")
        with video.Y4MWriter(src, header) as wr, video.Y4MWriter(gt, header.multiplied(2)) as wg:     # (untimed set-up)
            for k in range(2 * args.frames):
                payload = frame(k)
                wg.write(payload)
                if k % 2 == 0:
                    wr.write(payload)
        yml = os.path.join(tmp, "o.yml")
        with open(yml, "w") as f:
            f.write(bench.HARNESS_YML.format(tmp=tmp))
        common = ["--opt", yml, "--precision", args.precision, "--input_video", src]
        runs = {"with --gt_video": ["--gt_video", gt, "--score_log", os.path.join(tmp, "s.tsv")], "without": []}
        fps = {name: [] for name in runs}
        stats = {}
        for rep in range(args.runs + 1):                        # alternating; the first pass of each is the warm-up
            for name, extra in runs.items():
                dst = os.path.join(tmp, "out.y4m")
                r = subprocess.run([sys.executable, "-c", CHILD] + common + extra + ["--output_video", dst], cwd=tmp,
                                   env=dict(os.environ, PYTHONPATH=B.REPO), capture_output=True, text=True, timeout=args.leg_timeout)
                if r.returncode != 0:                           # nothing is started after a run that failed
                    raise RuntimeError(f"{name}: exit status {r.returncode}\n{r.stderr[-2000:]}")
                stats[name] = json.loads(next(ln for ln in r.stdout.splitlines() if ln.startswith("STATS "))[6:])
                if rep:
                    fps[name].append(stats[name]["frames_out"] / stats[name]["wall"])
                os.remove(dst)
        rows = []
        for name, v in fps.items():
            rows.append({"what": "end_to_end", "run": name, "frames_out": stats[name]["frames_out"], "runs": len(v),
                         "frames_out_per_s": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                         "spread": round(max(v) - min(v), 3)})
            print(json.dumps(rows[-1]), flush=True)
        return rows
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def resources():
    """VGPRs, scratch and LDS of every kernel of the two files that include the walk, as the compiler reports them."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    rows = []
    for lib, name in (("libbinhip.so", "binhip_metrics.hip"), ("libbinscore.so", "binscore.hip")):
        tmp = tempfile.mkdtemp(prefix="bin_amd_video_score_")
        try:
            r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
                                "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.REPO, "bin_amd", "csrc", name), "-o",
                                os.path.join(tmp, "x.o")], capture_output=True, text=True)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        cur = None
        for ln in r.stderr.splitlines():
            m = re.search(r"remark:\s+(Function Name|VGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\S+)", ln)
            if not m:
                continue
            if m.group(1) == "Function Name":
                sym = m.group(2)
                loader = re.search(r"\d+(U8Pairs|FramePairs|PlanePairs)E", sym)
                kernel = re.search(r"\d+(score_tile_kernel|image_score_final_kernel|plane_score_final_kernel)", sym)
                cur = {"what": "resources", "library": lib, "kernel": (kernel.group(1) if kernel else sym) + (f"<{loader.group(1)}>" if loader else "")}
                rows.append(cur)
            elif cur is not None:
                cur[m.group(1).split(" [")[0]] = int(m.group(2))
    for row in rows:
        print(json.dumps(row), flush=True)
    return rows


def _markdown(clock, calls, e2e, res, args):
    lines = ["# Scoring a video run: the per-plane score call and the --gt_video path", "",
             "Written by `tools/bench_video_score.py` on one MI355X: device events on warmed shapes, the sides of every comparison",
             "alternating.  Figures of one run; compare within the run only (boxes differ by several per cent).", "",
             f"Run: {clock['utc']} UTC, {clock['device']}.", "",
             "## One call at 1280x720", "",
             "`binscore_planes`: a 4:2:0 payload pair with both SSIMs: one full-size plane with SSIM, two quarter-size planes without (two",
             "tile launches and the final launch).  `binhip_frame_score`: one pair of fp32 frames, three full-size planes with SSIM (one",
             "tile launch and the final launch).  The same tile walk (`bin_amd/csrc/binhip_score_walk.h`).", "",
             "| call | device us per call (min .. median .. max) | host us to issue one |", "|---|---|---|"]
    for r in calls:
        lines.append(f"| {r['name']} | {r['us_min']} .. {r['us_median']} .. {r['us_max']} | {r['host_issue_us']} |")
    med = {r["name"]: r["us_median"] for r in calls}
    lines += ["", f"`binscore_planes` / `binhip_frame_score` = {med['binscore_planes'] / med['binhip_frame_score']:.3f} (medians of "
              f"{calls[0]['samples']} event pairs of {BACK} calls each)."]
    bound = [r["name"] for r in calls if r["host_issue_us"] >= 0.9 * r["us_median"]]
    if bound:
        lines += ["", "The host needs as long to issue a call of " + ", ".join(f"`{n}`" for n in bound) + " as its device figure says: "
                  "that figure is the issue rate, an upper bound of the kernels' time."]
    if e2e:
        by = {r["run"]: r for r in e2e}
        diff = by["with --gt_video"]["median"] - by["without"]["median"]
        lines += ["", f"## End to end, 720p, factor 2, the same {args.frames}-frame 30 fps clip, Y4M file to Y4M file", "",
                  f"Every run is a fresh process; one untimed pass of both, then {args.runs} runs each, alternating.  Output frames per second,",
                  "IO included.", "", "| run | frames written | output frames/s per run | median | max - min |", "|---|---|---|---|---|"]
        for r in e2e:
            lines.append(f"| {r['run']} | {r['frames_out']} | {', '.join(str(x) for x in r['frames_out_per_s'])} | {r['median']} | {r['spread']} |")
        lines += ["", f"With `--gt_video` minus without: {diff:+.3f} output frames/s (medians), next to a run-to-run spread of "
                  f"{max(r['spread'] for r in e2e):.3f}."]
    lines += ["", "## Registers and LDS of the tile walk", "",
              "`hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage` on `binhip_metrics.hip` and `binscore.hip`:", "",
              "| library | kernel | VGPRs | VGPR spills | scratch B/lane | LDS B/block | waves/SIMD |", "|---|---|---|---|---|---|---|"]
    for r in res:
        lines.append(f"| {r['library']} | {r['kernel']} | {r.get('VGPRs')} | {r.get('VGPRs Spill')} | {r.get('ScratchSize')} | {r.get('LDS Size')} | "
                     f"{r.get('Occupancy')} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=21)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--parent_lib", default=None, help="another libbinhip.so (the parent commit's): its frame score in the same run")
    ap.add_argument("--leg_timeout", type=int, default=240, help="seconds a child run may take")
    ap.add_argument("--no_end_to_end", action="store_true")
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "video_score.md"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_video_score needs a GPU"
    clock = {"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()), "device": torch.cuda.get_device_name(0)}
    print(json.dumps(clock), flush=True)
    res = resources()
    calls = call(args)
    e2e = [] if args.no_end_to_end else end_to_end(args)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(_markdown(clock, calls, e2e, res, args))
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
