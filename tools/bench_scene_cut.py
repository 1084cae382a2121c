"""What scene-cut detection costs and where its threshold sits (bin_amd/scene.py over binscene_luma_stats), measured on one MI355X and
written to profiles/scene_cut.md.  Needs no files on disk; prints one JSON line per measurement.

  * kernels  : binscene_luma_stats straight through the C ABI at 1280x720 and 3840x2160 luma on random content, an all-black and an
    all-255 plane (both planes of the pair alike), BACK calls between one hipEvent pair after a warm-up, blocks alternating, median
    and spread; beside it, in the same blocks, a plain device copy of the same 2 H W bytes (torch's copy_ between two device tensors) and an
    empty launch (a 1x1 plane without a previous one: the clearing of the record and a kernel that touches one byte).  The entry
    point's own clearing of the record is part of every figure.
  * distances: `distance` over the non-cut and the cut pairs of streams made by concatenating clips of bin_amd/data/synthetic.py
    rendered under different seeds (the six blurry frames of a sample are six consecutive frames of one scene), the luma taken from
    ops.frame_to_yuv as a video would carry it.  Rendered data, not footage.
  * video    : the 720p Y4M run of tools/bench_video_io.py, file to file through `bin_amd.test`, with the option off and on, in one
    process, alternating, two passes each, the second reported.  `--tree PATH` imports bin_amd from another checkout (the parent
    commit, built) and runs the option-off pass there: the third column.
usage: python tools/bench_scene_cut.py --leg kernels|distances|video|video_parent [--tree PATH] [--frames 41] [--md PATH]
       python tools/bench_scene_cut.py --md PATH --from-json FILE ...    (assemble the markdown from the JSON lines of the legs)"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import bench_common as B

SHAPES = ((720, 1280), (2160, 3840))
BACK = 50
H, W = 720, 1280
FMT = (420, "bt709", "limited")
CLIP_SCENES = 5                      # cuts in the video run's stream: frames // CLIP_SCENES frames per scene


def kernels(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    lib = L.scenelib()
    g = torch.Generator(device="cuda").manual_seed(5)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = torch.empty(264, dtype=torch.uint8, device="cuda")
    legs, keep = {}, []

    def back_to_back(fn):
        def run():
            for _ in range(BACK):
                rc = fn()
            assert rc == 0
        return run

    def copy(src, dst):
        dst.copy_(src, non_blocking=True)
        return 0
    one = torch.zeros(16, dtype=torch.uint8, device="cuda")
    legs["empty launch"] = back_to_back(lambda: lib.binscene_luma_stats(one.data_ptr(), None, 1, 1, rec.data_ptr(), stream()))
    for h, w in SHAPES:
        n = h * w
        planes = {"random": (torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g),
                             torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)),
                  "black": (torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.zeros(n, dtype=torch.uint8, device="cuda")),
                  "all 255": (torch.full((n,), 255, dtype=torch.uint8, device="cuda"), torch.full((n,), 255, dtype=torch.uint8, device="cuda"))}
        src, dst = torch.empty(2 * n, dtype=torch.uint8, device="cuda"), torch.empty(2 * n, dtype=torch.uint8, device="cuda")
        keep += [planes, src, dst]
        for kind, (cur, prev) in planes.items():
            legs[f"{w}x{h} {kind}"] = back_to_back(lambda cur=cur, prev=prev, h=h, w=w: lib.binscene_luma_stats(
                cur.data_ptr(), prev.data_ptr(), h, w, rec.data_ptr(), stream()))
        legs[f"{w}x{h} device copy of 2HW bytes"] = back_to_back(lambda src=src, dst=dst: copy(src, dst))
    for fn in legs.values():
        fn()
        fn()
    torch.cuda.synchronize()
    dev, host = B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))
    rows = []
    for name, ms in dev.items():
        us = sorted(v / BACK * 1e3 for v in ms)
        host_us = sorted(v / BACK * 1e3 for v in host[name])[len(us) // 2]
        rows.append({"what": "kernel", "name": name, "us_min": round(us[0], 2), "us_median": round(us[len(us) // 2], 2), "us_max": round(us[-1], 2),
                     "host_issue_us": round(host_us, 2), "samples": len(us), "calls_per_event_pair": BACK})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def distances(args):
    import numpy as np
    import torch
    from bin_amd import harness, ops, scene, video
    from bin_amd.data.synthetic import moving_texture_clip
    size = args.size
    header = video.Y4MHeader(size, size, (30, 1), "p", "1:1", "420mpeg2", ("COLORRANGE=LIMITED",))
    inside, across = [], []
    for stream_id in range(args.streams):
        payloads, cuts = [], []
        for k in range(args.scenes):
            lq = moving_texture_clip(1000 + stream_id, k, size)[0]                  # six consecutive blurry frames of one scene
            if k:
                cuts.append(len(payloads))
            for f in lq:
                payloads.append(ops.frame_to_yuv(f[None].cuda(), 0, 0, size, size, FMT))
        recs = harness.luma_records(torch.stack(payloads), header)
        for i in range(1, len(recs)):
            (across if i in cuts else inside).append(scene.distance(recs[i - 1][1], recs[i][1], size, size))
    q = lambda v, p: float(np.quantile(np.array(v), p))
    row = {"what": "distances", "size": size, "streams": args.streams, "scenes_per_stream": args.scenes}
    for name, v in (("inside", inside), ("across", across)):
        row[name] = {"pairs": len(v), "min": round(min(v), 4), "q10": round(q(v, 0.1), 4), "median": round(q(v, 0.5), 4),
                     "q90": round(q(v, 0.9), 4), "q99": round(q(v, 0.99), 4), "max": round(max(v), 4)}
    row["across_below_largest_inside"] = sum(1 for d in across if d <= max(inside))
    print(json.dumps(row), flush=True)
    return row


def _stream(path, frames, scenes):
    """The 720p pictures of tools/bench_video_io.py, cut into `scenes` scenes: the pattern's phase and brightness jump at every cut."""
    import numpy as np
    import torch
    from bin_amd import ops, video
    g = np.random.Generator(np.random.PCG64(1))
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    noise = g.normal(0, 2.0, (H, W, 3)).astype(np.float32)
    header = video.Y4MHeader(W, H, (30, 1), "p", "1:1", "420mpeg2", ("COLORRANGE=LIMITED",))
    per = -(-frames // scenes)
    with video.Y4MWriter(path, header) as wr:
        for k in range(frames):
            s = k // per
            base = (127, 60, 180, 90, 150)[s % 5]
            img = np.stack([base + 60 * np.sin((xx + 9 * k) / (37.0 + 11 * s) + c + s) * np.cos((yy - 5 * k) / (53.0 - 7 * s) - c) for c in range(3)], -1)
            img = (img + np.roll(noise, 7 * k, axis=1)).clip(0, 255).astype(np.uint8)
            bgr = torch.from_numpy(np.ascontiguousarray(img[:, :, ::-1])).cuda()
            wr.write(ops.frame_to_yuv(ops.u8_to_frame(bgr, (0, 0, 0, 0)), 0, 0, H, W, FMT).cpu().numpy())
    return [per * s for s in range(1, scenes) if per * s < frames]


def video_run(args, parent=False):
    import bench
    from bin_amd import test as run_test
    tmp = tempfile.mkdtemp(prefix="bin_amd_scene_cut_")
    try:
        src = os.path.join(tmp, "in.y4m")
        cuts = _stream(src, args.frames, CLIP_SCENES)
        yml = os.path.join(tmp, "o.yml")
        with open(yml, "w") as f:
            f.write(bench.HARNESS_YML.format(tmp=tmp))
        common = ["--opt", yml, "--precision", args.precision, "--input_video", src]
        runs = {"option off": []} if parent else {"option off": [], "option on": ["--scene_cut", str(args.threshold)]}
        rows = {}
        for rep in range(2):                                    # alternating; the second pass of each is the one reported
            for name, extra in runs.items():
                stats = {}
                cpu0 = time.process_time()
                run_test.main(common + ["--output_video", os.path.join(tmp, f"out{rep}{len(extra)}.y4m")] + extra, stats=stats)
                rows[name] = {"what": "video", "tree": "parent" if parent else "this", "run": name, "windows": stats["windows"],
                              "wall_s": round(stats["wall"], 3), "frames_per_s": round(stats["windows"] / stats["wall"], 3),
                              "ms_per_input_frame": round(stats["wall"] / (stats["windows"] + 1) * 1e3, 3),
                              "host_cpu_s": round(time.process_time() - cpu0, 2),
                              "net_and_glue_ms_per_window": round(stats["net_s_per_window"] * 1e3, 2), "frames_out": stats["frames_out"],
                              "cuts_found": stats.get("cuts"), "cuts_made": cuts, "pass": rep}
        for row in rows.values():
            print(json.dumps(row), flush=True)
        return list(rows.values())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def _markdown(rows):
    clock = next(r for r in rows if r["what"] == "clock")
    kern = [r for r in rows if r["what"] == "kernel"]
    dist = next((r for r in rows if r["what"] == "distances"), None)
    vid = [r for r in rows if r["what"] == "video"]
    lines = ["# Scene cuts: the luma statistics kernel, the video run and the threshold", "",
             "Written by `tools/bench_scene_cut.py` on one MI355X: device events on warmed shapes, the sides of every comparison alternating.",
             "Figures of one run; compare within the run only.", "", f"Run: {clock['utc']} UTC, {clock['device']}.", ""]
    if kern:
        lines += ["## `binscene_luma_stats`: histogram and SAD of one frame pair", "",
                  f"{BACK} calls between one event pair; every call clears the record (a 264-byte memset node) and launches the kernel.  The",
                  "copy is `Tensor.copy_` between two device tensors of the 2 H W bytes the kernel reads; the empty launch is the entry point on a",
                  "1x1 plane.", "",
                  "| call | device us per call (min .. median .. max) | host us to issue one |", "|---|---|---|"]
        for r in kern:
            lines.append(f"| {r['name']} | {r['us_min']} .. {r['us_median']} .. {r['us_max']} | {r['host_issue_us']} |")
        med = {r["name"]: r["us_median"] for r in kern}
        issue = {r["name"]: r["host_issue_us"] for r in kern}
        empty = med["empty launch"]
        lines += ["", f"The entry point is two queue entries, the clearing of the record and the kernel, and the host needs {issue['empty launch']} us to issue "
                  f"them: the empty call's {empty} us per call is that issue rate, not a kernel's time, and so is every figure at or below it.  "
                  "Above the empty call:", ""]
        for h, w in SHAPES:
            kinds = {k: med[f"{w}x{h} {k}"] for k in ("random", "black", "all 255")}
            lines.append(f"* {w}x{h} ({2 * h * w / 1e6:.1f} MB read): random +{kinds['random'] - empty:.2f} us, black +{kinds['black'] - empty:.2f} us, all 255 "
                         f"+{kinds['all 255'] - empty:.2f} us; the copy of the same bytes {med[f'{w}x{h} device copy of 2HW bytes']} us per call "
                         f"(host issue {issue[f'{w}x{h} device copy of 2HW bytes']} us: one queue entry).")
        lines += ["", "A flat plane is the cheapest content, not the dearest: a lane adds the run of equal bins it has counted in a register, so a",
                  "flat plane costs one LDS add per lane, and random content (a new bin at almost every pixel) is the worst case of the run",
                  "counting.  At 0.9 MB the call sits at the issue rate of its two queue entries; the kernel's own time shows at 3840x2160.", ""]
    if vid:
        lines += ["## The 720p Y4M run, file to file", "",
                  "| tree | run | windows | wall s | frames/s (IO included) | ms per input frame | host CPU s | net + glue ms / window | cuts found |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in vid:
            lines.append(f"| {r['tree']} | {r['run']} | {r['windows']} | {r['wall_s']} | {r['frames_per_s']} | {r['ms_per_input_frame']} | {r['host_cpu_s']} | "
                         f"{r['net_and_glue_ms_per_window']} | {r['cuts_found']} |")
        by = {(r["tree"], r["run"]): r for r in vid}
        off, on, parent = by.get(("this", "option off")), by.get(("this", "option on")), by.get(("parent", "option off"))
        lines.append("")
        if off and parent:
            lines.append(f"Option off against the parent commit (a process of its own on the same box, the same stream): wall x{off['wall_s'] / parent['wall_s']:.3f}.")
        if off and on:
            lines += [f"Option on against off (one process, alternating): wall x{on['wall_s'] / off['wall_s']:.3f}, "
                      f"{on['ms_per_input_frame'] - off['ms_per_input_frame']:+.3f} ms per input frame; cuts made at {on['cuts_made']}.  With the option on the "
                      "stream has a forward less per cut (the window before a cut holds a frame instead of interpolating), which is part of the "
                      "difference.",
                      "`net + glue ms / window` is the host's time inside the runner's flush.  With the option off the host runs ahead until the "
                      "writer's queue is full and waits there, inside flush; with it on the host meets the device earlier, at the event of a "
                      "frame's record, outside flush (the likely cause, not taken apart here: the upload stream's kernel and copy share the "
                      "device's hardware queues with the forwards queued before them).  The wall time is the device's in both."]
        lines.append("")
    if dist:
        lines += [f"## `distance` on rendered streams ({dist['streams']} streams of {dist['scenes_per_stream']} scenes, {dist['size']}x{dist['size']})", "",
                  "| pairs | count | min | 10 % | median | 90 % | 99 % | max |", "|---|---|---|---|---|---|---|---|"]
        for name, label in (("inside", "inside a scene"), ("across", "across a cut")):
            d = dist[name]
            lines.append(f"| {label} | {d['pairs']} | {d['min']} | {d['q10']} | {d['median']} | {d['q90']} | {d['q99']} | {d['max']} |")
        lo, hi = dist["inside"]["max"], dist["across"]["min"]
        lines += ["", f"Cut pairs at or below the largest non-cut distance: {dist['across_below_largest_inside']}.  Largest non-cut {lo}, smallest cut {hi}: "
                  f"a starting threshold between them is their geometric mean, {(lo * hi) ** 0.5:.2f}.  These are rendered textures in uniform motion "
                  "of a few pixels per frame, not footage: fast motion, lighting changes and noise raise the distances inside a scene, so on film "
                  "the threshold belongs higher, and `--scene_cut_min_mad` guards against histogram changes of a nearly still picture.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=["kernels", "distances", "video", "video_parent"], default=None)
    ap.add_argument("--tree", default=None, help="another checkout of the project (built) to import bin_amd from: the parent commit")
    ap.add_argument("--frames", type=int, default=41)
    ap.add_argument("--precision", default="f16x3")
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--streams", type=int, default=8)
    ap.add_argument("--scenes", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--md", default=None)
    ap.add_argument("--from-json", nargs="*", default=None)
    args = ap.parse_args()
    if args.from_json is not None:
        rows = [json.loads(ln) for p in args.from_json for ln in open(p) if ln.startswith("{")]
        with open(args.md or os.path.join(B.REPO, "profiles", "scene_cut.md"), "w") as f:
            f.write(_markdown(rows))
        return
    if args.tree is not None:
        sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    assert torch.cuda.is_available(), "bench_scene_cut needs a GPU"
    import bin_amd
    print(json.dumps({"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()), "device": torch.cuda.get_device_name(0),
                      "package": os.path.dirname(os.path.abspath(bin_amd.__file__))}), flush=True)
    {"kernels": kernels, "distances": distances, "video": video_run, "video_parent": lambda a: video_run(a, parent=True)}[args.leg](args)


if __name__ == "__main__":
    main()
