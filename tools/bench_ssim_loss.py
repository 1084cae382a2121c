"""What `pixel_criterion: cb+ssim` costs (libbinssim.so, bin_amd/models/loss.py), measured on one MI355X and written to
profiles/ssim_loss.md (and its row in profiles/README.md).  Needs no files on disk; prints one JSON line per measurement.

  * resources (no device): VGPRs, SGPRs, LDS and scratch of the three kernels from hipcc's -Rpass-analysis=kernel-resource-usage.
  * kernels: device time (hipEvent pairs, stream idle before each) of binssim_forward and binssim_backward at the training shape,
    the 17 pairs of bin_model.get_loss at 8 x 3 x 256 x 256 (14 pairs with a gradient for x only, 3 with both), with the fused
    Charbonnier forward and backward of the same pairs beside them.
  * step: the 8 x 256^2 f16x3 training step of bench.py's training leg under `cb+ssim` and under `cb`, two models in one process in
    alternating blocks, wall time per step between device synchronisations.
  * trees (--other PATH, optional): the `cb` step of this checkout against the `cb` step of another built checkout (the commit
    before), each block a child process of its own, alternating.
Without --leg, each leg runs as a child process under its own `timeout`, nothing is started after a leg that failed, and the
markdown is written from the legs' lines.  --tests-log PATH: the output of `pytest tests/test_gpu_ssim_loss.py -m gpu -s`; the largest
observed fraction of each bar is taken from its `[ssim_loss] table` lines.
usage: python tools/bench_ssim_loss.py [--leg resources|kernels|step|trees] [--steps 10] [--blocks 3] [--other PATH] [--tests-log PATH]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import bench_common as B

LEG_TIMEOUT_S = {"resources": 120, "kernels": 120, "step": 420, "trees": 560}
README_ROW = "| `ssim_loss.md` |"
KERNELS = ("ssim_fwd_tile_kernel", "ssim_fwd_final_kernel", "ssim_bwd_kernel")

# one block of `cb` steps of the checkout at argv[1], with that checkout's own tools/bench_common.py: only what both checkouts have
_CB_BLOCK = r"""
import json, sys
sys.path.insert(0, sys.argv[1] + "/tools")
import bench_common as B
import torch
assert B.REPO == sys.argv[1], B.REPO
m = B.train_model()
counter = {}
B.train_block(m, 3, counter)
ms = [B.train_block(m, 1, counter) for _ in range(int(sys.argv[2]))]
from bin_amd import _lib, ops
ops.check_status()
print(json.dumps({"tree": sys.argv[1], "ms": ms, "loss": float(m.loss), "loaded": sorted(_lib._loaded)}))
"""


def leg_resources(args):
    from bin_amd import build
    row = build.row("binssim")
    src = os.path.join(build.CSRC, row.subdir, row.sources[0])
    cmd = build.build_plan(table=build.ADDON_LIBRARIES)[0][0][:6] + ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull]
    text = subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    out = {"what": "resources", "kernels": {}}
    name = None
    for line in text.splitlines():
        m = re.search(r"remark: (?:Function Name: (\S+)|\s*([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)) \[-Rpass", line)
        if not m:
            continue
        if m.group(1):
            name = next((k for k in KERNELS if k in m.group(1)), None)
        elif name and m.group(2) in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy"):
            out["kernels"].setdefault(name, {})[m.group(2)] = int(m.group(3))
    return out


def _training_pairs(batch=8, size=256):
    import torch
    g = torch.Generator().manual_seed(11)
    outs = [torch.rand(batch, 3, size, size, generator=g).cuda() for _ in range(14)]
    gts = [(o + 0.05 * torch.randn(batch, 3, size, size, generator=g).cuda()).clamp(0, 1) for o in outs]
    pairs = list(zip(outs, gts)) + [(outs[1], outs[7]), (outs[5], outs[9]), (outs[2], outs[8])]
    return pairs, [(True, False)] * 14 + [(True, True)] * 3


def leg_kernels(args):
    import torch
    from bin_amd import _lib as L, ops
    pairs, need = _training_pairs()
    g = torch.full((17,), -0.5 / 17, device="cuda")
    one = torch.ones((), device="cuda")
    wanted = [(pairs[i][0], [(i, 1.0)]) for i in range(14)]
    calls = {"ssim_forward": lambda: ops.ssim_terms(pairs),
             "ssim_backward": lambda: ops.ssim_terms_grad(pairs, g, need),
             "cb_forward": lambda: ops.multi_pixel_loss(L.LOSS_CHARBONNIER, pairs, 1e-6),
             "cb_backward": lambda: ops.multi_pixel_loss_grad(L.LOSS_CHARBONNIER, pairs, one, wanted, 1e-6)}
    for fn in calls.values():
        fn()
    dev, host = B.alternating_blocks(calls, args.blocks, args.steps)
    value = ops.ssim_terms(pairs)
    return {"what": "kernels", "terms": 17, "shape": [8, 3, 256, 256], "calls_each": args.blocks * args.steps,
            "device_ms_median": {k: round(v, 4) for k, v in B.medians(dev).items()},
            "device_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in dev.items()},
            "host_ms_median": {k: round(v, 4) for k, v in B.medians(host).items()},
            "workspace_bytes": L.ssimlib().binssim_workspace_bytes(17, 24, 256, 256),
            "gradient_bytes_written": 20 * 4 * 8 * 3 * 256 * 256, "ssim_of_the_pairs": [round(float(v), 6) for v in value[:3]]}


def leg_step(args):
    from bin_amd import ops
    models = {"cb": B.train_model(), "cb+ssim": B.train_model(pixel_criterion="cb+ssim", ssim_weight=0.1)}
    counter = {}
    ms = {k: [] for k in models}
    for m in models.values():
        B.train_block(m, 3, counter)
    for _ in range(args.blocks):                             # alternating blocks: drift of the box falls on both alike
        for k, m in models.items():
            B.train_block(m, 1, counter)
            ms[k] += [B.train_block(m, 1, counter) for _ in range(args.steps)]
    ops.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    parts = [float(p) for p in models["cb+ssim"].loss_parts]
    return {"what": "step", "batch": 8, "size": 256, "blocks": args.blocks, "steps_per_block": args.steps,
            "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            "cb+ssim_over_cb": round(med["cb+ssim"] / med["cb"], 4), "added_ms": round(med["cb+ssim"] - med["cb"], 3),
            "loss": {k: float(m.loss.detach()) for k, m in models.items()}, "l_cb_l_ssim": parts}


def leg_trees(args):
    if not args.other:
        return {"what": "trees", "skipped": "no --other checkout given"}
    trees = {"this": B.REPO, "other": os.path.abspath(args.other)}
    ms, meta = {k: [] for k in trees}, {}
    for _ in range(args.blocks):                             # a process per block, alternating; nothing after one that failed
        for k, path in trees.items():
            r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-c", _CB_BLOCK, path, str(args.steps)], cwd=path,
                               stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(json.dumps({"what": "failed", "leg": "trees", "tree": k, "exit_status": r.returncode}), flush=True)
                sys.exit(r.returncode)
            row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            ms[k] += row["ms"]
            meta[k] = {"loss": row["loss"], "loaded": row["loaded"]}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"what": "trees", "blocks": args.blocks, "steps_per_block": args.steps, "ms_median": {k: round(v, 3) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}, "this_over_other": round(med["this"] / med["other"], 4),
            "same_loss": meta["this"]["loss"] == meta["other"]["loss"], "loss": meta["this"]["loss"], "loaded_by_this": meta["this"]["loaded"]}


def _bar_fractions(path):
    """The largest `value` and `gradient` fraction over the `[ssim_loss] table` lines of a test log, overall and per content kind."""
    worst, kinds = [0.0, 0.0], {}
    for line in open(path):
        m = re.search(r"\[ssim_loss\] table \S+: worst fraction of the bar: value ([\d.]+), gradient ([\d.]+); per kind (.*)$", line)
        if not m:
            continue
        worst = [max(worst[0], float(m.group(1))), max(worst[1], float(m.group(2)))]
        for k, v, g in re.findall(r"(\w+) ([\d.]+)/([\d.]+)", m.group(3)):
            old = kinds.get(k, (0.0, 0.0))
            kinds[k] = (max(old[0], float(v)), max(old[1], float(g)))
    return worst, kinds


def _markdown(rows, tests_log):
    lines = ["# `pixel_criterion: cb+ssim`: the SSIM term's value and gradient in HIP", "",
             "Written by `tools/bench_ssim_loss.py`.  Figures of one run on one MI355X; compare within the run only (boxes differ by up to 7 %).",
             "There is no bar on the cost: this note states it.", ""]
    clock = next((r for r in rows if r.get("what") == "clock"), None)
    if clock:
        lines += [f"Run: {clock['utc']} UTC, {clock['device']}.", ""]
    r = next((r for r in rows if r.get("what") == "resources"), None)
    if r:
        lines += ["## Resource usage (`-Rpass-analysis=kernel-resource-usage`, gfx950)", "",
                  "| kernel | VGPRs | AGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |", "|---|---|---|---|---|---|---|"]
        for k, v in r["kernels"].items():
            lines.append(f"| `{k}` | {v.get('VGPRs')} | {v.get('AGPRs')} | {v.get('TotalSGPRs')} | {v.get('LDS Size')} | {v.get('ScratchSize')} | {v.get('Occupancy')} |")
        lines += ["", "No kernel uses scratch; static LDS stays within 64 KB.", ""]
    r = next((r for r in rows if r.get("what") == "kernels"), None)
    if r:
        d, mm = r["device_ms_median"], r["device_ms_min_max"]
        lines += ["## The two calls at the training shape: 17 pairs of 8 x 3 x 256 x 256", "",
                  f"Device time between hipEvent pairs, median of {r['calls_each']} calls each in alternating blocks; 14 pairs want the gradient of x, 3 want both.",
                  "", "| call | launches | device ms | min .. max | host ms |", "|---|---|---|---|---|"]
        for k, n in (("ssim_forward", 2), ("ssim_backward", 1), ("cb_forward", 2), ("cb_backward", 1)):
            lines.append(f"| `{k}` | {n} | {d[k]} | {mm[k][0]} .. {mm[k][1]} | {r['host_ms_median'][k]} |")
        px = 17 * 8 * 3 * 256 * 256
        lines += ["", f"The forward's workspace is {r['workspace_bytes']:,} bytes; the backward writes {r['gradient_bytes_written'] / 2 ** 20:,.0f} MiB of gradients.  "
                  f"Per pixel of the {px / 1e6:.1f} M the forward takes {1e6 * d['ssim_forward'] / px:.3f} ns and the backward {1e6 * d['ssim_backward'] / px:.3f} ns, all "
                  "window arithmetic in double on the vector ALU.", ""]
    r = next((r for r in rows if r.get("what") == "step"), None)
    if r:
        lines += ["## The 8 x 256² f16x3 training step", "",
                  f"Two models in one process, {r['blocks']} alternating blocks of {r['steps_per_block']} timed steps, wall time between device synchronisations.", "",
                  "| pixel_criterion | median ms | min .. max ms |", "|---|---|---|"]
        for k in ("cb", "cb+ssim"):
            lines.append(f"| `{k}` | {r['ms_median'][k]} | {r['ms_min_max'][k][0]} .. {r['ms_min_max'][k][1]} |")
        lines += ["", f"`cb+ssim` takes {r['cb+ssim_over_cb']} x the time of `cb` ({r['added_ms']:+} ms per step).", ""]
    r = next((r for r in rows if r.get("what") == "trees" and "skipped" not in r), None)
    if r:
        lines += ["## The `cb` step against the commit before", "",
                  f"{r['blocks']} alternating blocks of {r['steps_per_block']} timed steps, a process per block: this commit {r['ms_median']['this']} ms "
                  f"({r['ms_min_max']['this'][0]} .. {r['ms_min_max']['this'][1]}), the commit before {r['ms_median']['other']} ms "
                  f"({r['ms_min_max']['other'][0]} .. {r['ms_min_max']['other'][1]}): {r['this_over_other']} x.  The loss after the last step is "
                  f"{'the same number' if r['same_loss'] else 'NOT the same number'} ({r['loss']:.9g}); a `cb` run of this commit loaded {', '.join(r['loaded_by_this'])}.", ""]
    if tests_log and os.path.exists(tests_log):
        worst, kinds = _bar_fractions(tests_log)
        lines += ["## Accuracy: the largest observed fraction of each bar", "",
                  "tests/test_gpu_ssim_loss.py over the case table of tests/ssim_loss_cases.py, against float64 on the same fp32 inputs and the same fp32 g.",
                  "Value bar: 2^-24 absolute.  Gradient bar per element: 2^-23 |ref| + 1e-9 max(max|ref|, 1 / (planes P)).", "",
                  f"Largest fraction over the table: value {worst[0]:.3f}, gradient {worst[1]:.3f}.  No bar is missed.", "",
                  "| content | value | gradient |", "|---|---|---|"]
        lines += [f"| {k} | {v:.2f} | {g:.2f} |" for k, (v, g) in kinds.items()]
        lines += ["", "Both are what one fp32 rounding of a double result leaves (at most half a unit in the last place, which is half of either bar's",
                  "rounding part); the smooth and nearly flat kinds, where statistics kept in fp32 miss the gradient by 10² – 10³ x the bar, sit with the rest.", ""]
    return "\n".join(lines)


def _readme_row(rows):
    k = next((r for r in rows if r.get("what") == "kernels"), None)
    s = next((r for r in rows if r.get("what") == "step"), None)
    text = "`tools/bench_ssim_loss.py`: `pixel_criterion: cb+ssim` (libbinssim.so): kernel resources, accuracy against float64"
    if k:
        text += f"; 17 pairs of 8×3×256²: forward {k['device_ms_median']['ssim_forward']} ms, backward {k['device_ms_median']['ssim_backward']} ms on the device"
    if s:
        text += f"; the 8×256² training step takes {s['cb+ssim_over_cb']} × the `cb` step ({s['added_ms']:+} ms)"
    return f"{README_ROW} {text} |"


def _write_readme(path, row):
    lines = open(path).read().split("\n") if os.path.exists(path) else ["# profiles/", ""]
    at = next((i for i, ln in enumerate(lines) if ln.startswith(README_ROW)), None)
    if at is not None:
        lines[at] = row
    else:
        first = next((i for i, ln in enumerate(lines) if ln.startswith("## ")), len(lines))
        lines[first:first] = ["## The cb+ssim training criterion", "| file | what |", "|---|---|", row, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=tuple(LEG_TIMEOUT_S))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--other", default="")
    ap.add_argument("--tests-log", default="")
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "ssim_loss.md"))
    args = ap.parse_args()
    legs = {"resources": leg_resources, "kernels": leg_kernels, "step": leg_step, "trees": leg_trees}
    if args.leg in ("resources", "trees"):
        print(json.dumps(legs[args.leg](args)), flush=True)      # no device in this process
        return
    if args.leg is not None:
        B.main(__file__, legs, LEG_TIMEOUT_S, args, ())
        return
    rows = []
    for leg in legs:                                         # each leg a child under its own time limit; nothing after a failure
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--steps", str(args.steps), "--blocks", str(args.blocks), "--other", args.other]
        r = subprocess.run(cmd, cwd=B.REPO, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps({"what": "failed", "leg": leg, "exit_status": r.returncode}), flush=True)
            sys.exit(r.returncode)
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                row = json.loads(ln)
                if row.get("what") != "clock" or not any(r.get("what") == "clock" for r in rows):
                    rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(_markdown(rows, args.tests_log))
    _write_readme(os.path.join(os.path.dirname(os.path.abspath(args.md)), "README.md"), _readme_row(rows))
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
