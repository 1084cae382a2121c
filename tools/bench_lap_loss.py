"""What `pixel_criterion: cb+lap` costs (libbinlap.so, bin_amd/models/loss.py), measured on one MI355X and written to
profiles/lap_loss.md (and its row in profiles/README.md).  Needs no files on disk; prints one JSON line per measurement.

  * resources (no device): VGPRs, SGPRs, LDS and scratch of the five kernels from hipcc's -Rpass-analysis=kernel-resource-usage.
  * kernels: device time (hipEvent pairs, stream idle before each) of binlap_forward and binlap_backward at the training shape, the
    17 pairs of bin_model.get_loss at 8 x 3 x 256 x 256 with 5 levels (14 pairs with a gradient for x only, 3 with both), with the
    fused Charbonnier forward and backward of the same pairs beside them; then each kernel's device time from torch.profiler over a
    few more calls, next to the bytes it moves by construction (counted here, level by level) and the fraction of the HBM rate
    that implies.
  * step: the 8 x 256^2 f16x3 training step of bench.py's training leg under `cb+lap` and under `cb`, two models in one process in
    alternating blocks, wall time per step between device synchronisations.
  * trees (--other PATH, optional): the `cb+lap` and the `cb` step of this checkout against the `cb` step of another built checkout
    (the commit before), each block a child process of its own, alternating.
Without --leg, each leg runs as a child process under its own `timeout`, nothing is started after a leg that failed, and the
markdown is written from the legs' lines.  --tests-log PATH: the output of `pytest tests/test_gpu_lap_loss.py -m gpu -s`; the largest
observed fraction of the bar is taken from its `[lap_loss] table` lines.
usage: python tools/bench_lap_loss.py [--leg resources|kernels|step|trees] [--steps 10] [--blocks 3] [--other PATH] [--tests-log PATH]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import bench_common as B

LEG_TIMEOUT_S = {"resources": 120, "kernels": 150, "step": 420, "trees": 560}
README_ROW = "| `lap_loss.md` |"
KERNELS = ("lap_down_kernel<false>", "lap_down_kernel<true>", "lap_up_kernel<false>", "lap_up_kernel<true>", "lap_final_kernel")
WHAT = {"lap_down_kernel<false>": "reduce R, level l -> l + 1 (forward and backward)", "lap_down_kernel<true>": "G - E^T r in place (backward)",
        "lap_up_kernel<false>": "band and its Charbonnier sum (forward)", "lap_up_kernel<true>": "G = r + R^T(...), gx / gy at level 0 (backward)",
        "lap_final_kernel": "the slots of a term, level by level (forward)"}
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12     # bytes / s: the part's specification, and what a float4 copy reaches on it
LEVELS, LAP_WEIGHT = 5, 0.5

# one block of steps of the checkout at argv[1] under the criterion argv[3], with that checkout's own tools/bench_common.py
_BLOCK = r"""
import json, sys
sys.path.insert(0, sys.argv[1] + "/tools")
import bench_common as B
import torch
assert B.REPO == sys.argv[1], B.REPO
extra = {"pixel_criterion": "cb+lap", "lap_weight": 0.5} if sys.argv[3] == "cb+lap" else {}
m = B.train_model(**extra)
counter = {}
B.train_block(m, 3, counter)
ms = [B.train_block(m, 1, counter) for _ in range(int(sys.argv[2]))]
from bin_amd import _lib, ops
ops.check_status()
print(json.dumps({"tree": sys.argv[1], "ms": ms, "loss": float(m.loss), "loaded": sorted(_lib._loaded)}))
"""


def leg_resources(args):
    from bin_amd import build
    row = build.row("binlap")
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
            name = _kernel_of(m.group(1))
        elif name and m.group(2) in ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "LDS Size", "Occupancy"):
            out["kernels"].setdefault(name, {})[m.group(2)] = int(m.group(3))
    return out


def _kernel_of(symbol):
    """The entry of KERNELS a mangled or demangled kernel name belongs to, or None."""
    for base in ("lap_down_kernel", "lap_up_kernel"):
        if base in symbol:
            flag = re.search(base + r"(?:<(true|false)>|ILb([01])E)", symbol)
            if flag:
                return f"{base}<{flag.group(1) or ('true' if flag.group(2) == '1' else 'false')}>"
    return "lap_final_kernel" if "lap_final_kernel" in symbol else None


def _training_pairs(batch=8, size=256):
    import torch
    g = torch.Generator().manual_seed(11)
    outs = [torch.rand(batch, 3, size, size, generator=g).cuda() for _ in range(14)]
    gts = [(o + 0.05 * torch.randn(batch, 3, size, size, generator=g).cuda()).clamp(0, 1) for o in outs]
    pairs = list(zip(outs, gts)) + [(outs[1], outs[7]), (outs[5], outs[9]), (outs[2], outs[8])]
    return pairs, [(True, False)] * 14 + [(True, True)] * 3


def _bytes_by_construction(terms, planes, size, levels, outputs):
    """Per kernel the bytes one forward plus one backward call read and write by construction, tile halos not counted: level 0 is
    read as two fp32 planes, the levels above and the adjoint as doubles, the gradients are written as fp32."""
    from bin_amd import _lib as L
    n = [terms * planes * ((size + (1 << l) - 1) >> l) ** 2 for l in range(levels)]
    fine = lambda l: 8 * n[l]                                        # 2 x fp32 at level 0, one double above: 8 bytes per pixel either way
    tiles = lambda l: terms * planes * -(-((size + (1 << l) - 1) >> l) // L.LAP_UP_TILE[0]) * -(-((size + (1 << l) - 1) >> l) // L.LAP_UP_TILE[1])
    out = dict.fromkeys(KERNELS, 0)
    for l in range(levels - 1):
        out["lap_down_kernel<false>"] += 2 * (fine(l) + 8 * n[l + 1])                    # once in the forward, once in the backward
        out["lap_down_kernel<true>"] += fine(l) + 8 * n[l + 1] + 16 * n[l + 1]
    for l in range(levels):
        coarse = 8 * n[l + 1] if l < levels - 1 else 0
        out["lap_up_kernel<false>"] += fine(l) + coarse + 8 * tiles(l)
        out["lap_up_kernel<true>"] += fine(l) + 2 * coarse + (8 * n[l] if l else 4 * outputs * planes * size * size)
    out["lap_final_kernel"] = 8 * sum(tiles(l) for l in range(levels)) + 4 * terms
    return out


def _profiled_kernels(fn, calls):
    """{kernel: (launches, device ms in all)} of `calls` calls of fn from torch.profiler, or None where it gives no device rows."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    seen = {}
    for ev in prof.key_averages():
        k = _kernel_of(ev.key)
        us = getattr(ev, "device_time_total", None)
        if us is None:
            us = getattr(ev, "cuda_time_total", 0)
        if k and us:
            n, t = seen.get(k, (0, 0.0))
            seen[k] = (n + ev.count, t + us / 1e3)
    return seen or None


def leg_kernels(args):
    import torch
    from bin_amd import _lib as L, ops
    pairs, need = _training_pairs()
    g = torch.full((17,), LAP_WEIGHT / 17, device="cuda")
    one = torch.ones((), device="cuda")
    wanted = [(pairs[i][0], [(i, 1.0)]) for i in range(14)]
    calls = {"lap_forward": lambda: ops.lap_terms(pairs, LEVELS, 1e-6),
             "lap_backward": lambda: ops.lap_terms_grad(pairs, g, need, LEVELS, 1e-6),
             "cb_forward": lambda: ops.multi_pixel_loss(L.LOSS_CHARBONNIER, pairs, 1e-6),
             "cb_backward": lambda: ops.multi_pixel_loss_grad(L.LOSS_CHARBONNIER, pairs, one, wanted, 1e-6)}
    for fn in calls.values():
        fn()
    dev, host = B.alternating_blocks(calls, args.blocks, args.steps)
    value = ops.lap_terms(pairs, LEVELS, 1e-6)
    out = {"what": "kernels", "terms": 17, "shape": [8, 3, 256, 256], "levels": LEVELS, "calls_each": args.blocks * args.steps,
           "device_ms_median": {k: round(v, 4) for k, v in B.medians(dev).items()},
           "device_ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in dev.items()},
           "host_ms_median": {k: round(v, 4) for k, v in B.medians(host).items()},
           "forward_workspace_bytes": L.laplib().binlap_forward_workspace_bytes(17, 24, 256, 256, LEVELS),
           "backward_workspace_bytes": L.laplib().binlap_backward_workspace_bytes(17, 24, 256, 256, LEVELS),
           "gradient_bytes_written": 20 * 4 * 8 * 3 * 256 * 256, "lap_of_the_pairs": [round(float(v), 6) for v in value[:3]]}
    n = 5
    try:
        seen = _profiled_kernels(lambda: (calls["lap_forward"](), calls["lap_backward"]()), n)
    except Exception as e:                                           # the profiler is an instrument, not the product: say so and go on
        seen, out["per_kernel_error"] = None, repr(e)[:200]
    if seen:
        moved = _bytes_by_construction(17, 24, 256, LEVELS, 20)
        out["per_kernel"] = {k: {"launches_per_pair_of_calls": seen[k][0] // n, "device_ms_per_pair_of_calls": round(seen[k][1] / n, 4),
                                 "bytes": moved[k], "tb_per_s": round(moved[k] / (seen[k][1] / n * 1e-3) / 1e12, 3),
                                 "of_hbm_peak": round(moved[k] / (seen[k][1] / n * 1e-3) / HBM_PEAK, 3),
                                 "of_hbm_copy": round(moved[k] / (seen[k][1] / n * 1e-3) / HBM_COPY, 3)} for k in KERNELS if k in seen}
    return out


def leg_step(args):
    from bin_amd import ops
    models = {"cb": B.train_model(), "cb+lap": B.train_model(pixel_criterion="cb+lap", lap_weight=LAP_WEIGHT)}
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
    parts = [float(p) for p in models["cb+lap"].loss_parts]
    return {"what": "step", "batch": 8, "size": 256, "blocks": args.blocks, "steps_per_block": args.steps,
            "ms_median": {k: round(v, 3) for k, v in med.items()}, "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            "cb+lap_over_cb": round(med["cb+lap"] / med["cb"], 4), "added_ms": round(med["cb+lap"] - med["cb"], 3),
            "loss": {k: float(m.loss.detach()) for k, m in models.items()}, "l_cb_l_lap": parts}


def leg_trees(args):
    if not args.other:
        return {"what": "trees", "skipped": "no --other checkout given"}
    other = os.path.abspath(args.other)
    runs = {"this cb+lap": (B.REPO, "cb+lap"), "this cb": (B.REPO, "cb"), "other cb": (other, "cb")}
    ms, meta = {k: [] for k in runs}, {}
    for _ in range(args.blocks):                             # a process per block, alternating; nothing after one that failed
        for k, (path, criterion) in runs.items():
            r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, "-c", _BLOCK, path, str(args.steps), criterion], cwd=path,
                               stdout=subprocess.PIPE, text=True)
            if r.returncode != 0:
                print(json.dumps({"what": "failed", "leg": "trees", "run": k, "exit_status": r.returncode}), flush=True)
                sys.exit(r.returncode)
            row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
            ms[k] += row["ms"]
            meta[k] = {"loss": row["loss"], "loaded": row["loaded"]}
    med = {k: statistics.median(v) for k, v in ms.items()}
    pairs = [a / b for a, b in zip(*[[statistics.median(ms[k][i:i + args.steps]) for i in range(0, len(ms[k]), args.steps)]
                                     for k in ("this cb+lap", "other cb")])]
    return {"what": "trees", "blocks": args.blocks, "steps_per_block": args.steps, "ms_median": {k: round(v, 3) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
            "lap_over_other_cb": round(med["this cb+lap"] / med["other cb"], 4), "lap_over_other_cb_per_pair": [round(p, 4) for p in pairs],
            "cb_over_other_cb": round(med["this cb"] / med["other cb"], 4),
            "same_cb_loss": meta["this cb"]["loss"] == meta["other cb"]["loss"], "cb_loss": meta["this cb"]["loss"],
            "loaded_by_this_cb": meta["this cb"]["loaded"]}


def _bar_fractions(path):
    """The largest `value` and `gradient` fraction over the `[lap_loss] table` lines of a test log, overall and per content kind."""
    worst, kinds = [0.0, 0.0], {}
    for line in open(path):
        m = re.search(r"\[lap_loss\] table \S+: worst fraction of the bar: value ([\d.]+), gradient ([\d.]+); per kind (.*)$", line)
        if not m:
            continue
        worst = [max(worst[0], float(m.group(1))), max(worst[1], float(m.group(2)))]
        for k, v, g in re.findall(r"(\w+) ([\d.]+)/([\d.]+)", m.group(3)):
            old = kinds.get(k, (0.0, 0.0))
            kinds[k] = (max(old[0], float(v)), max(old[1], float(g)))
    return worst, kinds


def _markdown(rows, tests_log):
    lines = ["# `pixel_criterion: cb+lap`: the Laplacian-pyramid term's value and gradient in HIP", "",
             "Written by `tools/bench_lap_loss.py`.  Figures of one run on one MI355X; compare within the run only (boxes differ by up to 7 %).",
             "There is no bar on the cost: this note states it.  Whether `cb+lap` trains a better network is not judged here: that takes real",
             "footage and a long run, and nothing below says anything about it.", ""]
    clock = next((r for r in rows if r.get("what") == "clock"), None)
    if clock:
        lines += [f"Run: {clock['utc']} UTC, {clock['device']}.", ""]
    r = next((r for r in rows if r.get("what") == "resources"), None)
    if r:
        lines += ["## Resource usage (`-Rpass-analysis=kernel-resource-usage`, gfx950)", "",
                  "| kernel | VGPRs | AGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |", "|---|---|---|---|---|---|---|"]
        for k, v in r["kernels"].items():
            lines.append(f"| `{k}` | {v.get('VGPRs')} | {v.get('AGPRs')} | {v.get('TotalSGPRs')} | {v.get('LDS Size')} | {v.get('ScratchSize')} | {v.get('Occupancy')} |")
        lines += [""]
    r = next((r for r in rows if r.get("what") == "kernels"), None)
    if r:
        d, mm = r["device_ms_median"], r["device_ms_min_max"]
        L = r["levels"]
        lines += [f"## The two calls at the training shape: 17 pairs of 8 x 3 x 256 x 256, {L} levels", "",
                  f"Device time between hipEvent pairs, median of {r['calls_each']} calls each in alternating blocks; 14 pairs want the gradient of x, 3 want both.",
                  "", "| call | launches | device ms | min .. max | host ms |", "|---|---|---|---|---|"]
        for k, n in (("lap_forward", 2 * L), ("lap_backward", 3 * L - 2), ("cb_forward", 2), ("cb_backward", 1)):
            lines.append(f"| `{k}` | {n} | {d[k]} | {mm[k][0]} .. {mm[k][1]} | {r['host_ms_median'][k]} |")
        lines += ["", f"The forward's workspace is {r['forward_workspace_bytes']:,} bytes and the backward's {r['backward_workspace_bytes']:,} (levels >= 1 in double); "
                  f"the backward writes {r['gradient_bytes_written'] / 2 ** 20:,.0f} MiB of gradients.  For scale, `cb+ssim`'s two calls take 0.51 ms and 1.27 ms "
                  "(`ssim_loss.md`, another run).  All arithmetic is double on the vector ALU.", ""]
        if r.get("per_kernel"):
            lines += ["### Per kernel: time, bytes by construction, fraction of the HBM rate", "",
                      "Device time from torch.profiler over one forward plus one backward call, all levels of a kernel together (level 0 is 3/4 of",
                      "the pixels).  Bytes: what the kernel reads and writes by construction, counted level by level in `_bytes_by_construction`",
                      "(tile halos and cache hits not counted, so this is the traffic a perfect cache would leave, not a counter reading).  The",
                      f"fractions are of the {HBM_PEAK / 1e12:.1f} TB/s specification and of the {HBM_COPY / 1e12:.2f} TB/s a float4 copy reaches.", "",
                      "| kernel | what | launches | device ms | MB | TB/s | of peak | of copy rate |", "|---|---|---|---|---|---|---|---|"]
            for k, v in r["per_kernel"].items():
                lines.append(f"| `{k}` | {WHAT[k]} | {v['launches_per_pair_of_calls']} | {v['device_ms_per_pair_of_calls']} | {v['bytes'] / 1e6:,.1f} | "
                             f"{v['tb_per_s']} | {v['of_hbm_peak']} | {v['of_hbm_copy']} |")
            lines += [""]
        elif r.get("per_kernel_error"):
            lines += [f"Per-kernel times were not taken: torch.profiler failed with `{r['per_kernel_error']}`.", ""]
    r = next((r for r in rows if r.get("what") == "step"), None)
    if r:
        lines += ["## The 8 x 256² f16x3 training step", "",
                  f"Two models in one process, {r['blocks']} alternating blocks of {r['steps_per_block']} timed steps, wall time between device synchronisations.", "",
                  "| pixel_criterion | median ms | min .. max ms |", "|---|---|---|"]
        for k in ("cb", "cb+lap"):
            lines.append(f"| `{k}` | {r['ms_median'][k]} | {r['ms_min_max'][k][0]} .. {r['ms_min_max'][k][1]} |")
        lines += ["", f"`cb+lap` takes {r['cb+lap_over_cb']} x the time of `cb` ({r['added_ms']:+} ms per step); `cb+ssim` took 1.02 x in its own run.", ""]
    r = next((r for r in rows if r.get("what") == "trees" and "skipped" not in r), None)
    if r:
        m, mm = r["ms_median"], r["ms_min_max"]
        lines += ["## Against the `cb` step of the commit before", "",
                  f"{r['blocks']} alternating rounds of {r['steps_per_block']} timed steps, a process per block, in the order `cb+lap` of this commit, `cb` of this commit, "
                  "`cb` of the commit before.", "", "| run | median ms | min .. max ms |", "|---|---|---|"]
        lines += [f"| {k} | {m[k]} | {mm[k][0]} .. {mm[k][1]} |" for k in m]
        lines += ["", f"`cb+lap` of this commit takes {r['lap_over_other_cb']} x the `cb` step of the commit before; round by round "
                  f"{', '.join(str(p) for p in r['lap_over_other_cb_per_pair'])}.  `cb` of this commit takes {r['cb_over_other_cb']} x; its loss after the last step is "
                  f"{'the same number' if r['same_cb_loss'] else 'NOT the same number'} ({r['cb_loss']:.9g}), and a `cb` run of this commit loaded "
                  f"{', '.join(r['loaded_by_this_cb'])}.", ""]
    if tests_log and os.path.exists(tests_log):
        worst, kinds = _bar_fractions(tests_log)
        lines += ["## Accuracy: the largest observed fraction of the bar", "",
                  "tests/test_gpu_lap_loss.py over the case table of tests/lap_loss_cases.py, against float64 on the same fp32 inputs and the same fp32 g.",
                  "The bar, on every value and every gradient element: 2^-23 |ref| + 2^-40 max|ref|.", "",
                  f"Largest fraction over the table: value {worst[0]:.3f}, gradient {worst[1]:.3f}.  The bar is not missed anywhere.", "",
                  "| content | value | gradient |", "|---|---|---|"]
        lines += [f"| {k} | {v:.2f} | {g:.2f} |" for k, (v, g) in kinds.items()]
        lines += ["", "Both are what one fp32 rounding of a double result leaves: at most half a unit in the last place, which is half of the bar's",
                  "rounding part.  Double is not too slow for this (the tables above), so nothing was traded for it.", ""]
    return "\n".join(lines)


def _readme_row(rows):
    k = next((r for r in rows if r.get("what") == "kernels"), None)
    s = next((r for r in rows if r.get("what") == "step"), None)
    text = "`tools/bench_lap_loss.py`: `pixel_criterion: cb+lap` (libbinlap.so): kernel resources, bytes and HBM fraction per kernel, accuracy against float64"
    if k:
        text += f"; 17 pairs of 8×3×256², 5 levels: forward {k['device_ms_median']['lap_forward']} ms, backward {k['device_ms_median']['lap_backward']} ms on the device"
    if s:
        text += f"; the 8×256² training step takes {s['cb+lap_over_cb']} × the `cb` step ({s['added_ms']:+} ms)"
    return f"{README_ROW} {text} |"


def _write_readme(path, row):
    lines = open(path).read().split("\n") if os.path.exists(path) else ["# profiles/", ""]
    at = next((i for i, ln in enumerate(lines) if ln.startswith(README_ROW)), None)
    if at is not None:
        lines[at] = row
    else:
        first = next((i for i, ln in enumerate(lines) if ln.startswith("## ")), len(lines))
        lines[first:first] = ["## The cb+lap training criterion", "| file | what |", "|---|---|", row, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=tuple(LEG_TIMEOUT_S))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--other", default="")
    ap.add_argument("--tests-log", default="")
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "lap_loss.md"))
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
