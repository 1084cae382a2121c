"""What `train.micro_batch` costs and saves (bin_model.optimize_parameters as ceil(B / m) forward / backward passes and one optimizer
step), measured on one MI355X and written to profiles/micro_batch.md (and its row in profiles/README.md).  Needs no files on disk;
prints one JSON line per measurement.

  * b8    (one process): the f16x3 training step of bench.py's training leg, 8 x 256^2, `train.optimizer: hip`, on ONE model with
    `micro_batch` absent, 4, 2 and 1 in alternating blocks: wall time of each step between device synchronisations (median of the
    timed steps), and the peak of torch's allocator over a step (`torch.cuda.max_memory_allocated`, the cached kernel workspaces
    released before each configuration so that none inherits a larger one).  Every split step is reported as a ratio to the unsplit
    step of the same run, which is the path without the option.
  * b64   (one process): the reference's whole-job batch on one GPU: 64 x 256^2 with `micro_batch: 8`, then the same batch unsplit;
    if that does not fit, the allocator's refusal is what is recorded.
  * small (one process): B = 4 at 128 x 128, peak of the `micro_batch: 1` step and of the unsplit step with
    17 x (binhip_rdn_workspace_bytes(N=4) - binhip_rdn_workspace_bytes(N=1)) beside them; and B = 4 at 64 x 64: whether the 14 outputs
    of the split step are the unsplit step's bit for bit, with the loss and gradient differences.
Without --leg, each leg runs as a child process under its own `timeout`, nothing is started after a leg that failed, and the
markdown is written from the legs' lines.
usage: python tools/bench_micro_batch.py [--leg b8|b64|small] [--steps 10] [--blocks 3] [--md profiles/micro_batch.md]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import bench_common as B

LEG_TIMEOUT_S = {"b8": 420, "b64": 420, "small": 240}
README_ROW = "| `micro_batch.md` |"


def _step_ms(model, counter):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counter[0] += 1
    model.optimize_parameters(counter[0])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def _peak(model, counter):
    """Peak bytes of torch's allocator over one step, with the cached kernel workspaces dropped first (a warm-up step regrows them)."""
    import torch
    from bin_amd.rdn_plan import release_workspaces
    release_workspaces()
    torch.cuda.empty_cache()
    _step_ms(model, counter)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    _step_ms(model, counter)
    return torch.cuda.max_memory_allocated(), before


def leg_b8(args):
    from bin_amd import ops
    m = B.train_model()
    counter = [0]
    configs = (None, 4, 2, 1)
    out = {"what": "b8_256_f16x3", "batch": 8, "size": 256, "steps_per_block": args.steps, "blocks": args.blocks, "configs": [str(c) for c in configs]}
    peaks = {}
    for c in configs:
        m.micro_batch = c
        peaks[str(c)] = _peak(m, counter)
    ms = {str(c): [] for c in configs}
    for _ in range(args.blocks):                             # alternating blocks: drift of the box falls on all of them alike
        for c in configs:
            m.micro_batch = c
            _step_ms(m, counter)                             # untimed: the first step after a change of shape
            ms[str(c)] += [_step_ms(m, counter) for _ in range(args.steps)]
    ops.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out["ms_median"] = {k: round(v, 3) for k, v in med.items()}
    out["ms_min_max"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()}
    out["over_unsplit"] = {k: round(v / med["None"], 4) for k, v in med.items()}
    out["peak_bytes"] = {k: v[0] for k, v in peaks.items()}
    out["allocated_before_the_step_bytes"] = {k: v[1] for k, v in peaks.items()}
    out["peak_over_unsplit"] = {k: round(v[0] / peaks["None"][0], 4) for k, v in peaks.items()}
    out["loss"] = float(m.loss)
    return out


def leg_b64(args):
    import torch
    from bin_amd import ops
    m = B.train_model(batch=64)
    counter = [0]
    out = {"what": "b64_256_f16x3", "batch": 64, "size": 256, "steps": args.steps}
    m.micro_batch = 8
    peak, before = _peak(m, counter)
    ms = [_step_ms(m, counter) for _ in range(args.steps)]
    out["micro_8"] = {"ms_median": round(statistics.median(ms), 2), "ms_min_max": [round(min(ms), 2), round(max(ms), 2)],
                      "peak_bytes": peak, "allocated_before_the_step_bytes": before, "loss": float(m.loss)}
    m.micro_batch = None
    try:
        peak, before = _peak(m, counter)
        ms = [_step_ms(m, counter) for _ in range(max(2, args.steps // 2))]
        out["unsplit"] = {"fits": True, "ms_median": round(statistics.median(ms), 2), "ms_min_max": [round(min(ms), 2), round(max(ms), 2)],
                          "peak_bytes": peak, "allocated_before_the_step_bytes": before, "loss": float(m.loss)}
        out["micro_8_over_unsplit"] = round(out["micro_8"]["ms_median"] / out["unsplit"]["ms_median"], 4)
    except torch.cuda.OutOfMemoryError as e:                 # the allocator's refusal: that it does not fit is the result
        out["unsplit"] = {"fits": False, "error": str(e).splitlines()[0].split(" Of the allocated")[0][:300]}
    out["device_total_bytes"] = torch.cuda.get_device_properties(0).total_memory
    ops.check_status()
    return out


def leg_small(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L, ops
    from bin_amd.rdn_plan import c_shape
    out = {"what": "small_shapes_f16x3"}
    m = B.train_model(batch=4, size=128, lr_G=0.0)
    counter = [0]
    peaks = {}
    for c in (1, None):
        m.micro_batch = c
        peaks[str(c)] = _peak(m, counter)
    ws = {}
    for mod in m.netG.module.rdn_modules():
        shape = c_shape(mod.kernel_weights(3).shape)
        ws[mod.N_INPUTS] = [L.lib().binhip_rdn_workspace_bytes(n, 128, 128, mod.N_INPUTS, 3, C.byref(shape)) for n in (1, 4)]
    # the pyramid's 17 calls: 5 on model1 (2 inputs), 6 on model2 (3 inputs), 4 on model3 and 2 on model4 (5 inputs each); training
    # runs them batched along N as four calls, whose workspaces are those of the same images
    calls = {2: 5, 3: 6, 5: 6}
    out["b4_128"] = {"peak_bytes": {k: v[0] for k, v in peaks.items()}, "allocated_before_the_step_bytes": {k: v[1] for k, v in peaks.items()},
                     "peak_unsplit_minus_split": peaks["None"][0] - peaks["1"][0],
                     "workspace_bytes_N1_N4_by_inputs": ws,
                     "17x_two_input_workspace_N4_minus_N1": 17 * (ws[2][1] - ws[2][0]),
                     "17_calls_workspace_N4_minus_N1": sum(k * (ws[i][1] - ws[i][0]) for i, k in calls.items())}
    del m
    torch.cuda.empty_cache()
    whole, split = B.train_model(batch=4, size=64, lr_G=0.0), B.train_model(batch=4, size=64, lr_G=0.0, micro_batch=1)
    whole.optimize_parameters(1)
    split.optimize_parameters(1)
    torch.cuda.synchronize()
    rel = 0.0
    for p, q in zip(split.netG.module.parameters(), whole.netG.module.parameters()):
        rel = max(rel, float((p.grad - q.grad).abs().max()) / max(float(q.grad.abs().max()), 1e-30))
    out["b4_64"] = {"outputs_bit_identical": all(torch.equal(a, b.detach()) for a, b in zip(split.Ft_p, whole.Ft_p)),
                    "outputs_max_abs_diff": max(float((a - b.detach()).abs().max()) for a, b in zip(split.Ft_p, whole.Ft_p)),
                    "loss_split": float(split.loss), "loss_unsplit": float(whole.loss.detach()), "gradients_worst_relative_diff": rel}
    ops.check_status()
    return out


def _mb(n):
    return f"{n / 2 ** 20:,.0f} MiB"


def _markdown(rows):
    lines = ["# `train.micro_batch`: one optimizer step as several forward / backward passes", "",
             "Written by `tools/bench_micro_batch.py`: f16x3, `train.optimizer: hip`, synthetic batches, wall time of each step between device",
             "synchronisations, peak of torch's allocator over one step with the cached kernel workspaces released before each configuration.",
             "Figures of one run on one MI355X; compare within the run only.  There is no pass bar on time: every split step is given as a",
             "ratio to the unsplit step of the same run, which is the path a run without the option takes.", ""]
    clock = next((r for r in rows if r.get("what") == "clock"), None)
    if clock:
        lines += [f"Run: {clock['utc']} UTC, {clock['device']}.", ""]
    r = next((r for r in rows if r.get("what") == "b8_256_f16x3"), None)
    if r:
        lines += ["## 8 x 256², one model, alternating blocks", "",
                  f"{r['blocks']} blocks of {r['steps_per_block']} timed steps per configuration.", "",
                  "| micro_batch | passes | median ms | min .. max ms | / unsplit | peak | / unsplit | allocated before the step |", "|---|---|---|---|---|---|---|---|"]
        for k in r["configs"]:
            passes = 1 if k == "None" else -(-r["batch"] // int(k))
            lines.append(f"| {'absent' if k == 'None' else k} | {passes} | {r['ms_median'][k]} | {r['ms_min_max'][k][0]} .. {r['ms_min_max'][k][1]} | "
                         f"{r['over_unsplit'][k]} | {_mb(r['peak_bytes'][k])} | {r['peak_over_unsplit'][k]} | {_mb(r['allocated_before_the_step_bytes'][k])} |")
        lines.append("")
    r = next((r for r in rows if r.get("what") == "b64_256_f16x3"), None)
    if r:
        a, u = r["micro_8"], r["unsplit"]
        lines += ["## 64 x 256²: the reference's whole-job batch on one GPU", "",
                  f"`micro_batch: 8` (8 passes): median {a['ms_median']} ms per step ({a['ms_min_max'][0]} .. {a['ms_min_max'][1]}), peak {_mb(a['peak_bytes'])} "
                  f"({_mb(a['allocated_before_the_step_bytes'])} allocated before the step: weights, optimizer state, the fed batch, the step before's outputs and cached workspaces), loss {a['loss']:.6f}.", ""]
        if u["fits"]:
            lines += [f"Unsplit: it fits in the device's {_mb(r['device_total_bytes'])}: median {u['ms_median']} ms per step ({u['ms_min_max'][0]} .. {u['ms_min_max'][1]}), "
                      f"peak {_mb(u['peak_bytes'])}, loss {u['loss']:.6f}; the split step takes {r['micro_8_over_unsplit']} of its time.", ""]
        else:
            lines += [f"Unsplit: does not fit in the device's {_mb(r['device_total_bytes'])}: `{u['error']}`.", ""]
    r = next((r for r in rows if r.get("what") == "small_shapes_f16x3"), None)
    if r:
        s, t = r["b4_128"], r["b4_64"]
        lines += ["## The shapes of tests/test_gpu_micro_batch.py", "",
                  f"B = 4 at 128 x 128: peak of the `micro_batch: 1` step {_mb(s['peak_bytes']['1'])}, of the unsplit step {_mb(s['peak_bytes']['None'])}: "
                  f"{_mb(s['peak_unsplit_minus_split'])} less.  Beside them: 17 x (`binhip_rdn_workspace_bytes(N=4)` − `(N=1)`) of the two-input RDN = "
                  f"{_mb(s['17x_two_input_workspace_N4_minus_N1'])}; the same difference summed over the pyramid's 17 calls with each call's own number of "
                  f"inputs (5 + 6 + 4 + 2 calls) = {_mb(s['17_calls_workspace_N4_minus_N1'])}, which is what the saved forward workspaces of three more samples hold.", "",
                  f"B = 4 at 64 x 64, `micro_batch: 1` against the unsplit step on a second model: the 14 outputs are "
                  f"{'bit-identical' if t['outputs_bit_identical'] else 'NOT bit-identical (max abs difference %.3g)' % t['outputs_max_abs_diff']}; "
                  f"loss {t['loss_split']:.9g} against {t['loss_unsplit']:.9g}; worst relative gradient difference {t['gradients_worst_relative_diff']:.3g}.", ""]
    return "\n".join(lines)


def _readme_row(rows):
    b8 = next((r for r in rows if r.get("what") == "b8_256_f16x3"), None)
    b64 = next((r for r in rows if r.get("what") == "b64_256_f16x3"), None)
    text = "`tools/bench_micro_batch.py`: the 8×256² f16x3 training step with `train.micro_batch` absent, 4, 2 and 1 on one model in alternating blocks"
    if b8:
        text += " — " + ", ".join(f"m = {k}: {b8['over_unsplit'][k]} × the time and {b8['peak_over_unsplit'][k]} × the peak memory of the unsplit step"
                                  for k in b8["configs"] if k != "None")
    if b64:
        text += f"; 64×256² with `micro_batch: 8`: {b64['micro_8']['ms_median']} ms per step, peak {_mb(b64['micro_8']['peak_bytes'])}"
        text += (f" (unsplit: {b64['unsplit']['ms_median']} ms, {_mb(b64['unsplit']['peak_bytes'])})" if b64["unsplit"]["fits"] else " (unsplit: does not fit)")
    return f"{README_ROW} {text} |"


def _write_readme(path, row):
    lines = open(path).read().split("\n") if os.path.exists(path) else ["# profiles/", ""]
    at = next((i for i, ln in enumerate(lines) if ln.startswith(README_ROW)), None)
    if at is not None:
        lines[at] = row
    else:
        first = next((i for i, ln in enumerate(lines) if ln.startswith("## ")), len(lines))
        lines[first:first] = ["## A training step in micro-batches", "| file | what |", "|---|---|", row, ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=tuple(LEG_TIMEOUT_S))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "micro_batch.md"))
    args = ap.parse_args()
    legs = {"b8": leg_b8, "b64": leg_b64, "small": leg_small}
    if args.leg is not None:
        B.main(__file__, legs, LEG_TIMEOUT_S, args, ())
        return
    rows = []
    for leg in legs:                                         # each leg a child under its own time limit; nothing after a failure
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg,
               "--steps", str(args.steps), "--blocks", str(args.blocks)]
        r = subprocess.run(cmd, cwd=B.REPO, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            print(json.dumps({"what": "failed", "leg": leg, "exit_status": r.returncode}), flush=True)
            sys.exit(r.returncode)
        for ln in r.stdout.splitlines():
            if ln.startswith("{"):
                row = json.loads(ln)
                if row.get("what") != "clock" or not rows:
                    rows.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
    with open(args.md, "w") as f:
        f.write(_markdown(rows))
    _write_readme(os.path.join(os.path.dirname(os.path.abspath(args.md)), "README.md"), _readme_row(rows))
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
