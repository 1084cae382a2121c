"""Cost of the test-time self-ensemble (bin_amd/ensemble.py over binens_orient / binens_merge).  Needs no files on disk; prints one
JSON line per measurement and, run without --leg, writes profiles/self_ensemble.md from them.

  * kernels: binens_orient (1 frame -> 3 flips) and binens_merge (M = 4 and 8, 3 and 14 slots) at [1,3,768,1344] (a padded 720p
    frame), BACK calls back to back between one hipEvent pair after a warm-up, blocks alternating with the same function composed
    from torch.flip, adds and a scale (the tree of bin_amd.ensemble.tree_sum), median over all samples, and the spread (min .. max)
    of both.  Bytes moved (what the algorithm needs: every source read once, every destination written once) over the median, as a
    share of the HBM rate.  Before timing, the two are compared bit for bit.
  * window : f16x3, resident padded 720p frames, windows streamed over a clip with the memo on: a plain window against `hv` and
    `hvt`, the ratio to M x the plain window, and the glue (one orient launch per new frame, one merge of the 3 consumed slots)
    timed on its own as a share of the ensembled window.
  * small  : 256x256 frames (padded 320x320), `hvt`: windows/s of the batched strategy (one forward at N = 8) against the streamed
    one (8 forwards at N = 1, memo on).
Each leg runs as a child process under its own `timeout`, and nothing is started after a leg that failed.  No figure printed here is
comparable across boxes: compare within one run.
usage: python tools/bench_ensemble.py [--leg kernels|window|small] [--samples 40] [--blocks 4] [--windows 6] [--repeat 3]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import bench_common as B

LEG_TIMEOUT_S = {"kernels": 300, "window": 420, "small": 300}
BACK = 5
FRAME = (1, 3, 768, 1344)
HBM_SPEC_TBPS, HBM_COPY_TBPS = 8.0, 6.29             # MI355X: HBM3E peak by specification; a measured float4 copy


def _torch_merge(srcs, flip_of):
    from bin_amd.ensemble import tree_sum
    import torch
    dims = {0: None, 1: (-1,), 2: (-2,), 3: (-2, -1)}
    return tree_sum([s if dims[f] is None else torch.flip(s, dims[f]) for s, f in zip(srcs, flip_of)]) * (1.0 / len(flip_of))


def leg_kernels(args):
    import torch
    from bin_amd import ops
    from bin_amd.ensemble import orientations
    numel = FRAME[0] * FRAME[1] * FRAME[2] * FRAME[3]
    g = torch.Generator(device="cuda").manual_seed(3)
    frame = torch.rand(FRAME, device="cuda", generator=g) * 3 - 1
    dst = [torch.empty_like(frame) for _ in range(3)]
    out = []

    def measure(what, kernel, composed, nbytes, same, extra):
        legs = {"kernel": lambda: [kernel() for _ in range(BACK)], "torch": lambda: [composed() for _ in range(BACK)]}
        for fn in legs.values():
            fn()
            fn()
        dev = B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))[0]
        ms = {k: [v / BACK for v in d] for k, d in dev.items()}
        med = B.medians(ms)
        row = {"what": what, "bytes": nbytes, "bit_identical_to_torch": bool(same), "samples_each": len(ms["kernel"]),
               "calls_per_event_pair": BACK}
        for k in ms:
            row[f"{k}_us_median"], row[f"{k}_us_min"], row[f"{k}_us_max"] = (round(v * 1e3, 1) for v in (med[k], min(ms[k]), max(ms[k])))
        rate = nbytes / (med["kernel"] * 1e-3) / 1e12
        row.update({"kernel_TBps": round(rate, 3), "share_of_hbm_spec": round(rate / HBM_SPEC_TBPS, 3),
                    "share_of_measured_copy": round(rate / HBM_COPY_TBPS, 3), "kernel_over_torch": round(med["kernel"] / med["torch"], 4),
                    "not_slower_than_torch_beyond_spread": bool(med["kernel"] <= max(ms["torch"]))})
        row.update(extra)
        print(json.dumps(row), flush=True)
        out.append(row)

    flips = [1, 2, 3]
    got = ops.ens_orient([frame], [dst], [flips])[0]
    want = [torch.flip(frame, d) for d in ((-1,), (-2,), (-2, -1))]
    torch.cuda.synchronize()
    measure("orient_1_frame_3_flips", lambda: ops.ens_orient([frame], [dst], [flips]),
            lambda: [torch.flip(frame, d) for d in ((-1,), (-2,), (-2, -1))], 4 * numel * 4,
            all(torch.equal(a, b) for a, b in zip(got, want)), {"launches": 1, "torch_launches": 3})
    for M, group in ((4, "hv"), (8, "hvt")):
        flip_of = [f for f, _ in orientations(group)]
        for slots in (3, 14):
            srcs = [[torch.rand(FRAME, device="cuda", generator=g) * 3 - 1 for _ in range(M)] for _ in range(slots)]
            outs = [torch.empty_like(frame) for _ in range(slots)]
            got = ops.ens_merge(srcs, flip_of, out=outs)
            want = [_torch_merge(s, flip_of) for s in srcs]
            torch.cuda.synchronize()
            same = all(torch.equal(a, b) for a, b in zip(got, want))
            del want
            measure(f"merge_M{M}_{slots}_slots", lambda: ops.ens_merge(srcs, flip_of, out=outs),
                    lambda: [_torch_merge(s, flip_of) for s in srcs], slots * (M + 1) * numel * 4, same,
                    {"launches": 1, "torch_launches": slots * (sum(1 for f in flip_of if f) + M)})
            del srcs, outs
    return {"what": "kernels_done", "rows": len(out)}


def _net(prec="f16x3"):
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval().set_precision(prec)


def _stream_windows(run, n_windows, reset):
    """Wall ms per window of `n_windows` consecutive windows after one untimed first window (the memo's cold start)."""
    import torch
    reset()
    run(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(1, n_windows + 1):
        run(i)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n_windows


def leg_window(args):
    import torch
    from bin_amd import ops
    from bin_amd.ensemble import SelfEnsemble
    net = _net()
    g = torch.Generator(device="cuda").manual_seed(5)
    clip = [torch.rand(FRAME, device="cuda", generator=g) for _ in range(args.windows + 6)]
    cache = {}
    runs = {"plain": (lambda i: net(*clip[i:i + 6], stage1_cache=cache), cache.clear)}
    ens = {grp: SelfEnsemble(net, grp) for grp in ("hv", "hvt")}
    for grp, e in ens.items():
        assert e.strategy_for(clip[0]) == "streamed"
        runs[grp] = (lambda i, e=e: e.window(list(range(i, i + 6)), clip[i:i + 6], slots=(13, 8, 12)), e.reset)
    with torch.no_grad():
        for run, reset in runs.values():                     # warm-up: relayouts, workspaces, code objects
            _stream_windows(run, 1, reset)
        ms = {k: [] for k in runs}
        for _ in range(args.repeat):                         # alternating
            for k, (run, reset) in runs.items():
                ms[k].append(_stream_windows(run, args.windows, reset))
    ops.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = {"what": "window_720p_f16x3", "frame": list(FRAME), "windows_per_block": args.windows, "blocks_each": args.repeat,
           "ms_per_window": {k: [round(x, 2) for x in v] for k, v in ms.items()}, "ms_median": {k: round(v, 2) for k, v in med.items()}}
    for grp, e in ens.items():
        flips = e.spatial[1:]
        srcs = [[torch.rand(FRAME, device="cuda", generator=g) for _ in range(e.M)] for _ in range(3)]
        legs = {"orient": lambda: ops.ens_orient([clip[0]], None, [flips]), "merge": lambda: ops.ens_merge(srcs, e.flip_of)}
        for fn in legs.values():
            fn()
        glue = B.medians(B.alternating_blocks(legs, 2, 10)[0])
        glue_ms = glue["orient"] + glue["merge"]
        out[grp] = {"M": e.M, "over_M_plain_windows": round(med[grp] / (e.M * med["plain"]), 4),
                    "orient_us": round(glue["orient"] * 1e3, 1), "merge_3_slots_us": round(glue["merge"] * 1e3, 1),
                    "glue_share_of_window": round(glue_ms / med[grp], 5)}
    return out


def leg_small(args):
    import torch
    from bin_amd import ops
    from bin_amd.ensemble import SelfEnsemble
    from bin_amd.utils import util
    net = _net()
    g = torch.Generator(device="cuda").manual_seed(6)
    pads = util.pad_sizes(256, 256)
    n_windows = max(args.windows, 8)
    clip = [util.replicate_pad(torch.rand(1, 3, 256, 256, device="cuda", generator=g), pads) for _ in range(n_windows + 6)]
    ens = {s: SelfEnsemble(net, "hvt", strategy=s) for s in ("batched", "streamed")}
    assert SelfEnsemble(net, "hvt").strategy_for(clip[0]) == "batched"
    runs = {s: (lambda i, e=e: e.window(list(range(i, i + 6)), clip[i:i + 6], slots=(13, 8, 12)), e.reset) for s, e in ens.items()}
    with torch.no_grad():
        for run, reset in runs.values():
            _stream_windows(run, 1, reset)
        ms = {k: [] for k in runs}
        for _ in range(args.repeat):
            for k, (run, reset) in runs.items():
                ms[k].append(_stream_windows(run, n_windows, reset))
    ops.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"what": "small_frames_256_hvt", "padded": list(clip[0].shape), "windows_per_block": n_windows, "blocks_each": args.repeat,
            "ms_per_window": {k: [round(x, 2) for x in v] for k, v in ms.items()},
            "windows_per_s": {k: round(1e3 / v, 2) for k, v in med.items()},
            "batched_over_streamed_windows_per_s": round(med["streamed"] / med["batched"], 3)}


def _markdown(rows):
    lines = ["# Self-ensemble: what the glue costs", "",
             "Written by `tools/bench_ensemble.py` (device events, warmed shapes, the two sides of every comparison alternating in one",
             "process).  Figures of one run on one MI355X; compare within the run only.", ""]
    clock = next((r for r in rows if r.get("what") == "clock"), None)
    if clock:
        lines += [f"Run: {clock['utc']} UTC, {clock['device']}.", ""]
    k = [r for r in rows if "kernel_us_median" in r]
    if k:
        lines += ["## Kernels at [1,3,768,1344]", "",
                  "| call | bytes | kernel us (min .. median .. max) | torch.flip/add us (min .. median .. max) | TB/s | of 8.0 TB/s spec | of 6.29 TB/s copy | kernel / torch | same bits |",
                  "|---|---|---|---|---|---|---|---|---|"]
        for r in k:
            lines.append(f"| {r['what']} | {r['bytes'] / 1e6:.1f} MB | {r['kernel_us_min']} .. {r['kernel_us_median']} .. {r['kernel_us_max']} | "
                         f"{r['torch_us_min']} .. {r['torch_us_median']} .. {r['torch_us_max']} | {r['kernel_TBps']} | {r['share_of_hbm_spec']} | "
                         f"{r['share_of_measured_copy']} | {r['kernel_over_torch']} | {r['bit_identical_to_torch']} |")
        lines.append("")
    w = next((r for r in rows if r.get("what") == "window_720p_f16x3"), None)
    if w:
        lines += ["## Streamed 720p window, f16x3, resident frames", "",
                  f"ms per window (blocks of {w['windows_per_block']} windows, alternating): " +
                  ", ".join(f"{name} {v}" for name, v in w["ms_per_window"].items()) + ".", "",
                  "| group | M | median ms | / (M x plain) | orient us | merge (3 slots) us | glue share of the window |", "|---|---|---|---|---|---|---|"]
        for grp in ("hv", "hvt"):
            e = w[grp]
            lines.append(f"| {grp} | {e['M']} | {w['ms_median'][grp]} | {e['over_M_plain_windows']} | {e['orient_us']} | {e['merge_3_slots_us']} | "
                         f"{e['glue_share_of_window']} |")
        lines += ["", f"Plain window: {w['ms_median']['plain']} ms.", ""]
    s = next((r for r in rows if r.get("what") == "small_frames_256_hvt"), None)
    if s:
        lines += ["## 256x256 frames, hvt", "",
                  f"Windows/s: batched {s['windows_per_s']['batched']}, streamed {s['windows_per_s']['streamed']} "
                  f"(batched / streamed = {s['batched_over_streamed_windows_per_s']}); ms per window per block: {s['ms_per_window']}.", ""]
    lines += ["The PSNR change of the ensemble was not measured: no trained checkpoint exists here, and with initialiser weights the "
              "number means nothing.", ""]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=tuple(LEG_TIMEOUT_S))
    ap.add_argument("--samples", type=int, default=40)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--windows", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--md", default=os.path.join(B.REPO, "profiles", "self_ensemble.md"))
    args = ap.parse_args()
    legs = {"kernels": leg_kernels, "window": leg_window, "small": leg_small}
    if args.leg is not None:
        B.main(__file__, legs, LEG_TIMEOUT_S, args, ())
        return
    rows = []
    for leg in legs:                                         # each leg a child under its own time limit; nothing after a failure
        cmd = ["timeout", "-k", "10", str(LEG_TIMEOUT_S[leg]), sys.executable, os.path.abspath(__file__), "--leg", leg]
        for name in ("samples", "blocks", "windows", "repeat"):
            cmd += ["--" + name, str(getattr(args, name))]
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
    print(json.dumps({"what": "written", "path": args.md}), flush=True)


if __name__ == "__main__":
    main()
