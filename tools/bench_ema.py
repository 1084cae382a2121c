"""Cost of the weight average (`train.ema_decay`, bin_amd.optim.WeightEMA over binema_step) on bin_stage4's 540 parameters
(11.44 M floats).  Needs no files on disk; prints one JSON line per measurement.

  * pass  (one process): the averaging pass alone — binema_step on the class's own row table (540 rows, the shadows in their flat
    buffer), BACK calls back to back between one hipEvent pair so that the stream stays busy, after a warm-up, blocks alternating
    with the two yardsticks, median over all timed samples.  Yardstick 1: a device-to-device copy that moves the same 12 B per
    element (6 read + 6 written), timed the same way in the same process.  Yardstick 2: torch._foreach_lerp_ on the same tensors
    with the same weight, timed the same way.  Before timing, one pass of each from the same state is compared.
  * train (one process): the 8 x 256^2 f16x3 training step of bench.py's training leg with and without `ema_decay`, blocks
    alternating, --repeat repetitions each.
Without --leg, each leg runs as a child process under its own `timeout`, and nothing is started after a leg that failed.  No frame
or step figure printed here is comparable across boxes: compare within one run.
usage: python tools/bench_ema.py [--leg pass|train] [--samples 60] [--blocks 4] [--repeat 3] [--train_steps 10]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

LEG_TIMEOUT_S = {"pass": 240, "train": 420}
BACK = 10
DECAY = 0.999


def _timed(fn, n):
    """n calls of fn, each between a hipEvent pair on the current stream -> device ms per call."""
    import torch
    dev = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
    return dev


def leg_pass(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    from bin_amd.optim import WeightEMA
    from bin_amd.weights import canonical_weights
    params = [torch.nn.Parameter(torch.from_numpy(v).cuda()) for v in canonical_weights(0).values()]
    numel = sum(p.numel() for p in params)
    ema = WeightEMA(params, DECAY)
    with torch.no_grad():
        for p in params:
            p.add_(torch.randn_like(p) * 1e-3)
    # the same function: one pass of each from the same state
    twins = [e.clone() for e in ema.shadow]
    plain = [p.detach() for p in params]
    ema.update()
    torch._foreach_lerp_(twins, plain, 1.0 - DECAY)
    torch.cuda.synchronize()
    worst = max(float((a - b).abs().max()) for a, b in zip(ema.shadow, twins))
    # yardstick 1: a device copy that moves the same 12 B per element (6 read + 6 written)
    words = numel * 3 // 2
    src, dst = torch.empty(words, dtype=torch.float32, device="cuda").normal_(), torch.empty(words, dtype=torch.float32, device="cuda")
    _, table = ema._tables[params[0].device]
    n = len(params)
    lib, stream = L.emalib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    launches = -(-n // L.EMA_MAX_TENSORS)

    def kernel():
        for _ in range(BACK):
            L.check(lib.binema_step(table, n, DECAY, stream), "ema_step")

    def lerp():
        for _ in range(BACK):
            torch._foreach_lerp_(twins, plain, 1.0 - DECAY)

    def copy():
        for _ in range(BACK):
            dst.copy_(src)

    def update():
        for _ in range(BACK):
            ema.update()
    legs = {"kernel": kernel, "update": update, "foreach_lerp": lerp, "copy": copy}
    for fn in legs.values():                                  # warm-up
        fn()
        fn()
    ms = {k: [] for k in legs}
    per_block = max(1, args.samples // args.blocks)
    for _ in range(args.blocks):                              # alternating blocks
        for k, fn in legs.items():
            ms[k] += [v / BACK for v in _timed(fn, per_block)]
    med = {k: statistics.median(v) for k, v in ms.items()}
    nbytes = 12 * numel
    rate = {k: nbytes / (med[k] * 1e-3) / 1e12 for k in med}
    out = {"what": "ema_pass", "tensors": n, "elements": numel, "bytes_per_pass": nbytes, "launches_per_pass": launches,
           "calls_per_event_pair": BACK, "samples_each": len(ms["kernel"]), "blocks": args.blocks}
    for k in legs:
        out[f"{k}_us_median"] = round(med[k] * 1e3, 2)
        out[f"{k}_us_min"] = round(min(ms[k]) * 1e3, 2)
        out[f"{k}_TBps"] = round(rate[k], 3)
    out.update({"kernel_over_foreach_lerp": round(med["kernel"] / med["foreach_lerp"], 4),
                "kernel_over_copy": round(med["kernel"] / med["copy"], 4),
                "not_slower_than_foreach_lerp": bool(med["kernel"] <= med["foreach_lerp"]),
                "max_abs_difference_to_foreach_lerp_after_one_pass": worst,
                "note": "kernel: binema_step on WeightEMA's row table; update: WeightEMA.update() (the table check, the call and the "
                        "version bump); foreach_lerp: torch._foreach_lerp_ on the same 540 tensors; copy: a device-to-device copy of "
                        "6 B per element read + 6 B written; each 10 calls back to back per event pair, per-call figures"})
    return out


def _train_model(ema_decay):
    """The training model of bench.py's training leg (8 x 256^2, f16x3) with `train.ema_decay` set or absent, one synthetic batch fed."""
    import tempfile
    import torch
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    tmp = tempfile.mkdtemp()
    opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3", "backward_precision": None},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": tmp, "training_state": tmp},
           "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "optimizer": "hip",
                     "lr_G": 1e-4, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    if ema_decay:
        opt["train"]["ema_decay"] = ema_decay
    m = create_model(opt)
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    g = torch.Generator().manual_seed(7)
    B, S = 8, 256
    m.feed_data({"LQs": torch.rand(B, 6, 3, S, S, generator=g), "GTenh": torch.rand(B, 6, 3, S, S, generator=g),
                 "GTinp": torch.rand(B, 5, 3, S, S, generator=g)})
    return m


def leg_train(args):
    import torch
    models = {"off": _train_model(None), "ema": _train_model(DECAY)}
    assert models["off"].weight_ema is None and type(models["ema"].weight_ema).__name__ == "WeightEMA"
    n = {k: 0 for k in models}

    def block(k, steps):
        m = models[k]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            n[k] += 1
            m.optimize_parameters(n[k])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps
    for k in models:
        block(k, 3)                                           # warm-up
    ms = {k: [] for k in models}
    for _ in range(args.repeat):                              # alternating
        for k in models:
            ms[k].append(block(k, args.train_steps))
    losses = {k: float(models[k].loss.detach()) for k in models}
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"what": "training_step", "workload": "8 x 256^2 crops, f16x3, fwd + loss + bwd + Adam (hip)", "steps_per_block": args.train_steps,
            "off_ms_per_step": [round(v, 3) for v in ms["off"]], "ema_ms_per_step": [round(v, 3) for v in ms["ema"]],
            "off_ms_median": round(med["off"], 3), "ema_ms_median": round(med["ema"], 3),
            "ema_minus_off_ms": round(med["ema"] - med["off"], 3), "ema_over_off": round(med["ema"] / med["off"], 4),
            "last_loss": losses, "note": "wall time of a block of steps between device synchronisations, blocks alternating"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("pass", "train"))
    ap.add_argument("--samples", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--train_steps", type=int, default=10)
    args = ap.parse_args()
    assert args.samples >= 50, "median of at least 50 samples"
    if args.leg is None:
        for leg, limit in LEG_TIMEOUT_S.items():              # each GPU step under its own time limit; stop at the first failure
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--leg", leg, "--samples", str(args.samples),
                   "--blocks", str(args.blocks), "--repeat", str(args.repeat), "--train_steps", str(args.train_steps)]
            rc = subprocess.run(cmd, cwd=REPO).returncode
            if rc != 0:
                print(json.dumps({"what": "failed", "leg": leg, "exit_status": rc}), flush=True)
                sys.exit(rc)
        return
    import torch
    assert torch.cuda.is_available(), "bench_ema needs a GPU"
    print(json.dumps({"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    print(json.dumps(leg_pass(args) if args.leg == "pass" else leg_train(args)), flush=True)


if __name__ == "__main__":
    main()
