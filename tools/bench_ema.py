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
import statistics

import bench_common as B

LEG_TIMEOUT_S = {"pass": 240, "train": 420}
BACK = 10
DECAY = 0.999


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
    ms = {k: [v / BACK for v in dev] for k, dev in B.alternating_blocks(legs, args.blocks, max(1, args.samples // args.blocks))[0].items()}
    med = B.medians(ms)
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


def leg_train(args):
    import torch
    models = {"off": B.train_model(), "ema": B.train_model(ema_decay=DECAY)}
    assert models["off"].weight_ema is None and type(models["ema"].weight_ema).__name__ == "WeightEMA"
    n = {}
    for m in models.values():
        B.train_block(m, 3, n)                                # warm-up
    ms = {k: [] for k in models}
    for _ in range(args.repeat):                              # alternating
        for k, m in models.items():
            ms[k].append(B.train_block(m, args.train_steps, n))
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
    B.main(__file__, {"pass": leg_pass, "train": leg_train}, LEG_TIMEOUT_S, args, ("samples", "blocks", "repeat", "train_steps"))


if __name__ == "__main__":
    main()
