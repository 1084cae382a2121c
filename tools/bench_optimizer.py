"""Cost of the Adam update on bin_stage4's 540 parameters (11.44 M floats) with torch.optim.Adam (its default path) and with
bin_amd.optim.Adam (binopt_adam_step, `train.optimizer: hip`).  Needs no files on disk; prints one JSON line per measurement.

  * step  (one process): device time of optimizer.step() with gradients present — hipEvent pairs on the stream, after a warm-up,
    blocks of the two classes alternating, median over all timed steps; the host time of the call beside it; the kernel's rate as
    28 B x elements / time, and that rate as a fraction of what a device copy of the same number of bytes (half read, half
    written) reaches in the same run on the same box — the bound used here, not a data-sheet figure.  Before timing, the two
    classes' parameters after the same steps are compared.
  * train (one process): the 8 x 256^2 f16x3 training step of bench.py's training leg with each optimizer, blocks alternating,
    --repeat repetitions each.
Without --leg, each leg runs as a child process under its own `timeout`, and nothing is started after a leg that failed.
usage: python tools/bench_optimizer.py [--leg step|train] [--steps 60] [--blocks 4] [--repeat 3] [--train_steps 10]"""
import argparse
import statistics

import bench_common as B

LEG_TIMEOUT_S = {"step": 240, "train": 420}


def _params_and_grads(seed):
    import torch
    from bin_amd.weights import canonical_weights
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.from_numpy(v).cuda()) for v in canonical_weights(0).values()]
    for p in params:
        p.grad = (torch.randn(p.shape, generator=g) * 1e-3).cuda()
    return params


def leg_step(args):
    import torch
    from bin_amd.optim import Adam
    kw = dict(lr=1e-4, betas=(0.9, 0.99))
    sets = {"torch": _params_and_grads(1), "hip": _params_and_grads(1)}
    opts = {"torch": torch.optim.Adam(sets["torch"], **kw), "hip": Adam(sets["hip"], **kw)}
    numel = sum(p.numel() for p in sets["hip"])
    for _ in range(5):                                        # warm-up; and the same function: the parameters after five steps are compared
        for o in opts.values():
            o.step()
    torch.cuda.synchronize()
    worst = max(float((a.detach() - b.detach()).abs().max()) for a, b in zip(sets["torch"], sets["hip"]))
    # the bound: a device copy that moves the same 28 B per element (14 read + 14 written)
    words = numel * 7 // 2
    src, dst = torch.empty(words, dtype=torch.float32, device="cuda").normal_(), torch.empty(words, dtype=torch.float32, device="cuda")
    for _ in range(5):
        dst.copy_(src)
    # the kernel alone: the library call on a prebuilt row table (9 launches), BACK back-to-back calls between one event pair so that
    # the stream stays busy and the host's launch time hides behind the device; the copy is timed the same way
    from bin_amd import ops
    st = opts["hip"].state
    table = ops.adam_rows(len(sets["hip"]))
    for i, p in enumerate(sets["hip"]):
        ops.adam_row(table, i, p, p.grad, st[p]["exp_avg"], st[p]["exp_avg_sq"], 1e-4, 1.0)
    # ... and the same bytes as ONE row (one launch instead of nine): what splitting into launches of 64 rows costs
    flat = [torch.zeros(numel, device="cuda") for _ in range(4)]
    flat[1].normal_(std=1e-3)
    one = ops.adam_rows(1)
    ops.adam_row(one, 0, *flat, 1e-4, 1.0)
    import ctypes as C
    from bin_amd import _lib as L
    lib, stream = L.optlib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    BACK = 10

    def kernel(t=table, n=len(sets["hip"])):
        for _ in range(BACK):
            L.check(lib.binopt_adam_step(t, n, 0.9, 0.99, 1e-8, 0.0, stream), "adam_step")

    def kernel_one_row():
        kernel(one, 1)

    def copy():
        for _ in range(BACK):
            dst.copy_(src)
    kernel()
    kernel_one_row()
    calls = {"torch": opts["torch"].step, "hip": opts["hip"].step, "kernel": kernel, "kernel_one_row": kernel_one_row, "copy": copy}
    ms, host = B.alternating_blocks(calls, args.blocks, max(1, args.steps // args.blocks))
    for k in ("kernel", "kernel_one_row", "copy"):
        ms[k] = [v / BACK for v in ms[k]]
    med = B.medians(ms)
    nbytes = 28 * numel
    rate = {k: nbytes / (med[k] * 1e-3) / 1e12 for k in med}
    return {"what": "optimizer_step", "tensors": len(sets["hip"]), "elements": numel, "bytes_per_step": nbytes,
            "steps_timed_each": len(ms["hip"]), "blocks": args.blocks,
            "torch_ms_median": round(med["torch"], 4), "torch_ms_min": round(min(ms["torch"]), 4),
            "hip_ms_median": round(med["hip"], 4), "hip_ms_min": round(min(ms["hip"]), 4),
            "hip_over_torch": round(med["hip"] / med["torch"], 4),
            "torch_host_ms_median": round(statistics.median(host["torch"]), 4),
            "hip_host_ms_median": round(statistics.median(host["hip"]), 4),
            "kernel_ms_median": round(med["kernel"], 4), "kernel_ms_min": round(min(ms["kernel"]), 4),
            "kernel_one_row_ms_median": round(med["kernel_one_row"], 4), "kernel_one_row_TBps": round(rate["kernel_one_row"], 3),
            "copy_ms_median": round(med["copy"], 4), "copy_TBps": round(rate["copy"], 3),
            "kernel_TBps": round(rate["kernel"], 3), "kernel_fraction_of_copy_rate": round(rate["kernel"] / rate["copy"], 4),
            "max_abs_parameter_difference_after_5_steps": worst,
            "note": "torch / hip: hipEvents around optimizer.step() with the stream idle before it, so the host's share of the call is "
                    "inside (hip: 9 launches of adam_step_kernel; torch: its default foreach path); kernel: binopt_adam_step on a prebuilt "
                    "table, 10 calls back to back per event pair; kernel_one_row: the same number of elements as one row = one launch; copy: a device-to-device copy of 14 B per element read + 14 B written, "
                    "timed the same way"}


def leg_train(args):
    import torch
    models = {k: B.train_model(optimizer=k) for k in ("torch", "hip")}
    assert type(models["hip"].optimizer_G).__module__ == "bin_amd.optim" and type(models["torch"].optimizer_G) is torch.optim.Adam
    n = {}
    for m in models.values():
        B.train_block(m, 3, n)                                # warm-up
    ms = {k: [] for k in models}
    for _ in range(args.repeat):                              # alternating
        for k, m in models.items():
            ms[k].append(B.train_block(m, args.train_steps, n))
    losses = {k: float(models[k].loss) for k in models}
    return {"what": "training_step", "workload": "8 x 256^2 crops, f16x3, fwd + loss + bwd + Adam", "steps_per_block": args.train_steps,
            "torch_ms_per_step": [round(v, 3) for v in ms["torch"]], "hip_ms_per_step": [round(v, 3) for v in ms["hip"]],
            "torch_ms_median": round(statistics.median(ms["torch"]), 3), "hip_ms_median": round(statistics.median(ms["hip"]), 3),
            "hip_over_torch": round(statistics.median(ms["hip"]) / statistics.median(ms["torch"]), 4),
            "last_loss": losses, "note": "wall time of a block of steps between device synchronisations, blocks alternating"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("step", "train"))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--train_steps", type=int, default=10)
    args = ap.parse_args()
    assert args.steps >= 50, "median of at least 50 steps"
    B.main(__file__, {"step": leg_step, "train": leg_train}, LEG_TIMEOUT_S, args, ("steps", "blocks", "repeat", "train_steps"))


if __name__ == "__main__":
    main()
