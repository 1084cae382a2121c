"""Cost of the gradient guard (bin_amd.optim.GradGuard over bingrad_norm / bingrad_scale; `train.grad_clip`, `train.skip_bad_steps`)
on bin_stage4's 540 gradients (11.44 M floats, 45.77 MB).  Needs no files on disk; prints one JSON line per measurement.

  * pass  (one process): the norm pass over the 540 gradients as separate tensors and as views into FlatGradAllReduce's flat buffer,
    and the scale pass at coef == 1 and at coef < 1 — library calls on a prebuilt row table, BACK calls back to back between one
    hipEvent pair so that the stream stays busy — against a device-to-device copy of the same 45.77 MB timed the same way in the same
    process (the yardstick of profiles/optimizer_step.md; the norm reads the bytes once, the copy reads and writes them).  Beside it
    the host and device time of GradGuard.apply() and of torch.nn.utils.clip_grad_norm_ on the same gradients, stream idle before
    each call.
  * train (one process): the 8 x 256^2 f16x3 training step of bench.py's training leg, `train.optimizer: hip`, in alternating
    same-box pairs: grad_clip on against off, and skip_bad_steps on against off, --repeat pairs each.
Without --leg, each leg runs as a child process under its own `timeout`, and nothing is started after a leg that failed.
usage: python tools/bench_gradguard.py [--leg pass|train] [--steps 60] [--blocks 4] [--repeat 3] [--train_steps 10]"""
import argparse
import statistics

import bench_common as B

LEG_TIMEOUT_S = {"pass": 240, "train": 500}


def leg_pass(args):
    import ctypes as C
    import torch
    from bin_amd import _lib as L, ops
    from bin_amd.models.bin_model import FlatGradAllReduce
    from bin_amd.optim import GradGuard
    from bin_amd.weights import canonical_weights
    gen = torch.Generator().manual_seed(1)
    shapes = [v.shape for v in canonical_weights(0).values()]
    params = {k: [torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes] for k in ("separate", "flat")}
    for p in params["separate"]:
        p.grad = (torch.randn(p.shape, generator=gen) * 1e-3).cuda()
    sync = FlatGradAllReduce(params["flat"])
    sync.attach()
    sync.flat.copy_(torch.cat([p.grad.reshape(-1) for p in params["separate"]]))
    numel = sync.numel
    lib, stream = L.gradlib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = {k: ops.grad_rows([p.grad for p in ps]) for k, ps in params.items()}
    ws = torch.empty(rows["flat"].workspace_bytes // 8, dtype=torch.float64, device="cuda")
    rec = {k: ops.grad_record("cuda") for k in ("one", "clip")}
    ops.grad_norm(rows["separate"], ws, rec["one"], 0.0)
    torch.cuda.synchronize()
    norm = ops.grad_record_read(rec["one"].cpu()).norm
    torch.cuda.synchronize()
    # a record whose coef is just below 1 (max_norm a millionth under the norm): every scale call with it multiplies again
    ops.grad_norm(rows["separate"], ws, rec["clip"], norm * (1.0 - 2.0 ** -20))
    torch.cuda.synchronize()
    assert 0.99999 < ops.grad_record_read(rec["clip"].cpu()).coef < 1.0
    src, dst = torch.empty(numel, device="cuda").normal_(), torch.empty(numel, device="cuda")
    BACK = 10

    def norm_call(k):
        def f():
            for _ in range(BACK):
                L.check(lib.bingrad_norm(rows[k].table, rows[k].n, 0.0, None, 0, C.c_void_p(ws.data_ptr()), C.c_void_p(rec["one"].data_ptr()),
                                         stream), "grad_norm")
        return f

    def scale_call(k, r):
        def f():
            for _ in range(BACK):
                L.check(lib.bingrad_scale(rows[k].table, rows[k].n, C.c_void_p(rec[r].data_ptr()), stream), "grad_scale")
        return f

    def copy():
        for _ in range(BACK):
            dst.copy_(src)
    calls = {"norm_separate": norm_call("separate"), "norm_flat": norm_call("flat"), "scale_coef1": scale_call("separate", "one"),
             "scale_clipping": scale_call("separate", "clip"), "scale_clipping_flat": scale_call("flat", "clip"), "copy": copy}
    # GradGuard.apply() against torch.nn.utils.clip_grad_norm_, both CLIPPING on every timed call: the gradients are restored from a
    # saved copy (untimed) before each call, so the norm is twice the cap every time and both multiply all 540 tensors
    plist = params["separate"]
    saved = [p.grad.clone() for p in plist]

    def restore():
        torch._foreach_copy_([p.grad for p in plist], saved)
    ops.grad_norm(rows["separate"], ws, rec["one"], 0.0)
    torch.cuda.synchronize()
    norm = ops.grad_record_read(rec["one"].cpu()).norm         # the scale calls above shrank the gradients a little
    guard = GradGuard(plist, max_norm=0.5 * norm)
    guard_skip = GradGuard(plist, max_norm=0.0, skip_bad_steps=2)
    host_calls = {"guard_apply_clip": guard.apply, "guard_apply_skip": guard_skip.apply,
                  "torch_clip_grad_norm": lambda: torch.nn.utils.clip_grad_norm_(plist, 0.5 * norm)}
    for f in calls.values():
        f()
    for f in host_calls.values():
        restore()
        f()
    assert 0.49 < guard.last.coef < 0.51
    both, host = B.alternating_blocks({**calls, **host_calls}, args.blocks, max(1, args.steps // args.blocks),
                                      before={k: restore for k in host_calls})
    ms = {k: [v / BACK for v in both[k]] for k in calls}
    dev = {k: both[k] for k in host_calls}
    med = B.medians(ms)
    nbytes = 4 * numel
    out = {"what": "grad_guard_passes", "tensors": len(shapes), "elements": numel, "bytes": nbytes, "calls_timed_each": len(ms["copy"]),
           "blocks": args.blocks, "norm_of_the_test_gradients": norm}
    for k in calls:
        out[k + "_ms_median"], out[k + "_ms_min"] = round(med[k], 4), round(min(ms[k]), 4)
    for k in calls:
        if k != "copy":
            out[k + "_over_copy"] = round(med[k] / med["copy"], 4)
    out["norm_flat_TBps_read"] = round(nbytes / (med["norm_flat"] * 1e-3) / 1e12, 3)
    out["copy_TBps_read_plus_written"] = round(2 * nbytes / (med["copy"] * 1e-3) / 1e12, 3)
    for k in host_calls:
        out[k + "_host_ms_median"] = round(statistics.median(host[k]), 4)
        out[k + "_device_ms_median"] = round(statistics.median(dev[k]), 4)
    out["note"] = ("norm_* / scale_* / copy: 10 calls back to back per hipEvent pair, per call; norm = 5 launches of grad_sumsq_kernel + "
                   "grad_final_kernel; copy: a device-to-device copy of the same 4 B per element (read + written); guard_* / torch_*: one "
                   "call per event pair with the stream idle before it and the gradients restored to twice the cap (untimed) before "
                   "every call, so guard_apply_clip and torch_clip_grad_norm both clip all 540 tensors each time; guard_apply_skip does "
                   "not clip and includes its event wait; host = wall time of the call, device = the event pair")
    return out


def leg_train(args):
    import torch
    out = {"what": "training_step", "workload": "8 x 256^2 crops, f16x3, fwd + loss + bwd + guard + Adam (train.optimizer: hip)",
           "steps_per_block": args.train_steps, "pairs": args.repeat}
    off = B.train_model()
    assert off.grad_guard is None
    n = {}

    def block(m, steps):
        return B.train_block(m, steps, n)
    block(off, 3)                                             # warm-up
    for name, train in (("clip", {"grad_clip": 1.0}), ("skip", {"skip_bad_steps": 5})):
        on = B.train_model(**train)                            # two models alive at a time
        assert on.grad_guard is not None and (on.grad_guard.max_norm, on.grad_guard.skip_bad_steps) == (train.get("grad_clip", 0.0), train.get("skip_bad_steps", 0))
        block(on, 3)
        ms = {"on": [], "off": []}
        for _ in range(args.repeat):                          # alternating same-box pairs: on, off, on, off, ...
            ms["on"].append(block(on, args.train_steps))
            ms["off"].append(block(off, args.train_steps))
        out[f"{name}_on_ms_per_step"] = [round(v, 3) for v in ms["on"]]
        out[f"{name}_off_ms_per_step"] = [round(v, 3) for v in ms["off"]]
        out[f"{name}_on_ms_median"] = round(statistics.median(ms["on"]), 3)
        out[f"{name}_off_ms_median"] = round(statistics.median(ms["off"]), 3)
        out[f"{name}_on_minus_off_ms"] = round(statistics.median(ms["on"]) - statistics.median(ms["off"]), 3)
        g = on.grad_guard.last
        out[f"{name}_last_norm_coef_flags"] = [g.norm, g.coef, g.flags]
        out[f"{name}_skipped_steps"] = on.grad_guard.skipped_total
        del on
        torch.cuda.empty_cache()
    out["note"] = "wall time of a block of steps between device synchronisations; grad_clip: 1.0, skip_bad_steps: 5"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("pass", "train"))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--train_steps", type=int, default=10)
    args = ap.parse_args()
    assert args.steps >= 50, "median of at least 50 calls"
    B.main(__file__, {"pass": leg_pass, "train": leg_train}, LEG_TIMEOUT_S, args, ("steps", "blocks", "repeat", "train_steps"))


if __name__ == "__main__":
    main()
