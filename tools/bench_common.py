"""What tools/bench_optimizer.py, bench_gradguard.py and bench_ema.py share: hipEvent timing of a call, blocks of several calls
alternating, the training model of bench.py's training leg, and the runner that starts each leg as a child process under its own
`timeout` and starts nothing after a leg that failed."""
import json
import os
import statistics
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def timed(fn, n, before=None):
    """n calls of fn, each between a hipEvent pair on the current stream with the stream idle before it (`before`, untimed, runs
    first) -> (device ms per call, host ms per call)."""
    import torch
    dev, host = [], []
    for _ in range(n):
        if before is not None:
            before()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        host.append((time.perf_counter() - t0) * 1e3)
        e1.synchronize()
        dev.append(e0.elapsed_time(e1))
    return dev, host


def alternating_blocks(calls, blocks, per_block, before=None):
    """`blocks` rounds over `calls` ({name: fn}, in their order), `per_block` timed calls of each per round, so that drift of the box
    falls on all of them alike -> ({name: device ms of every call}, {name: host ms}).  `before`: {name: untimed fn before each call}."""
    dev, host = {k: [] for k in calls}, {k: [] for k in calls}
    for _ in range(blocks):
        for k, fn in calls.items():
            d, h = timed(fn, per_block, (before or {}).get(k))
            dev[k] += d
            host[k] += h
    return dev, host


def medians(ms):
    return {k: statistics.median(v) for k, v in ms.items()}


def train_model(batch=8, size=256, **train):
    """The training model of bench.py's training leg (8 x 256^2, f16x3, `train.optimizer: hip`) with the given train options on top,
    one synthetic batch fed (`batch` x `size`^2 where another shape is asked for)."""
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
    opt["train"].update(train)
    m = create_model(opt)
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    g = torch.Generator().manual_seed(7)
    B, S = batch, size
    m.feed_data({"LQs": torch.rand(B, 6, 3, S, S, generator=g), "GTenh": torch.rand(B, 6, 3, S, S, generator=g),
                 "GTinp": torch.rand(B, 5, 3, S, S, generator=g)})
    return m


def train_block(model, steps, counter):
    """Wall ms per step of `steps` training steps of `model` between device synchronisations; `counter`: {id(model): steps so far}."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        counter[id(model)] = counter.get(id(model), 0) + 1
        model.optimize_parameters(counter[id(model)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / steps


def main(script, legs, leg_timeout_s, args, options):
    """With --leg: that leg in this process, a clock line and the leg's JSON line.  Without: every leg of `legs` ({name: fn(args)}) as
    a child process under its own `timeout`, the `options` of `args` passed on; nothing is started after a leg that failed."""
    if args.leg is None:
        for leg in legs:
            cmd = ["timeout", "-k", "10", str(leg_timeout_s[leg]), sys.executable, os.path.abspath(script), "--leg", leg]
            for name in options:
                cmd += ["--" + name, str(getattr(args, name))]
            rc = subprocess.run(cmd, cwd=REPO).returncode
            if rc != 0:
                print(json.dumps({"what": "failed", "leg": leg, "exit_status": rc}), flush=True)
                sys.exit(rc)
        return
    import torch
    assert torch.cuda.is_available(), os.path.splitext(os.path.basename(script))[0] + " needs a GPU"
    print(json.dumps({"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    print(json.dumps(legs[args.leg](args)), flush=True)
