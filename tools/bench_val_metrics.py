"""Cost of validation scoring on the device (binhip_frame_score, `train.val_metrics: device`).  Needs no files on disk; prints
one JSON line per measurement.

  * kernel: ops.frame_scores on the 14 pairs of a window (targets repeated as bin_model.get_info repeats them) against the path
    one could assemble from the u8 kernels: 28 binhip_frame_to_u8 launches straight into two preallocated [14,H,W,3] stacks
    (no extra copy) + ops.image_scores(n = 14).  hipEvents in one process, after a warm-up, the two legs alternating, median of
    --reps repetitions; random frames at every size, and the outputs of bin_stage4 on one synthetic 256 x 256 validation window.
  * validate: wall time per window of train.validate() with val_metrics host and device on the same --windows synthetic windows
    (model warm, the modes alternating --repeat times), and the share of it the forward pass (feed_data + test + get_loss,
    synchronised) takes.
usage: python tools/bench_val_metrics.py [--sizes 128x128,256x256,352x640] [--reps 30] [--windows 8] [--repeat 2] [--kernel_only]"""
import argparse
import json
import logging
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

ORDER = [2, 4, 6, 8, 3, 5, 7, 4, 6, 5, 10, 9, 8, 7]         # bin_model.get_info: the target of each of the 14 outputs


def _random_window(h, w):
    import torch
    g = torch.Generator().manual_seed(1)
    gt = {k: torch.rand((3, h, w), generator=g).cuda() for k in range(2, 11)}
    xs = [(gt[k] + 0.03 * torch.randn((3, h, w), generator=g).cuda()) for k in ORDER]
    return xs, [gt[k] for k in ORDER]


def _composed(xs, ys, stacks):
    import ctypes as C
    import torch
    from bin_amd import _lib as L
    from bin_amd import ops
    lib, s = L.lib(), C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, w = xs[0].shape[-2:]
    for frames, stack in zip((xs, ys), stacks):
        for i, f in enumerate(frames):
            L.check(lib.binhip_frame_to_u8(C.c_void_p(f.data_ptr()), h, w, 0, 0, h, w, C.c_void_p(stack[i].data_ptr()), s), "frame_to_u8")
    return ops.image_scores(stacks[0], stacks[1])


def kernel_times(xs, ys, reps, what):
    import torch
    from bin_amd import ops
    h, w = xs[0].shape[-2:]
    stacks = [torch.empty((len(xs), h, w, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    legs = {"fused": lambda: ops.frame_scores(xs, ys), "composed": lambda: _composed(xs, ys, stacks)}
    a, b = legs["fused"]().cpu(), legs["composed"]().cpu()
    assert torch.equal(a[:, :2], b[:, :2]) and float((a[:, 2:] - b[:, 2:]).abs().max()) <= 1e-9
    for _ in range(10):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, f in legs.items():                             # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: statistics.median(v) for k, v in ms.items()}
    return {"what": what, "size": f"{h}x{w}", "pairs": len(xs), "reps": reps,
            "fused_ms_median": round(med["fused"], 4), "fused_ms_min": round(min(ms["fused"]), 4),
            "composed_ms_median": round(med["composed"], 4), "composed_ms_min": round(min(ms["composed"]), 4),
            "fused_over_composed": round(med["fused"] / med["composed"], 4),
            "note": "hipEvents around the whole call: fused = 2 launches + 2 small copies; composed = 28 frame_to_u8 launches into "
                    "preallocated stacks + image_scores (2 launches + 2 small copies)"}


def _model(tmp):
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    m = create_model(_opt(tmp, None))
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    return m


def _opt(tmp, metrics):
    from bin_amd.options import options as option
    train = {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "lr_G": 1e-4, "beta1": 0.9,
             "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000], "restarts": None, "restart_weights": None,
             "lr_gamma": 0.5, "clear_state": False}
    if metrics:
        train["val_metrics"] = metrics
    return option.dict_to_nonedict({
        "model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
        "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
        "path": {"pretrain_model_G": None, "strict_load": True, "models": tmp, "training_state": tmp, "val_images": tmp},
        "train": train})


def _windows(n, size):
    from bin_amd.data import create_dataset
    ds = create_dataset({"mode": "synthetic_texture", "name": "v", "phase": "val", "LQ_size": [3, size, size], "num_windows": n,
                         "seed": None, "max_speed": None})
    out = []
    for i in range(n):
        s = ds[i]
        out.append({"LQs": s["LQs"][None].cuda(), "GTenh": s["GTenh"][None].cuda(), "GTinp": s["GTinp"][None].cuda(),
                    "key": [s["key"]]})
    return out


def validate_times(model, windows, repeat, tmp):
    import torch
    from bin_amd import train
    log = logging.getLogger("bench_val_metrics")

    def forward_only():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in windows:
            model.feed_data(b)
            model.test()
            with torch.no_grad():
                loss, _ = model.get_loss(ret=1)
            loss.item()
        return (time.perf_counter() - t0) / len(windows)

    def one(mode):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train.validate(model, windows, 1, _opt(tmp, mode), log)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / len(windows)
    forward_only()
    one("device")                                             # warm
    fwd, t = [], {"host": [], "device": []}
    for _ in range(repeat):
        fwd.append(forward_only())
        for mode in t:                                        # alternating
            t[mode].append(one(mode))
    f = statistics.median(fwd)
    res = {"what": "validate", "size": "x".join(str(v) for v in windows[0]["LQs"].shape[-2:]), "windows": len(windows),
           "repeat": repeat, "forward_ms_per_window": round(f * 1e3, 3)}
    for mode, v in t.items():
        m = statistics.median(v)
        res[f"{mode}_ms_per_window"] = round(m * 1e3, 3)
        res[f"{mode}_forward_share"] = round(f / m, 4)
    res["host_over_device"] = round(statistics.median(t["host"]) / statistics.median(t["device"]), 2)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128x128,256x256,352x640")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--windows", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--kernel_only", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_val_metrics needs a GPU"
    assert args.reps >= 20
    print(json.dumps({"what": "clock", "utc": time.strftime("%Y-%m-%d %H:%M:%S", time.gmtime()),
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    for s in args.sizes.split(","):
        h, w = (int(v) for v in s.split("x"))
        print(json.dumps(kernel_times(*_random_window(h, w), args.reps, "kernel_random")), flush=True)
    with tempfile.TemporaryDirectory(prefix="bin_amd_val_") as tmp:
        model = _model(tmp)
        windows = _windows(args.windows, 256)
        model.feed_data(windows[0])
        model.test()
        _, gt = model.get_info(mode=1)
        xs, ys = [model.Ft_p[i][0].float().contiguous() for i in range(14)], [g[0].float().contiguous() for g in gt]
        print(json.dumps(kernel_times(xs, ys, args.reps, "kernel_validation_window")), flush=True)
        if not args.kernel_only:
            print(json.dumps(validate_times(model, windows, args.repeat, tmp)), flush=True)


if __name__ == "__main__":
    main()
