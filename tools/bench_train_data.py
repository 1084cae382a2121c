"""Training fed from the Adobe folder layout: host loader vs device frame cache (bin_amd/data/device_cache.py).

Generates a synthetic Adobe tree of 352x640 PNG frames (tests/host_fixtures.make_adobe_tree) under a temporary directory and
reports, as one JSON line:
  host_loader      ms per batch of create_dataloader at n_workers 3 and 16: consumed and discarded, then with feed_data
  device_loader    ms per batch of the device-cache loader (table, upload, one gather launch, synchronised)
  train_step       optimize_parameters ms per step (f16x3, 8 x 256^2) fed by each loader and by a resident batch
                   (--warmup steps, then --steps timed ones, each synchronised)
  cache            build seconds and arena bytes
  gather_kernel    device time per gather launch from events around --kernel-launches back-to-back launches, against
                   the HBM bound (3 B read + 12 B written per output pixel at 6.3 TB/s)

    python tools/bench_train_data.py                      # everything
    python tools/bench_train_data.py --only kernel        # cache + gather launches only (for rocprofv3 --kernel-trace --stats)

--blur_window N is a run of its own (the default run stays what it is): a sharp-only tree (tests/blur_cases.make_sharp_tree,
--clips clips of --sharp-files consecutive frames) whose blurry folders tools/make_blur_folder.py writes for window N, and
  train_step       optimize_parameters ms per step fed by today's device-cache loader (blurry PNGs in the arena) and by the
                   synthesising one (`blur_window: N`, sharp frames only), alternating, --rounds times each
  cache            build seconds and arena bytes of both
  gather_kernel    binhip_gather_windows_blur launches at the exposures --kernel-windows (default 1, N, 33) against the HBM
                   bound counted without any cache reuse (3 L B read + 12 B written per blurry pixel, 15 B per other pixel)

    python tools/bench_train_data.py --blur_window 11
    python tools/bench_train_data.py --blur_window 11 --only kernel --kernel-windows 33    # for rocprofv3, one exposure per run

--blur_window N --blur_gamma G [--blur_noise READ,SHOT] compares the exposure path (libbinexpose.so, `blur_gamma` / `blur_noise`)
with the `blur_window: N` path instead: no blurry folders are written, gather_kernel also times binexpose_gather without and
with noise at each exposure, and train_step alternates the `blur_window: N` loader with the one that has the options on top.

    python tools/bench_train_data.py --blur_window 11 --blur_gamma 2.2 --blur_noise 0.004,0.0004
"""
import argparse
import json
import os
import random
import shutil
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
CROP = 256


def make_tree(root, clips, n_blur):
    from host_fixtures import make_adobe_tree
    # a clip of n blurry frames gives n - 5 windows (the first clip's list omits its last frame: one fewer)
    spec = tuple((f"clip{c:02d}", 8 * c, n_blur) for c in range(clips))
    return make_adobe_tree(root, clips=spec, hw=(352, 640))


def dataset(root):
    from bin_amd.data import create_dataset
    random.seed(0)
    return create_dataset({"mode": "BIN", "name": "train", "dataroot_GT": root, "dataroot_LQ": root,
                           "LQ_size": [3, CROP, CROP], "data_type": "img", "phase": "train"})


def host_loader(ds, batch, workers, ratio):
    from bin_amd.data import create_dataloader
    from bin_amd.data.data_sampler import DistIterSampler
    sampler = DistIterSampler(ds, 1, 0, ratio)          # `ratio` passes over the windows without restarting the workers
    loader = create_dataloader(ds, {"phase": "train", "batch_size": batch, "n_workers": workers},
                               {"dist": False, "gpu_ids": [0]}, sampler)
    if workers:
        # fresh worker processes instead of forks of this one: they never touch the GPU, and a fork would inherit this
        # process's open device handle.  Start-up is excluded from the timings (time_batches skips the first batches).
        loader.multiprocessing_context = "spawn"
    return loader


def time_batches(it, n, per_batch=None, skip=2):
    """ms per batch over n batches after `skip` untimed ones (worker start-up), each followed by per_batch(batch)."""
    for _ in range(skip):
        b = next(it)
        if per_batch:
            per_batch(b)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        b = next(it)
        if per_batch:
            per_batch(b)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def time_steps(model, it, steps, warmup):
    """optimize_parameters ms per step; `it` None = the resident batch already fed."""
    def one(k):
        if it is not None:
            model.feed_data(next(it))
        model.optimize_parameters(k)
        torch.cuda.synchronize()
    for k in range(warmup):
        one(k + 1)
    t0 = time.perf_counter()
    for k in range(steps):
        one(warmup + k + 1)
    return (time.perf_counter() - t0) * 1e3 / steps


def forever(make):
    while True:
        yield from make()


def blur_leg(args):
    """The --blur_window run (module docstring)."""
    import importlib.util
    from blur_cases import make_sharp_tree
    from bin_amd import ops
    from bin_amd.data import create_dataset
    from bin_amd.data.BIN_dataset import draw_window_aug
    from bin_amd.data.device_cache import N_BLUR, DeviceFrameCache, DeviceWindowLoader
    spec = importlib.util.spec_from_file_location("make_blur_folder", os.path.join(REPO, "tools", "make_blur_folder.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    def blur_dataset(root, window, **exposure):
        random.seed(0)
        opt = {"mode": "BIN", "name": "train", "dataroot_GT": root, "dataroot_LQ": root, "LQ_size": [3, CROP, CROP],
               "data_type": "img", "phase": "train", "blur_window": window}
        return create_dataset(dict(opt, **exposure))

    exposure = {}
    if args.blur_gamma is not None:
        exposure["blur_gamma"] = tool.parse_gamma_flag(args.blur_gamma)
        if args.blur_noise is not None:
            exposure["blur_noise"] = tool.parse_noise_flag(args.blur_noise)

    N = args.blur_window
    dev = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="bin_train_data_")
    res = {"tool": "bench_train_data", "leg": "blur_window", "blur_window": N, "batch": args.batch, "crop": [CROP, CROP],
           "frame": [352, 640]}
    try:
        t = time.perf_counter()
        root = make_sharp_tree(os.path.join(tmp, "adobe"), clips=tuple((f"clip{c:02d}", 1 + 8 * c, args.sharp_files)
                                                                       for c in range(args.clips)))
        if not exposure:
            tool.make_blur_folder(root, "train", N)
        res["tree_s"] = round(time.perf_counter() - t, 2)
        print(f"tree: {args.clips} clips of {args.sharp_files} sharp frames in {res['tree_s']} s", file=sys.stderr, flush=True)

        # the kernel alone: an arena with room for h = 16, one batch's table per exposure, launched back to back
        wide = blur_dataset(root, 33)
        cache = DeviceFrameCache(wide.all_paths, dev, blur_half=16)
        wins = [wide.all_paths[i] for i in range(args.batch)]
        draws = [draw_window_aug((3, CROP, CROP)) for _ in wins]
        rows = []
        for L in args.kernel_windows or [1, N, 33]:
            tab = cache.table(wins, draws, [L // 2] * len(wins))
            for _ in range(10):
                ops.gather_windows_blur(cache.frames, tab, (CROP, CROP), N_BLUR, cache.clip_ranges)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.kernel_launches):
                ops.gather_windows_blur(cache.frames, tab, (CROP, CROP), N_BLUR, cache.clip_ranges)
            e1.record()
            torch.cuda.synchronize()
            nbytes = args.batch * CROP * CROP * (N_BLUR * (3 * L + 12) + (17 - N_BLUR) * 15)
            rows.append({"L": L, "us_per_launch_events": round(e0.elapsed_time(e1) * 1e3 / args.kernel_launches, 2),
                         "bytes_no_reuse": nbytes, "hbm_bound_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2)})
            print(f"gather_windows_blur {rows[-1]}", file=sys.stderr, flush=True)
            for noise in ([None] + ([exposure.get("blur_noise")] if exposure.get("blur_noise") else []) if exposure else []):
                import numpy as np
                curve = ops.exposure_curve(exposure["blur_gamma"], noise)
                keyed = np.concatenate([tab, np.arange(2 * len(wins), dtype=np.int32).reshape(-1, 2) * 2654435 + 1], axis=1)
                for _ in range(10):
                    ops.gather_windows_exposed(cache.frames, keyed, (CROP, CROP), N_BLUR, curve, cache.clip_ranges)
                e0.record()
                for _ in range(args.kernel_launches):
                    ops.gather_windows_exposed(cache.frames, keyed, (CROP, CROP), N_BLUR, curve, cache.clip_ranges)
                e1.record()
                torch.cuda.synchronize()
                rows.append({"L": L, "kernel": "binexpose_gather", "noise": noise,
                             "us_per_launch_events": round(e0.elapsed_time(e1) * 1e3 / args.kernel_launches, 2),
                             "bytes_no_reuse": nbytes, "hbm_bound_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2)})
                print(f"gather_windows_exposed {rows[-1]}", file=sys.stderr, flush=True)
        res["gather_kernel"] = {"arena_bytes": cache.nbytes, "rows": rows,
                                "note": "event-timed launches include the pinned table upload and launch gaps; "
                                        "rocprofv3 gives the kernel alone"}
        del cache
        if args.only == "kernel":
            print(json.dumps(res))
            return

        loaders, res["cache"] = {}, {}
        pair = ((("device_cache_blur_window", blur_dataset(root, N)), ("device_cache_exposed", blur_dataset(root, N, **exposure)))
                if exposure else (("device_cache", dataset(root)), ("device_cache_blur_window", blur_dataset(root, N))))
        for name, ds in pair:
            torch.cuda.synchronize()
            t = time.perf_counter()
            loaders[name] = DeviceWindowLoader(ds, args.batch, None, dev)
            torch.cuda.synchronize()
            c = loaders[name].cache
            res["cache"][name] = {"build_s": round(time.perf_counter() - t, 3), "bytes": c.nbytes, "frames": c.shape[0],
                                  "windows": len(ds)}
            print(f"cache {name}: {res['cache'][name]}", file=sys.stderr, flush=True)
        res["device_loader_ms_per_batch"] = {k: round(time_batches(forever(lambda dl=dl: iter(dl)), args.loader_batches), 3)
                                             for k, dl in loaders.items()}

        import bench
        model, _ = bench.make_train_model("f16x3", None, 1, 0, args.batch, S=CROP)
        ts = {k: [] for k in loaders}
        for r in range(args.rounds):                         # alternating: A B A B ...
            for k, dl in loaders.items():
                ts[k].append(round(time_steps(model, forever(lambda dl=dl: iter(dl)), args.steps, args.warmup if r == 0 else 2), 2))
                print(f"round {r}: step fed by {k}: {ts[k][-1]} ms", file=sys.stderr, flush=True)
        med = {k: sorted(v)[len(v) // 2] for k, v in ts.items()}
        res["train_step_ms"] = {"rounds": ts, "median": med}
        if exposure:
            res["exposure"] = exposure
            res["exposed_vs_blur_window"] = round(med["device_cache_exposed"] / med["device_cache_blur_window"], 4)
        else:
            res["blur_vs_device_cache"] = round(med["device_cache_blur_window"] / med["device_cache"], 4)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=9)
    ap.add_argument("--blurry", type=int, default=13, help="blurry frames per clip (n - 5 windows)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--workers", type=int, nargs="+", default=[3, 16])
    ap.add_argument("--loader-batches", type=int, default=24)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-launches", type=int, default=200)
    ap.add_argument("--only", choices=["all", "kernel"], default="all")
    ap.add_argument("--blur_window", type=int, default=None, help="run the blur_window leg with this exposure instead")
    ap.add_argument("--sharp-files", type=int, default=120, help="blur_window leg: consecutive sharp frames per clip")
    ap.add_argument("--kernel-windows", type=int, nargs="+", default=None, help="blur_window leg: exposures of the kernel launches")
    ap.add_argument("--rounds", type=int, default=3, help="blur_window leg: alternations of the two device-fed steps")
    ap.add_argument("--blur_gamma", default=None, help="blur_window leg: compare the exposure path (a number 1.0 .. 2.4 or srgb) with it")
    ap.add_argument("--blur_noise", default=None, help="blur_window leg, with --blur_gamma: READ,SHOT")
    args = ap.parse_args()
    if args.blur_window is not None:
        return blur_leg(args)
    from bin_amd.data.device_cache import DeviceWindowLoader

    dev = torch.device("cuda", 0)
    tmp = tempfile.mkdtemp(prefix="bin_train_data_")
    res = {"tool": "bench_train_data", "batch": args.batch, "crop": [CROP, CROP], "frame": [352, 640]}
    try:
        t = time.perf_counter()
        root = make_tree(os.path.join(tmp, "adobe"), args.clips, args.blurry)
        ds = dataset(root)
        res["windows"], res["tree_s"] = len(ds), round(time.perf_counter() - t, 2)
        print(f"tree: {len(ds)} windows in {res['tree_s']} s", file=sys.stderr, flush=True)

        torch.cuda.synchronize()
        t = time.perf_counter()
        dl = DeviceWindowLoader(ds, args.batch, None, dev)
        torch.cuda.synchronize()
        res["cache"] = {"build_s": round(time.perf_counter() - t, 3), "bytes": dl.cache.nbytes, "frames": dl.cache.shape[0]}
        print(f"cache: {res['cache']}", file=sys.stderr, flush=True)

        # the gather kernel alone: one batch's table, launched back to back
        from bin_amd import ops
        from bin_amd.data.BIN_dataset import draw_window_aug
        wins = [ds.all_paths[i] for i in range(args.batch)]
        tab = dl.cache.table(wins, [draw_window_aug((3, CROP, CROP)) for _ in wins])
        for _ in range(10):
            ops.gather_windows(dl.cache.frames, tab, (CROP, CROP))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_launches):
            ops.gather_windows(dl.cache.frames, tab, (CROP, CROP))
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.kernel_launches
        nbytes = args.batch * 17 * CROP * CROP * (3 + 12)
        res["gather_kernel"] = {"us_per_launch_events": round(us, 2), "bytes": nbytes,
                                "hbm_bound_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2),
                                "note": "event-timed launches include the pinned table upload and launch gaps; "
                                        "rocprofv3 gives the kernel alone"}
        res["device_loader_ms_per_batch"] = round(time_batches(forever(lambda: iter(dl)), args.loader_batches), 2)
        print(f"device loader: {res['device_loader_ms_per_batch']} ms/batch", file=sys.stderr, flush=True)
        if args.only == "kernel":
            print(json.dumps(res))
            return

        import bench
        model, _ = bench.make_train_model("f16x3", None, 1, 0, args.batch, S=CROP)
        ratio = 1 + (args.loader_batches + 4) * args.batch // len(ds)
        hl = {}
        for w in args.workers:
            row = {}
            row["discard"] = round(time_batches(iter(host_loader(ds, args.batch, w, ratio)), args.loader_batches), 2)
            row["feed_data"] = round(time_batches(iter(host_loader(ds, args.batch, w, ratio)), args.loader_batches,
                                                  model.feed_data), 2)
            hl[f"n_workers_{w}"] = row
            print(f"host loader n_workers {w}: {row}", file=sys.stderr, flush=True)
        res["host_loader_ms_per_batch"] = hl

        ts = {}
        steps_ratio = 1 + (args.steps + args.warmup + 4) * args.batch // len(ds)
        for w in args.workers:
            ts[f"host_n_workers_{w}"] = round(time_steps(model, iter(host_loader(ds, args.batch, w, steps_ratio)),
                                                         args.steps, args.warmup), 2)
            print(f"step fed by host loader ({w}): {ts[f'host_n_workers_{w}']} ms", file=sys.stderr, flush=True)
        ts["device_cache"] = round(time_steps(model, forever(lambda: iter(dl)), args.steps, args.warmup), 2)
        model.feed_data(next(iter(dl)))
        ts["resident"] = round(time_steps(model, None, args.steps, args.warmup), 2)
        print(f"step device-fed {ts['device_cache']} ms, resident {ts['resident']} ms", file=sys.stderr, flush=True)
        res["train_step_ms"] = ts
        res["device_vs_resident"] = round(ts["device_cache"] / ts["resident"], 4)
        w0 = f"n_workers_{args.workers[0]}"
        res["host_loader_vs_step"] = round(hl[w0]["feed_data"] / ts["resident"], 3)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
