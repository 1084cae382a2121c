"""Device time of binexpose_gather (libbinexpose.so) next to binhip_gather_windows_blur at the training shape: 8 samples, 17 slots
(6 blurry), 256x256 crops of 352x640 frames, one exposure per run (default 11).

Both entry points are called directly, with the table and the curve already on the device, --launches times back to back between
two HIP events after --warmup launches, in one process; one JSON line.  The bytes are counted without any cache reuse (3 L B read
+ 12 B written per blurry pixel, 15 B per other pixel) and set against 6.3 TB/s.

    python tools/bench_exposure_kernel.py [--window 11] [--gamma 2.2] [--noise 0.004,0.0004]
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
N, N_SLOTS, N_BLUR, CROP, H, W = 8, 17, 6, 256, 352, 640


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--window", type=int, default=11)
    ap.add_argument("--gamma", default="2.2")
    ap.add_argument("--noise", default="0.004,0.0004")
    ap.add_argument("--frames", type=int, default=120)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    from bin_amd import _lib, ops
    h = args.window // 2
    gamma = float(args.gamma) if args.gamma != "srgb" else "srgb"
    noise = tuple(float(v) for v in args.noise.split(","))
    g = np.random.Generator(np.random.PCG64(1))
    frames = torch.randint(0, 256, (args.frames, H, W, 3), dtype=torch.uint8, device="cuda")
    rows = np.zeros((N, N_SLOTS + 6), np.int32)
    rows[:, :N_SLOTS] = g.integers(h, args.frames - h, (N, N_SLOTS))
    rows[:, N_SLOTS] = g.integers(0, H - CROP + 1, N)
    rows[:, N_SLOTS + 1] = g.integers(0, W - CROP + 1, N)
    rows[:, N_SLOTS + 2] = g.integers(0, 2, N)
    rows[:, N_SLOTS + 3] = h
    rows[:, N_SLOTS + 4:] = g.integers(0, 2 ** 31, (N, 2))
    keyed = torch.from_numpy(rows).cuda()
    plain = torch.from_numpy(np.ascontiguousarray(rows[:, :N_SLOTS + 4])).cuda()
    out = torch.empty((N_SLOTS, N, 3, CROP, CROP), dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    blur, expose = _lib.lib().binhip_gather_windows_blur, _lib.exposelib().binexpose_gather
    curves = {name: torch.from_numpy(ops.exposure_curve(gamma, nz).reshape(-1).copy()).cuda() for name, nz in (("clean", None), ("noisy", noise))}
    calls = {"binhip_gather_windows_blur": lambda: blur(p(frames), args.frames, H, W, p(plain), N, N_SLOTS, N_BLUR, CROP, CROP, p(out), stream)}
    for name, curve in curves.items():
        calls["binexpose_gather, " + name] = lambda c=curve: expose(p(frames), args.frames, H, W, p(keyed), N, N_SLOTS, N_BLUR, CROP, CROP,
                                                                     p(c), p(out), stream)
    L = 2 * h + 1
    nbytes = N * CROP * CROP * (N_BLUR * (3 * L + 12) + (N_SLOTS - N_BLUR) * 15)
    res = {"tool": "bench_exposure_kernel", "window": L, "gamma": gamma, "noise": list(noise), "launches": args.launches,
           "bytes_no_reuse": nbytes, "hbm_bound_us": round(nbytes / HBM_BYTES_PER_S * 1e6, 2), "us_per_launch": {}}
    for rnd in range(3):                                     # three alternating rounds; the median is reported beside them
        for name, call in calls.items():
            for _ in range(args.warmup):
                assert call() == 0
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                call()
            e1.record()
            torch.cuda.synchronize()
            res["us_per_launch"].setdefault(name, []).append(round(e0.elapsed_time(e1) * 1e3 / args.launches, 2))
    res["median_us"] = {k: sorted(v)[1] for k, v in res["us_per_launch"].items()}
    res["fraction_of_hbm_bound"] = {k: round(res["hbm_bound_us"] / v, 3) for k, v in res["median_us"].items()}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
