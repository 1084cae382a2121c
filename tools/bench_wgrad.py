"""Isolated timing of the weight-gradient kernels (f16x3) at the training working size, one library against another.

Per round and per library one child process is started with BIN_AMD_LIB set to that library (bin_amd/_lib.py), under its own `timeout`;
the libraries alternate within a round, so that drift of the box falls on all of them alike, and nothing is started after a child that
failed.  The child times every layer with a hipEvent pair per call (bench_common.timed), 3 untimed calls first, and prints one JSON line
per layer: the median and the least of 20 calls.  No figure printed here is comparable across boxes: compare within one run.

Layers (ks, cin, cout): the dense-block 3x3 convs, SFENet2 and UPNet.0; LFF and GFF.0 (streaming 1x1 kernel); SFENet1 of the three
sub-networks and the fused UPNet's 5x5 (generic kernel).  WG_LAYERS="ks,cin,cout;..." picks others; WG_ZERO=1 feeds all-zero operands
(the same instruction stream on idle datapaths).
usage: python tools/bench_wgrad.py [--lib PATH]... [--rounds 5] [--size N H W]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import bench_common as B

LAYERS = "3,96,32;3,128,32;3,160,32;3,192,32;3,96,96;3,96,256;1,224,96;1,1152,96;5,24,96;5,36,96;5,60,96;5,96,12"
CHILD_TIMEOUT_S = 300
CALLS, WARMUP = 20, 3


def child(args):
    import torch
    from bin_amd import ops
    assert torch.cuda.is_available(), "bench_wgrad needs a GPU"
    n, h, w = args.size
    layers = [tuple(int(v) for v in l.split(",")) for l in os.environ.get("WG_LAYERS", LAYERS).split(";")]
    zero = 0.0 if os.environ.get("WG_ZERO") == "1" else 1.0
    g = torch.Generator(device="cuda").manual_seed(0)
    for ks, cin, cout in layers:
        x = ops.nchw_to_planes((torch.rand(n, cin, h, w, generator=g, device="cuda") - 0.3) * zero, 3)
        gy = ops.nchw_to_planes((torch.rand(n, cout, h, w, generator=g, device="cuda") - 0.5) * zero, 3)

        def f():
            ops.conv2d_bwd_weight(x, gy, cout, cin, ks, 3)
        for _ in range(WARMUP):
            f()
        us = [v * 1e3 for v in B.timed(f, CALLS)[0]]
        med = statistics.median(us)
        flops = 2.0 * n * h * w * cin * cout * ks * ks * 3
        print(json.dumps({"what": "wgrad", "round": args.child, "lib": os.environ.get("BIN_AMD_LIB", "built"), "ks": ks, "cin": cin,
                          "cout": cout, "size": [n, h, w], "us_median": round(med, 2), "us_min": round(min(us), 2),
                          "TFLOPs": round(flops / med / 1e6, 1)}), flush=True)
        del x, gy


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="a libbinhip.so to time; give it twice or more to compare builds")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, nargs=3, default=(40, 128, 128), metavar=("N", "H", "W"))
    ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child is not None:
        return child(args)
    for rnd in range(args.rounds):
        for lib in args.lib or [None]:                        # no --lib: the built library, BIN_AMD_LIB left as it is
            cmd = ["timeout", "-k", "10", str(CHILD_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--child", str(rnd), "--size"] + \
                  [str(v) for v in args.size]
            rc = subprocess.run(cmd, cwd=B.REPO, env=dict(os.environ, BIN_AMD_LIB=os.path.abspath(lib)) if lib else None).returncode
            if rc != 0:
                print(json.dumps({"what": "failed", "round": rnd, "lib": lib, "exit_status": rc}), flush=True)
                sys.exit(rc)


if __name__ == "__main__":
    main()
