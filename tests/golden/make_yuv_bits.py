"""Records tests/golden/yuv_bits.json: the sha256 of every output buffer of every case of tests/yuv_bit_cases.py, for
test_yuv_bits_are_the_recorded_ones.  Run on a GPU; `tree` is a built checkout of the commit to pin (default: this one), whose
bin_amd package and libraries are the ones imported:

    python tests/golden/make_yuv_bits.py <commit id> [out.json] [tree]

Every case is computed twice; a case whose two digests differ pins nothing, is left out of "bits" and named under "left_out".  These
kernels have no atomics and no summation order that depends on the device, so "left_out" has to be empty: the script returns 1
otherwise, and the test fails on a fixture that lists any.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [TREE, os.path.dirname(HERE)]

import yuv_bit_cases as YB  # noqa: E402


def main():
    import bin_amd
    recorded_from = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "yuv_bits.json")
    assert os.path.dirname(os.path.dirname(os.path.abspath(bin_amd.__file__))) == TREE, bin_amd.__file__
    bits, left_out = {}, []
    for key in YB.KEYS:
        first, second = YB.digests(key), YB.digests(key)
        if first == second:
            bits[key] = first
        else:
            left_out.append(key)
            print(key, "NOT REPRODUCIBLE", flush=True)
    with open(out, "w") as f:
        json.dump({"recorded_from": recorded_from, "left_out": left_out, "bits": bits}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(bits)} cases, {sum(len(v) for v in bits.values())} buffers recorded, {len(left_out)} left out -> {out}")
    return 1 if left_out else 0


if __name__ == "__main__":
    sys.exit(main())
