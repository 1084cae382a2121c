"""Records tests/golden/small_kernel_bits.json: the sha256 of every output buffer of every case of tests/small_kernel_bit_cases.py, for
test_small_kernel_bits_are_the_recorded_ones.  Run on a GPU with the library of the commit to pin (BIN_AMD_LIB, bin_amd/_lib.py):

    BIN_AMD_LIB=<that commit's libbinhip.so> python tests/golden/make_small_kernel_bits.py <commit id> [out.json]

Every case is computed twice; a case whose two digests differ pins nothing, is left out of "bits" and named under "left_out".  These
kernels have no atomics in their arithmetic and every reduction runs in a fixed order, so "left_out" has to be empty: the script returns 1
otherwise, and the test fails on a fixture that lists any.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import small_kernel_bit_cases as bc  # noqa: E402


def main():
    from bin_amd import _lib as L
    recorded_from = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "small_kernel_bits.json")
    bits, left_out = {}, []
    for key in bc.KEYS:
        first, second = bc.bits(key), bc.bits(key)
        if first == second:
            bits[key] = first
        else:
            left_out.append(key)
        print(key, "ok" if first == second else "NOT REPRODUCIBLE", flush=True)
    with open(out, "w") as f:
        json.dump({"cus": L.lib().binhip_device_cus(), "recorded_from": recorded_from, "left_out": left_out, "bits": bits}, f, indent=1)
        f.write("\n")
    print(f"{len(bits)} cases recorded, {len(left_out)} left out -> {out}")
    return 1 if left_out else 0


if __name__ == "__main__":
    sys.exit(main())
