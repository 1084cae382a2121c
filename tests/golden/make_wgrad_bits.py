"""Records tests/golden/wgrad_bits.json: the sha256 of dW and db of every case of tests/wgrad_cases.py x nterms in {3, 1} on the white-noise
operands (family C), for test_wgrad_white_noise_bits_are_the_recorded_ones.  The summation order depends on the CU count, which the file
carries.  Run on a GPU with the library of the commit to pin (BIN_AMD_LIB, bin_amd/_lib.py):

    BIN_AMD_LIB=<that commit's libbinhip.so> python tests/golden/make_wgrad_bits.py <commit id> [out.json]

Every case is computed twice; a case whose two digests differ pins nothing and is left out of "bits" and named under "left_out".
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import wgrad_cases as wc  # noqa: E402


def main():
    from bin_amd import _lib as L
    recorded_from = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "wgrad_bits.json")
    bits, left_out = {}, []
    for tag in wc.TAGS:
        for nterms in (3, 1):
            first, second = wc.white_noise_bits(wc.BY_TAG[tag], nterms), wc.white_noise_bits(wc.BY_TAG[tag], nterms)
            key = f"{tag}/{nterms}"
            if first == second:
                bits[key] = first
            else:
                left_out.append(key)
            print(key, "ok" if first == second else "NOT REPRODUCIBLE", first, flush=True)
    with open(out, "w") as f:
        json.dump({"cus": L.lib().binhip_device_cus(), "recorded_from": recorded_from, "left_out": left_out, "bits": bits}, f, indent=1)
        f.write("\n")
    print(f"{len(bits)} cases recorded, {len(left_out)} left out -> {out}")
    return 1 if left_out else 0


if __name__ == "__main__":
    sys.exit(main())
