"""Case table, reference and bars of the gradient-guard kernels (bingrad_norm / bingrad_scale, bin_amd.optim.GradGuard), shared by
tests/test_gpu_gradguard.py and tests/test_cpu_gradguard.py.

A case is a list of rows (one gradient each: numel, the offset in floats of its pointer from a 16-byte boundary, the decade of its
values).  The rows live in one arena (optim_cases.layout / arena / split, kind 1): a row starts `off` floats past a 16-byte boundary and
at least one guard float separates it from its neighbours, so one comparison of the arena outside the rows checks every guard.

reference   float64 numpy on the same fp32 inputs: sumsq = the sum over rows of dot(g64, g64).
bars        |sumsq - ref| <= N * 2^-53 * ref, N the total element count: every product of two converted floats is exact in double, so
            only the additions round, and N * 2^-53 relative is the worst case of ANY summation order of N non-negative terms.
            norm: within one fp32 ulp of float32(sqrt(ref)).  coef: within one fp32 ulp of min(1, max_norm / (sqrt(ref) + 1e-6)) in
            float64; exactly 1 when max_norm == 0 and when the norm is below max_norm.  Nothing is masked.
Most cases hold ONE decade, so that a dropped or doubled element of any row is far outside the bar; the mixed cases say so in their tag.
"""
import math
import re
import os

import numpy as np

import optim_cases as OC

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source_constants():
    src = open(os.path.join(REPO, "bin_amd", "csrc", "bingrad_norm.hip")).read()
    threads, unroll = (int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("GN_THREADS", "GN_UNROLL"))
    hdr = open(os.path.join(REPO, "include", "bingrad.h")).read()
    return threads * unroll * 4, int(re.search(r"#define\s+BINGRAD_MAX_TENSORS\s+(\d+)", hdr).group(1))


CHUNK, MAX_TENSORS = _source_constants()   # elements per workgroup (from the kernel source), rows per launch (from the header)
NUMELS = (1, 3, 4, 5, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 221184)
MAGNITUDES = (1e-30, 1e-12, 1.0, 1e4, 1e25)
OFFSETS = (0, 1, 2, 3)
MAX_NORMS = ("off", "far_above", "half", "milli")
GUARD = OC.GUARD
KIND = 1                                   # the arena helpers of optim_cases index (p, g, m, v): the gradients are kind 1

Row = OC.Row                               # (numel, offs, mag): offs = (off,) * 4
Case = __import__("collections").namedtuple("Case", "tag rows seed")


def _row(numel, off, mag):
    return Row(int(numel), (off,) * 4, mag)


def _build():
    cases, seed = [], 5000
    # every numel at every alignment, one decade per case (the decades cycle with the alignment) ...
    for off in OFFSETS:
        mag = MAGNITUDES[(off + 2) % len(MAGNITUDES)]
        numels = NUMELS[off:] + NUMELS[:off]
        cases.append(Case(f"numel_off{off}", tuple(_row(n, off, mag) for n in numels), seed + off))
    # ... and every decade on rows of every path: whole chunks + a tail, aligned and not, a 1-element and a 5-element row
    for k, mag in enumerate(MAGNITUDES):
        rows = (_row(2 * CHUNK + 1, 0, mag), _row(CHUNK + 1, 1 + k % 3, mag), _row(5, 2, mag), _row(1, 3, mag), _row(CHUNK, 0, mag))
        cases.append(Case(f"mag_{mag:g}", rows, seed + 10 + k))
    cases.append(Case("zeros", tuple(_row(n, i % 4, 0.0) for i, n in enumerate(NUMELS[:8])), seed + 20))
    cases.append(Case("mixed_1e-30_and_1e25", tuple(_row(n, i % 4, (1e-30, 1e25)[i % 2]) for i, n in enumerate(NUMELS[:8] + (257, 2))), seed + 21))
    cases.append(Case("mixed_decade_per_tensor", tuple(_row(n, i % 4, MAGNITUDES[i % 5]) for i, n in enumerate(NUMELS + (2, 257, 96))), seed + 22))
    # row counts around the per-launch limit: small tensors of every edge size, alignments cycling, one decade
    small = tuple(n for n in NUMELS if n <= CHUNK + 1) + (257, 96)
    for k, n in enumerate((1, MAX_TENSORS - 1, MAX_TENSORS, MAX_TENSORS + 1)):
        rows = tuple(_row(small[i % len(small)], i % 4, 1.0) for i in range(n)) if n > 1 else (_row(CHUNK + 1, 0, 1.0),)
        cases.append(Case(f"rows_{n}", rows, seed + 30 + k))
    cases.append(Case("rows_stage4", None, seed + 40))
    return cases


CASES = _build()
CASE_BY_TAG = {c.tag: c for c in CASES}
NON_REPRESENTABLE_IN_FP32_SQUARES = ("mag_1e-30", "mag_1e+25", "mixed_1e-30_and_1e25")


def rows_of(case):
    if case.rows is None:                  # bin_stage4's own 540 shapes, aligned as torch allocates them, a decade per tensor
        return tuple(_row(n, 0, (1e-12, 1.0, 1e4)[i % 3]) for i, n in enumerate(OC.stage4_numels()))
    return case.rows


def make_inputs(case):
    """The float32 gradients of a case, seeded: normal * the row's decade, a tenth exact zeros."""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    out = []
    for r in rows_of(case):
        x = (rng.standard_normal(r.numel) * r.mag).astype(np.float32)
        x[rng.random(r.numel) < 0.1] = 0.0
        assert np.isfinite(x).all()
        out.append(x)
    return out


# ----------------------------------------------------------------------------------------------------------------- references
def reference_sumsq(grads):
    """float64 on the fp32 inputs, row by row (numpy's blocked dot), rows added first to last."""
    total = 0.0
    for g in grads:
        g64 = g.astype(np.float64).ravel()
        total += float(np.dot(g64, g64))
    return total


def reference_sumsq_other_order(grads):
    """The same sum strictly element by element, last row first and each row backwards."""
    flat = np.concatenate([g.astype(np.float64).ravel()[::-1] for g in grads[::-1]])
    return float(np.cumsum(flat * flat)[-1])


def fp32_squares_sumsq(grads):
    """What squaring in float32 gives (the squares of torch's foreach norm), even when they are then added in float64."""
    with np.errstate(over="ignore", under="ignore"):
        return float(sum(np.sum((g * g).astype(np.float64)) for g in grads))


def coef64(max_norm, sumsq):
    """The clip coefficient in float64 from the float32 max_norm the kernel receives."""
    if max_norm == 0 or not math.isfinite(sumsq):
        return 1.0
    return min(1.0, float(np.float32(max_norm)) / (math.sqrt(sumsq) + 1e-6))


def max_norm_of(kind, sumsq):
    """The float32 max_norm of a MAX_NORMS kind for a table of this reference norm."""
    norm = math.sqrt(sumsq)
    if kind == "off":
        return 0.0
    if norm == 0.0:
        return 1.0
    return float(np.float32({"far_above": 1e3, "half": 0.5, "milli": 1e-3}[kind] * norm))


def _ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def check(tag, n_elements, ref, sumsq, norm, coef, max_norm):
    """The bars of the module docstring; prints one `[gradguard]` line with the figures before it asserts."""
    bar = n_elements * 2.0 ** -53 * ref
    err = abs(sumsq - ref)
    n32 = float(np.float32(math.sqrt(ref)))
    c64 = coef64(max_norm, ref)
    c32 = float(np.float32(c64))
    print(f"[gradguard] {tag} max_norm {max_norm:.6g}: N {n_elements} sumsq {sumsq!r} ref {ref!r} err {err:.3e} bar {bar:.3e}"
          f" norm {norm!r} want {n32!r} coef {coef!r} want {c32!r}")
    assert math.isfinite(sumsq) and err <= bar, f"{tag}: sumsq {sumsq!r} is {err:.3e} from {ref!r}, bar {bar:.3e}"
    assert abs(norm - n32) <= _ulp32(n32), f"{tag}: norm {norm!r}, float32(sqrt(ref)) {n32!r}"
    assert abs(coef - c64) <= _ulp32(c32), f"{tag}: coef {coef!r}, float64 formula {c64!r}"
    if max_norm == 0 or math.sqrt(ref) + 1e-6 <= float(np.float32(max_norm)):
        assert coef == 1.0, f"{tag}: coef {coef!r} must be exactly 1 at max_norm {max_norm}"


def check_norm_and_coef(tag, grads, norm, coef, max_norm):
    """For callers that see only GradGuard.last (norm, coef; no sumsq): norm and coef against the float64 reference over `grads`, the
    gradients as the backward left them.  The sumsq bar is the kernel-level tests' business and is not looked at here."""
    ref = reference_sumsq(grads)
    check(tag + " (norm and coef only)", sum(int(g.size) for g in grads), ref, ref, norm, coef, max_norm)
