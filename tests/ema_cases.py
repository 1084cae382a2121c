"""Case table, references and bars of the weight-average kernel (binema_step, bin_amd.optim.WeightEMA), shared by
tests/test_gpu_ema.py and tests/test_cpu_ema.py.

A case is a list of rows (one tensor each: numel, the offsets in floats of e and p from a 16-byte boundary, the magnitude of its
weights) plus the decay, the start of the shadows and the number of consecutive steps K.  Step 1 sees the seeded weights p, every
later step the weights moved by one move of a seeded random walk (a tenth of the magnitude per move).  The shadows start at

    zero   exact zeros
    near   the weights of step 1
    far    100 x the weights of step 1

reference64  e' = e + (1 - decay) * (p - e) evaluated in float64 on the same fp32 inputs, 1 - decay from the decimal as written
numpy32      a plain numpy float32 restatement with w = float32(1.0 - decay) (what the kernel computes, without its fused
             multiply-add); e32 = its max-abs error against reference64
naive32      the same with the weight float32(1) - float32(decay): the mistake the library's shortest-decimal step exists to avoid
bar          per case and magnitude group: max(4 * e32, 2^-23 * max|reference64|), both taken over the rows of that magnitude in the
             case (the rule of tests/optim_cases.py: the second term is one fp32 ulp of the largest value; per magnitude because a
             bar over mixed magnitudes would see only the largest).  Nothing is masked.

`near` with K = 1 is not in the table: there p == e, the update is the identity, and a kernel that does nothing would pass.

The buffers of a case live in one arena per kind (e, p): row i starts `off` floats past a 16-byte boundary and at least one guard
float separates it from its neighbours, so one comparison of the arena outside the rows checks every guard."""
import functools
from collections import namedtuple

import numpy as np

EMA_MAX_TENSORS = 136                      # BINEMA_MAX_TENSORS (tests/test_cpu_ema.py holds it to the header)
CHUNK = 2048                               # elements per workgroup of ema_step_kernel
NUMELS = (1, 3, 4, 5, 255, 256, 257, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 221184)
ALIGNMENTS = (("aligned", (0, 0)), ("e_off", (1, 0)), ("p_off", (0, 3)), ("both_off_alike", (2, 2)), ("both_off_differently", (1, 3)))
MAGNITUDES = (1e-6, 1e-3, 1.0, 1e4)        # no denormals: 1e-6 * (1 - 0.9999) * a small draw stays far above 1.2e-38
DECAYS = (0.0, 0.5, 0.9, 0.999, 0.9999)
STEPS = (1, 3, 10)
STARTS = ("zero", "near", "far")
GUARD = np.float32(-7.25e7)                # sentinel between the rows of an arena

Row = namedtuple("Row", "numel offs mag")
Case = namedtuple("Case", "tag rows decay start steps seed")


@functools.lru_cache(maxsize=None)
def stage4_numels():
    """The sizes of bin_stage4's 540 parameter tensors (3 .. 221 184 elements, 11.44 M in all)."""
    from bin_amd.weights import canonical_weights
    return tuple(int(v.size) for v in canonical_weights(0).values())


def _rows(numels, offs=None, shift=0):
    """Rows over `numels`; magnitudes cycle, and so do the alignments unless `offs` fixes one."""
    return tuple(Row(n, offs if offs is not None else ALIGNMENTS[i % len(ALIGNMENTS)][1], MAGNITUDES[(i + shift) % len(MAGNITUDES)])
                 for i, n in enumerate(numels))


def combos():
    """Every decay x start x K except `near` with K = 1."""
    return [(d, s, k) for d in DECAYS for s in STARTS for k in STEPS if not (s == "near" and k == 1)]


def _build():
    cases = []
    seed = 2000
    # every numel at every alignment (and at every magnitude over the table: the magnitudes cycle with the row, shifted per case)
    for k, (name, offs) in enumerate(ALIGNMENTS):
        numels = NUMELS[k:] + NUMELS[:k]
        cases.append(Case(f"numel_{name}", _rows(numels, offs), DECAYS[(k + 3) % len(DECAYS)], STARTS[k % 3], 3, seed + k))
    seed += 100
    # every decay x start x K: four magnitudes, aligned (whole chunks + a tail) and not
    for k, (decay, start, steps) in enumerate(combos()):
        rows = _rows((2 * CHUNK + 1,) * 4, (0, 0)) + _rows((257,) * 4, (1, 3))
        cases.append(Case(f"decay{decay:g}_{start}_k{steps}", rows, decay, start, steps, seed + k))
    seed += 100
    # row counts around the per-launch limit: small tensors of every edge size, alignments and magnitudes cycling
    small = tuple(n for n in NUMELS if n < 5000)
    for k, n in enumerate((1, EMA_MAX_TENSORS - 1, EMA_MAX_TENSORS, EMA_MAX_TENSORS + 1, 2 * EMA_MAX_TENSORS + 1)):
        numels = tuple(small[i % len(small)] for i in range(n)) if n > 1 else (2 * CHUNK + 1,)
        cases.append(Case(f"rows_{n}", _rows(numels), 0.999, STARTS[k % 3], 3, seed + k))
    cases.append(Case("rows_stage4", None, 0.999, "zero", 3, seed + 50))
    return cases


CASES = _build()
CASE_BY_TAG = {c.tag: c for c in CASES}
TAGS = [c.tag for c in CASES]


def rows_of(case):
    if case.rows is None:                                    # bin_stage4's own 540 shapes, every tensor aligned as torch allocates them
        return _rows(stage4_numels(), (0, 0))
    return case.rows


# ----------------------------------------------------------------------------------------------------------------- inputs
def layout(rows, kind):
    """(starts, total): row i of kind 0..1 (e, p) occupies arena[starts[i] : starts[i] + numel], starts[i] % 4 == its offset;
    4 guard floats lead, at least one separates two rows, 4 or more trail."""
    starts, cur = [], 4
    for r in rows:
        s = (cur + 3) // 4 * 4 + r.offs[kind]
        starts.append(s)
        cur = s + r.numel + 1
    return starts, (cur + 3) // 4 * 4 + 4


def make_inputs(case):
    """{"e": [row arrays], "p": [per step: [row arrays]]}: float32, seeded by the case."""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    rows = rows_of(case)
    p = [[(rng.standard_normal(r.numel) * r.mag).astype(np.float32) for r in rows]]
    for _ in range(case.steps - 1):
        p.append([(x + (rng.standard_normal(r.numel) * (0.1 * r.mag)).astype(np.float32)).astype(np.float32)
                  for x, r in zip(p[-1], rows)])
    if case.start == "zero":
        e = [np.zeros(r.numel, np.float32) for r in rows]
    elif case.start == "near":
        e = [x.copy() for x in p[0]]
    elif case.start == "far":
        e = [(x * np.float32(100.0)).astype(np.float32) for x in p[0]]
    else:
        raise ValueError(case.start)
    return {"e": e, "p": p}


def arena(rows, kind, values):
    """One float32 arena of GUARD with `values[i]` at row i's place."""
    starts, total = layout(rows, kind)
    a = np.full(total, GUARD, np.float32)
    for i, (s, r) in enumerate(zip(starts, rows)):
        a[s:s + r.numel] = values[i]
    return a


def split(rows, kind, a):
    """(row arrays, the arena with the rows blanked to GUARD) — the second must equal an untouched arena of guards."""
    starts, _ = layout(rows, kind)
    a = np.array(a, copy=True)
    out = []
    for s, r in zip(starts, rows):
        out.append(a[s:s + r.numel].copy())
        a[s:s + r.numel] = GUARD
    return out, a


# ------------------------------------------------------------------------------------------------------------- references
def recursion(e, ps, w):
    """e' = e + w * (p - e) over the steps `ps` in the dtype of `w` -> list of row arrays."""
    f = type(w)
    e = [x.astype(f) for x in e]
    for step in ps:
        for i in range(len(e)):
            e[i] = e[i] + w * (step[i].astype(f) - e[i])
    assert all(x.dtype == f for x in e)
    return e


def reference64(case, inp):
    return recursion(inp["e"], inp["p"], np.float64(1.0 - case.decay))


def numpy32(case, inp):
    return recursion(inp["e"], inp["p"], np.float32(1.0 - case.decay))


def naive32(case, inp):
    return recursion(inp["e"], inp["p"], np.float32(1.0) - np.float32(case.decay))


def no_update(case, inp):
    return [x.copy() for x in inp["e"]]


def _err(a, r64):
    return float(np.abs(a.astype(np.float64) - r64).max(initial=0.0))


def _groups(rows):
    """{magnitude: [row indices]}: the rows of one magnitude, which share a bar."""
    out = {}
    for i, r in enumerate(rows):
        out.setdefault(r.mag, []).append(i)
    return out


def bars(rows, r64, r32):
    """{magnitude: (e32, bar)}: e32 and max|reference| are taken over all rows of one magnitude of the case."""
    out = {}
    for mag, idx in _groups(rows).items():
        e32 = max(_err(r32[i], r64[i]) for i in idx)
        top = max(float(np.abs(r64[i]).max(initial=0.0)) for i in idx)
        out[mag] = (e32, max(4.0 * e32, 2.0 ** -23 * top))
    return out


def ratios(rows, got, r64, r32, scale=1.0):
    """{magnitude: (largest error of `got` over the group's rows) / (scale * bar)}."""
    b = bars(rows, r64, r32)
    out = {}
    for mag, idx in _groups(rows).items():
        err = max(_err(got[i], r64[i]) for i in idx)
        bar = scale * b[mag][1]
        out[mag] = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
    return out


def compare(tag, rows, got, r64, r32, scale=1.0):
    """Every row of `got` within `scale` x its bar; prints one `[ema]` line with the case's largest error / bar and returns it."""
    b = bars(rows, r64, r32)
    worst = (0.0, -1, 0.0, 0.0, 0.0)
    fails = []
    for i, (a, r) in enumerate(zip(got, r64)):
        e32, bar = b[rows[i].mag]
        bar *= scale
        err = _err(a, r)
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        if ratio >= worst[0]:
            worst = (ratio, i, err, bar, e32)
        if not err <= bar:
            fails.append((i, int(a.size), err, bar, e32))
    print(f"[ema] {tag}: worst row {worst[1]} error {worst[2]:.3e} bar {worst[3]:.3e} (e32 {worst[4]:.3e}) ratio {worst[0]:.3f}")
    assert not fails, f"{tag}: (row, numel, error, bar, e32) beyond the bar: {fails[:8]}"
    return worst[0]


# ------------------------------------------------------------------------------------------- bars for a run of K steps
def decade(x):
    top = float(np.abs(x).max(initial=0.0))
    return int(np.floor(np.log10(top))) if top > 0 else None


def walk_reference(e0, ps, decay):
    """For tensors that come from a class or a network rather than from the table (K steps over the per-step weights `ps`):
    (r64, bars) with r64 the float64 recursion and bars[i] = K x the largest ONE-step bar along it.  The one-step bar of step t is
    the table's rule applied to a single step started from the fp32 rounding of the reference's state before it:
    max(4 * e32_t, 2^-23 * max|reference after t|), e32_t the error of one plain float32 step from that state against the float64
    step from the same state; as in the table, both terms are pooled over the tensors of one magnitude, here the decade of a
    tensor's largest first-step weight (a per-tensor e32 of a 1-element tensor is a single sample of rounding).  Each step adds at
    most one step's error (plus half an ulp for the state's rounding, inside the ulp term) and the recursion never amplifies what
    is already there (its factor is decay <= 1), so K steps stay within K bars."""
    w64, w32 = np.float64(1.0 - decay), np.float32(1.0 - decay)
    e = [x.astype(np.float64) for x in e0]
    group = [decade(x) for x in ps[0]]
    bar = {g: 0.0 for g in group}
    for step in ps:
        for i in range(len(e)):
            s32 = e[i].astype(np.float32)
            s64 = s32.astype(np.float64)
            one32 = s32 + w32 * (step[i] - s32)
            one64 = s64 + w64 * (step[i].astype(np.float64) - s64)
            e[i] = e[i] + w64 * (step[i].astype(np.float64) - e[i])
            bar[group[i]] = max(bar[group[i]], 4.0 * _err(one32, one64), 2.0 ** -23 * float(np.abs(e[i]).max(initial=0.0)))
    return e, [len(ps) * bar[g] for g in group]


def within(tag, got, r64, bars_):
    """Every tensor of `got` within its bar; prints the largest error / bar and returns it."""
    worst, fails = 0.0, []
    for i, (a, r, bar) in enumerate(zip(got, r64, bars_)):
        err = _err(a, r)
        ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
        worst = max(worst, ratio)
        if not err <= bar:
            fails.append((i, int(a.size), err, bar))
    print(f"[ema] {tag}: largest error / bar {worst:.3f} over {len(got)} tensors")
    assert not fails, f"{tag}: (tensor, numel, error, bar) beyond the bar: {fails[:8]}"
    return worst
