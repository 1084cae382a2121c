"""Case table, references and bars of the Adam kernel (binopt_adam_step, bin_amd/optim.py), shared by tests/test_gpu_optim.py and
tests/test_cpu_optim.py.

A case is a list of rows (one tensor each: numel, the offsets in floats of p, g, m, v from a 16-byte boundary, the decade of its
gradients) plus the hyper-parameters and the number of consecutive steps.  The state starts at zero and step t = 1 .. steps sees a
fresh seeded gradient, a tenth of it exact zeros, all of one magnitude per tensor: a max-abs error over a tensor of mixed decades
would see only the largest.

reference64  the four formulas of include/binopt.h evaluated in float64 on the same fp32 inputs
torch32      torch.optim.Adam(foreach=False) in float32 on the CPU; e32 = its max-abs error against reference64
numpy32      a plain numpy float32 restatement of the formulas (what the kernel computes, without its fused multiply-adds)
bar          per case, output (p, m, v) and gradient decade: max(4 * e32, 2^-23 * max|reference64|), both taken over the rows of that
             decade in the case; the second term is one fp32 ulp of the largest value, which no float32 result can be held tighter
             than.  Nothing is masked.  Per decade, because one bar over a case of mixed decades would see only the largest; not per
             row, because e32 of a 1-element tensor is a single sample of torch's rounding and says nothing about another
             float32 evaluation order (the plain numpy restatement misses such a bar by 3 - 17 % on 1-, 3- and 5-element rows).

The buffers of a case live in one arena per kind (p, g, m, v): row i starts `off` floats past a 16-byte boundary and at least one
guard float separates it from its neighbours, so one comparison of the arena outside the rows checks every guard."""
import functools
import math
from collections import namedtuple

import numpy as np

ADAM_MAX_TENSORS = 64                      # BINOPT_ADAM_MAX_TENSORS (tests/test_cpu_optim.py holds it to the header)
CHUNK = 2048                               # elements per workgroup of adam_step_kernel: 2047 / 2048 / 2049 sit on its edge too
NUMELS = (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 221184)
MAGNITUDES = (1e-12, 1e-6, 1e-3, 1.0, 1e4)
ALIGNMENTS = (             # offsets of (p, g, m, v) in floats from a 16-byte boundary
    ("aligned", (0, 0, 0, 0)), ("p_off", (1, 0, 0, 0)), ("g_off", (0, 2, 0, 0)), ("m_off", (0, 0, 3, 0)), ("v_off", (0, 0, 0, 1)),
    ("all_off_differently", (1, 2, 3, 2)), ("all_off_alike", (3, 3, 3, 3)))
STEPS = (1, 3, 10)
WEIGHT_DECAYS = (0.0, 1e-2)
EPSILONS = (1e-8, 1e-3)
BETAS = ((0.9, 0.999), (0.9, 0.99), (0.5, 0.9))
LRS = (2e-4, 0.0)
GUARD = np.float32(-7.25e7)                # sentinel between the rows of an arena

Row = namedtuple("Row", "numel offs mag")
Case = namedtuple("Case", "tag rows steps lr betas eps weight_decay cpu seed")


@functools.lru_cache(maxsize=None)
def stage4_numels():
    """The sizes of bin_stage4's 540 parameter tensors (3 .. 221 184 elements, 11.44 M in all)."""
    from bin_amd.weights import canonical_weights
    return tuple(int(v.size) for v in canonical_weights(0).values())


def _rows(numels, offs=None):
    """Rows over `numels`; magnitudes cycle, and so do the alignments unless `offs` fixes one."""
    return tuple(Row(n, offs if offs is not None else ALIGNMENTS[i % len(ALIGNMENTS)][1], MAGNITUDES[i % len(MAGNITUDES)])
                 for i, n in enumerate(numels))


def _build():
    cases = []
    seed = 1000
    # every numel at every alignment (and at every magnitude over the table: the magnitudes cycle with the row, shifted per case)
    for k, (name, offs) in enumerate(ALIGNMENTS):
        numels = NUMELS[k % len(NUMELS):] + NUMELS[:k % len(NUMELS)]
        cases.append(Case(f"numel_{name}", _rows(numels + (2047, 2048, 2049), offs), 3, 2e-4, (0.9, 0.999), 1e-8, 0.0, True, seed + k))
    seed += 100
    # every combination of the hyper-parameters; the step counts cycle.  Five magnitudes, aligned (a whole chunk + tail) and not.
    k = 0
    for wd in WEIGHT_DECAYS:
        for eps in EPSILONS:
            for betas in BETAS:
                for lr in LRS:
                    rows = _rows((4097,) * 5, (0, 0, 0, 0)) + _rows((257,) * 5, (0, 1, 0, 0))
                    cases.append(Case(f"hyper_wd{wd:g}_eps{eps:g}_b{betas[0]:g}-{betas[1]:g}_lr{lr:g}", rows, STEPS[k % 3], lr, betas,
                                      eps, wd, True, seed + k))
                    k += 1
    seed += 100
    # row counts around the per-launch limit: small tensors of every edge size, alignments and magnitudes cycling
    small = tuple(n for n in NUMELS if n < 5000)
    for k, n in enumerate((1, ADAM_MAX_TENSORS - 1, ADAM_MAX_TENSORS, ADAM_MAX_TENSORS + 1)):
        numels = tuple(small[i % len(small)] for i in range(n)) if n > 1 else (4097,)
        cases.append(Case(f"rows_{n}", _rows(numels), 3, 2e-4, (0.9, 0.999), 1e-8, 1e-2, True, seed + k))
    cases.append(Case("rows_stage4", None, 3, 2e-4, (0.9, 0.99), 1e-8, 0.0, False, seed + 50))
    return cases


CASES = _build()
CASE_BY_TAG = {c.tag: c for c in CASES}
CPU_TAGS = [c.tag for c in CASES if c.cpu]


def rows_of(case):
    if case.rows is None:                                    # bin_stage4's own 540 shapes, every tensor aligned as torch allocates them
        return _rows(stage4_numels(), (0, 0, 0, 0))
    return case.rows


# ----------------------------------------------------------------------------------------------------------------- inputs
def layout(rows, kind):
    """(starts, total): row i of kind 0..3 (p, g, m, v) occupies arena[starts[i] : starts[i] + numel], starts[i] % 4 == its offset;
    4 guard floats lead, at least one separates two rows, 4 or more trail."""
    starts, cur = [], 4
    for r in rows:
        s = (cur + 3) // 4 * 4 + r.offs[kind]
        starts.append(s)
        cur = s + r.numel + 1
    return starts, (cur + 3) // 4 * 4 + 4


def make_inputs(case):
    """{"p": [row arrays], "g": [per step: [row arrays]]}: float32, seeded by the case."""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    rows = rows_of(case)
    p = [(rng.standard_normal(r.numel) * 0.1).astype(np.float32) for r in rows]
    g = []
    for _ in range(case.steps):
        step = []
        for r in rows:
            x = (rng.standard_normal(r.numel) * r.mag).astype(np.float32)
            x[rng.random(r.numel) < 0.1] = 0.0               # a tenth exact zeros
            assert float(np.abs(x).max(initial=0.0)) <= 1e15  # above that g * g overflows fp32 and float64 is no reference
            step.append(x)
        g.append(step)
    return {"p": p, "g": g}


def arena(rows, kind, values):
    """One float32 arena of GUARD with `values[i]` (or zeros when None) at row i's place."""
    starts, total = layout(rows, kind)
    a = np.full(total, GUARD, np.float32)
    for i, (s, r) in enumerate(zip(starts, rows)):
        a[s:s + r.numel] = 0.0 if values is None else values[i]
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


def bias_factors(case, t, dtype=np.float64):
    """(step_size, inv_sqrt_bc2) of step t, computed in double (and rounded once for float32)."""
    b1, b2 = case.betas
    return dtype(case.lr / (1.0 - b1 ** t)), dtype(1.0 / math.sqrt(1.0 - b2 ** t))


# ------------------------------------------------------------------------------------------------------------- references
def formulas(case, inp, dtype):
    """The four formulas of include/binopt.h over all steps in `dtype` (float64: the reference; float32: the plain restatement)
    -> {"p", "m", "v"}: lists of row arrays."""
    f = dtype
    b1, b2 = case.betas
    w1, beta2, w2, eps, wd = f(1.0 - b1), f(b2), f(1.0 - b2), f(case.eps), f(case.weight_decay)
    p = [x.astype(f) for x in inp["p"]]
    m = [x.astype(f) for x in inp["m"]] if "m" in inp else [np.zeros_like(x) for x in p]      # a state to continue from
    v = [x.astype(f) for x in inp["v"]] if "v" in inp else [np.zeros_like(x) for x in p]
    t0 = inp.get("t0", 0)                                                                    # ... after t0 steps
    with np.errstate(all="ignore"):
        for t in range(t0 + 1, t0 + case.steps + 1):
            step_size, inv_sqrt_bc2 = bias_factors(case, t, f)
            for i in range(len(p)):
                g = inp["g"][t - t0 - 1][i].astype(f)
                if case.weight_decay != 0:
                    g = g + wd * p[i]
                m[i] = m[i] + w1 * (g - m[i])
                v[i] = beta2 * v[i] + (w2 * g) * g
                p[i] = p[i] - step_size * (m[i] / (np.sqrt(v[i]) * inv_sqrt_bc2 + eps))
    return {"p": p, "m": m, "v": v}


def reference64(case, inp):
    return formulas(case, inp, np.float64)


def numpy32(case, inp):
    out = formulas(case, inp, np.float32)
    assert all(a.dtype == np.float32 for k in out for a in out[k])
    return out


def torch32(case, inp, cls=None, device="cpu"):
    """torch.optim.Adam(foreach=False) in float32 (or `cls`, on `device`) over the same steps -> {"p", "m", "v"} as numpy rows."""
    import torch
    params = [torch.nn.Parameter(torch.from_numpy(x.copy()).to(device)) for x in inp["p"]]
    kw = {"foreach": False} if cls is None else {}
    opt = (cls or torch.optim.Adam)(params, lr=case.lr, betas=case.betas, eps=case.eps, weight_decay=case.weight_decay, **kw)
    if "m" in inp:
        for q, m0, v0 in zip(params, inp["m"], inp["v"]):
            opt.state[q] = {"step": torch.tensor(float(inp.get("t0", 0)), dtype=torch.float32),
                            "exp_avg": torch.from_numpy(m0.copy()).to(device), "exp_avg_sq": torch.from_numpy(v0.copy()).to(device)}
    for t in range(case.steps):
        for q, g in zip(params, inp["g"][t]):
            q.grad = torch.from_numpy(g.copy()).to(device)
        opt.step()
    return {"p": [q.detach().cpu().numpy() for q in params],
            "m": [opt.state[q]["exp_avg"].cpu().numpy() for q in params],
            "v": [opt.state[q]["exp_avg_sq"].cpu().numpy() for q in params]}


def _err(a, r64, mask=None):
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - r64)
    if mask is not None:
        d = d[mask]
    return float(d.max(initial=0.0))


def rows_by_decade(grads):
    """Rows for tensors that come from a network rather than from the table: the "magnitude" of a row is the decade of its own
    largest gradient, so tensors of one decade share a bar as the table's rows do."""
    out = []
    for g in grads:
        top = float(np.abs(g).max(initial=0.0))
        out.append(Row(int(g.size), (0, 0, 0, 0), 10.0 ** math.floor(math.log10(top)) if top > 0 else 0.0))
    return tuple(out)


def _groups(rows):
    """{magnitude: [row indices]}: the rows of one gradient decade, which share a bar."""
    out = {}
    for i, r in enumerate(rows):
        out.setdefault(r.mag, []).append(i)
    return out


def bars(rows, r64, r32, mask=None):
    """{"p" | "m" | "v": {magnitude: (e32, bar)}}: e32 and max|reference| are taken over all rows of one gradient decade of the case;
    `mask` (same structure as r64, bool rows) restricts both to the elements it selects."""
    out = {}
    for k in ("p", "m", "v"):
        out[k] = {}
        for mag, idx in _groups(rows).items():
            e32 = top = 0.0
            for i in idx:
                mk = None if mask is None else mask[k][i]
                e32 = max(e32, _err(r32[k][i], r64[k][i], mk))
                top = max(top, float(np.abs(r64[k][i] if mk is None else r64[k][i][mk]).max(initial=0.0)))
            out[k][mag] = (e32, max(4.0 * e32, 2.0 ** -23 * top))
    return out


def compare(tag, rows, got, r64, r32, mask=None):
    """Every row and output of `got` within its bar; prints one `[optim]` line per output with the case's largest error / bar and
    returns {"p" | "m" | "v": that ratio}."""
    b = bars(rows, r64, r32, mask)
    worst = {}
    fails = []
    for k in ("p", "m", "v"):
        w = (0.0, -1, 0.0, 0.0, 0.0)
        for i, (a, r) in enumerate(zip(got[k], r64[k])):
            e32, bar = b[k][rows[i].mag]
            err = _err(a, r, None if mask is None else mask[k][i])
            ratio = err / bar if bar > 0 else (0.0 if err == 0 else float("inf"))
            if ratio >= w[0]:
                w = (ratio, i, err, bar, e32)
            if not err <= bar:
                fails.append((k, i, int(a.size), err, bar, e32))
        worst[k] = w[0]
        print(f"[optim] {tag} {k}: worst row {w[1]} error {w[2]:.3e} bar {w[3]:.3e} (e32 {w[4]:.3e}) ratio {w[0]:.3f}")
    assert not fails, f"{tag}: (output, row, numel, error, bar, e32) beyond the bar: {fails[:8]}"
    return worst
