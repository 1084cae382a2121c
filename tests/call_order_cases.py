"""Case table and helpers of tests/test_gpu_call_order.py and tests/test_cpu_call_order.py: one RDN module driven through interleaved
call orders (inference between a forward and its backward, validation right after a parameter update, two outstanding forwards, precision
changes), compared bit for bit with a fresh module that executes the probed call alone.

A scenario is a list of steps over ONE module:
    ("eval", tag, prec, shape)        a no_grad forward on frames of `shape`; prec None = the module's current precision, else for this call
    ("train_fwd", tag, shape)         a differentiable forward (every frame and every parameter requests a gradient)
    ("bwd", tag)                      the backward of that forward; the runner then takes the gradients out of .grad (clone, then None), so
                                      every tag's gradients are its own call's
    ("update", seed)                  an in-place, seeded perturbation of every parameter (bumps the version counters, as an optimizer step)
    ("set_precision", prec)           module.precision = prec, until changed again
    ("zero_grad",)                    every .grad = None
    ("drop", tag)                     forget the result of a train_fwd without running its backward
Every scenario names ONE probe: the tag whose outputs (and, for a train_fwd, gradients) are compared with the clean run.  The clean run
replays on a fresh module only what the probe's result may depend on by contract — the updates and the precision setting in force at the
probe's forward — and then executes the probe alone.

Shapes are (N, H, W) at full resolution, taken from backward_cases.RDN_CASES: (2, 12, 14) is half-resolution 6 x 7 (the ring kernels' h <= 6
band, N = 2), (1, 22, 38) is 11 x 19 (odd, nothing falls on a tile).  `ks`: the frame counts (weight sets, backward_cases.SET_FOR_K) a
scenario runs for; `modes` as in backward_cases.RDN_BARS."""
import zlib

import torch

from backward_cases import SET_FOR_K, oracle_rdn_grads

SMALL, ODD = (2, 12, 14), (1, 22, 38)
SHAPES = (SMALL, ODD)
SHAPE_FOR_K = {3: SMALL, 5: ODD}              # k = 3, 5 run the starred scenarios at one shape each; k = 2 runs everything at both

STEP_ARITY = {"eval": 4, "train_fwd": 3, "bwd": 2, "update": 2, "set_precision": 2, "zero_grad": 1, "drop": 2}


def _s(steps, probe, ks=(2,), modes=("f16x3",), also=()):
    return {"steps": steps, "probe": probe, "ks": tuple(ks), "modes": tuple(modes), "also": tuple(also)}


def scenarios(shape, other):
    """The table at one frame size (`other`: the second size of the two-forward scenarios).  `also`: eval tags whose outputs must equal
    the probe's as well."""
    T = {}
    # 1*: inference, then a training step, on one parameter version
    s1 = [("eval", "e", None, shape), ("train_fwd", "p", shape), ("bwd", "p")]
    T["1_eval_then_train"] = _s(s1, "p", ks=(2, 3, 5))
    # 2*: the validation-after-step schedule
    T["2_validation_after_update"] = _s([("train_fwd", "a", shape), ("bwd", "a"), ("update", 1), ("eval", "e", None, shape),
                                         ("train_fwd", "p", shape), ("bwd", "p")], "p", ks=(2, 3, 5))
    # 3: an f16 inference call between a forward and its backward
    s3 = [("train_fwd", "p", shape), ("eval", "e", "f16", shape), ("bwd", "p")]
    T["3_f16_eval_between"] = _s(s3, "p")
    # 4: set_precision + a forward between a forward and its backward, fp32-class and mixed backward
    T["4_set_precision_between"] = _s([("train_fwd", "p", shape), ("set_precision", "f16"), ("eval", "e", None, shape),
                                       ("set_precision", None), ("bwd", "p")], "p", modes=("f16x3", "mixed"))
    # 5: two outstanding forwards, same and different frame sizes, backward in LIFO and FIFO order; each of the two is probed
    for sizes, (sa, sb) in (("same", (shape, shape)), ("diff", (other, shape))):
        for order, tags in (("lifo", ("b", "a")), ("fifo", ("a", "b"))):
            for probe in ("a", "b"):
                steps = [("train_fwd", "a", sa), ("train_fwd", "b", sb), ("bwd", tags[0]), ("bwd", tags[1])]
                T[f"5_two_forwards_{sizes}_{order}_probe_{probe}"] = _s(steps, probe)
    # 6: inference before and after a training step
    T["6_eval_train_eval"] = _s([("eval", "e1", None, shape), ("train_fwd", "a", shape), ("bwd", "a"), ("eval", "p", None, shape)], "p",
                                also=("e1",))
    # 7: scenarios 1 and 3 on the two-layer UPNet
    T["7_eval_then_train_two_layer"] = _s(s1, "p", modes=("two_layer",))
    T["7_f16_eval_between_two_layer"] = _s(s3, "p", modes=("two_layer",))
    # a dropped forward and an explicit zero_grad before the probe (what a skipped batch leaves behind)
    T["8_dropped_forward_then_train"] = _s([("train_fwd", "a", shape), ("drop", "a"), ("zero_grad",), ("train_fwd", "p", shape),
                                            ("bwd", "p")], "p")
    return T


def cases():
    """[(id, k, mode, scenario)] of every (scenario, shape, k, mode) that runs."""
    out = []
    for shape, other in ((SMALL, ODD), (ODD, SMALL)):
        for name, sc in scenarios(shape, other).items():
            for k in sc["ks"]:
                if k != 2 and SHAPE_FOR_K[k] != shape:
                    continue
                for mode in sc["modes"]:
                    out.append((f"{name}-k{k}-{'x'.join(map(str, shape))}-{mode}", k, mode, sc))
    return out


def check_scenario(sc):
    """Well-formedness: known step kinds with the right arity, unique tags, every bwd / drop names an earlier train_fwd that is still
    outstanding, exactly one probe, and the probe is a call that completes (an eval, or a train_fwd with its bwd)."""
    open_fwd, done, evals, seen = set(), set(), set(), set()
    for st in sc["steps"]:
        assert st[0] in STEP_ARITY and len(st) == STEP_ARITY[st[0]], st
        if st[0] in ("eval", "train_fwd"):
            assert st[1] not in seen, f"tag {st[1]!r} used twice"
            seen.add(st[1])
            (evals if st[0] == "eval" else open_fwd).add(st[1])
            assert len(st[-1]) == 3 and st[-1][1] % 2 == 0 and st[-1][2] % 2 == 0, st
        elif st[0] in ("bwd", "drop"):
            assert st[1] in open_fwd, f"{st[0]} of {st[1]!r} without an outstanding train_fwd"
            open_fwd.discard(st[1])
            if st[0] == "bwd":
                done.add(st[1])
        elif st[0] == "set_precision":
            assert st[1] in (None, "f16", "f16x3")
    probes = [sc["probe"]] if isinstance(sc["probe"], str) else list(sc["probe"])
    assert len(probes) == 1 and (probes[0] in done or probes[0] in evals), f"probe {sc['probe']!r} is not a completed call"
    assert all(t in evals for t in sc["also"])
    return True


def probe_context(sc):
    """(kind, shape, updates, precision) of the probe: what its result may depend on besides the module's switches — the update seeds
    applied before its forward, in order, and the precision setting in force at its forward (a per-call `prec` of an eval wins)."""
    updates, prec = [], None
    for st in sc["steps"]:
        if st[0] == "update":
            updates.append(st[1])
        elif st[0] == "set_precision":
            prec = st[1]
        elif st[0] in ("eval", "train_fwd") and st[1] == sc["probe"]:
            if st[0] == "eval" and st[2] is not None:
                prec = st[2]
            return st[0], st[-1], tuple(updates), prec
    raise AssertionError("no probe")


def clean_steps(sc):
    """The clean run of a scenario: the same updates and precision on a fresh module, then the probe alone."""
    kind, shape, updates, prec = probe_context(sc)
    steps = [("update", s) for s in updates] + [("set_precision", prec)]
    if kind == "eval":
        return steps + [("eval", sc["probe"], None, shape)]
    return steps + [("train_fwd", sc["probe"], shape), ("bwd", sc["probe"])]


# ------------------------------------------------------------------------------------------------ inputs, updates
def _seed(*key):
    return zlib.crc32(repr(key).encode())


def inputs(k, shape, salt=0):
    """k frames in [0, 1) and a white-noise upstream gradient, fixed per (k, shape, salt) (salt 0: what tests/test_gpu_backward_shapes.py
    feeds the same shape)."""
    n, H, W = shape
    gen = torch.Generator().manual_seed(_seed(k, n, H, W) if salt == 0 else _seed(k, n, H, W, salt))
    ins = [torch.rand(n, 3, H, W, generator=gen) for _ in range(k)]
    gout = torch.randn(n, 3, H, W, generator=gen) * 1e-3
    return ins, gout


def tag_salt(tag):
    """The probe-independent input choice of a tag: the calls "p" and "a" see the canonical inputs, any other tag its own."""
    return 0 if tag in ("p", "a", "e", "e1") else 1


UPDATE_SCALE = 1e-3


def perturbation(weights, seed):
    """{name: float32 delta} of one `update` step for `weights` {local name: CPU tensor}: UPDATE_SCALE * max|w| * N(0, 1) per entry, from a
    CPU generator seeded by (seed, name) — a function of the seed and the shapes alone."""
    out = {}
    for nm, w in weights.items():
        gen = torch.Generator().manual_seed(_seed("update", seed, nm))
        out[nm] = (torch.randn(w.shape, generator=gen) * (UPDATE_SCALE * float(w.abs().max()))).float()
    return out


def local_weights(canon_cpu, k):
    from bin_amd.weights import rdn_param_shapes
    return {n: canon_cpu[f"{SET_FOR_K[k]}.{n}"].clone() for n in rdn_param_shapes(k)}


def updated_weights(canon_cpu, k, seeds):
    """The canonical weight set of class k after the given `update` steps, in float32 as the device applies them (w += delta)."""
    w = local_weights(canon_cpu, k)
    for s in seeds:
        for nm, d in perturbation(w, s).items():
            w[nm] = w[nm] + d
    return w


def apply_update(mod, seed):
    """The `update` step on a module: the same perturbation, added in place on the module's device (bumps every version counter)."""
    params = dict(mod.named_parameters())
    delta = perturbation({n: p.detach().cpu() for n, p in params.items()}, seed)
    with torch.no_grad():
        for n, p in params.items():
            p.add_(delta[n].to(p.device))


# ------------------------------------------------------------------------------------------------ float64 reference
def float64_masks(weights, k, ins):
    """The dense-block ReLU masks of float64 itself, in call order (what saved_relu_masks reads off the device, for CPU-only use)."""
    import torch.nn.functional as F
    from oracle import rdn_oracle as O
    s = SET_FOR_K[k]
    masks = []

    def rdb_conv(x, w, b):
        z = F.conv2d(x, w, b, padding=1)
        masks.append(z.detach() > 0)
        return torch.cat((x, torch.relu(z)), 1)
    orig = O.rdb_conv
    O.rdb_conv = rdb_conv
    try:
        with torch.no_grad():
            O.rdn([t.double() for t in ins], {f"{s}.{n}": w.double() for n, w in weights.items()}, s)
    finally:
        O.rdb_conv = orig
    return masks


def oracle_grads(weights, k, ins, gout, masks, label=""):
    """{name: float64 gradient} of one call of weight class k with `weights` {local name: CPU float32}: every parameter under its local
    name, the frames as in0 .. in{k-1}.  backward_cases.oracle_rdn_grads with its TIE rule, unchanged; prints the ties decided."""
    s = SET_FOR_K[k]
    W = {f"{s}.{n}": w.double().requires_grad_(True) for n, w in weights.items()}
    xs = [t.double().requires_grad_(True) for t in ins]
    leaves = {n: W[f"{s}.{n}"] for n in weights}
    leaves.update({f"in{j}": x for j, x in enumerate(xs)})
    (ref,), ties, flips = oracle_rdn_grads(W, s, leaves, xs, [gout], masks)
    print(f"oracle {label} k={k} {tuple(ins[0].shape)}: {ties} ReLU ties, {flips} decided otherwise than float64 by the kernels")
    return ref
