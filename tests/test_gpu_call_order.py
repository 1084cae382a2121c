"""-m gpu: RDN training and inference under interleaved call orders.  Case table and helpers: tests/call_order_cases.py.

What a call computes also depends on state that survives between calls — the module's one-entry kernel-weight cache, the fused UPNet's
operands on it, the per-weight-set count of owed backward calls, the workspace a forward keeps for its backward, the per-stream workspaces.
The rest of the suite drives a fresh module through one canonical sequence; here the sequence is varied and the contract pinned:

C1  History independence.  The result of a call is a function of its inputs, the parameter values, the precision settings, grad mode and
    the module's switches (plan_flags, backward_precision, wgrad_side_stream, the BIN_AMD_* defaults read at construction) — never of the
    calls that came before on the same parameter version.  Inference outputs, training outputs and every gradient; equality is torch.equal.
C2  A backward uses the weight objects its own forward used.  Changing precision, or running other calls on the module between a forward
    and its backward, does not change that backward's result.
C3  A call that cannot be honoured (a second backward through a released graph, a backward after the weights changed) raises RuntimeError
    naming the cause, on the host before any kernel is launched (the checks sit ahead of binhip_rdn_backward in _RdnFn.backward), and
    leaves no residue: the next complete forward and backward behaves as on a fresh module, including exactly one gradients-ready callback.

Per scenario, on the probe: (a) outputs and every gradient torch.equal to the clean run (a fresh module with the same weights executing the
probe alone); (b) the UPNet path that ran is the one the switches select, observed from the plan flags the forward passed to the library
(and from the backward's debug-hook info); (c) the clean run meets backward_cases.RDN_BARS against float64 with the unchanged tie rule, so
bit-equality to a wrong run cannot pass; (d) ops.check_status() is clean."""
import hashlib

import pytest
import torch

import call_order_cases as CO
from backward_cases import RDN_BARS, rel, saved_relu_masks

pytestmark = pytest.mark.gpu

RDN_SHAPE = (96, 12, 4, 32)
_CLEAN = {}             # (k, mode, kind, shape, updates, precision, salt) -> clean-run result
_ORACLE = {}            # (k, shape, updates, salt, mask hash) -> float64 gradients: one oracle backward per (k, shape, weights), shared by modes


def _env(monkeypatch, mode):
    for v in ("BIN_AMD_PRECISION", "BIN_AMD_TRAIN_PRECISION", "BIN_AMD_BACKWARD_PRECISION", "BIN_AMD_FUSED_UPNET", "BIN_AMD_WGRAD_STREAM"):
        monkeypatch.delenv(v, raising=False)
    if mode == "two_layer":
        monkeypatch.setenv("BIN_AMD_FUSED_UPNET_TRAIN", "0")
    else:
        monkeypatch.delenv("BIN_AMD_FUSED_UPNET_TRAIN", raising=False)


def _module(canon_cpu, k, mode, weights=None):
    from bin_amd.models.archs import RDN as A
    cls = {2: A.RDN_residual_interp_2_input, 3: A.RDN_residual_interp_2_1_input, 5: A.RDN_residual_interp_4_1_input}[k]
    mod = cls(G0=96, D=12)
    mod.load_state_dict(weights if weights is not None else CO.local_weights(canon_cpu, k))
    mod = mod.cuda()
    assert mod.precision is None
    mod.backward_precision = "f16" if mode == "mixed" else None
    return mod


class _Watch:
    """Observes what ran: the plan flags of every differentiable forward (wrapping the `rdn_forward` that bin_amd.autograd calls) and the
    debug-hook info of every forward / backward of one module."""

    def __init__(self, monkeypatch, mod):
        from bin_amd import _lib as L
        from bin_amd import autograd as ag
        self.fwd_fused, self.bwd_info, self.masks = [], [], []
        inner = ag.rdn_forward

        def rdn_forward(weights, frames, **kw):
            self.fwd_fused.append(bool(kw["flags"] & L.PLAN_FUSED_UPNET_TRAIN))
            return inner(weights, frames, **kw)
        monkeypatch.setattr(ag, "rdn_forward", rdn_forward)

        def hook(kind, module, dims, ws, info):
            if kind == "forward":
                self.masks.append(saved_relu_masks(ws, dims, RDN_SHAPE))
            else:
                self.bwd_info.append(dict(info))
        mod.debug_hook = hook


def _take_grads(mod, xs):
    g = {n: p.grad.detach().cpu().clone() for n, p in mod.named_parameters()}
    assert all(x.grad is not None for x in xs)
    g.update({f"in{i}": x.grad.cpu() for i, x in enumerate(xs)})
    for p in mod.parameters():
        p.grad = None
    return g


def run_steps(mod, k, steps, watch):
    """Execute `steps` on `mod`; {tag: {"out", "grads", "fused", "masks"}} of every call."""
    from bin_amd import ops
    res, live = {}, {}
    for st in steps:
        kind = st[0]
        if kind == "eval":
            _, tag, prec, shape = st
            ins, _ = CO.inputs(k, shape, CO.tag_salt(tag))
            keep = mod.precision
            if prec is not None:
                mod.precision = prec
            with torch.no_grad():
                res[tag] = {"out": mod(*[t.cuda() for t in ins]).cpu()}
            mod.precision = keep
        elif kind == "train_fwd":
            _, tag, shape = st
            ins, gout = CO.inputs(k, shape, CO.tag_salt(tag))
            xs = [t.cuda().requires_grad_(True) for t in ins]
            nf = len(watch.fwd_fused)
            out = mod(*xs)
            assert len(watch.fwd_fused) == nf + 1 and len(watch.masks) == nf + 1
            live[tag] = (out, xs, gout)
            res[tag] = {"out": out.detach().cpu().clone(), "fused": watch.fwd_fused[-1], "masks": watch.masks[-1]}
        elif kind == "bwd":
            out, xs, gout = live.pop(st[1])
            nb = len(watch.bwd_info)
            out.backward(gout.cuda())
            assert len(watch.bwd_info) == nb + 1
            res[st[1]]["grads"] = _take_grads(mod, xs)
            res[st[1]]["bwd_fused"] = watch.bwd_info[-1].get("fused_upnet")
        elif kind == "update":
            CO.apply_update(mod, st[1])
        elif kind == "set_precision":
            mod.precision = st[1]
        elif kind == "zero_grad":
            for p in mod.parameters():
                p.grad = None
        elif kind == "drop":
            live.pop(st[1])
        else:
            raise AssertionError(st)
    assert not live
    torch.cuda.synchronize()
    ops.check_status()                                                            # (d)
    return res


def _check_oracle(canon_cpu, k, mode, shape, updates, salt, got, label):
    """(c): the clean run's gradients against float64 at RDN_BARS[mode]; the float64 backward is computed once per (k, shape, weights, masks)."""
    masks = got["masks"]
    key = (k, shape, updates, salt, hashlib.sha1(b"".join(m.numpy().tobytes() for m in masks)).hexdigest())
    if key not in _ORACLE:
        ins, gout = CO.inputs(k, shape, salt)
        _ORACLE[key] = CO.oracle_grads(CO.updated_weights(canon_cpu, k, updates), k, ins, gout, masks, label)
    ref = _ORACLE[key]
    assert len(got["grads"]) == len(ref) == 132 + k
    errs = {n: rel(got["grads"][n], ref[n]) for n in ref}
    worst = max(errs, key=errs.get)
    print(f"{label}: clean run vs float64, worst relative error {errs[worst]:.2e} ({worst}; bar {RDN_BARS[mode]:.0e})")
    bad = {n: e for n, e in errs.items() if not e <= RDN_BARS[mode]}
    assert not bad, bad


def clean_run(canon_cpu, monkeypatch, k, mode, sc):
    """The probe of `sc` executed alone on a fresh module with the same weights, updates and precision; checked against float64 (c)."""
    kind, shape, updates, prec = CO.probe_context(sc)
    salt = CO.tag_salt(sc["probe"])
    key = (k, mode, kind, shape, updates, prec, salt)
    label = f"k={k} {shape} {mode} updates={updates} precision={prec} inputs#{salt}"
    if key not in _CLEAN:
        mod = _module(canon_cpu, k, mode)
        got = run_steps(mod, k, CO.clean_steps(sc), _Watch(monkeypatch, mod))[sc["probe"]]
        want = CO.updated_weights(canon_cpu, k, updates)
        assert all(torch.equal(p.detach().cpu(), want[n]) for n, p in mod.named_parameters()), "the updates did not replay"
        _CLEAN[key] = got
    got = _CLEAN[key]
    if kind == "train_fwd":
        _check_oracle(canon_cpu, k, mode, shape, updates, salt, got, label)
    return got


def _same(a, b, what):
    diff = [n for n in a if not torch.equal(a[n], b[n])]
    assert set(a) == set(b) and not diff, f"{what}: {len(diff)} of {len(a)} tensors differ bit for bit, first {diff[:4]}; " \
                                          f"worst relative difference {max(rel(a[n], b[n]) for n in diff):.2e}"


CASES = CO.cases()


@pytest.mark.parametrize("cid,k,mode,sc", CASES, ids=[c[0] for c in CASES])
def test_probe_equals_the_clean_run(cid, k, mode, sc, canon_cpu, monkeypatch):
    """One scenario of call_order_cases.scenarios: (a) - (d) of the module docstring on its probe."""
    _env(monkeypatch, mode)
    clean = clean_run(canon_cpu, monkeypatch, k, mode, sc)
    mod = _module(canon_cpu, k, mode)
    res = run_steps(mod, k, sc["steps"], _Watch(monkeypatch, mod))
    got = res[sc["probe"]]
    assert torch.equal(got["out"], clean["out"]), f"{cid}: the probe's output differs from the clean run's, " \
                                                  f"max-abs {float((got['out'] - clean['out']).abs().max()):.2e}"
    for tag in sc["also"]:
        assert torch.equal(res[tag]["out"], clean["out"]), f"{cid}: output of {tag!r} differs from the clean run's"
    if "grads" in clean:
        want = mode != "two_layer"
        for tag, r in res.items():                                                # (b), for every differentiable call of the scenario
            if "fused" in r:
                assert r["fused"] == want, f"{cid}: forward {tag!r} ran the {'fused' if r['fused'] else 'two-layer'} UPNet"
            if r.get("bwd_fused") is not None:
                assert r["bwd_fused"] == want, f"{cid}: backward {tag!r} ran the {'fused' if r['bwd_fused'] else 'two-layer'} UPNet"
        assert clean["fused"] == want
        assert all(torch.equal(a, b) for a, b in zip(got["masks"], clean["masks"])), f"{cid}: saved ReLU masks differ from the clean run's"
        _same(got["grads"], clean["grads"], cid)                                   # (a)


# ------------------------------------------------------------------------------------------------ wrapper level
def _opt(tmp_path, lr=1e-4):
    return {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
            "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": None},
            "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp_path), "training_state": str(tmp_path)},
            "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None,
                      "lr_G": lr, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                      "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}


def _batch(seed, S=32):
    g = torch.Generator().manual_seed(seed)
    return {"LQs": torch.rand(1, 6, 3, S, S, generator=g), "GTenh": torch.rand(1, 6, 3, S, S, generator=g),
            "GTinp": torch.rand(1, 5, 3, S, S, generator=g)}


def test_training_is_reproducible_across_the_validation_schedule(tmp_path, monkeypatch):
    """bin_model: three optimize_parameters steps on fixed 1 x 32 x 32 batches, once with a no_grad validation forward (the wrapper's
    test()) after every step and once without: every parameter after step 3 is the same bits, and each validation output equals that
    of a fresh model loaded with the weights of that step."""
    from bin_amd import ops
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    _env(monkeypatch, "f16x3")
    val = tuple(_batch(100)["LQs"][:, i] for i in range(6)) + (None,)

    def run(validate):
        m = create_model(_opt(tmp_path))
        m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
        outs, states = [], []
        for step in (1, 2, 3):
            m.feed_data(_batch(step))
            m.optimize_parameters(step)
            if validate:
                m.test_set_input(val)
                outs.append([o.clone() for o in m.test()])
                states.append({n: t.detach().clone() for n, t in m.netG.module.state_dict().items()})
        torch.cuda.synchronize()
        ops.check_status()
        return {n: p.detach().clone() for n, p in m.netG.module.named_parameters()}, outs, states

    with_val, outs, states = run(True)
    without, _, _ = run(False)
    diff = [n for n in without if not torch.equal(with_val[n], without[n])]
    assert not diff, f"{len(diff)} of {len(without)} parameters depend on the validation schedule, first {diff[:4]}"
    assert any(not torch.equal(states[0][n], states[2][n]) for n in states[0]), "the steps did not move the weights"
    for step, (got, sd) in enumerate(zip(outs, states), 1):
        fresh = create_model(_opt(tmp_path))
        fresh.netG.module.load_state_dict(sd, strict=True)
        fresh.test_set_input(val)
        ref = fresh.test()
        assert len(ref) == len(got) == 14
        bad = [i for i in range(14) if not torch.equal(ref[i], got[i])]
        assert not bad, f"validation after step {step}: outputs {bad} differ from a fresh model's with the same weights"


# ------------------------------------------------------------------------------------------------ gradient routing
ROUTE_K, ROUTE_SHAPE = 2, CO.SMALL
_FULL = {"steps": [("train_fwd", "p", ROUTE_SHAPE), ("bwd", "p")], "probe": "p", "also": ()}


def _call(mod, k, shape, salt, direct, requires_frames=True):
    """One forward + backward under direct_param_grads(direct), leaving .grad as the call left it; the frame gradients."""
    ins, gout = CO.inputs(k, shape, salt)
    xs = [t.cuda().requires_grad_(requires_frames) for t in ins]
    out = mod(*xs)
    with mod.direct_param_grads(direct):
        out.backward(gout.cuda())
    return {f"in{i}": x.grad.cpu() for i, x in enumerate(xs) if x.grad is not None}


@pytest.mark.parametrize("direct", [False, True], ids=["autograd", "direct"])
def test_only_the_frames_require_a_gradient(direct, canon_cpu, monkeypatch):
    """Frozen parameters: the frame gradients are the full run's bit for bit and no .grad appears."""
    from bin_amd import ops
    _env(monkeypatch, "f16x3")
    full = clean_run(canon_cpu, monkeypatch, ROUTE_K, "f16x3", _FULL)["grads"]
    mod = _module(canon_cpu, ROUTE_K, "f16x3")
    for p in mod.parameters():
        p.requires_grad_(False)
    gin = _call(mod, ROUTE_K, ROUTE_SHAPE, 0, direct)
    torch.cuda.synchronize()
    ops.check_status()
    assert set(gin) == {"in0", "in1"}
    _same(gin, {n: full[n] for n in gin}, "frame gradients with frozen parameters")
    assert all(p.grad is None for p in mod.parameters())
    assert mod._bwd_pending == 0


@pytest.mark.parametrize("direct", [False, True], ids=["autograd", "direct"])
@pytest.mark.parametrize("prefix", ["UPNet.", "SFENet1."])
def test_a_subset_of_the_parameters_requires_a_gradient(prefix, direct, canon_cpu, monkeypatch):
    """Partially frozen: the trainable parameters' gradients and the frame gradients are the full run's bit for bit, the others stay None."""
    from bin_amd import ops
    _env(monkeypatch, "f16x3")
    full = clean_run(canon_cpu, monkeypatch, ROUTE_K, "f16x3", _FULL)["grads"]
    mod = _module(canon_cpu, ROUTE_K, "f16x3")
    for n, p in mod.named_parameters():
        p.requires_grad_(n.startswith(prefix))
    got = _call(mod, ROUTE_K, ROUTE_SHAPE, 0, direct)
    torch.cuda.synchronize()
    ops.check_status()
    named = dict(mod.named_parameters())
    on = [n for n in named if n.startswith(prefix)]
    assert len(on) in (2, 4) and all(named[n].grad is None for n in named if n not in on)
    got.update({n: named[n].grad.cpu() for n in on})
    _same(got, {n: full[n] for n in got}, f"gradients with only {prefix}* trainable")
    assert mod._bwd_pending == 0


def test_mixed_grad_state_equals_autograd_accumulation(canon_cpu, monkeypatch):
    """Some .grad set (to zeros), some None: direct_param_grads gives what plain autograd accumulation gives, bit for bit, and that is the
    call's gradient (the full run's, which (c) holds against float64)."""
    from bin_amd import ops
    _env(monkeypatch, "f16x3")
    full = clean_run(canon_cpu, monkeypatch, ROUTE_K, "f16x3", _FULL)["grads"]
    res = {}
    for direct in (False, True):
        mod = _module(canon_cpu, ROUTE_K, "f16x3")
        for i, p in enumerate(mod.parameters()):
            p.grad = torch.zeros_like(p) if i % 3 == 0 else None
        res[direct] = _call(mod, ROUTE_K, ROUTE_SHAPE, 0, direct)
        res[direct].update({n: p.grad.cpu() for n, p in mod.named_parameters()})
        torch.cuda.synchronize()
        ops.check_status()
    _same(res[True], res[False], "mixed .grad state, direct against autograd accumulation")
    _same(res[False], full, "mixed .grad state against the full run")


def test_two_micro_batches_accumulate_as_autograd_does(canon_cpu, monkeypatch):
    """Two forward + backward calls without zero_grad in between: direct_param_grads (first call writes, second accumulates in the kernels)
    equals plain autograd accumulation bit for bit, and the sum meets the f16x3 bar against the float64 gradient of the summed loss (one
    float64 call on the concatenated batch; additive by tests/test_cpu_call_order.py)."""
    from bin_amd import ops
    _env(monkeypatch, "f16x3")
    k, shape = ROUTE_K, ROUTE_SHAPE
    res, masks = {}, None
    for direct in (False, True):
        mod = _module(canon_cpu, k, "f16x3")
        watch = _Watch(monkeypatch, mod)
        ga = _call(mod, k, shape, 0, direct)
        gb = _call(mod, k, shape, 1, direct)
        torch.cuda.synchronize()
        ops.check_status()
        res[direct] = {n: p.grad.cpu() for n, p in mod.named_parameters()}
        res[direct].update({f"in{j}": torch.cat((ga[f"in{j}"], gb[f"in{j}"])) for j in range(k)})
        assert len(watch.masks) == 2 and watch.fwd_fused == [True, True]
        masks = [torch.cat((x, y)) for x, y in zip(*watch.masks)]
        assert mod._bwd_pending == 0
    _same(res[True], res[False], "two accumulated micro-batches, direct against autograd accumulation")
    (ia, gA), (ib, gB) = CO.inputs(k, shape, 0), CO.inputs(k, shape, 1)
    ref = CO.oracle_grads(CO.local_weights(canon_cpu, k), k, [torch.cat((x, y)) for x, y in zip(ia, ib)], torch.cat((gA, gB)), masks,
                          "two micro-batches")
    errs = {n: rel(res[True][n], ref[n]) for n in ref}
    worst = max(errs, key=errs.get)
    print(f"two accumulated micro-batches vs float64 of the summed loss: worst {errs[worst]:.2e} ({worst}; bar {RDN_BARS['f16x3']:.0e})")
    bad = {n: e for n, e in errs.items() if not e <= RDN_BARS["f16x3"]}
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ error paths (C3)
def _counted(mod):
    calls = []
    mod._grads_ready_cb = lambda: calls.append(mod._bwd_pending)
    return calls


def _complete_step_is_clean(mod, calls, full):
    """One complete forward + backward on `mod`: gradients of a fresh module, exactly one callback, nothing owed."""
    from bin_amd import ops
    for p in mod.parameters():
        p.grad = None
    before = len(calls)
    got = _call(mod, ROUTE_K, ROUTE_SHAPE, 0, True)
    got.update({n: p.grad.cpu() for n, p in mod.named_parameters()})
    torch.cuda.synchronize()
    ops.check_status()
    _same(got, full, "the step after a refused backward")
    assert len(calls) == before + 1 and calls[-1] == 0, f"gradients-ready callback fired {len(calls) - before} times"
    assert mod._bwd_pending == 0


def test_second_backward_raises_and_leaves_no_residue(canon_cpu, monkeypatch):
    """backward(retain_graph=True) twice: the forward's workspace is released by the first backward, so the second raises a RuntimeError
    that says so (on the host: `saved_ws is None` is the first thing _RdnFn.backward looks at) and changes nothing."""
    _env(monkeypatch, "f16x3")
    full = clean_run(canon_cpu, monkeypatch, ROUTE_K, "f16x3", _FULL)["grads"]
    mod = _module(canon_cpu, ROUTE_K, "f16x3")
    calls = _counted(mod)
    ins, gout = CO.inputs(ROUTE_K, ROUTE_SHAPE, 0)
    xs = [t.cuda().requires_grad_(True) for t in ins]
    out = mod(*xs)
    with mod.direct_param_grads():
        out.backward(gout.cuda(), retain_graph=True)
        first = {n: p.grad.clone() for n, p in mod.named_parameters()}
        assert len(calls) == 1 and mod._bwd_pending == 0
        with pytest.raises(RuntimeError, match="saved activations of this RDN call were released"):
            out.backward(gout.cuda())
    assert len(calls) == 1 and mod._bwd_pending == 0
    assert all(torch.equal(p.grad, first[n]) for n, p in mod.named_parameters()), "the refused backward touched a gradient"
    _complete_step_is_clean(mod, calls, full)


def test_backward_after_a_weight_change_raises_and_leaves_no_residue(canon_cpu, monkeypatch):
    """The "modified in place" refusal (the version check ahead of everything else in the backward) gives back the backward call this
    forward owed: the next step's callback fires, once."""
    _env(monkeypatch, "f16x3")
    full = clean_run(canon_cpu, monkeypatch, ROUTE_K, "f16x3", _FULL)["grads"]
    mod = _module(canon_cpu, ROUTE_K, "f16x3")
    calls = _counted(mod)
    ins, gout = CO.inputs(ROUTE_K, ROUTE_SHAPE, 0)
    out = mod(*[t.cuda().requires_grad_(True) for t in ins])
    assert mod._bwd_pending == 1
    with torch.no_grad():
        mod.SFENet1.weight.mul_(1.0)                      # same values, new version
    with mod.direct_param_grads():
        with pytest.raises(RuntimeError, match="modified in place"):
            out.backward(gout.cuda())
        with pytest.raises(RuntimeError, match="saved activations of this RDN call were released"):
            out.backward(gout.cuda())                     # the refusal released the workspace: asking again does not count twice
    assert not calls and mod._bwd_pending == 0
    assert all(p.grad is None for p in mod.parameters())
    _complete_step_is_clean(mod, calls, full)


def test_attach_restores_the_count_after_a_dropped_forward(monkeypatch):
    """A grad-enabled forward whose result is dropped leaves its owed backward calls on the weight sets; FlatGradAllReduce.attach() (every
    step of a data-parallel run starts with it) resets them, so the next step's callback fires once per watched weight set."""
    from bin_amd import ops
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.models.bin_model import FlatGradAllReduce
    from bin_amd.weights import reference_state_dict, synthetic_frames
    _env(monkeypatch, "f16x3")
    frames = [f.cuda() for f in synthetic_frames(3, 1, 32, 32, 6)]
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    net = net.cuda().train()
    sync = FlatGradAllReduce(net.parameters()).watch(net)
    mods = [m for m, _, _ in sync._buckets]
    assert len(mods) == 4
    fired = {id(m): 0 for m in mods}
    for m in mods:
        inner = m._grads_ready_cb

        def cb(m=m, inner=inner):
            fired[id(m)] += 1
            inner()
        m._grads_ready_cb = cb
    sync.attach()
    out = net(*frames)
    assert all(m._bwd_pending >= 1 for m in mods)
    del out                                               # a skipped batch: no backward
    sync.attach()
    assert all(m._bwd_pending == 0 for m in mods)
    loss = sum((o * o).mean() for o in net(*frames))
    with net.direct_param_grads():
        loss.backward()
    torch.cuda.synchronize()
    ops.check_status()
    assert [fired[id(m)] for m in mods] == [1, 1, 1, 1] and all(m._bwd_pending == 0 for m in mods)
    assert sync._views_intact()
