"""-m gpu: the Adam kernel (binopt_adam_step), bin_amd.optim.Adam over it and `train.optimizer: hip` through the wrappers.
Case table, references and the bar max(4 * e32, 2^-23 * max|reference|): optim_cases.py; CPU pins: test_cpu_optim.py.  Each
comparison prints the case's largest error / bar per output on a line that starts with `[optim]`.

Measured on an MI355X when this module was written, largest error / bar over the case table: see DESIGN.md ("The Adam kernel")."""
import ctypes as C
import functools
from collections import defaultdict

import numpy as np
import pytest
import torch

import optim_cases as OC
from conftest import load_golden

pytestmark = pytest.mark.gpu

KINDS = ("p", "g", "m", "v")


def _lib():
    from bin_amd import _lib as L
    return L, L.optlib()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _make_refs(tag):
    case = OC.CASE_BY_TAG[tag]
    inp = OC.make_inputs(case)
    return inp, OC.reference64(case, inp), OC.torch32(case, inp)


_cached_refs = functools.lru_cache(maxsize=None)(_make_refs)


def _refs(tag):
    """(inputs, float64 reference, float32 torch on the CPU) of a case: computed once, shared by the tests that need it, never
    written to.  (The 11.44 M-element case is used once and not kept.)"""
    return _cached_refs(tag) if OC.CASE_BY_TAG[tag].cpu else _make_refs(tag)


def _run_kernel(case, inp, order=None):
    """All steps of `case` through the C ABI on arenas with guards (optim_cases.layout); `order`: a permutation of the rows in the
    table handed to the library.  -> ({"p", "m", "v"}: row arrays, the four arenas with the rows blanked, the g arena as left)."""
    L, lib = _lib()
    rows = OC.rows_of(case)
    dev = torch.device("cuda")
    host = {"p": OC.arena(rows, 0, inp["p"]), "m": OC.arena(rows, 2, inp.get("m")), "v": OC.arena(rows, 3, inp.get("v"))}
    buf = {k: torch.from_numpy(a).to(dev) for k, a in host.items()}
    buf["g"] = torch.empty(OC.layout(rows, 1)[1], dtype=torch.float32, device=dev)
    starts = {k: OC.layout(rows, i)[0] for i, k in enumerate(KINDS)}
    for k in KINDS:
        assert buf[k].data_ptr() % 16 == 0
    idx = list(range(len(rows))) if order is None else list(order)
    table = (L.BinAdamTensor * len(rows))()
    g_host = None
    t0 = inp.get("t0", 0)
    for t in range(t0 + 1, t0 + case.steps + 1):
        g_host = OC.arena(rows, 1, inp["g"][t - t0 - 1])
        buf["g"].copy_(torch.from_numpy(g_host))
        step_size, inv_sqrt_bc2 = OC.bias_factors(case, t)
        for slot, i in enumerate(idx):
            r = table[slot]
            r.p, r.g, r.m, r.v = (buf[k].data_ptr() + 4 * starts[k][i] for k in KINDS)
            r.numel, r.step_size, r.inv_sqrt_bc2 = rows[i].numel, step_size, inv_sqrt_bc2
        L.check(lib.binopt_adam_step(table, len(rows), case.betas[0], case.betas[1], case.eps, case.weight_decay, _stream()),
                "adam_step")
    torch.cuda.synchronize()
    got, blank = {}, {}
    for i, k in enumerate(KINDS):
        vals, blank[k] = OC.split(rows, i, buf[k].cpu().numpy())
        if k != "g":
            got[k] = vals
    return got, blank, (buf["g"].cpu().numpy(), g_host)


def _guards_intact(case, blank, g_pair):
    rows = OC.rows_of(case)
    for i, k in enumerate(KINDS):
        want = np.full(OC.layout(rows, i)[1], OC.GUARD, np.float32)
        assert np.array_equal(blank[k].view(np.uint32), want.view(np.uint32)), f"{case.tag}: a float outside the rows of {k} changed"
    assert np.array_equal(g_pair[0].view(np.uint32), g_pair[1].view(np.uint32)), f"{case.tag}: the gradients were written"


# ------------------------------------------------------------------------------------------------ 1. the kernel against float64
@pytest.mark.parametrize("tag", [c.tag for c in OC.CASES])
def test_adam_step_vs_float64(tag):
    """binopt_adam_step over the case table: p, m and v of every row within max(4 * e32, 2^-23 * max|reference|) of the formulas in
    float64, the float on either side of every buffer untouched, the gradients unwritten."""
    case = OC.CASE_BY_TAG[tag]
    inp, r64, r32 = _refs(tag)
    got, blank, g_pair = _run_kernel(case, inp)
    _guards_intact(case, blank, g_pair)
    OC.compare(tag, OC.rows_of(case), got, r64, r32)


# ------------------------------------------------------------------------------------------------ 2. exactness
@pytest.mark.parametrize("tag", [c.tag for c in OC.CASES if c.lr == 0.0 and c.cpu])
def test_zero_lr_leaves_the_parameters_bit_unchanged(tag):
    case = OC.CASE_BY_TAG[tag]
    inp, _, _ = _refs(tag)
    got, _, _ = _run_kernel(case, inp)
    for i, (a, b) in enumerate(zip(got["p"], inp["p"])):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (tag, i)
        assert np.abs(got["m"][i]).max() > 0 and np.abs(got["v"][i]).max() > 0, "m and v must advance"


@pytest.mark.parametrize("tag", ["numel_all_off_differently", "numel_aligned", f"rows_{OC.ADAM_MAX_TENSORS + 1}"])
def test_two_runs_and_reversed_rows_give_the_same_bits(tag):
    case = OC.CASE_BY_TAG[tag]
    inp, _, _ = _refs(tag)
    n = len(OC.rows_of(case))
    a, _, _ = _run_kernel(case, inp)
    b, _, _ = _run_kernel(case, inp)
    c, blank, g_pair = _run_kernel(case, inp, order=range(n - 1, -1, -1))
    _guards_intact(case, blank, g_pair)
    for k in ("p", "m", "v"):
        for i in range(n):
            assert np.array_equal(a[k][i].view(np.uint32), b[k][i].view(np.uint32)), (tag, k, i, "second run")
            assert np.array_equal(a[k][i].view(np.uint32), c[k][i].view(np.uint32)), (tag, k, i, "reversed rows")


# ------------------------------------------------------------------------------------------------ 3. non-finite gradients
def test_non_finite_gradients_spread_as_in_float32_torch():
    """NaN, +inf and -inf at known places of the first step's gradients (the vector body, the partial chunk, a misaligned row, a
    3-element row), a finite second step: p, m and v are non-finite exactly where float32 torch on the CPU is, and every other
    element stays within the bar."""
    rows = (OC.Row(4097, (0, 0, 0, 0), 1.0), OC.Row(257, (0, 1, 0, 0), 1e-3), OC.Row(3, (0, 0, 0, 0), 1.0), OC.Row(2048, (2, 2, 2, 2), 1e-6))
    case = OC.Case("non_finite", rows, 2, 2e-4, (0.9, 0.999), 1e-8, 1e-2, True, 4242)
    inp = OC.make_inputs(case)
    places = {0: ((0, np.nan), (5, np.inf), (2047, -np.inf), (4096, np.nan), (4094, np.inf)), 1: ((0, -np.inf), (256, np.nan), (100, np.inf)),
              2: ((1, np.inf),), 3: ((2047, np.nan), (1, -np.inf))}
    for i, items in places.items():
        for j, val in items:
            inp["g"][0][i][j] = val
    r64, r32 = OC.reference64(case, inp), OC.torch32(case, inp)
    got, blank, g_pair = _run_kernel(case, inp)
    assert np.array_equal(blank["p"].view(np.uint32), np.full_like(blank["p"], OC.GUARD).view(np.uint32))
    mask = {}
    for k in ("p", "m", "v"):
        mask[k] = []
        for i in range(len(rows)):
            bad32, bad = ~np.isfinite(r32[k][i]), ~np.isfinite(got[k][i])
            assert np.array_equal(bad, bad32), (k, i, np.flatnonzero(bad), np.flatnonzero(bad32))
            assert np.array_equal(bad, ~np.isfinite(r64[k][i])), (k, i)
            assert set(np.flatnonzero(bad)) == {j for j, _ in places[i]}, (k, i)
            mask[k].append(~bad)
    OC.compare("non_finite", rows, got, r64, r32, mask)


# ------------------------------------------------------------------------------------------------ the entry point's contract
def test_entry_point_rejects_bad_arguments_before_any_launch():
    L, lib = _lib()
    dev = torch.device("cuda")
    bufs = [torch.full((64,), 3.0, device=dev) for _ in range(8)]
    table = (L.BinAdamTensor * 2)()
    for slot in range(2):
        r = table[slot]
        r.p, r.g, r.m, r.v = (bufs[4 * slot + j].data_ptr() for j in range(4))
        r.numel, r.step_size, r.inv_sqrt_bc2 = 64, 1e-3, 1.0
    args = (0.9, 0.999, 1e-8, 0.0)
    assert lib.binopt_adam_step(table, 0, *args, _stream()) == 0
    assert lib.binopt_adam_step(None, 0, *args, _stream()) == 0
    assert lib.binopt_adam_step(table, -1, *args, _stream()) == -1
    assert lib.binopt_adam_step(None, 2, *args, _stream()) == -1
    for b1, b2 in ((1.0, 0.999), (0.9, 1.0), (-0.1, 0.999), (0.9, -1e-3), (float("nan"), 0.999), (0.9, float("nan")), (1.5, 0.5)):
        assert lib.binopt_adam_step(table, 2, b1, b2, 1e-8, 0.0, _stream()) == -1, (b1, b2)
    for field in ("p", "g", "m", "v"):                     # a bad SECOND row: the first must not have been launched
        keep = getattr(table[1], field)
        setattr(table[1], field, None)
        assert lib.binopt_adam_step(table, 2, *args, _stream()) == -1, field
        setattr(table[1], field, keep)
    for numel in (0, -5):
        table[1].numel = numel
        assert lib.binopt_adam_step(table, 2, *args, _stream()) == -1, numel
    table[1].numel = 64
    torch.cuda.synchronize()
    assert all(float(b.min()) == 3.0 == float(b.max()) for b in bufs), "a refused call wrote something"
    assert lib.binopt_adam_step(table, 2, *args, _stream()) == 0
    torch.cuda.synchronize()
    assert float(bufs[0].max()) < 3.0 and float(bufs[4].max()) < 3.0 and float(bufs[1].min()) == 3.0


def test_ops_adam_step_checks_its_tensors():
    from bin_amd import ops
    dev = torch.device("cuda")
    ok = lambda: torch.ones(8, 4, device=dev)
    ops.adam_step([], 0.9, 0.999, 1e-8, 0.0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.adam_step([(torch.ones(4), torch.ones(4), torch.ones(4), torch.ones(4), 1e-3, 1.0)], 0.9, 0.999, 1e-8, 0.0)
    for bad in range(4):
        ts = [ok() for _ in range(4)]
        ts[bad] = ts[bad].double()
        with pytest.raises(ValueError, match="float32"):
            ops.adam_step([(*ts, 1e-3, 1.0)], 0.9, 0.999, 1e-8, 0.0)
        ts = [ok() for _ in range(4)]
        ts[bad] = torch.ones(4, 8, device=dev).t()
        with pytest.raises(ValueError, match="contiguous"):
            ops.adam_step([(*ts, 1e-3, 1.0)], 0.9, 0.999, 1e-8, 0.0)
    p, g, m, v = ok(), ok(), torch.zeros(8, 4, device=dev), torch.zeros(8, 4, device=dev)
    ops.adam_step([(p, g, m, v, 1e-3, 1.0)], 0.9, 0.999, 1e-8, 0.0)
    assert float(p.max()) < 1.0 and float(m.min()) > 0 and float(v.min()) > 0 and float(g.min()) == 1.0


# ------------------------------------------------------------------------------------------------ 4. the Adam class
def _params(values, device="cuda"):
    return [torch.nn.Parameter(torch.from_numpy(x.copy()).to(device)) for x in values]


def _set_grads(params, grads):
    for q, g in zip(params, grads):
        q.grad = None if g is None else torch.from_numpy(g.copy()).to(q.device)


def _state_of(opt, params):
    return {"p": [q.detach().cpu().numpy() for q in params], "m": [opt.state[q]["exp_avg"].cpu().numpy() for q in params],
            "v": [opt.state[q]["exp_avg_sq"].cpu().numpy() for q in params]}


_CLASS_ROWS = (OC.Row(4097, (0,) * 4, 1.0), OC.Row(257, (0,) * 4, 1e-3), OC.Row(5, (0,) * 4, 1e-6), OC.Row(2048, (0,) * 4, 1e4),
               OC.Row(96, (0,) * 4, 1e-12))


def test_adam_class_matches_float64_and_counts_steps_per_parameter():
    """Five steps; parameter 1 has no gradient until step 3, parameter 2 never has one: it keeps its values and gets no state,
    parameter 1 ends with step == 3 (after its first gradient at step 3 it had step == 1), and every parameter that moved is
    within the bar of float64 Adam over the steps IT saw."""
    from bin_amd.optim import Adam
    case = OC.Case("class", _CLASS_ROWS, 5, 2e-4, (0.9, 0.99), 1e-8, 1e-2, True, 77)
    inp = OC.make_inputs(case)
    params = _params(inp["p"])
    opt = Adam(params, lr=case.lr, betas=case.betas, eps=case.eps, weight_decay=case.weight_decay)
    versions = [q._version for q in params]
    for t in range(5):
        grads = list(inp["g"][t])
        grads[2] = None
        if t < 2:
            grads[1] = None
        _set_grads(params, grads)
        opt.step()
        if t == 2:
            assert float(opt.state[params[1]]["step"]) == 1.0
    assert params[2] not in opt.state or len(opt.state[params[2]]) == 0
    assert np.array_equal(params[2].detach().cpu().numpy().view(np.uint32), inp["p"][2].view(np.uint32))
    assert params[2]._version == versions[2]
    assert [float(opt.state[q]["step"]) for q in (params[0], params[1], params[3], params[4])] == [5.0, 3.0, 5.0, 5.0]
    for q in (params[0], params[1]):
        st = opt.state[q]
        assert st["step"].dtype == torch.float32 and st["step"].device.type == "cpu" and st["step"].dim() == 0
        assert st["exp_avg"].is_cuda and st["exp_avg"].shape == q.shape and st["exp_avg_sq"].dtype == torch.float32
    assert all(q._version > v for q, v in zip((params[0], params[1], params[3]), (versions[0], versions[1], versions[3])))
    full = [0, 3, 4]                                        # saw all five steps
    got = _state_of(opt, [params[i] for i in full])
    inp_f = {"p": [inp["p"][i] for i in full], "g": [[s[i] for i in full] for s in inp["g"]]}
    OC.compare("class/all-steps", [_CLASS_ROWS[i] for i in full], got, OC.reference64(case, inp_f), OC.torch32(case, inp_f))
    late = case._replace(steps=3)                           # parameter 1: steps 3..5 are ITS steps 1..3
    inp_l = {"p": [inp["p"][1]], "g": [[s[1]] for s in inp["g"][2:]]}
    OC.compare("class/late-start", [_CLASS_ROWS[1]], _state_of(opt, [params[1]]), OC.reference64(late, inp_l), OC.torch32(late, inp_l))


def test_two_groups_with_their_own_rates_and_an_empty_group():
    from bin_amd.optim import Adam
    case = OC.Case("groups", _CLASS_ROWS[:2], 3, 2e-4, (0.9, 0.999), 1e-8, 0.0, True, 78)
    inp = OC.make_inputs(case)
    params = _params(inp["p"])
    opt = Adam([{"params": [params[0]], "lr": 2e-4}, {"params": [params[1]], "lr": 5e-3}, {"params": []}], lr=1.0,
               betas=case.betas, eps=case.eps)
    assert [len(g["params"]) for g in opt.param_groups] == [1, 1, 0]
    for t in range(3):
        _set_grads(params, inp["g"][t])
        opt.step()
    for i, lr in ((0, 2e-4), (1, 5e-3)):
        c = case._replace(lr=lr)
        one = {"p": [inp["p"][i]], "g": [[s[i]] for s in inp["g"]]}
        OC.compare(f"groups/{i}", [_CLASS_ROWS[i]], _state_of(opt, [params[i]]), OC.reference64(c, one), OC.torch32(c, one))
    opt.param_groups[0]["lr"] = 0                           # the rate is read from the group at every step
    before = params[0].detach().clone()
    _set_grads(params, inp["g"][0])
    opt.step()
    assert torch.equal(params[0].detach(), before) and float(opt.state[params[0]]["step"]) == 4.0


def test_assigning_a_fresh_state_restarts_the_moments():
    """`optimizer.state = defaultdict(dict)` (MultiStepLR_Restart(clear_state=True)) between steps: the next step is step 1 of new
    moments from the parameters as they are then."""
    from bin_amd.optim import Adam
    case = OC.Case("restart", _CLASS_ROWS[:3], 2, 2e-4, (0.9, 0.999), 1e-8, 0.0, True, 79)
    inp = OC.make_inputs(case)
    params = _params(inp["p"])
    opt = Adam(params, lr=case.lr, betas=case.betas, eps=case.eps)
    for t in range(2):
        _set_grads(params, inp["g"][t])
        opt.step()
    mid = [q.detach().cpu().numpy().copy() for q in params]
    opt.state = defaultdict(dict)
    _set_grads(params, inp["g"][0])
    opt.step()
    assert all(float(opt.state[q]["step"]) == 1.0 for q in params)
    one = case._replace(steps=1)
    again = {"p": mid, "g": [inp["g"][0]]}
    OC.compare("restart", _CLASS_ROWS[:3], _state_of(opt, params), OC.reference64(one, again), OC.torch32(one, again))


@pytest.mark.parametrize("first", ["hip", "torch"])
def test_state_dicts_interchange_with_torch_adam(first):
    """K steps with one class, state_dict() -> load_state_dict() of the other, M more steps: within the bar of K + M steps of float64
    Adam, as are K + M steps of either class alone."""
    from bin_amd.optim import Adam
    K, M = 2, 3
    case = OC.Case("interchange", _CLASS_ROWS, K + M, 2e-4, (0.9, 0.99), 1e-8, 1e-2, True, 80)
    inp = OC.make_inputs(case)
    r64, r32 = OC.reference64(case, inp), OC.torch32(case, inp)
    classes = {"hip": Adam, "torch": torch.optim.Adam}
    kw = dict(lr=case.lr, betas=case.betas, eps=case.eps, weight_decay=case.weight_decay)
    alone = OC.torch32(case, inp, cls=classes[first], device="cuda")
    OC.compare(f"interchange/{first} alone", _CLASS_ROWS, alone, r64, r32)
    params = _params(inp["p"])
    a = classes[first](params, **kw)
    for t in range(K):
        _set_grads(params, inp["g"][t])
        a.step()
    sd = a.state_dict()
    b = classes["torch" if first == "hip" else "hip"](params, **kw)
    b.load_state_dict(sd)
    assert all(float(b.state[q]["step"]) == K and b.state[q]["step"].device.type == "cpu" for q in params)
    for t in range(K, K + M):
        _set_grads(params, inp["g"][t])
        b.step()
    assert all(float(b.state[q]["step"]) == K + M for q in params)
    OC.compare(f"interchange/{first} then the other", _CLASS_ROWS, _state_of(b, params), r64, r32)
    sd_b, sd_ref = b.state_dict(), classes[first](_params(inp["p"]), **kw).state_dict()
    assert [sorted(g) for g in sd_b["param_groups"]] == [sorted(g) for g in sd_ref["param_groups"]]


def test_gradients_that_are_views_into_the_flat_all_reduce_buffer():
    """FlatGradAllReduce.attach() makes every .grad a view into one flat buffer: with odd sizes the views start at every 4-byte
    offset, the parameters and moments stay 16-byte aligned."""
    from bin_amd.models.bin_model import FlatGradAllReduce
    from bin_amd.optim import Adam
    rows = tuple(OC.Row(n, (0,) * 4, mag) for n, mag in ((3, 1.0), (257, 1e-3), (4097, 1.0), (2, 1e-6), (2049, 1e4), (96, 1.0)))
    case = OC.Case("flat", rows, 2, 2e-4, (0.9, 0.999), 1e-8, 0.0, True, 81)
    inp = OC.make_inputs(case)
    params = _params(inp["p"])
    sync = FlatGradAllReduce(params)
    opt = Adam(params, lr=case.lr, betas=case.betas, eps=case.eps)
    for t in range(2):
        opt.zero_grad()
        sync.attach()
        assert len({q.grad.data_ptr() % 16 for q in params}) >= 3 and all(q.data_ptr() % 16 == 0 for q in params)
        sync.flat.copy_(torch.from_numpy(np.concatenate(inp["g"][t])))
        opt.step()
        assert sync._views_intact()
    OC.compare("flat", rows, _state_of(opt, params), OC.reference64(case, inp), OC.torch32(case, inp))


# ------------------------------------------------------------------------------------------------ 5. version counters
def test_step_bumps_the_versions_the_relayout_cache_and_the_backward_rest_on():
    from bin_amd.models.archs.RDN import RDN_residual_interp_2_input
    from bin_amd.optim import Adam
    from bin_amd.weights import general_rdn_weights
    shape = (96, 2, 4, 32)
    weights = {nm: torch.from_numpy(v) for nm, v in general_rdn_weights(0, 2, shape).items()}
    mod = RDN_residual_interp_2_input(*shape)
    mod.load_state_dict(weights, strict=True)
    mod = mod.cuda().train()
    gen = torch.Generator().manual_seed(5)
    frames = [torch.rand(1, 3, 32, 32, generator=gen).cuda() for _ in range(2)]
    opt = Adam(mod.parameters(), lr=1e-3)
    out0 = mod(*frames)
    out0.square().mean().backward()
    stale = mod(*frames)                                     # a graph recorded before the step
    versions = {n: p._version for n, p in mod.named_parameters()}
    opt.step()
    assert all(p._version > versions[n] for n, p in mod.named_parameters()), "every parameter's _version must rise"
    with torch.no_grad():
        out1 = mod(*frames)                                  # no invalidate_kernel_weights(): the cache key saw the versions
    fresh = RDN_residual_interp_2_input(*shape)
    fresh.load_state_dict({n: p.detach().cpu() for n, p in mod.state_dict().items()}, strict=True)
    fresh = fresh.cuda().train()
    with torch.no_grad():
        want = fresh(*frames)
    assert torch.equal(out1, want), "the forward after step() ran on stale kernel weights"
    assert not torch.equal(out1, out0.detach())
    with pytest.raises(RuntimeError, match="modified in place"):
        stale.square().mean().backward()


# ------------------------------------------------------------------------------------------------ 6. through the wrappers
def _bin_opt(tmp_path, optimizer):
    opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp_path), "training_state": str(tmp_path)},
           "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None,
                     "lr_G": 1e-4, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    if optimizer is not None:
        opt["train"]["optimizer"] = optimizer
    return opt


def _check_last_step(tag, m, before, state_before, t):
    """The step `m` just made, against float64 Adam recomputed from the parameters (and moments) before it and the .grad it left."""
    params = list(m.netG.module.parameters())
    grads = [q.grad.detach().cpu().numpy().reshape(-1) for q in params]
    inp = {"p": [b.reshape(-1) for b in before], "g": [grads], "t0": t - 1}
    if state_before is not None:
        inp["m"] = [x.reshape(-1) for x in state_before[0]]
        inp["v"] = [x.reshape(-1) for x in state_before[1]]
    tr = m.opt["train"]
    case = OC.Case(tag, None, 1, m.optimizer_G.param_groups[0]["lr"], (tr["beta1"], tr["beta2"]), 1e-8, tr["weight_decay_G"], False, 0)
    rows = OC.rows_by_decade(grads)
    got = {"p": [q.detach().cpu().numpy().reshape(-1) for q in params],
           "m": [m.optimizer_G.state[q]["exp_avg"].cpu().numpy().reshape(-1) for q in params],
           "v": [m.optimizer_G.state[q]["exp_avg_sq"].cpu().numpy().reshape(-1) for q in params]}
    OC.compare(tag, rows, got, OC.reference64(case, inp), OC.torch32(case, inp))


def _batch(g):
    return {"LQs": torch.from_numpy(g["LQs"]), "GTenh": torch.from_numpy(g["GTenh"]), "GTinp": torch.from_numpy(g["GTinp"])}


def test_three_training_steps_with_the_hip_optimizer_match_reference_golden(tmp_path):
    """test_gpu_train.py::test_three_training_steps_match_reference_golden with `"optimizer": "hip"`: the same fixture and bars; and
    after step 1 every parameter within the kernel test's bar of float64 Adam."""
    from bin_amd.models import create_model
    from bin_amd.optim import Adam
    from bin_amd.weights import reference_state_dict
    g = load_golden("g9_train_steps")
    m = create_model(_bin_opt(tmp_path, "hip"))
    assert type(m.optimizer_G) is Adam
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    batch = _batch(g)
    got = []
    for step in (1, 2, 3):
        before = [q.detach().cpu().numpy().copy() for q in m.netG.module.parameters()] if step == 1 else None
        m.feed_data(batch)
        m.optimize_parameters(step)
        got.append(float(m.loss))
        if step == 1:
            _check_last_step("wrapper/step1", m, before, None, 1)
    ref = [float(v) for v in g["losses"]]
    print("losses", got, "reference", ref)
    assert abs(got[0] - ref[0]) <= 2e-6
    assert abs(got[1] - ref[1]) <= 2e-5 and abs(got[2] - ref[2]) <= 2e-5, (got, ref)
    assert abs(got[1] - got[0]) > 1e-3, "the second step must see updated weights"
    named = dict(m.netG.module.named_parameters())
    for key in g.files:
        if key.startswith("after3."):
            d = (named[key[7:]].detach().cpu() - torch.from_numpy(g[key])).abs()
            assert float(d.mean()) <= 2e-6 and float((d > 5e-5).float().mean()) <= 0.01, (key, float(d.mean()), float(d.max()))


@pytest.mark.parametrize("first,second", [("torch", "hip"), ("hip", "torch")])
def test_training_state_resumes_across_the_two_optimizers(tmp_path, first, second):
    """save_training_state with one optimizer, resume_training with the other, one more step: that step is step 2 of float64 Adam
    from the saved moments."""
    from bin_amd.models import create_model
    from bin_amd.optim import Adam
    from bin_amd.weights import reference_state_dict
    import os
    g = load_golden("g9_train_steps")
    batch = _batch(g)
    a = create_model(_bin_opt(tmp_path, first))
    a.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    a.feed_data(batch)
    a.optimize_parameters(1)
    a.save_training_state(0, 1)
    a.save(1)
    b = create_model(_bin_opt(tmp_path, second))
    assert (type(b.optimizer_G) is Adam) == (second == "hip") and (type(a.optimizer_G) is Adam) == (first == "hip")
    b.load_network(os.path.join(str(tmp_path), "1_G.pth"), b.netG, True)
    b.resume_training(torch.load(os.path.join(str(tmp_path), "1.state"), weights_only=False))
    params = list(b.netG.module.parameters())
    assert all(float(b.optimizer_G.state[q]["step"]) == 1.0 for q in params)
    before = [q.detach().cpu().numpy().copy() for q in params]
    moments = ([b.optimizer_G.state[q]["exp_avg"].cpu().numpy().copy() for q in params],
               [b.optimizer_G.state[q]["exp_avg_sq"].cpu().numpy().copy() for q in params])
    for qa, qb in zip(a.netG.module.parameters(), params):
        assert torch.equal(qa.detach(), qb.detach())
        assert torch.equal(a.optimizer_G.state[qa]["exp_avg_sq"], b.optimizer_G.state[qb]["exp_avg_sq"])
    b.feed_data(batch)
    b.optimize_parameters(2)
    assert all(float(b.optimizer_G.state[q]["step"]) == 2.0 for q in params)
    _check_last_step(f"resume/{first}->{second}", b, before, moments, 2)


def test_video_base_model_with_the_hip_optimizer_and_ft_tsa_only(tmp_path):
    """VideoBaseModel over the stand-in generator of videobase_cases.py with `optimizer: hip` and ft_tsa_only: two groups,
    set_params_lr_zero honoured (group 0 frozen for steps 1 and 2), the reference fixture met at the torch path's tolerance."""
    import videobase_cases as VC
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.optim import Adam
    g = load_golden("g13_videobase_step")
    case = "cb_pair_ft"
    ft, crit, method, _ = VC.CASES[case]
    o = VC.opt(tmp_path, ft, crit)
    o["gpu_ids"] = [0]
    o["train"]["optimizer"] = "hip"
    m = VideoBaseModel(o, netG=VC.StubVSR())
    assert type(m.optimizer_G) is Adam
    assert [len(grp["params"]) for grp in m.optimizer_G.param_groups] == g[f"{case}/groups"].tolist() and len(m.optimizer_G.param_groups) == 2
    data = VC.batch()
    frozen = [p.detach().clone() for p in m.optimizer_G.param_groups[0]["params"]]
    fusion = [p.detach().clone() for p in m.optimizer_G.param_groups[1]["params"]]
    for step in range(1, VC.STEPS + 1):
        m.feed_data(data)
        getattr(m, method)(step)
        assert [grp["lr"] for grp in m.optimizer_G.param_groups] == pytest.approx(g[f"{case}/s{step}/lr_used"].tolist(), rel=1e-12, abs=0)
        if step < ft:
            assert m.optimizer_G.param_groups[0]["lr"] == 0
            assert all(torch.equal(p.detach(), f) for p, f in zip(m.optimizer_G.param_groups[0]["params"], frozen))
        m.update_learning_rate(step, warmup_iter=-1)
        assert m.get_current_log()["l_pix"] == pytest.approx(float(g[f"{case}/s{step}/l_pix"]), rel=5e-6)
        for n, p in m.netG.module.named_parameters():
            assert np.abs(p.detach().cpu().numpy() - g[f"{case}/s{step}/{n}"]).max() <= 2e-5, (step, n)
    assert not any(torch.equal(p.detach(), f) for p, f in zip(m.optimizer_G.param_groups[1]["params"], fusion)), "group 1 trains throughout"
