"""CPU: what can be pinned about the weight average (train.ema_decay) without a device — its case table (ema_cases.py), that the
float64 reference and the bars are not vacuous, the ABI bookkeeping of libbinema.so and its refusals, `train.ema_decay`, what
WeightEMA does on CPU tensors (it refuses to update; building, the parameter exchange and the state round trip need no launch), and
that nothing changes with the option absent.  GPU side: test_gpu_ema.py."""
import ctypes as C
import logging
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_cases as EC
from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "binema.h")).read()


def _source():
    return open(os.path.join(REPO, "bin_amd", "csrc", "binema_step.hip")).read()


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_the_edges_the_issue_names():
    from bin_amd import _lib
    assert len(set(EC.TAGS)) == len(EC.CASES)
    assert EC.EMA_MAX_TENSORS == _lib.EMA_MAX_TENSORS and EC.CHUNK == 2048
    assert re.search(r"EM_CHUNK = EM_THREADS \* EM_UNROLL \* 4;\s+// 2048 elements", _source())
    assert EC.NUMELS == (1, 3, 4, 5, 255, 256, 257, EC.CHUNK - 1, EC.CHUNK, EC.CHUNK + 1, 2 * EC.CHUNK + 1, 221184)
    assert [o for _, o in EC.ALIGNMENTS] == [(0, 0), (1, 0), (0, 3), (2, 2), (1, 3)]
    assert EC.MAGNITUDES == (1e-6, 1e-3, 1.0, 1e4) and EC.DECAYS == (0.0, 0.5, 0.9, 0.999, 0.9999) and EC.STEPS == (1, 3, 10)
    rows = [r for c in EC.CASES if c.rows is not None for r in c.rows]
    assert {(n, o) for n in EC.NUMELS for _, o in EC.ALIGNMENTS} <= {(r.numel, r.offs) for r in rows}, "every numel at every alignment"
    assert {(n, m) for n in EC.NUMELS for m in EC.MAGNITUDES} <= {(r.numel, r.mag) for r in rows}, "every numel at every magnitude"
    got = {(c.decay, c.start, c.steps) for c in EC.CASES}
    assert set(EC.combos()) <= got and len(EC.combos()) == 5 * 3 * 3 - 5
    assert not any(c.start == "near" and c.steps == 1 for c in EC.CASES), "p == e: the update is the identity there"
    for c in EC.CASES:
        if c.tag.startswith("decay"):
            assert {(r.mag, r.offs != (0, 0)) for r in c.rows} == {(m, a) for m in EC.MAGNITUDES for a in (False, True)}
    counts = {len(EC.rows_of(c)) for c in EC.CASES}
    m = EC.EMA_MAX_TENSORS
    assert {1, m - 1, m, m + 1, 2 * m + 1, 540} <= counts
    inp = EC.make_inputs(EC.CASE_BY_TAG["decay0.9_far_k3"])
    again = EC.make_inputs(EC.CASE_BY_TAG["decay0.9_far_k3"])
    assert len(inp["p"]) == 3 and all(a.dtype == np.float32 for step in inp["p"] for a in step)
    assert all(np.array_equal(a, b) for s, t in zip(inp["p"], again["p"]) for a, b in zip(s, t))
    assert all(np.array_equal(e, p * np.float32(100)) for e, p in zip(inp["e"], inp["p"][0]))
    assert not np.array_equal(inp["p"][0][0], inp["p"][1][0]), "the weights walk"
    tiny = min(float(np.abs(a[a != 0]).min()) for c in EC.CASES[:8] for step in EC.make_inputs(c)["p"] for a in step)
    assert tiny * 1e-4 > 1.2e-38, "no denormals, not even after one step at decay 0.9999 from zero"
    # the arenas: every row at its offset, a guard float on either side
    case = EC.CASE_BY_TAG["numel_both_off_differently"]
    inp = EC.make_inputs(case)
    for kind, vals in ((0, inp["e"]), (1, inp["p"][0])):
        starts, total = EC.layout(case.rows, kind)
        a = EC.arena(case.rows, kind, vals)
        assert a.size == total
        for s, r in zip(starts, case.rows):
            assert s % 4 == r.offs[kind] and a[s - 1] == EC.GUARD and a[s + r.numel] == EC.GUARD
        back, rest = EC.split(case.rows, kind, a)
        assert all(np.array_equal(x, y) for x, y in zip(back, vals)) and (rest == EC.GUARD).all()
    # the by-value table takes as many rows as fit under the kernel-argument limit the Adam kernel keeps to: one more would not
    size = lambda n: n * 24 + ((n + 1) * 4 + 4 + 7) // 8 * 8 + 4
    assert size(m) <= 3840 < size(m + 1)
    assert re.search(r"static_assert\(sizeof\(EmaTable\) \+ [^;]*<= 3840", _source())
    assert re.search(r"static_assert\(sizeof\(BinEmaTensor\) == 24", _source())


def _combo_case(k, decay, start, steps):
    return EC.Case(f"table_{decay:g}_{start}_{steps}", EC._rows((4097,) * 4, (0, 0)), decay, start, steps, 5000 + k)


def test_the_bar_refuses_a_kernel_that_does_nothing():
    """`No update at all` misses the bar of every decay x start x K of the table by 6 x or more, at numel 4097 and each magnitude."""
    worst = float("inf")
    for k, (decay, start, steps) in enumerate(EC.combos()):
        case = _combo_case(k, decay, start, steps)
        inp = EC.make_inputs(case)
        r64, r32 = EC.reference64(case, inp), EC.numpy32(case, inp)
        assert max(EC.ratios(case.rows, r32, r64, r32).values()) <= 0.25 + 1e-12       # the restatement itself: e32 <= bar / 4
        miss = min(EC.ratios(case.rows, EC.no_update(case, inp), r64, r32).values())
        worst = min(worst, miss)
        assert miss >= 6.0, (case.tag, miss)
        with pytest.raises(AssertionError, match="beyond the bar"):
            EC.compare(case.tag, case.rows, EC.no_update(case, inp), r64, r32)
    print(f"[ema] no update: the smallest miss over the table is {worst:.1f} x the bar")


def test_the_bar_refuses_the_naive_weight():
    """w = float32(1) - float32(decay) is off from 1 - decay by 1.3e-5 relative at 0.999 and 1.7e-4 at 0.9999.  From a `zero` start
    the shadow is w times a sum of weights, so the result carries that relative error whole, against a bar of a few fp32 ulps
    (2^-23 = 1.2e-7 relative each): an order of magnitude outside at 0.999, two at 0.9999, for every K and magnitude.  (Where the
    decay is a short binary fraction, or 1 - decay keeps enough bits, the naive weight is the right one and must pass.)"""
    seen = {}
    for k, (decay, start, steps) in enumerate(EC.combos()):
        case = _combo_case(k, decay, start, steps)
        inp = EC.make_inputs(case)
        r64, r32 = EC.reference64(case, inp), EC.numpy32(case, inp)
        miss = EC.ratios(case.rows, EC.naive32(case, inp), r64, r32)
        if decay in (0.0, 0.5):
            assert np.float32(1.0) - np.float32(decay) == np.float32(1.0 - decay) and max(miss.values()) <= 0.25 + 1e-12
        if start == "zero" and decay in (0.999, 0.9999):
            seen.setdefault(decay, []).extend(miss.values())
    for decay, least in ((0.999, 10.0), (0.9999, 100.0)):
        print(f"[ema] naive weight at decay {decay}: {min(seen[decay]):.1f} .. {max(seen[decay]):.1f} x the zero-start bar")
        assert len(seen[decay]) == 3 * len(EC.MAGNITUDES) and min(seen[decay]) >= least, (decay, min(seen[decay]))
    w = np.float32(1.0) - np.float32(0.9999)
    assert 1.6e-4 < abs(float(w) - 1e-4) / 1e-4 < 1.8e-4, "the figure the header quotes"


def test_walk_reference_bars_hold_a_plain_float32_run_and_refuse_a_lagging_one():
    rng = np.random.Generator(np.random.PCG64(7))
    ps = [[(rng.standard_normal(n) * s).astype(np.float32) for n, s in ((1, 1.0), (5, 1e-3), (4097, 1.0), (300, 1e-3))]]
    for _ in range(9):
        ps.append([(x + (rng.standard_normal(x.size) * 0.01 * np.abs(x).max()).astype(np.float32)).astype(np.float32) for x in ps[-1]])
    e0 = [x.copy() for x in ps[0]]
    r64, bars = EC.walk_reference(e0, ps, 0.9)
    got = EC.recursion(e0, ps, np.float32(1.0 - 0.9))
    assert EC.within("plain float32", got, r64, bars) <= 1.0
    lag = EC.recursion(e0, ps[:-1], np.float32(1.0 - 0.9))
    with pytest.raises(AssertionError, match="beyond the bar"):
        EC.within("one step short", lag, r64, bars)


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_ema_library_header_and_binding_agree():
    """What is binema's own beside the bookkeeping of test_cpu_libraries.py: the row, the codes and the limit, and what the header
    says of inf / NaN and of the decay."""
    from bin_amd import _lib
    hdr = _header()
    assert re.search(r"typedef struct BinEmaTensor \{\s*float\* e;\s*const float\* p;\s*int64_t numel;\s*\} BinEmaTensor;", hdr)
    assert C.sizeof(_lib.BinEmaTensor) == 24 and [f[0] for f in _lib.BinEmaTensor._fields_] == ["e", "p", "numel"]
    assert _lib.BinEmaTensor.p.offset == 8 and _lib.BinEmaTensor.numel.offset == 16
    for name, value in (("BINEMA_E_ARG", -1), ("BINEMA_E_SHAPE", -2)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value
    assert int(re.search(r"#define\s+BINEMA_MAX_TENSORS\s+(\d+)", hdr).group(1)) == _lib.EMA_MAX_TENSORS == EC.EMA_MAX_TENSORS
    assert "propagates into e" in hdr and "No flags are kept" in hdr, "the header says what happens to inf / NaN"
    assert "shortest decimal" in hdr


def test_entry_point_refuses_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.emalib()
    step = lambda t, n, decay=0.999: lib.binema_step(t, n, decay, None)
    table = (_lib.BinEmaTensor * 2)()
    assert step(table, 0) == 0 and step(None, 0) == 0       # nothing to do, nothing launched
    assert step(table, -1) == -1 and step(None, 1) == -1
    assert step(table, 2) == -1                              # null pointers in the rows
    for r in table:
        r.e, r.p, r.numel = 64, 128, 5
    for bad in (1.0, 1.5, -0.1, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert step(table, 2, bad) == -1, bad
        assert step(table, 0, bad) == -1, bad                # ... whatever n is
    table[1].e = None
    assert step(table, 2) == -1
    table[1].e, table[1].p = 64, None
    assert step(table, 2) == -1
    table[1].p = 128
    for numel in (0, -3):
        table[1].numel = numel
        assert step(table, 2) == -1                          # numel < 1, in the second row
    table[1].numel = (2 ** 31 - 1) * EC.CHUNK + 1            # one workgroup more than a grid holds
    assert step(table, 2) == -2
    table[0].numel, table[1].numel = 2 ** 31 * EC.CHUNK, 5
    assert step(table, 2) == -2
    table[0].numel = 2 ** 62
    assert step(table, 2) == -2


def test_kernel_source_keeps_to_plain_cxx_without_atomics_allocation_or_sync():
    code = "\n".join(ln.split("//")[0] for ln in _source().splitlines())
    for word in ("atomic", "asm", "hipMalloc", "Synchronize", "hipMemcpy", "static int", "static double", "static float"):
        assert word not in code, word
    # both data paths evaluate the one expression, and a path's loads all come before its first store.  The expression is this
    # file's, handed as one functor to the walk both paths share (binhip_multi_tensor.h), which only e is written back from
    assert code.count("e + w * (p - e)") == 1 and code.count("ema_update(") == 1 + 1
    assert code.count("walk_chunk<EM_THREADS, EM_UNROLL, 0b01>(") == 1 and "EmaElement{w}, r.e, r.p);" in code
    walk = open(os.path.join(REPO, "bin_amd", "csrc", "binhip_multi_tensor.h")).read()
    walk = "\n".join(ln.split("//")[0] for ln in walk[walk.index("void walk_chunk("):walk.index("inline double shortest_decimal")].splitlines())
    for word in ("atomic", "asm", "hipMalloc", "Synchronize", "hipMemcpy", "static int", "static double", "static float"):
        assert word not in walk, word
    fast, slow = walk[walk.index("if ((low_bits & 15) == 0 &&"):walk.index("} else {")], walk[walk.index("} else {"):]
    for path, load, call, store in ((fast, "*(const float4*)(ptr[j] +", "f(x[k], true);", "*(float4*)const_cast<float*>(ptr[j] +"),
                                    (slow, "x[k][j] = ptr[j][e];", "f(x[k], base + k * THREADS + t < numel);", "const_cast<float*>(ptr[j])[e] = x[k][j];")):
        assert path.count(load) == path.count(call) == path.count(store) == 1, "one load, one call of the functor, one store per path"
        assert path.index(load) < path.index(call) < path.index(store)
    assert "(float)(1.0 - multi_tensor::shortest_decimal(decay))" in code


# ------------------------------------------------------------------------------------------------ the option
def test_ema_decay_option_values():
    from bin_amd.options import options as option
    for empty in ({}, {"train": {}}, {"train": {"ema_decay": None}}, {"train": {"ema_decay": 0}}, {"train": {"ema_decay": 0.0}},
                  option.dict_to_nonedict({"train": {"lr_G": 1e-4}})):
        assert option.ema_decay(empty) == 0.0 and option.weight_ema(empty, []) is None
    for good in (0.5, 0.9, 0.999, 0.9999, 1e-3):
        assert option.ema_decay({"train": {"ema_decay": good}}) == good
    for bad in (1, 1.0, 1.5, -0.1, -1, float("nan"), float("inf"), "0.999", True, False, [0.9]):
        with pytest.raises(ValueError, match=r"train\.ema_decay"):
            option.ema_decay({"train": {"ema_decay": bad}})
    from bin_amd.optim import WeightEMA
    ema = option.weight_ema({"train": {"ema_decay": 0.25}}, [torch.nn.Parameter(torch.ones(3))])
    assert type(ema) is WeightEMA and ema.decay == 0.25 and len(ema.shadow) == 1
    for name in ("bin_stage4_synthetic.yml", "bin_stage4_adobe240.yml"):
        y = open(os.path.join(REPO, "bin_amd", "options", name)).read()
        assert y.count("  # ema_decay: 0.999") == 1 and y.index("# grad_clip") < y.index("# ema_decay") < y.index("\nlogger:")


def test_a_wrong_value_stops_the_run_when_the_file_is_parsed(tmp_path):
    from bin_amd.options import options as option
    src = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    for value, ok in (("0.999", True), ("1.0", False), ("-0.5", False), ("yes", False), ("abc", False)):
        f = tmp_path / f"v_{value}.yml"
        f.write_text(src.replace("  # ema_decay: 0.999 ", f"  ema_decay: {value} "))
        env_before = os.environ.get("CUDA_VISIBLE_DEVICES")
        try:
            if ok:
                assert option.ema_decay(option.parse(str(f), is_train=True)) == 0.999
            else:
                with pytest.raises(ValueError, match=r"train\.ema_decay"):
                    option.parse(str(f), is_train=True)
        finally:
            if env_before is None:
                os.environ.pop("CUDA_VISIBLE_DEVICES", None)
            else:
                os.environ["CUDA_VISIBLE_DEVICES"] = env_before
    assert option.ema_decay(option.parse(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml"))) == 0.0


def test_with_the_option_off_nothing_of_it_is_imported_or_loaded():
    code = ("import sys\n"
            "from bin_amd.options import options as option\n"
            "from bin_amd import _lib\n"
            "assert option.weight_ema({'train': {'lr_G': 1e-4}}, []) is None\n"
            "assert option.weight_ema({'train': {'ema_decay': 0}}, []) is None\n"
            "assert 'bin_amd.optim' not in sys.modules, 'bin_amd.optim imported'\n"
            "assert 'binema' not in _lib._loaded, 'libbinema.so loaded'\n"
            "print('clean')\n")
    out = subprocess.run([sys.executable, "-c", code], cwd=REPO, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "clean", out.stderr[-2000:]


def test_check_resume_names_the_averaged_weights_beside_the_generator():
    from bin_amd.options import options as option
    opt = {"model": "bin", "path": {"resume_state": "/x/5.state", "models": "/m", "pretrain_model_G": None}}
    option.check_resume(opt, 5)
    assert opt["path"]["pretrain_model_G"] == os.path.join("/m", "5_G.pth")
    assert opt["path"]["pretrain_model_G_ema"] == os.path.join("/m", "5_G_ema.pth")
    opt = {"model": "bin", "path": {"resume_state": None, "models": "/m"}}
    option.check_resume(opt, 5)
    assert "pretrain_model_G_ema" not in opt["path"]


# ------------------------------------------------------------------------------------------------ the class, on CPU tensors
def _params():
    torch.manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s)) for s in ((3,), (4, 5), (1,), (2, 3, 3, 3))]


def test_weight_ema_refuses_cpu_parameters_and_bad_decays():
    from bin_amd.optim import WeightEMA
    for bad in (1.0, 1, -0.1, float("nan"), "0.9", True, None):
        with pytest.raises(ValueError, match="decay"):
            WeightEMA(_params(), bad)
    params = _params()
    ema = WeightEMA(params, 0.9)
    assert [tuple(e.shape) for e in ema.shadow] == [tuple(p.shape) for p in params]
    assert all(torch.equal(e, p.detach()) and e.dtype == torch.float32 and e.data_ptr() % 16 == 0 for e, p in zip(ema.shadow, params))
    flat = ema._flat[params[0].device]
    assert all(e.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for e in ema.shadow), "one flat buffer"
    before = [e.clone() for e in ema.shadow]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ema.update()
    assert all(torch.equal(a, b) for a, b in zip(before, ema.shadow))
    assert WeightEMA(_params(), 0).decay == 0.0                  # the class takes 0 (the shadows follow the weights); the option reads it as off


def test_applied_exchanges_and_restores_without_a_copy():
    from bin_amd.optim import WeightEMA

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.ParameterList(_params())
            self.inner = torch.nn.Linear(2, 2)
            self.calls = self.inner.calls = 0

    def count(mod):
        mod.calls += 1
    net = Net()
    net.invalidate_kernel_weights = lambda: count(net)
    net.inner.invalidate_kernel_weights = lambda: count(net.inner)
    params = list(net.parameters())
    ema = WeightEMA(params, 0.5)
    with torch.no_grad():
        for e in ema.shadow:
            e.mul_(2.0)
        params[1].add_(1.0)                                  # a version counter that is not zero
    values = [p.detach().clone() for p in params]
    avg = [e.clone() for e in ema.shadow]
    ids = [(p.data_ptr(), p._version, id(p)) for p in params]
    sids = [(e.data_ptr(), e._version) for e in ema.shadow]
    with ema.applied(net) as inside:
        assert inside is ema and (net.calls, net.inner.calls) == (1, 1)
        assert all(torch.equal(p.detach(), a) and p.data_ptr() == e.data_ptr() for p, a, e in zip(params, avg, ema.shadow))
        assert all(p.requires_grad and isinstance(p, torch.nn.Parameter) for p in params)
        assert all(torch.equal(v, a) for v, a in zip(net.state_dict().values(), avg))
        with pytest.raises(RuntimeError, match="not re-entrant"):
            with ema.applied(net):
                pass
        with pytest.raises(RuntimeError, match="inside applied"):
            ema.update()
    assert (net.calls, net.inner.calls) == (2, 2)
    assert [(p.data_ptr(), p._version, id(p)) for p in params] == ids
    assert [(e.data_ptr(), e._version) for e in ema.shadow] == sids
    assert all(torch.equal(p.detach(), v) for p, v in zip(params, values)) and all(torch.equal(e, a) for e, a in zip(ema.shadow, avg))
    with pytest.raises(KeyError):
        with ema.applied([net]):                             # a list of modules works too; an exception still restores
            assert net.calls == 3
            raise KeyError("inside")
    assert net.calls == 4 and [(p.data_ptr(), p._version, id(p)) for p in params] == ids
    assert all(torch.equal(p.detach(), v) for p, v in zip(params, values))
    with ema.applied():                                      # and so does no module at all
        assert torch.equal(params[0].detach(), avg[0])
    # an optimizer that holds the parameters sees the training values again
    opt = torch.optim.SGD(params, lr=1.0)
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    assert all(torch.equal(p.detach(), v - 1.0) for p, v in zip(params, values)) and all(torch.equal(e, a) for e, a in zip(ema.shadow, avg))


def test_state_dict_round_trip_and_mismatches():
    from bin_amd.optim import WeightEMA
    a = WeightEMA(_params(), 0.9)
    with torch.no_grad():
        for k, e in enumerate(a.shadow):
            e.add_(float(k + 1))
    state = a.state_dict()
    assert set(state) == {"decay", "shadow"} and state["decay"] == 0.9
    assert all(t.device.type == "cpu" and torch.equal(t, e) and t.data_ptr() != e.data_ptr() for t, e in zip(state["shadow"], a.shadow))
    b = WeightEMA(_params(), 0.5)
    ptrs = [e.data_ptr() for e in b.shadow]
    b.load_state_dict(state)
    assert b.decay == 0.9 and all(torch.equal(x, y) for x, y in zip(a.shadow, b.shadow)) and [e.data_ptr() for e in b.shadow] == ptrs
    with pytest.raises(ValueError, match=r"3 shadow tensors for 4 parameters"):
        b.load_state_dict({"decay": 0.9, "shadow": state["shadow"][:3]})
    bad = [t.clone() for t in state["shadow"]]
    bad[1], bad[3] = torch.zeros(5, 4), torch.zeros(2)
    before = [e.clone() for e in b.shadow]
    with pytest.raises(ValueError, match=r"shadow 1 has shape \(5, 4\), parameter 1 has \(4, 5\)"):
        b.load_state_dict({"decay": 0.9, "shadow": bad})
    assert all(torch.equal(x, y) for x, y in zip(before, b.shadow)), "nothing is loaded from a refused state"
    with pytest.raises(ValueError, match="decay"):
        b.load_state_dict({"decay": 1.0, "shadow": state["shadow"]})


# ------------------------------------------------------------------------------------------------ the wrappers, on a stand-in net
class TinyNet(torch.nn.Module):
    """6 frames -> 14 frames, pointwise: fast on the CPU."""

    def __init__(self):
        super().__init__()
        self.mix = torch.nn.Conv2d(18, 42, 1)
        self.prev_state = self.hidden_state = None
        self.invalidated = 0

    def invalidate_kernel_weights(self):
        self.invalidated += 1

    def forward(self, *frames):
        y = self.mix(torch.cat(frames, dim=1))
        return list(y.split(3, dim=1))


def _opt(tmp_path, ema):
    from bin_amd.options import options as option
    train = {"lr_G": 1e-2, "beta1": 0.9, "beta2": 0.99, "pixel_criterion": "l1", "pixel_weight": 1.0, "lr_scheme": "MultiStepLR",
             "lr_steps": [100], "lr_gamma": 0.5}
    if ema is not None:
        train["ema_decay"] = ema
    for d in ("models", "training_state"):
        os.makedirs(tmp_path / d, exist_ok=True)
    return option.dict_to_nonedict({"is_train": True, "dist": False, "gpu_ids": None, "model": "bin", "train": train,
                                    "network_G": {"nframes": 6, "version": 1},
                                    "path": {"models": str(tmp_path / "models"), "training_state": str(tmp_path / "training_state"),
                                             "pretrain_model_G": None, "strict_load": True}})


def _wrapper(tmp_path, ema, seed=0):
    from bin_amd.models.bin_model import bin_model
    torch.manual_seed(seed)
    return bin_model(_opt(tmp_path, ema), netG=TinyNet(), cri_pix=torch.nn.L1Loss(reduction="sum"))


def test_wrapper_builds_the_average_only_when_asked_and_saves_it_beside_the_generator(tmp_path):
    off = _wrapper(tmp_path / "off", None)
    assert off.weight_ema is None
    with off.ema_scope():                                    # a no-op context
        pass
    off.save("7")
    assert sorted(os.listdir(tmp_path / "off" / "models")) == ["7_G.pth"]
    on = _wrapper(tmp_path / "on", 0.9)
    params = list(on.netG.parameters())
    assert on.weight_ema is not None and on.weight_ema.decay == 0.9 and len(on.weight_ema.shadow) == len(params) == 2
    assert all(torch.equal(e, p.detach()) for e, p in zip(on.weight_ema.shadow, params))
    with torch.no_grad():
        for e in on.weight_ema.shadow:
            e.add_(0.5)
    net = on.netG.module
    with on.ema_scope():
        assert net.invalidated == 1 and all(torch.equal(e, p.detach()) for e, p in zip(on.weight_ema.shadow, params))
    assert net.invalidated == 2
    on.save("7")
    assert sorted(os.listdir(tmp_path / "on" / "models")) == ["7_G.pth", "7_G_ema.pth"]
    raw = torch.load(tmp_path / "on" / "models" / "7_G.pth")
    avg = torch.load(tmp_path / "on" / "models" / "7_G_ema.pth")
    assert list(raw) == list(avg) == list(net.state_dict())
    assert all(torch.equal(avg[k], raw[k] + 0.5) for k in raw), "an ordinary generator checkpoint holding the averaged values"
    assert all(torch.equal(raw[k], v) for k, v in net.state_dict().items())
    # the CPU step cannot average: there is no fallback
    frames = {"LQs": torch.rand(1, 6, 3, 4, 4), "GTenh": torch.rand(1, 6, 3, 4, 4), "GTinp": torch.rand(1, 5, 3, 4, 4)}
    on.feed_data(frames)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        on.optimize_parameters(1)


def test_resume_loads_the_average_and_warns_once_when_the_file_is_missing(tmp_path, caplog):
    from bin_amd.options import options as option
    a = _wrapper(tmp_path, 0.9)
    with torch.no_grad():
        for k, e in enumerate(a.weight_ema.shadow):
            e.mul_(0.5).add_(float(k))
    a.save(3)
    a.save_training_state(0, 3)
    state = torch.load(tmp_path / "training_state" / "3.state", weights_only=False)
    assert set(state) == {"epoch", "iter", "schedulers", "optimizers"}, "`.state` files do not change"

    def resumed():
        from bin_amd.models.bin_model import bin_model
        opt = _opt(tmp_path, 0.9)
        opt["path"]["resume_state"] = str(tmp_path / "training_state" / "3.state")
        option.check_resume(opt, state["iter"])
        torch.manual_seed(99)
        m = bin_model(opt, netG=TinyNet(), cri_pix=torch.nn.L1Loss(reduction="sum"))
        with caplog.at_level(logging.WARNING, logger="base"):
            caplog.clear()
            m.resume_training(state)
        return m, [r.getMessage() for r in caplog.records if "ema_decay" in r.getMessage()]
    b, warned = resumed()
    assert not warned
    assert all(torch.equal(x, y) for x, y in zip(a.weight_ema.shadow, b.weight_ema.shadow))
    assert all(torch.equal(p, q) for p, q in zip(a.netG.parameters(), b.netG.parameters()))
    assert not any(torch.equal(e, p.detach()) for e, p in zip(b.weight_ema.shadow, b.netG.parameters()))
    os.remove(tmp_path / "models" / "3_G_ema.pth")
    c, warned = resumed()
    assert len(warned) == 1 and "3_G_ema.pth" in warned[0] and "starts from the loaded weights" in warned[0]
    assert all(torch.equal(e, p.detach()) for e, p in zip(c.weight_ema.shadow, c.netG.parameters()))
    assert all(torch.equal(p, q) for p, q in zip(a.netG.parameters(), c.netG.parameters()))
