"""CPU: what can be pinned about the Adam kernel without a device — its case table (optim_cases.py), that the float64 reference
and the bar are not vacuous (a plain numpy float32 restatement of the formulas passes), the ABI bookkeeping, `train.optimizer`,
bin_amd.optim.Adam's state format, and that nothing changes with the option absent.  GPU side: test_gpu_optim.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import optim_cases as OC
from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "binopt.h")).read()


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_is_well_formed():
    assert len({c.tag for c in OC.CASES}) == len(OC.CASES)
    n_max = int(re.search(r"#define\s+BINOPT_ADAM_MAX_TENSORS\s+(\d+)", _header()).group(1))
    from bin_amd import _lib
    assert OC.ADAM_MAX_TENSORS == n_max == _lib.ADAM_MAX_TENSORS
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binopt_adam.hip")).read()
    threads, unroll = (int(re.search(rf"constexpr int {n} = (\d+);", src).group(1)) for n in ("AD_THREADS", "AD_UNROLL"))
    assert OC.CHUNK == threads * unroll * 4, "the table's chunk-edge sizes follow the kernel's work split"
    rows = [r for c in OC.CASES for r in OC.rows_of(c)]
    assert set(OC.NUMELS) <= {r.numel for r in rows} and {OC.CHUNK - 1, OC.CHUNK, OC.CHUNK + 1} <= {r.numel for r in rows}
    assert OC.NUMELS == (1, 3, 4, 5, 255, 256, 257, 4095, 4096, 4097, 221184)
    for r in rows:
        assert r.numel >= 1 and len(r.offs) == 4 and all(0 <= o <= 3 for o in r.offs) and r.mag in OC.MAGNITUDES
    offs = {r.offs for r in rows}
    assert (0, 0, 0, 0) in offs
    for k in range(4):                                       # each single tensor misaligned, the other three aligned
        assert any(o[k] != 0 and sum(1 for x in o if x) == 1 for o in offs), k
    assert any(all(o) and len(set(o)) > 1 for o in offs), "all four misaligned, not all alike"
    # every numel at every alignment, every magnitude at every numel
    for name, o in OC.ALIGNMENTS:
        assert {r.numel for r in OC.rows_of(OC.CASE_BY_TAG[f"numel_{name}"])} >= set(OC.NUMELS), name
    seen = {(r.numel, r.mag) for c in OC.CASES if c.tag.startswith("numel_") for r in c.rows}
    assert all(sum((n, m) in seen for m in OC.MAGNITUDES) >= 3 for n in OC.NUMELS)
    counts = {len(OC.rows_of(c)) for c in OC.CASES}
    assert {1, n_max - 1, n_max, n_max + 1, 540} <= counts
    assert {c.steps for c in OC.CASES} == set(OC.STEPS) == {1, 3, 10}
    combos = {(c.weight_decay, c.eps, c.betas, c.lr) for c in OC.CASES}
    assert combos >= {(wd, e, b, lr) for wd in OC.WEIGHT_DECAYS for e in OC.EPSILONS for b in OC.BETAS for lr in OC.LRS}
    assert OC.WEIGHT_DECAYS == (0.0, 1e-2) and OC.EPSILONS == (1e-8, 1e-3) and OC.LRS == (2e-4, 0.0)
    assert OC.BETAS == ((0.9, 0.999), (0.9, 0.99), (0.5, 0.9)) and OC.MAGNITUDES == (1e-12, 1e-6, 1e-3, 1.0, 1e4)
    nm = OC.stage4_numels()
    assert len(nm) == 540 and min(nm) == 3 and max(nm) == 221184 and 11.43e6 < sum(nm) < 11.45e6


def test_inputs_hold_one_decade_per_tensor_and_a_tenth_zeros():
    case = OC.CASE_BY_TAG["numel_aligned"]
    inp = OC.make_inputs(case)
    again = OC.make_inputs(case)
    for r, p, g, g2 in zip(case.rows, inp["p"], inp["g"][0], again["g"][0]):
        assert p.dtype == g.dtype == np.float32 and p.size == g.size == r.numel and np.array_equal(g, g2)
        if r.numel >= 4095:
            nz = np.abs(g[g != 0])
            assert 0.07 < float((g == 0).mean()) < 0.13
            assert 0.3 * r.mag < float(np.median(nz)) < 1.2 * r.mag and nz.max() < r.mag * 10
    assert not np.array_equal(inp["g"][0][-1], inp["g"][1][-1]), "every step sees a fresh gradient"


def test_arena_layout_places_every_row_at_its_offset_between_guards():
    rows = OC.CASE_BY_TAG["numel_all_off_differently"].rows
    for kind in range(4):
        starts, total = OC.layout(rows, kind)
        a = OC.arena(rows, kind, None)
        assert a.size == total and total % 4 == 0
        end = 0
        for s, r in zip(starts, rows):
            assert s % 4 == r.offs[kind] and s > end, "at least one guard float before every row"
            assert a[s - 1] == OC.GUARD and a[s + r.numel] == OC.GUARD
            end = s + r.numel
        vals, blank = OC.split(rows, kind, a)
        assert all(v.size == r.numel and not v.any() for v, r in zip(vals, rows)) and (blank == OC.GUARD).all()


# ------------------------------------------------------------------------------------------------ reference and bar
@pytest.mark.parametrize("tag", OC.CPU_TAGS)
def test_numpy_float32_restatement_stays_within_the_bar(tag):
    """The formulas in plain numpy float32 against the float64 reference with the bar of test_gpu_optim.py: the reference alone
    passes, so the bar is not vacuous — and a wrong bias correction or swapped betas do not."""
    case = OC.CASE_BY_TAG[tag]
    inp = OC.make_inputs(case)
    r64, r32 = OC.reference64(case, inp), OC.torch32(case, inp)
    rows = OC.rows_of(case)
    OC.compare(tag, rows, OC.numpy32(case, inp), r64, r32)
    if tag in ("hyper_wd0_eps1e-08_b0.9-0.999_lr0.0002", "numel_aligned"):
        swapped = OC.numpy32(case._replace(betas=case.betas[::-1]), inp)
        with pytest.raises(AssertionError, match="beyond the bar"):
            OC.compare(tag + " swapped betas", rows, swapped, r64, r32)
        real = OC.bias_factors
        try:                                                 # bias correction 2 left out
            OC.bias_factors = lambda c, t, dtype=np.float64: (real(c, t, dtype)[0], dtype(1.0))
            wrong = OC.numpy32(case, inp)
        finally:
            OC.bias_factors = real
        with pytest.raises(AssertionError, match="beyond the bar"):
            OC.compare(tag + " no bias correction", rows, wrong, r64, r32)


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_optimizer_library_header_and_binding_agree():
    """What is binopt's own beside the bookkeeping of test_cpu_libraries.py: libbinhip.so's header knows nothing of Adam, the row
    struct, the error code and the refusals."""
    from bin_amd import _lib
    hdr = _header()
    assert "adam" not in open(os.path.join(REPO, "include", "binhip.h")).read().lower()
    assert re.search(r"typedef struct BinAdamTensor \{\s*float\* p;\s*const float\* g;\s*float\* m;\s*float\* v;\s*int64_t numel;\s*"
                     r"float step_size;\s*float inv_sqrt_bc2;\s*\} BinAdamTensor;", hdr)
    assert C.sizeof(_lib.BinAdamTensor) == 48
    assert [f[0] for f in _lib.BinAdamTensor._fields_] == ["p", "g", "m", "v", "numel", "step_size", "inv_sqrt_bc2"]
    lib = _lib.optlib()
    assert lib.binopt_adam_step.restype is C.c_int and len(lib.binopt_adam_step.argtypes) == 7
    assert int(re.search(r"#define\s+BINOPT_E_ARG\s+\((-?\d+)\)", hdr).group(1)) == -1
    # the refusals come before any HIP call, so they run without a device
    table = (_lib.BinAdamTensor * 2)()
    assert lib.binopt_adam_step(table, 0, 0.9, 0.999, 1e-8, 0.0, None) == 0
    assert lib.binopt_adam_step(None, 0, 0.9, 0.999, 1e-8, 0.0, None) == 0
    assert lib.binopt_adam_step(table, -1, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert lib.binopt_adam_step(None, 1, 0.9, 0.999, 1e-8, 0.0, None) == -1
    assert lib.binopt_adam_step(table, 2, 0.9, 0.999, 1e-8, 0.0, None) == -1       # null pointers in the rows
    for r in table:
        r.p = r.g = r.m = r.v = 64
        r.numel = 0
    assert lib.binopt_adam_step(table, 2, 0.9, 0.999, 1e-8, 0.0, None) == -1       # numel < 1
    for r in table:
        r.numel = 4
    for b1, b2 in ((1.0, 0.9), (0.9, 1.0), (-0.5, 0.9), (0.9, float("nan"))):
        assert lib.binopt_adam_step(table, 2, b1, b2, 1e-8, 0.0, None) == -1


def test_kernel_source_keeps_to_ieee_arithmetic_and_plain_cxx():
    src = open(os.path.join(REPO, "bin_amd", "csrc", "binopt_adam.hip")).read()
    code = "\n".join(ln.split("//")[0] for ln in src.splitlines())
    for word in ("__fdividef", "rsqrt", "__shared__", "atomic", "asm", "__frsqrt_rn", "__fsqrt_rn", "hipMalloc", "Synchronize"):
        assert word not in code, word
    assert "sqrtf(" in code and " / " in code


# ------------------------------------------------------------------------------------------------ train.optimizer
def test_optimizer_option_values(tmp_path):
    from bin_amd.options import options as option
    assert option.optimizer({"train": {}}) == "torch" and option.optimizer({}) == "torch"
    assert option.optimizer(option.dict_to_nonedict({"train": {"lr_G": 1e-4}})) == "torch"
    assert option.optimizer({"train": {"optimizer": "torch"}}) == "torch"
    assert option.optimizer({"train": {"optimizer": "hip"}}) == "hip"
    for bad in ("HIP", "adam", "fused", True, 1):
        with pytest.raises(ValueError, match=r"train\.optimizer.*torch, hip"):
            option.optimizer({"train": {"optimizer": bad}})
    assert option.adam_class({"train": {}}) is torch.optim.Adam
    from bin_amd.optim import Adam
    assert option.adam_class({"train": {"optimizer": "hip"}}) is Adam
    # the shipped files stay on torch and carry the key as a comment; a misspelt value stops the run when the file is parsed
    y = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    assert "  # optimizer: hip" in y
    assert "  # optimizer: hip" in open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_adobe240.yml")).read()
    p = str(tmp_path / "o.yml")
    env = os.environ.get("CUDA_VISIBLE_DEVICES")
    try:
        open(p, "w").write(y.replace("  # optimizer: hip", "  optimizer: rocm"))
        with pytest.raises(ValueError, match=r"train\.optimizer"):
            option.parse(p, is_train=True)
        open(p, "w").write(y.replace("  # optimizer: hip", "  optimizer: hip"))
        assert option.parse(p, is_train=True)["train"]["optimizer"] == "hip"
        assert option.parse(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml"))["train"].get("optimizer") is None
    finally:                                                 # parse() exports gpu_ids as CUDA_VISIBLE_DEVICES
        if env is None:
            os.environ.pop("CUDA_VISIBLE_DEVICES", None)
        else:
            os.environ["CUDA_VISIBLE_DEVICES"] = env


# ------------------------------------------------------------------------------------------------ the class on the host
def _cpu_params():
    g = torch.Generator().manual_seed(3)
    return [torch.nn.Parameter(torch.randn(s, generator=g)) for s in ((4, 3, 3, 3), (4,), (7,))]


def test_state_dict_structure_is_torch_adams():
    """Constructible on CPU parameters; after load_state_dict of a torch Adam state its state_dict() is torch's key for key and dtype
    for dtype, and torch's class loads it back."""
    from bin_amd.optim import Adam
    kw = dict(lr=3e-4, betas=(0.8, 0.95), eps=1e-6, weight_decay=1e-2)
    params = _cpu_params()
    ref = torch.optim.Adam([{"params": params[:2]}, {"params": params[2:], "lr": 1e-5}], **kw)
    for q in params:
        q.grad = torch.ones_like(q)
    ref.step()
    ref.step()
    want = ref.state_dict()
    ours = Adam([{"params": params[:2]}, {"params": params[2:], "lr": 1e-5}], **kw)
    fresh, fresh_ref = ours.state_dict(), torch.optim.Adam(_cpu_params(), **kw).state_dict()
    assert fresh["state"] == {} and [sorted(g) for g in fresh["param_groups"]][:1] == [sorted(g) for g in fresh_ref["param_groups"]]
    for a, b in zip(fresh["param_groups"], want["param_groups"]):
        assert a == b, (a, b)                                # every key and value torch.optim.Adam keeps in a group
    ours.load_state_dict(want)
    got = ours.state_dict()
    assert got["param_groups"] == want["param_groups"] and sorted(got["state"]) == sorted(want["state"])
    for i in want["state"]:
        assert list(got["state"][i]) == list(want["state"][i]) == ["step", "exp_avg", "exp_avg_sq"]
        for k in want["state"][i]:
            a, b = got["state"][i][k], want["state"][i][k]
            assert a.dtype == b.dtype and a.device == b.device and a.shape == b.shape and torch.equal(a, b), (i, k)
        assert got["state"][i]["step"].dtype == torch.float32 and float(got["state"][i]["step"]) == 2.0
    back = torch.optim.Adam([{"params": params[:2]}, {"params": params[2:]}], lr=1.0)
    back.load_state_dict(got)
    back.step()
    assert float(back.state[params[0]]["step"]) == 3.0 and back.param_groups[1]["lr"] == 1e-5
    assert ours.param_groups[0]["betas"] == (0.8, 0.95) and ours.param_groups[1]["lr"] == 1e-5


def test_step_on_cpu_parameters_raises_without_touching_the_state():
    from bin_amd.optim import Adam
    params = _cpu_params()
    opt = Adam(params, lr=1e-3)
    opt.step()                                               # no gradients: nothing to do, nothing to refuse
    assert len(opt.state) == 0
    for q in params:
        q.grad = torch.ones_like(q)
    before = [q.detach().clone() for q in params]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert all(torch.equal(q.detach(), b) for q, b in zip(params, before)) and len(opt.state) == 0
    from bin_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.adam_step([(params[0].data, params[0].grad, torch.zeros_like(params[0]), torch.zeros_like(params[0]), 1e-3, 1.0)],
                      0.9, 0.999, 1e-8, 0.0)


def test_unsupported_constructor_flags_raise():
    from bin_amd.optim import Adam
    for flag in ("amsgrad", "maximize", "capturable", "differentiable"):
        with pytest.raises(NotImplementedError, match=flag):
            Adam(_cpu_params(), lr=1e-3, **{flag: True})
        Adam(_cpu_params(), lr=1e-3, **{flag: False})
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            Adam(_cpu_params(), **kw)
    opt = Adam(_cpu_params(), lr=1e-3)
    opt.param_groups[0]["amsgrad"] = True                    # as a loaded amsgrad state would leave it
    for q in opt.param_groups[0]["params"]:
        q.grad = torch.ones_like(q)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        opt.step()


# ------------------------------------------------------------------------------------------------ the wrappers, option absent
def test_wrappers_build_torch_adam_when_the_option_is_absent_and_ours_when_asked(tmp_path):
    import videobase_cases as VC
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.optim import Adam
    from test_cpu_host import _Cb, _opt
    from bin_amd.models.bin_model import bin_model
    from oracle_net import OracleNet

    def both(choice, ft):
        o = _opt(tmp_path)
        o["train"]["ft_tsa_only"] = ft
        v = VC.opt(tmp_path, ft)
        if choice is not None:
            o["train"]["optimizer"] = v["train"]["optimizer"] = choice
        return bin_model(o, netG=OracleNet(), cri_pix=_Cb()), VideoBaseModel(v, netG=VC.StubVSR())

    for ft in (None, 3):
        for choice in (None, "torch"):
            for m in both(choice, ft):
                assert type(m.optimizer_G) is torch.optim.Adam and m.optimizers == [m.optimizer_G]
                grp = m.optimizer_G.param_groups
                assert len(grp) == (2 if ft else 1) and grp[0]["betas"] == (0.9, 0.99) and grp[0]["weight_decay"] == 0
        b, v = both("hip", ft)
        assert type(b.optimizer_G) is Adam and type(v.optimizer_G) is Adam
        assert [len(g["params"]) for g in b.optimizer_G.param_groups] == ([540, 0] if ft else [540])
        assert [len(g["params"]) for g in v.optimizer_G.param_groups] == ([2, 2] if ft else [4])
        assert b.optimizer_G.param_groups[0]["lr"] == 1e-4 and b.optimizer_G.param_groups[0]["betas"] == (0.9, 0.99)
        assert b.schedulers[0].optimizer is b.optimizer_G
    bad = _opt(tmp_path)
    bad["train"]["optimizer"] = "cuda"
    with pytest.raises(ValueError, match=r"train\.optimizer"):
        bin_model(bad, netG=OracleNet(), cri_pix=_Cb())
