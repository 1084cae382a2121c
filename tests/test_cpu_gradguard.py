"""CPU: what can be pinned about the gradient guard without a device — its case table (gradguard_cases.py), that the float64
reference and the bars are not vacuous, the ABI bookkeeping of libbingrad.so and its refusals, `train.grad_clip` /
`train.skip_bad_steps`, GradGuard's counting on canned flags, the data-parallel agreement over gloo, and that nothing changes with the
options absent.  GPU side: test_gpu_gradguard.py."""
import ctypes as C
import math
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch

import gradguard_cases as GC
from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "bingrad.h")).read()


def _source():
    return open(os.path.join(REPO, "bin_amd", "csrc", "bingrad_norm.hip")).read()


# ------------------------------------------------------------------------------------------------ the case table
def test_case_table_covers_the_edges_the_issue_names():
    from bin_amd import _lib
    assert len({c.tag for c in GC.CASES}) == len(GC.CASES)
    assert GC.MAX_TENSORS == _lib.GRAD_MAX_TENSORS and GC.CHUNK == 4096
    assert GC.NUMELS == (1, 3, 4, 5, GC.CHUNK - 1, GC.CHUNK, GC.CHUNK + 1, 2 * GC.CHUNK + 1, 221184)
    assert GC.MAGNITUDES == (1e-30, 1e-12, 1.0, 1e4, 1e25) and GC.MAX_NORMS == ("off", "far_above", "half", "milli")
    rows = [r for c in GC.CASES for r in GC.rows_of(c)]
    assert {(n, o) for n in GC.NUMELS for o in GC.OFFSETS} <= {(r.numel, r.offs[0]) for r in rows}, "every numel at every alignment"
    for mag in GC.MAGNITUDES:
        got = {(r.numel, r.offs[0] != 0) for r in GC.CASE_BY_TAG[f"mag_{mag:g}"].rows}
        assert {(2 * GC.CHUNK + 1, False), (GC.CHUNK + 1, True), (1, True)} <= got
    counts = {len(GC.rows_of(c)) for c in GC.CASES}
    assert {1, GC.MAX_TENSORS - 1, GC.MAX_TENSORS, GC.MAX_TENSORS + 1, 540} <= counts
    assert all(r.mag == 0.0 for r in GC.CASE_BY_TAG["zeros"].rows)
    assert {r.mag for r in GC.CASE_BY_TAG["mixed_1e-30_and_1e25"].rows} == {1e-30, 1e25}
    assert set(GC.NON_REPRESENTABLE_IN_FP32_SQUARES) <= set(GC.CASE_BY_TAG)
    g = GC.make_inputs(GC.CASE_BY_TAG["mag_1"])
    assert all(a.dtype == np.float32 for a in g) and 0.07 < float((g[0] == 0).mean()) < 0.13
    assert all(np.array_equal(a, b) for a, b in zip(g, GC.make_inputs(GC.CASE_BY_TAG["mag_1"])))
    # the arena: every row at its offset, a guard float on either side
    case = GC.CASE_BY_TAG["numel_off3"]
    starts, total = GC.OC.layout(case.rows, GC.KIND)
    a = GC.OC.arena(case.rows, GC.KIND, GC.make_inputs(case))
    for s, r in zip(starts, case.rows):
        assert s % 4 == 3 and a[s - 1] == GC.GUARD and a[s + r.numel] == GC.GUARD
    # the by-value table stays well under the kernel-argument limit
    assert GC.MAX_TENSORS * 16 + (GC.MAX_TENSORS + 1) * 4 + 64 <= 3072
    assert re.search(r"static_assert\(sizeof\(GradTable\) \+ [^;]*<= 3072", _source())


# ------------------------------------------------------------------------------------------------ reference and bars
@pytest.mark.parametrize("tag", [c.tag for c in GC.CASES])
def test_float64_reference_in_two_orders_meets_the_bars_and_fp32_squares_do_not(tag):
    case = GC.CASE_BY_TAG[tag]
    grads = GC.make_inputs(case)
    n = sum(g.size for g in grads)
    ref, other = GC.reference_sumsq(grads), GC.reference_sumsq_other_order(grads)
    for kind in GC.MAX_NORMS:
        mn = GC.max_norm_of(kind, ref)
        coef = float(np.float32(GC.coef64(mn, other)))
        GC.check(f"{tag}/{kind} other order", n, ref, other, float(np.float32(math.sqrt(other))), coef, mn)
        if kind in ("half", "milli") and ref > 0:
            assert coef < 1.0
    if tag == "zeros":
        assert ref == 0.0 and other == 0.0
    sq32 = GC.fp32_squares_sumsq(grads)
    if tag in GC.NON_REPRESENTABLE_IN_FP32_SQUARES:
        with pytest.raises(AssertionError, match="sumsq"):
            GC.check(f"{tag} fp32 squares", n, ref, sq32, float(np.float32(math.sqrt(sq32))), 1.0, 0.0)
    if tag == "mag_1":                                       # a dropped, a doubled element and a wrong coefficient are far outside
        one = float(np.abs(grads[0]).max()) ** 2
        for wrong in (ref - one, ref + one):
            with pytest.raises(AssertionError, match="sumsq"):
                GC.check(tag + " wrong", n, ref, wrong, float(np.float32(math.sqrt(ref))), 1.0, 0.0)
        mn = GC.max_norm_of("half", ref)
        with pytest.raises(AssertionError, match="coef"):
            GC.check(tag + " wrong coef", n, ref, ref, float(np.float32(math.sqrt(ref))), float(np.float32(0.5 * (1 + 3e-7))), mn)


def test_fp32_squares_lose_both_ends_of_the_range():
    """The figures of the issue: squares taken in float32 give norm 0 at magnitude 1e-30 and inf at 1e25; float64 squares do not."""
    for tag, want in (("mag_1e-30", 0.0), ("mag_1e+25", math.inf)):
        grads = GC.make_inputs(GC.CASE_BY_TAG[tag])
        assert GC.fp32_squares_sumsq(grads) == want
        ref = GC.reference_sumsq(grads)
        assert math.isfinite(ref) and ref > 0
        assert abs(GC.reference_sumsq_other_order(grads) - ref) <= 1e-13 * ref


# ------------------------------------------------------------------------------------------------ ABI bookkeeping
def test_gradient_library_header_and_binding_agree():
    """What is bingrad's own beside the bookkeeping of test_cpu_libraries.py: the row and the record, the codes, flags and limits, and
    what the header says of torch's clip."""
    from bin_amd import _lib
    hdr = _header()
    assert re.search(r"typedef struct BinGradTensor \{\s*float\* g;\s*int64_t numel;\s*\} BinGradTensor;", hdr)
    assert re.search(r"typedef struct BinGradRecord \{\s*double sumsq;[^}]*?float norm;[^}]*?float coef;[^}]*?int32_t flags;[^}]*?"
                     r"uint32_t status;[^}]*?int32_t reserved\[2\];[^}]*?\} BinGradRecord;", hdr)
    assert C.sizeof(_lib.BinGradTensor) == 16 and [f[0] for f in _lib.BinGradTensor._fields_] == ["g", "numel"]
    assert C.sizeof(_lib.BinGradRecord) == 32 and _lib.BinGradRecord.flags.offset == 16 and _lib.BinGradRecord.status.offset == 20
    assert [f[0] for f in _lib.BinGradRecord._fields_] == ["sumsq", "norm", "coef", "flags", "status", "reserved"]
    for name, value in (("BINGRAD_E_ARG", -1), ("BINGRAD_E_SHAPE", -2)):
        assert int(re.search(rf"#define\s+{name}\s+\((-?\d+)\)", hdr).group(1)) == value
    for name, value in (("BINGRAD_FLAG_NONFINITE", _lib.GRAD_FLAG_NONFINITE), ("BINGRAD_FLAG_STATUS", _lib.GRAD_FLAG_STATUS),
                        ("BINGRAD_MAX_TENSORS", _lib.GRAD_MAX_TENSORS)):
        assert int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1)) == value
    assert "clip_grad_norm_" in hdr and "left exactly as it is" in hdr, "the header states the difference from torch"
    from bin_amd import ops
    assert ops.GRAD_RECORD_WORDS * 4 == 32 and ops.GRAD_FLAGS_WORD * 4 == _lib.BinGradRecord.flags.offset
    rec = ops.grad_record_read(np.frombuffer(np.float64(2.25).tobytes() + np.float32([1.5, 0.5]).tobytes()
                                             + np.int32([3, 1, 0, 0]).tobytes(), dtype=np.int32))
    assert (rec.sumsq, rec.norm, rec.coef, rec.flags, rec.status) == (2.25, 1.5, 0.5, 3, 1)


def test_entry_points_refuse_bad_arguments_before_any_hip_call():
    """Every refusal comes before the first HIP call, so it runs without a device (the pointers below are never dereferenced)."""
    from bin_amd import _lib
    lib = _lib.gradlib()
    table = (_lib.BinGradTensor * 2)()
    ok = 4096                                               # any non-null value: nothing is launched
    norm = lambda t, n, mn=1.0, ws=ok, rec=ok: lib.bingrad_norm(t, n, mn, None, 0, ws, rec, None)
    assert lib.bingrad_norm_workspace_bytes(table, 0) == 8 and lib.bingrad_norm_workspace_bytes(None, 0) == 8
    for fn in (lib.bingrad_norm_workspace_bytes, norm, lambda t, n: lib.bingrad_scale(t, n, ok, None)):
        assert fn(table, -1) == -1 and fn(None, 1) == -1
        assert fn(table, 2) == -1                            # null g in the rows
        for r in table:
            r.g, r.numel = 64, 0
        assert fn(table, 2) == -1                            # numel < 1
        table[0].numel, table[1].numel = 4, -3
        assert fn(table, 2) == -1                            # ... in the second row
        for r in table:
            r.g, r.numel = None, 0
    for r in table:
        r.g, r.numel = 64, 5
    table[1].numel = 2 * GC.CHUNK + 1
    assert lib.bingrad_norm_workspace_bytes(table, 2) == 8 * (1 + 3) and lib.bingrad_norm_workspace_bytes(table, 1) == 8
    for bad in (-1.0, -1e-30, float("nan"), -float("inf")):
        assert norm(table, 2, mn=bad) == -1, bad
    assert norm(table, 2, ws=None) == -1 and norm(table, 2, rec=None) == -1 and norm(table, 0, rec=None) == -1
    assert lib.bingrad_scale(table, 2, None, None) == -1
    assert lib.bingrad_scale(table, 0, ok, None) == 0       # nothing to do, nothing launched
    table[1].numel = (2 ** 24 - 1) * GC.CHUNK             # the most one launch holds: 256 x 2^24 threads would be a 2^32 grid
    assert lib.bingrad_norm_workspace_bytes(table, 2) == 8 * 2 ** 24
    table[1].numel += 1
    assert lib.bingrad_norm_workspace_bytes(table, 2) == -2 and norm(table, 2) == -2 and lib.bingrad_scale(table, 2, ok, None) == -2
    table[1].numel = 2 ** 31 * GC.CHUNK + 1
    assert lib.bingrad_norm_workspace_bytes(table, 2) == -2 and norm(table, 2) == -2


def test_kernel_source_keeps_to_plain_cxx_without_atomics_allocation_or_sync():
    code = "\n".join(ln.split("//")[0] for ln in _source().splitlines())
    for word in ("atomic", "asm", "hipMalloc", "Synchronize", "hipMemcpy", "static int", "static double"):
        assert word not in code, word
    assert "double" in code and "fma(" in code and "__shfl_down" in code
    assert code.index("if (coef == 1.0f) return;") < code.index("find_row(tab);", code.index("grad_scale_kernel"))


# ------------------------------------------------------------------------------------------------ the options
def test_grad_clip_and_skip_bad_steps_option_values(tmp_path):
    from bin_amd.options import options as option
    for empty in ({}, {"train": {}}, {"train": {"grad_clip": None, "skip_bad_steps": None}}, option.dict_to_nonedict({"train": {"lr_G": 1e-4}})):
        assert option.grad_clip(empty) == 0.0 and option.skip_bad_steps(empty) == 0 and option.grad_guard(empty, []) is None
    assert option.grad_clip({"train": {"grad_clip": 0}}) == 0.0 and option.grad_clip({"train": {"grad_clip": 2}}) == 2.0
    assert option.grad_clip({"train": {"grad_clip": 0.5}}) == 0.5 and option.skip_bad_steps({"train": {"skip_bad_steps": 3}}) == 3
    for bad in (-1, -1e-9, float("nan"), float("inf"), "1.0", "1e3", True, [1.0]):
        with pytest.raises(ValueError, match=r"train\.grad_clip"):
            option.grad_clip({"train": {"grad_clip": bad}})
    for bad in (-1, 1.0, 2.5, float("nan"), "2", True, [1]):
        with pytest.raises(ValueError, match=r"train\.skip_bad_steps"):
            option.skip_bad_steps({"train": {"skip_bad_steps": bad}})
    from bin_amd.optim import GradGuard
    g = option.grad_guard({"train": {"grad_clip": 0.25}}, [])
    assert type(g) is GradGuard and g.max_norm == 0.25 and g.skip_bad_steps == 0
    g = option.grad_guard({"train": {"skip_bad_steps": 4}}, [])
    assert type(g) is GradGuard and g.max_norm == 0.0 and g.skip_bad_steps == 4
    # both shipped files carry the keys as comments; a wrong value stops the run when the file is parsed
    y = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    for name in ("bin_stage4_synthetic.yml", "bin_stage4_adobe240.yml"):
        text = open(os.path.join(REPO, "bin_amd", "options", name)).read()
        assert "  # grad_clip: 1.0" in text and "  # skip_bad_steps: 5" in text
    p = str(tmp_path / "o.yml")
    env = os.environ.get("CUDA_VISIBLE_DEVICES")
    try:
        for old, new, key in (("  # grad_clip: 1.0", "  grad_clip: -1.0", "grad_clip"), ("  # grad_clip: 1.0", "  grad_clip: .nan", "grad_clip"),
                              ("  # grad_clip: 1.0", "  grad_clip: big", "grad_clip"),
                              ("  # skip_bad_steps: 5", "  skip_bad_steps: 1.5", "skip_bad_steps"),
                              ("  # skip_bad_steps: 5", "  skip_bad_steps: -2", "skip_bad_steps")):
            open(p, "w").write(y.replace(old, new))
            with pytest.raises(ValueError, match=rf"train\.{key}"):
                option.parse(p, is_train=True)
        open(p, "w").write(y.replace("  # grad_clip: 1.0", "  grad_clip: 1.0").replace("  # skip_bad_steps: 5", "  skip_bad_steps: 5"))
        tr = option.parse(p, is_train=True)["train"]
        assert tr["grad_clip"] == 1.0 and tr["skip_bad_steps"] == 5
        tr = option.parse(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml"))["train"]
        assert tr.get("grad_clip") is None and tr.get("skip_bad_steps") is None
    finally:                                                 # parse() exports gpu_ids as CUDA_VISIBLE_DEVICES
        if env is None:
            os.environ.pop("CUDA_VISIBLE_DEVICES", None)
        else:
            os.environ["CUDA_VISIBLE_DEVICES"] = env


def test_wrappers_build_no_guard_and_load_no_library_when_the_options_are_absent(tmp_path, monkeypatch):
    import videobase_cases as VC
    from bin_amd import _lib
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.models.bin_model import bin_model
    from bin_amd.optim import GradGuard
    from oracle_net import OracleNet
    from test_cpu_host import _Cb, _opt
    monkeypatch.delitem(_lib._loaded, "bingrad", raising=False)

    def both(clip, skip, ft):
        o, v = _opt(tmp_path), VC.opt(tmp_path, ft)
        o["train"]["ft_tsa_only"] = ft
        for d in (o, v):
            if clip is not None:
                d["train"]["grad_clip"] = clip
            if skip is not None:
                d["train"]["skip_bad_steps"] = skip
        return bin_model(o, netG=OracleNet(), cri_pix=_Cb()), VideoBaseModel(v, netG=VC.StubVSR())

    for ft in (None, 3):
        for clip, skip in ((None, None), (0, 0), (0.0, None)):
            for m in both(clip, skip, ft):
                assert m.grad_guard is None
        assert "bingrad" not in _lib._loaded, "nothing of the guard is loaded when both options are off"
        for clip, skip in ((1.5, None), (None, 2), (1.5, 2)):
            b, v = both(clip, skip, ft)
            for m, n in ((b, 540), (v, 4)):
                assert type(m.grad_guard) is GradGuard and len(m.grad_guard.params) == n, "both groups' parameters"
                assert m.grad_guard.max_norm == (clip or 0.0) and m.grad_guard.skip_bad_steps == (skip or 0)
    bad = _opt(tmp_path)
    bad["train"]["grad_clip"] = -3.0
    with pytest.raises(ValueError, match=r"train\.grad_clip"):
        bin_model(bad, netG=OracleNet(), cri_pix=_Cb())


# ------------------------------------------------------------------------------------------------ the class on the host
def test_guard_counts_consecutive_skips_and_names_the_cause():
    from bin_amd import _lib
    from bin_amd.optim import GradGuard
    NF, ST = _lib.GRAD_FLAG_NONFINITE, _lib.GRAD_FLAG_STATUS
    g = GradGuard([], max_norm=1.0, skip_bad_steps=2)
    assert g.last == (0.0, 1.0, 0, False, 0)
    assert g._judge(0) is True and g.consecutive == 0
    assert g._judge(NF) is False and g.consecutive == 1 and g.skipped_total == 1
    assert g._judge(0) is True and g.consecutive == 0, "a clean step resets the count"
    assert g._judge(NF) is False and g._judge(ST) is False and g.consecutive == 2
    with pytest.raises(RuntimeError, match=r"non-finite gradient norm and fp16 saturation on 3 consecutive") as e:
        g._judge(NF | ST)
    assert "tolerates 2" in str(e.value) and "not been stepped" in str(e.value)
    assert g.skipped_total == 4
    assert g._judge(0) is True and g.consecutive == 0
    for flags, words in ((NF, "non-finite gradient norm on 2"), (ST, "fp16 saturation on 2")):
        g = GradGuard([], skip_bad_steps=1)
        assert g._judge(flags) is False
        with pytest.raises(RuntimeError, match=words):
            g._judge(flags)
    for kw in (dict(max_norm=-1.0), dict(max_norm=float("nan")), dict(max_norm=float("inf")), dict(skip_bad_steps=-1), dict(skip_bad_steps=1.5),
               dict(skip_bad_steps=True)):
        with pytest.raises(ValueError):
            GradGuard([], **kw)


def test_guard_leaves_out_gradless_parameters_and_refuses_cpu_gradients():
    from bin_amd import ops
    from bin_amd.optim import GradGuard
    params = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(5))]
    g = GradGuard(params, max_norm=1.0, skip_bad_steps=1)
    assert g.apply() is True and g.last.norm == 0.0, "no gradients: nothing to do, nothing to refuse"
    params[1].grad = torch.full((5,), 2.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        g.apply()
    assert torch.equal(params[1].grad, torch.full((5,), 2.0))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.grad_rows([params[1].grad])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _agree_worker(rank, world, port, q):
    import torch.distributed as dist
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bin_amd import _lib
        from bin_amd.optim import GradGuard
        guard = GradGuard([], skip_bad_steps=2)
        out = []
        for mine in ((0, _lib.GRAD_FLAG_STATUS), (0, 0), (_lib.GRAD_FLAG_NONFINITE, _lib.GRAD_FLAG_NONFINITE)):
            flags = torch.tensor([mine[rank]], dtype=torch.int32)
            guard._agree(flags)
            out.append((int(flags), guard._judge(int(flags)), guard.consecutive))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_ranks_agree_on_skipping_over_gloo():
    """The status word is per rank: rank 1 alone flagged means BOTH skip; both clean means both step."""
    import torch.multiprocessing as mp
    from bin_amd import _lib
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_agree_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want = [(_lib.GRAD_FLAG_STATUS, False, 1), (0, True, 0), (_lib.GRAD_FLAG_NONFINITE, False, 1)]
    assert got[0] == want and got[1] == want, got
