"""-m gpu: the gradient-guard kernels (bingrad_norm / bingrad_scale), bin_amd.optim.GradGuard over them and `train.grad_clip` /
`train.skip_bad_steps` through the wrappers.  Case table, float64 reference and the bars (|sumsq - ref| <= N * 2^-53 * ref; norm and
coef within one fp32 ulp): gradguard_cases.py; CPU pins: test_cpu_gradguard.py.  Each comparison prints its figures on a line that
starts with `[gradguard]` before it asserts."""
import ctypes as C
import functools
import math
import threading

import numpy as np
import pytest
import torch

import gradguard_cases as GC
from conftest import load_golden

pytestmark = pytest.mark.gpu
OC = GC.OC


def _lib():
    from bin_amd import _lib as L
    return L, L.gradlib()


def _stream(s=None):
    return C.c_void_p((s or torch.cuda.current_stream()).cuda_stream)


@functools.lru_cache(maxsize=None)
def _refs(tag):
    """(inputs, float64 sum of squares) of a case: computed once, shared, never written to."""
    grads = GC.make_inputs(GC.CASE_BY_TAG[tag])
    return grads, GC.reference_sumsq(grads)


class _Table:
    """The rows of a case in one device arena with guards, and the host row table over it."""

    def __init__(self, rows, grads):
        L, _ = _lib()
        self.rows, self.host = rows, OC.arena(rows, GC.KIND, grads)
        self.buf = torch.from_numpy(self.host).cuda()
        assert self.buf.data_ptr() % 16 == 0
        self.starts = OC.layout(rows, GC.KIND)[0]
        self.table = (L.BinGradTensor * len(rows))()
        for i, (s, r) in enumerate(zip(self.starts, rows)):
            self.table[i].g, self.table[i].numel = self.buf.data_ptr() + 4 * s, r.numel
        self.n = len(rows)
        self.elements = sum(r.numel for r in rows)
        nbytes = _lib()[1].bingrad_norm_workspace_bytes(self.table, self.n)
        assert nbytes >= 8
        self.ws = torch.full((nbytes // 8 + 1,), float("nan"), dtype=torch.float64, device="cuda")   # one slot more: it must stay NaN
        self.rec = torch.zeros(8, dtype=torch.int32, device="cuda")

    def norm(self, max_norm, status=None, mask=0, stream=None, ws=None, rec=None):
        L, lib = _lib()
        ws, rec = self.ws if ws is None else ws, self.rec if rec is None else rec
        L.check(lib.bingrad_norm(self.table, self.n, max_norm, None if status is None else C.c_void_p(status.data_ptr()), mask,
                                 C.c_void_p(ws.data_ptr()), C.c_void_p(rec.data_ptr()), _stream(stream)), "grad_norm")
        return rec

    def scale(self, rec=None, stream=None):
        L, lib = _lib()
        L.check(lib.bingrad_scale(self.table, self.n, C.c_void_p((self.rec if rec is None else rec).data_ptr()), _stream(stream)), "grad_scale")

    def read(self, rec=None):
        from bin_amd import ops
        torch.cuda.synchronize()
        return ops.grad_record_read((self.rec if rec is None else rec).cpu())

    def arena(self):
        torch.cuda.synchronize()
        return self.buf.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ 1. norm and coefficient vs float64
@pytest.mark.parametrize("tag", [c.tag for c in GC.CASES])
def test_norm_and_clip_coefficient_vs_float64(tag):
    """bingrad_norm over the case table at every max_norm kind: sumsq within N * 2^-53 * ref, norm and coef within one fp32 ulp, coef
    exactly 1 where nothing is to be clipped, no flag set, the arena (gradients and guards) unwritten, the slot past the workspace
    untouched; and the same record bytes from a second run."""
    L, _ = _lib()
    case = GC.CASE_BY_TAG[tag]
    grads, ref = _refs(tag)
    t = _Table(GC.rows_of(case), grads)
    for kind in GC.MAX_NORMS:
        mn = GC.max_norm_of(kind, ref)
        rec = t.read(t.norm(mn))
        assert rec.flags == 0 and rec.status == 0 and tuple(rec.reserved) == (0, 0)
        GC.check(f"{tag}/{kind}", t.elements, ref, rec.sumsq, rec.norm, rec.coef, mn)
        if tag == "zeros":
            assert rec.sumsq == 0.0 and rec.norm == 0.0 and rec.coef == 1.0
        elif kind in ("half", "milli"):
            assert rec.coef < 1.0
        first = t.rec.cpu().numpy().copy()
        t.rec.zero_()
        t.ws.fill_(float("nan"))
        t.norm(mn)
        torch.cuda.synchronize()
        assert np.array_equal(t.rec.cpu().numpy(), first), "two runs give the same record bytes"
    assert np.array_equal(_bits(t.arena()), _bits(t.host)), "bingrad_norm wrote to the gradients or the guards"
    assert math.isnan(float(t.ws[-1])) and not torch.isnan(t.ws[:-1]).any()


# ------------------------------------------------------------------------------------------------ 2. the scale pass
@pytest.mark.parametrize("tag", ["numel_off0", "numel_off1", "numel_off2", "numel_off3", "mag_1e-30", "mag_1e+25",
                                 f"rows_{GC.MAX_TENSORS + 1}", "mixed_decade_per_tensor"])
def test_scale_multiplies_in_fp32_bit_for_bit_and_only_when_clipping(tag):
    case = GC.CASE_BY_TAG[tag]
    grads, ref = _refs(tag)
    rows = GC.rows_of(case)
    t = _Table(rows, grads)
    # far above the norm AND above the formula's 1e-6: at magnitude 1e-30 a max_norm of 1000 norms is still 1e-19 of norm + 1e-6
    t.norm(max(GC.max_norm_of("far_above", ref), 1.0))
    t.scale()
    assert t.read().coef == 1.0 and np.array_equal(_bits(t.arena()), _bits(t.host)), "coef == 1 must write nothing"
    t.norm(GC.max_norm_of("half", ref))
    t.scale()
    coef = np.float32(t.read().coef)
    assert 0 < coef < 1
    got, blank = OC.split(rows, GC.KIND, t.arena())
    assert np.array_equal(_bits(blank), _bits(np.full_like(blank, GC.GUARD))), "a float outside the rows changed"
    with np.errstate(under="ignore"):
        for i, (a, g) in enumerate(zip(got, grads)):
            assert np.array_equal(_bits(a), _bits(g * coef)), (tag, i, rows[i])


def test_scale_with_coef_one_keeps_nan_payloads_and_negative_zero():
    rows = (GC._row(GC.CHUNK + 5, 0, 1.0), GC._row(7, 1, 1.0))
    grads = [np.linspace(-1, 1, r.numel).astype(np.float32) for r in rows]
    odd = np.array([0x7fc01234, 0xffc00001, 0x80000000, 0x7f800000, 0x00000001], dtype=np.uint32).view(np.float32)
    grads[0][:5], grads[0][-5:], grads[1][:5] = odd, odd, odd
    t = _Table(rows, grads)
    t.norm(1e-3)
    t.scale()
    rec = t.read()
    L, _ = _lib()
    assert rec.flags == L.GRAD_FLAG_NONFINITE and rec.coef == 1.0 and not math.isfinite(rec.sumsq)
    assert np.array_equal(_bits(t.arena()), _bits(t.host))


# ------------------------------------------------------------------------------------------------ 3. non-finite gradients
def test_non_finite_gradients_raise_the_flag_and_are_left_as_they_are():
    """+inf, -inf and NaN in turn at the first element of the first row, the last element of a partial chunk, a 1-element row and a row
    of the second launch: NONFINITE, coef exactly 1 although max_norm would clip, and bingrad_scale changes no byte."""
    L, _ = _lib()
    small = (5, 257, 96, 3)
    rows = [GC._row(2 * GC.CHUNK + 1, 0, 1.0), GC._row(GC.CHUNK + 77, 1, 1.0), GC._row(1, 2, 1.0)]
    rows += [GC._row(small[i % 4], i % 4, 1.0) for i in range(GC.MAX_TENSORS - 2)]          # row MAX + 1 (index MAX) is in launch 2
    rows = tuple(rows)
    assert len(rows) == GC.MAX_TENSORS + 1
    case = GC.Case("non_finite", rows, 777)
    grads = GC.make_inputs(case)
    clean = GC.reference_sumsq(grads)
    places = ((0, 0), (0, 2 * GC.CHUNK), (1, GC.CHUNK + 76), (2, 0), (GC.MAX_TENSORS, rows[GC.MAX_TENSORS].numel - 1))
    t = _Table(rows, grads)
    for row, j in places:
        for val in (np.inf, -np.inf, np.nan):
            host = [g.copy() for g in grads]
            host[row][j] = val
            arena = OC.arena(rows, GC.KIND, host)
            t.buf.copy_(torch.from_numpy(arena))
            t.norm(0.5 * math.sqrt(clean))
            t.scale()
            rec = t.read()
            print(f"[gradguard] non_finite row {row} element {j} value {val}: flags {rec.flags} sumsq {rec.sumsq} coef {rec.coef}")
            assert rec.flags == L.GRAD_FLAG_NONFINITE and rec.coef == 1.0 and not math.isfinite(rec.sumsq), (row, j, val)
            assert np.array_equal(_bits(t.arena()), _bits(arena)), (row, j, val)
    t.buf.copy_(torch.from_numpy(t.host))                    # and clean again: the flag is per call
    rec = t.read(t.norm(0.0))
    assert rec.flags == 0
    GC.check("non_finite/clean", t.elements, clean, rec.sumsq, rec.norm, rec.coef, 0.0)


# ------------------------------------------------------------------------------------------------ 4. the status word
def test_status_word_is_read_under_the_mask_and_never_written():
    L, _ = _lib()
    grads, ref = _refs("mag_1")
    t = _Table(GC.rows_of(GC.CASE_BY_TAG["mag_1"]), grads)
    word = torch.tensor([L.STATUS_SATURATED | 8], dtype=torch.int32, device="cuda")
    for status, mask, flags, seen in ((word, L.STATUS_SATURATED, L.GRAD_FLAG_STATUS, L.STATUS_SATURATED), (word, 0xFFFFFFFF, L.GRAD_FLAG_STATUS, 9),
                                      (None, L.STATUS_SATURATED, 0, 0), (word, 2 | 4, 0, 0), (word, 0, 0, 0)):
        rec = t.read(t.norm(GC.max_norm_of("half", ref), status, mask))
        assert (rec.flags, rec.status) == (flags, seen), (mask, rec.flags, rec.status)
        assert rec.coef < 1.0, "the status flag does not change the coefficient"
        assert int(word.item()) == (L.STATUS_SATURATED | 8), "the word is only read"
    word.zero_()
    rec = t.read(t.norm(0.0, word, L.STATUS_SATURATED))
    assert (rec.flags, rec.status) == (0, 0)


# ------------------------------------------------------------------------------------------------ 5. determinism, re-entrancy
def test_four_host_threads_on_four_streams_give_the_serial_bytes():
    tag = "mixed_decade_per_tensor"
    grads, ref = _refs(tag)
    rows = GC.rows_of(GC.CASE_BY_TAG[tag])
    mn = GC.max_norm_of("half", ref)
    serial = _Table(rows, grads)
    serial.norm(mn)
    serial.scale()
    want_rec, want_arena = serial.rec.cpu().numpy().copy(), serial.arena()
    tables = [_Table(rows, grads) for _ in range(4)]
    streams = [torch.cuda.Stream() for _ in range(4)]
    torch.cuda.synchronize()
    errors = []

    def work(t, s):
        try:
            for _ in range(3):
                t.norm(mn, stream=s)
            t.scale(stream=s)
        except Exception as e:                              # noqa: BLE001 — surfaced below
            errors.append(e)
    threads = [threading.Thread(target=work, args=(t, s)) for t, s in zip(tables, streams)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    torch.cuda.synchronize()
    assert not errors, errors
    for t in tables:
        assert np.array_equal(t.rec.cpu().numpy(), want_rec)
        assert np.array_equal(_bits(t.arena()), _bits(want_arena))


# ------------------------------------------------------------------------------------------------ 6. both gradient layouts, through ops
def test_stage4_gradients_as_separate_tensors_and_as_views_into_the_flat_buffer():
    from bin_amd import ops
    from bin_amd.models.bin_model import FlatGradAllReduce
    grads, ref = _refs("rows_stage4")
    n = sum(g.size for g in grads)
    mn = GC.max_norm_of("half", ref)
    separate = [torch.from_numpy(g).cuda() for g in grads]
    params = [torch.nn.Parameter(torch.empty(g.size, device="cuda")) for g in grads]
    sync = FlatGradAllReduce(params)
    sync.attach()
    sync.flat.copy_(torch.from_numpy(np.concatenate(grads)))
    views = [p.grad for p in params]
    assert len({v.data_ptr() % 16 for v in views}) >= 3 and sync._views_intact()
    coefs = []
    for name, tensors in (("separate", separate), ("flat views", views)):
        rows = ops.grad_rows(tensors)
        assert rows.n == 540 and rows.numel == n and rows.workspace_bytes >= 8 * ((n + GC.CHUNK - 1) // GC.CHUNK)
        ws = torch.empty(rows.workspace_bytes // 8, dtype=torch.float64, device="cuda")
        rec = ops.grad_record("cuda")
        for kind in ("off", "half"):
            m = GC.max_norm_of(kind, ref)
            ops.grad_norm(rows, ws, rec, m)
            torch.cuda.synchronize()
            r = ops.grad_record_read(rec.cpu())
            assert r.flags == 0
            GC.check(f"stage4 {name}/{kind}", n, ref, r.sumsq, r.norm, r.coef, m)
        ops.grad_scale(rows, rec)
        torch.cuda.synchronize()
        coefs.append(np.float32(r.coef))
        for i in (0, 1, 17, 539):
            assert np.array_equal(_bits(tensors[i].cpu().numpy().ravel()), _bits(grads[i] * coefs[-1])), (name, i)
        with pytest.raises(ValueError, match="workspace"):
            ops.grad_norm(rows, ws[:4], rec, mn)
    assert np.array_equal(_bits(sync.flat.cpu().numpy()), _bits(np.concatenate(grads) * coefs[1]))
    with pytest.raises(ValueError, match="float32"):
        ops.grad_rows([separate[0].double()])
    with pytest.raises(ValueError, match="contiguous"):
        ops.grad_rows([torch.ones(4, 8, device="cuda").t()])


def test_guard_class_clips_like_float64_and_reads_its_record_lazily():
    from bin_amd.optim import GradGuard
    grads, ref = _refs("mixed_decade_per_tensor")
    params = [torch.nn.Parameter(torch.zeros(g.size, device="cuda")) for g in grads] + [torch.nn.Parameter(torch.zeros(3, device="cuda"))]
    for p, g in zip(params, grads):
        p.grad = torch.from_numpy(g.copy()).cuda()
    mn = GC.max_norm_of("half", ref)
    guard = GradGuard(params, max_norm=mn)
    versions = [p.grad._version for p in params[:-1]]
    assert guard.apply() is True and guard._pending, "skip_bad_steps == 0: the record is not read in apply()"
    last = guard.last
    assert not guard._pending and last.flags == 0 and last.skipped is False and last.consecutive == 0
    GC.check_norm_and_coef("guard class", grads, last.norm, last.coef, mn)
    for p, g, v in zip(params, grads, versions):
        assert np.array_equal(_bits(p.grad.cpu().numpy()), _bits(g * np.float32(last.coef))) and p.grad._version > v
    assert params[-1].grad is None
    rows_before = guard._rows[1]
    guard.apply()
    assert guard._rows[1] is rows_before, "the host row table is reused while no pointer changed"
    assert guard.last.coef == 1.0, "already at half the norm"
    params[0].grad = params[0].grad.clone()
    guard.apply()
    assert guard._rows[1] is not rows_before


# ------------------------------------------------------------------------------------------------ 7. through bin_model
def _bin_opt(tmp_path, optimizer, **train):
    opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp_path), "training_state": str(tmp_path)},
           "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "optimizer": optimizer,
                     "lr_G": 1e-4, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    opt["train"].update(train)
    return opt


def _model(tmp_path, optimizer, **train):
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    m = create_model(_bin_opt(tmp_path, optimizer, **train))
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    g = load_golden("g9_train_steps")
    m.feed_data({"LQs": torch.from_numpy(g["LQs"]), "GTenh": torch.from_numpy(g["GTenh"]), "GTinp": torch.from_numpy(g["GTinp"])})
    return m


def _snapshot(m):
    """Every parameter, Adam moment and step counter as host arrays, and the parameters' version counters."""
    params = list(m.netG.module.parameters())
    st = m.optimizer_G.state
    return ([p.detach().cpu().numpy().copy() for p in params],
            [st[p][k].cpu().numpy().copy() for p in params if p in st and len(st[p]) for k in ("exp_avg", "exp_avg_sq")],
            [float(st[p]["step"]) for p in params if p in st and len(st[p])], [p._version for p in params])


def _same(a, b, versions=True):
    assert len(a[0]) == len(b[0]) and len(a[1]) == len(b[1])
    for k in (0, 1):
        for i, (x, y) in enumerate(zip(a[k], b[k])):
            assert np.array_equal(_bits(x), _bits(y)), ("parameters" if k == 0 else "Adam state", i)
    assert a[2] == b[2], "step counters"
    if versions:
        assert a[3] == b[3], "parameter _version"


class _ByHand:
    """Stands where the guard stands and multiplies every gradient by the next of `coefs` in fp32, as a caller would by hand."""
    skip_bad_steps = 0

    def __init__(self, params, coefs):
        self.params, self.coefs = params, list(coefs)

    def apply(self):
        c = float(np.float32(self.coefs.pop(0)))
        for p in self.params:
            if p.grad is not None:
                p.grad.mul_(c)
        return True


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_grad_clip_through_bin_model(tmp_path, optimizer):
    """grad_clip far above the norm: three steps bit-identical to the run without the option.  grad_clip at half the first step's
    norm: bit-identical to multiplying the gradients by the same fp32 coefficients by hand between backward and step."""
    from bin_amd.optim import GradGuard
    plain = _model(tmp_path, optimizer)
    assert plain.grad_guard is None
    high = _model(tmp_path, optimizer, grad_clip=1e9)
    assert type(high.grad_guard) is GradGuard
    norms = []
    for step in (1, 2, 3):
        plain.optimize_parameters(step)
        high.optimize_parameters(step)
        norms.append(high.grad_guard.last.norm)
        assert high.grad_guard.last.coef == 1.0 and high.grad_guard.last.flags == 0
    _same(_snapshot(plain), _snapshot(high))
    assert float(plain.loss) == float(high.loss) and all(math.isfinite(v) and v > 0 for v in norms)
    # the norm the guard measured is the float64 norm of the gradients it left in place
    GC.check_norm_and_coef(f"bin_model/{optimizer} step 3", [p.grad.cpu().numpy() for p in high.netG.module.parameters()], norms[-1], 1.0, 0.0)
    del plain, high
    clipped = _model(tmp_path, optimizer, grad_clip=0.5 * norms[0])
    coefs = []
    for step in (1, 2):
        clipped.optimize_parameters(step)
        coefs.append(clipped.grad_guard.last.coef)
    print(f"[gradguard] bin_model/{optimizer}: norms {norms} coefs {coefs}")
    assert 0.4 < coefs[0] <= 0.5 and all(0 < c < 1 for c in coefs)
    hand = _model(tmp_path, optimizer)
    hand.grad_guard = _ByHand(list(hand.netG.module.parameters()), coefs)
    for step in (1, 2):
        hand.optimize_parameters(step)
    _same(_snapshot(clipped), _snapshot(hand), versions=False)
    assert float(clipped.loss) == float(hand.loss)


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_bad_steps_are_skipped_before_adam_writes_anything(tmp_path, optimizer):
    """skip_bad_steps: 2.  An inf written into one gradient after the backward: the step is skipped and parameters, moments, step counters
    and version counters are what they were; a clean step then proceeds and resets the count; three flagged steps in a row raise on
    the third with the weights still untouched; a SATURATED status word gives the same skip, is cleared, and check_status is quiet."""
    from bin_amd import _lib as L, ops
    m = _model(tmp_path, optimizer, skip_bad_steps=2)
    guard = m.grad_guard
    assert guard.max_norm == 0.0 and guard.skip_bad_steps == 2
    poison = {"on": False}
    real_apply = guard.apply

    def apply():
        if poison["on"]:
            p = list(m.netG.module.parameters())[3]
            p.grad.view(-1)[p.numel() // 2] = float("inf")   # an ordinary float store
        return real_apply()
    guard.apply = apply
    m.optimize_parameters(1)                                 # a clean step first: there is Adam state to protect
    assert guard.last.flags == 0 and guard.last.skipped is False
    before = _snapshot(m)
    assert all(s == 1.0 for s in before[2]) and len(before[2]) == 540
    poison["on"] = True
    m.optimize_parameters(2)
    assert guard.last.flags == L.GRAD_FLAG_NONFINITE and guard.last.skipped is True and guard.last.consecutive == 1
    assert math.isinf(guard.last.norm) and guard.last.coef == 1.0
    _same(before, _snapshot(m))
    ops.check_status(m.device)
    poison["on"] = False
    m.optimize_parameters(3)
    assert guard.last.flags == 0 and guard.consecutive == 0 and guard.skipped_total == 1
    after = _snapshot(m)
    assert all(s == 2.0 for s in after[2]) and not np.array_equal(after[0][0], before[0][0]), "the clean step proceeds"
    poison["on"] = True
    m.optimize_parameters(4)
    m.optimize_parameters(5)
    assert guard.consecutive == 2
    with pytest.raises(RuntimeError, match=r"non-finite gradient norm on 3 consecutive"):
        m.optimize_parameters(6)
    _same(after, _snapshot(m))
    poison["on"] = False
    # fp16 saturation reported by the status word: the same skip; the bit is cleared, other bits are not
    m.optimize_parameters(7)
    assert guard.consecutive == 0
    after = _snapshot(m)
    word = ops.status_word(m.device)
    word.fill_(L.STATUS_SATURATED)
    m.optimize_parameters(8)
    assert guard.last.flags == L.GRAD_FLAG_STATUS and guard.last.skipped is True and math.isfinite(guard.last.norm)
    _same(after, _snapshot(m))
    assert int(word.item()) == 0
    ops.check_status(m.device)                               # does not raise
    m.train_AverageMeter()
    m.train_AverageMeter_update()


def test_without_skip_bad_steps_the_status_word_is_not_consulted(tmp_path):
    """skip_bad_steps: 0 with a guard present (grad_clip): the step is taken and check_status raises after it, as it always did."""
    from bin_amd import _lib as L, ops
    m = _model(tmp_path, "hip", grad_clip=1e9)
    before = _snapshot(m)
    word = ops.status_word(m.device)
    word.fill_(L.STATUS_SATURATED)
    try:
        m.optimize_parameters(1)
        assert m.grad_guard.last.flags == 0 and m.grad_guard.last.skipped is False
        assert not np.array_equal(_snapshot(m)[0][0], before[0][0]), "the step was taken"
        assert int(word.item()) & L.STATUS_SATURATED
        m.train_AverageMeter()
        with pytest.raises(RuntimeError, match="fp16 range exceeded"):
            m.train_AverageMeter_update()
    finally:
        word.zero_()


# ------------------------------------------------------------------------------------------------ 8. VideoBaseModel
@pytest.mark.parametrize("method", ["optimize_parameters", "optimize_parameters_without_schudlue"])
def test_video_base_model_honours_both_options_with_two_groups(tmp_path, method):
    """Both step methods of VideoBaseModel with ft_tsa_only's two groups.  The stand-in generator runs torch's own convolutions, whose
    backward need not repeat bit for bit between two models, so everything is compared within one step: the gradients the optimizer
    sees against the gradients the backward left, and the parameters around a skipped step."""
    import videobase_cases as VC
    from bin_amd import _lib as L
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.optim import GradGuard

    def model(**train):
        o = VC.opt(tmp_path, 3, "cb")
        o["gpu_ids"] = [0]
        o["train"].update(train)
        m = VideoBaseModel(o, netG=VC.StubVSR())
        m.feed_data(VC.batch())
        return m

    def params(m):
        return [p.detach().cpu().numpy().copy() for p in m.netG.module.parameters()]

    def watch(m, poison=None):
        """Wrap the guard: keep the gradients as the backward left them (after an optional ordinary float store) and as apply() leaves them."""
        seen, real = {}, m.grad_guard.apply

        def apply():
            ps = list(m.netG.module.parameters())
            if poison is not None and seen.get("poison"):
                ps[-1].grad.view(-1)[0] = poison
            seen["before"] = [p.grad.cpu().numpy().copy() for p in ps]
            take = real()
            seen["after"] = [p.grad.cpu().numpy().copy() for p in ps]
            return take
        m.grad_guard.apply = apply
        return seen
    assert model().grad_guard is None
    m = model(grad_clip=1e9, skip_bad_steps=2)
    assert type(m.grad_guard) is GradGuard and len(m.grad_guard.params) == 4
    assert [len(g["params"]) for g in m.optimizer_G.param_groups] == [2, 2]
    seen = watch(m, poison=float("nan"))
    start = params(m)
    getattr(m, method)(3)                                    # step >= ft_tsa_only: both groups train
    last = m.grad_guard.last
    assert last.coef == 1.0 and last.flags == 0 and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(seen["before"], seen["after"]))
    GC.check_norm_and_coef(f"videobase/{method}", seen["before"], last.norm, last.coef, 1e9)
    moved = params(m)
    assert not any(np.array_equal(a, b) for a, b in zip(start, moved)), "the step was taken, in both groups"
    seen["poison"] = True                                    # a flagged step is skipped for both groups
    getattr(m, method)(4)
    assert m.grad_guard.last.flags == L.GRAD_FLAG_NONFINITE and m.grad_guard.last.skipped and m.grad_guard.consecutive == 1
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(moved, params(m)))
    seen["poison"] = False
    getattr(m, method)(5)
    assert m.grad_guard.consecutive == 0 and not any(np.array_equal(a, b) for a, b in zip(moved, params(m)))
    # clipping: the optimizer sees the backward's gradients times the fp32 coefficient, bit for bit
    c = model(grad_clip=0.5 * last.norm)
    seen = watch(c)
    getattr(c, method)(3)
    coef = c.grad_guard.last.coef
    assert 0.4 < coef < 1.0
    GC.check_norm_and_coef(f"videobase/{method} clipped", seen["before"], c.grad_guard.last.norm, coef, c.grad_guard.max_norm)
    assert all(np.array_equal(_bits(a), _bits(b * np.float32(coef))) for a, b in zip(seen["after"], seen["before"]))
