"""GPU: the weight average (train.ema_decay) — binema_step over the case table of ema_cases.py against float64, both data paths
bit for bit, bin_amd.optim.WeightEMA, the parameter exchange of applied(), and the option through bin_model, VideoBaseModel,
checkpoints, resume and bin_amd.train.  CPU side: test_cpu_ema.py."""
import functools
import logging
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ema_cases as EC
from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _refs(tag):
    """(inputs, float64 reference, float32 restatement) of a case: computed once, shared, never written to."""
    case = EC.CASE_BY_TAG[tag]
    inp = EC.make_inputs(case)
    return inp, EC.reference64(case, inp), EC.numpy32(case, inp)


class _Arenas:
    """The rows of a case in two device arenas (e, p) with guards, and the host row table over them, built by ops.ema_row."""

    def __init__(self, rows, e, p, offs=None):
        from bin_amd import ops
        if offs is not None:
            rows = tuple(EC.Row(r.numel, offs, r.mag) for r in rows)
        self.rows = rows
        self.host = [EC.arena(rows, 0, e), EC.arena(rows, 1, p)]
        self.buf = [torch.from_numpy(a).cuda() for a in self.host]
        assert all(b.data_ptr() % 16 == 0 for b in self.buf)
        self.starts = [EC.layout(rows, k)[0] for k in (0, 1)]
        self.n = len(rows)
        self.table = ops.ema_rows(self.n)
        for i, r in enumerate(rows):
            ev, pv = (self.buf[k][self.starts[k][i]:self.starts[k][i] + r.numel] for k in (0, 1))
            assert ev.data_ptr() % 16 == 4 * r.offs[0] and pv.data_ptr() % 16 == 4 * r.offs[1]
            ops.ema_row(self.table, i, ev, pv)

    def set_p(self, p):
        self.host[1] = EC.arena(self.rows, 1, p)
        self.buf[1].copy_(torch.from_numpy(self.host[1]))

    def step(self, decay):
        from bin_amd import ops
        ops.ema_launch(self.table, self.n, self.buf[0].device, decay)

    def read(self, kind):
        torch.cuda.synchronize()
        return EC.split(self.rows, kind, self.buf[kind].cpu().numpy())


# ------------------------------------------------------------------------------------------------ 1. the case table vs float64
@pytest.mark.parametrize("tag", EC.TAGS)
def test_case_table_vs_float64(tag):
    case = EC.CASE_BY_TAG[tag]
    rows = EC.rows_of(case)
    inp, r64, r32 = _refs(tag)
    t = _Arenas(rows, inp["e"], inp["p"][0])
    for k in range(case.steps):
        if k:
            t.set_p(inp["p"][k])
        t.step(case.decay)
    got, rest = t.read(0)
    ratio = EC.compare(tag, rows, got, r64, r32)
    assert ratio <= 1.0
    assert (rest == EC.GUARD).all(), "a guard float of the shadows' arena was written"
    assert np.array_equal(_bits(t.buf[1].cpu().numpy()), _bits(t.host[1])), "p and its guards are only read"


# ------------------------------------------------------------------------------------------------ 2. the two data paths agree
@pytest.mark.parametrize("tag", ["numel_aligned", "decay0.9999_zero_k3", "decay0.9_far_k10", f"rows_{2 * EC.EMA_MAX_TENSORS + 1}"])
def test_aligned_and_offset_rows_give_the_same_bits(tag):
    case = EC.CASE_BY_TAG[tag]
    inp = _refs(tag)[0]
    out = []
    for offs in ((0, 0), (1, 0), (0, 3), (2, 2), (1, 3)):
        t = _Arenas(EC.rows_of(case), inp["e"], inp["p"][0], offs)
        for k in range(case.steps):
            if k:
                t.set_p(inp["p"][k])
            t.step(case.decay)
        out.append(t.read(0)[0])
    for other in out[1:]:
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(out[0], other))


def test_stage4_rows_as_separate_tensors_and_as_views_into_one_flat_buffer():
    from bin_amd import ops
    inp, r64, r32 = _refs("rows_stage4")
    case = EC.CASE_BY_TAG["rows_stage4"]
    numels = [x.size for x in inp["e"]]
    assert len(numels) == 540

    def run(e, p):
        table = ops.ema_rows(540)
        for i in range(540):
            ops.ema_row(table, i, e[i], p[i])
        for k in range(case.steps):
            if k:
                for dst, src in zip(p, inp["p"][k]):
                    dst.copy_(torch.from_numpy(src))
            ops.ema_launch(table, 540, e[0].device, case.decay)
        torch.cuda.synchronize()
        return e
    separate = run([torch.from_numpy(x).cuda() for x in inp["e"]], [torch.from_numpy(x).cuda() for x in inp["p"][0]])
    flat_e = torch.from_numpy(np.concatenate(inp["e"])).cuda()
    flat_p = torch.from_numpy(np.concatenate(inp["p"][0])).cuda()
    cuts = np.concatenate([[0], np.cumsum(numels)])
    views_e = [flat_e[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    views_p = [flat_p[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert len({v.data_ptr() % 16 for v in views_e}) >= 3, "views at every 4-byte offset"
    views = run(views_e, views_p)
    assert all(torch.equal(a, b) for a, b in zip(separate, views))
    EC.compare("stage4 separate", EC.rows_of(case), [t.cpu().numpy() for t in separate], r64, r32)
    with pytest.raises(ValueError, match="float32"):
        ops.ema_row(ops.ema_rows(1), 0, separate[0].double(), separate[0].double())
    with pytest.raises(ValueError, match="contiguous"):
        ops.ema_row(ops.ema_rows(1), 0, torch.ones(4, 8, device="cuda").t(), torch.ones(8, 4, device="cuda"))
    with pytest.raises(ValueError, match="elements"):
        ops.ema_row(ops.ema_rows(1), 0, separate[0], separate[1][:1])
    with pytest.raises(RuntimeError):
        ops.ema_row(ops.ema_rows(1), 0, separate[0].cpu(), separate[0].cpu())


def test_non_finite_weights_propagate_into_the_shadow():
    from bin_amd import ops
    n = EC.CHUNK + 5
    p = torch.ones(n, device="cuda")
    p[3], p[EC.CHUNK + 1], p[7] = float("nan"), float("inf"), -float("inf")
    e = torch.zeros(n, device="cuda")
    table = ops.ema_rows(1)
    ops.ema_row(table, 0, e, p)
    ops.ema_launch(table, 1, e.device, 0.5)
    h = e.cpu().numpy()
    assert np.isnan(h[3]) and h[EC.CHUNK + 1] == np.inf and h[7] == -np.inf and np.isfinite(np.delete(h, [3, 7, EC.CHUNK + 1])).all()
    assert (np.delete(h, [3, 7, EC.CHUNK + 1]) == 0.5).all()


# ------------------------------------------------------------------------------------------------ 3. the class
def test_weight_ema_class_over_a_random_walk():
    from bin_amd.optim import WeightEMA
    K, decay = 10, 0.999
    rng = np.random.Generator(np.random.PCG64(41))
    shapes = [(1,), (3,), (5, 51), (EC.CHUNK,), (2, EC.CHUNK // 2 + 1), (64, 64, 3, 3), (257,)]
    mags = [1.0, 1e-3, 1.0, 1e-3, 1e4, 1.0, 1e-6]
    ps = [[(rng.standard_normal(s) * m).astype(np.float32) for s, m in zip(shapes, mags)]]
    for _ in range(K - 1):
        ps.append([(x + (rng.standard_normal(x.shape) * 0.1 * m).astype(np.float32)).astype(np.float32) for x, m in zip(ps[-1], mags)])
    start = [(x * np.float32(0.5)).astype(np.float32) for x in ps[0]]
    params = [torch.nn.Parameter(torch.from_numpy(x).cuda()) for x in start]
    ema = WeightEMA(params, decay)
    assert all(torch.equal(e, p.detach()) and e.data_ptr() % 16 == 0 and e.is_cuda for e, p in zip(ema.shadow, params))
    flat = ema._flat[params[0].device]
    assert all(e.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr() for e in ema.shadow), "one flat buffer"
    staged = [[torch.from_numpy(x).cuda() for x in step] for step in ps]
    ptrs = [p.data_ptr() for p in params]
    table = None
    for k in range(K):
        with torch.no_grad():
            for p, x in zip(params, staged[k]):
                p.copy_(x)
        versions = [e._version for e in ema.shadow]
        torch.cuda.synchronize()
        mem, count = torch.cuda.memory_allocated(), torch.cuda.memory_stats()["allocation.all.allocated"]
        ema.update()
        if k:                                                # no allocation after the first update(), not even a freed one
            assert torch.cuda.memory_allocated() == mem and torch.cuda.memory_stats()["allocation.all.allocated"] == count
            assert ema._tables[params[0].device][1] is table, "the host row table is reused while no pointer changed"
        table = ema._tables[params[0].device][1]
        assert all(e._version > v for e, v in zip(ema.shadow, versions)), "the shadows' version counters are bumped"
    assert [p.data_ptr() for p in params] == ptrs
    got = [e.cpu().numpy().reshape(-1) for e in ema.shadow]
    start_flat = [x.reshape(-1) for x in start]
    r64, bars = EC.walk_reference(start_flat, [[x.reshape(-1) for x in step] for step in ps], decay)
    assert EC.within("WeightEMA, 10 steps", got, r64, bars) <= 1.0
    # a parameter whose storage changed: the table is rebuilt and the new storage is what is read
    with torch.no_grad():
        params[2].data = torch.full_like(params[2], 3.0)
    before = [e.clone() for e in ema.shadow]
    ema.update()
    assert ema._tables[params[0].device][1] is not table
    want = before[2] + np.float32(1.0 - decay) * (3.0 - before[2])
    assert float((ema.shadow[2] - want).abs().max()) <= 2.0 ** -22 * 3.0
    # the state goes to the host and back
    state = ema.state_dict()
    other = WeightEMA([torch.nn.Parameter(torch.zeros(s, device="cuda")) for s in shapes], 0.5)
    other.load_state_dict(state)
    assert other.decay == decay and all(torch.equal(a, b) for a, b in zip(ema.shadow, other.shadow))


# ------------------------------------------------------------------------------------------------ 4. applied()
def test_applied_exchanges_and_restores_on_the_device():
    from bin_amd.optim import WeightEMA
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.Conv2d(8, 3, 3)).cuda()
    calls = []
    net[0].invalidate_kernel_weights = lambda: calls.append(0)
    params = list(net.parameters())
    ema = WeightEMA(params, 0.9)
    with torch.no_grad():
        for p in params:
            p.add_(0.25)
    ema.update()
    values = [p.detach().clone() for p in params]
    ids = [(p.data_ptr(), p._version) for p in params]
    assert not any(torch.equal(e, v) for e, v in zip(ema.shadow, values))
    with ema.applied(net):
        assert calls == [0]
        assert all(torch.equal(p.detach(), e) and p.data_ptr() == e.data_ptr() for p, e in zip(params, ema.shadow))
    assert calls == [0, 0]
    assert [(p.data_ptr(), p._version) for p in params] == ids and all(torch.equal(p.detach(), v) for p, v in zip(params, values))
    with pytest.raises(ZeroDivisionError):
        with ema.applied(net):
            1 / 0
    assert [(p.data_ptr(), p._version) for p in params] == ids and all(torch.equal(p.detach(), v) for p, v in zip(params, values))
    assert len(calls) == 4


# ------------------------------------------------------------------------------------------------ 5 - 8. through bin_model
@pytest.fixture(scope="module")
def weights_file(tmp_path_factory):
    """bin_stage4's canonical weights as a generator checkpoint: the wrappers load it, so the shadows start from LOADED weights."""
    from bin_amd.weights import reference_state_dict
    path = tmp_path_factory.mktemp("ema_weights") / "start_G.pth"
    torch.save(reference_state_dict(0), path)
    return str(path)


def _bin_opt(tmp_path, optimizer, pretrain, **train):
    os.makedirs(tmp_path, exist_ok=True)
    opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
           "path": {"pretrain_model_G": pretrain, "strict_load": True, "models": str(tmp_path), "training_state": str(tmp_path),
                    "resume_state": None},
           "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "optimizer": optimizer,
                     "lr_G": 1e-4, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    opt["train"].update(train)
    return opt


def _feed(m):
    g = load_golden("g9_train_steps")
    m.feed_data({"LQs": torch.from_numpy(g["LQs"]), "GTenh": torch.from_numpy(g["GTenh"]), "GTinp": torch.from_numpy(g["GTinp"])})
    return m


def _model(tmp_path, optimizer, pretrain, **train):
    from bin_amd.models import create_model
    return _feed(create_model(_bin_opt(tmp_path, optimizer, pretrain, **train)))


def _params(m):
    return [p.detach().clone() for p in m.netG.module.parameters()]


def _moments(m):
    st = m.optimizer_G.state
    return [st[p][k] for p in m.netG.module.parameters() for k in ("exp_avg", "exp_avg_sq")]


def _all_equal(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_ema_through_bin_model(tmp_path, weights_file, optimizer):
    """A: four steps with ema_decay 0.9.  B: the same with a validation forward under ema_scope() after step 2.  C: the option off.
    The average touches nothing of the training run, a scope in the middle touches nothing of either, and the shadows are the
    float64 recursion over A's per-step parameters."""
    from bin_amd.optim import WeightEMA
    a = _model(tmp_path / "a", optimizer, weights_file, ema_decay=0.9)
    b = _model(tmp_path / "b", optimizer, weights_file, ema_decay=0.9)
    c = _model(tmp_path / "c", optimizer, weights_file)
    assert type(a.weight_ema) is WeightEMA and a.weight_ema.decay == 0.9 and c.weight_ema is None
    assert len(a.weight_ema.shadow) == 540 and _all_equal(a.weight_ema.shadow, _params(a)), "the shadows start from the loaded weights"
    start = [e.cpu().numpy().reshape(-1) for e in a.weight_ema.shadow]
    steps = []
    for step in (1, 2, 3, 4):
        for m in (a, b, c):
            m.optimize_parameters(step)
        steps.append(_params(a))
        if step == 2:
            ids = [(p.data_ptr(), p._version) for p in b.netG.module.parameters()]
            with b.ema_scope():
                out = b.test()
            assert [(p.data_ptr(), p._version) for p in b.netG.module.parameters()] == ids
            assert all(torch.isfinite(o).all() for o in out)
    assert _all_equal(_params(a), _params(b)) and _all_equal(_params(a), _params(c))
    assert _all_equal(_moments(a), _moments(b)) and _all_equal(_moments(a), _moments(c))
    assert _all_equal(a.weight_ema.shadow, b.weight_ema.shadow)
    assert float(a.loss.detach()) == float(b.loss.detach()) == float(c.loss.detach())
    ps = [[p.cpu().numpy().reshape(-1) for p in step] for step in steps]
    r64, bars = EC.walk_reference(start, ps, 0.9)
    got = [e.cpu().numpy().reshape(-1) for e in a.weight_ema.shadow]
    assert EC.within(f"bin_model/{optimizer}, 4 steps", got, r64, bars) <= 1.0
    assert not any(np.array_equal(g, s) for g, s in zip(got, start)) and not any(np.array_equal(g, p) for g, p in zip(got, ps[-1]))


def test_validation_and_the_saved_file_see_the_averaged_weights(tmp_path, weights_file):
    m = _model(tmp_path / "m", "hip", weights_file, ema_decay=0.9)
    for step in (1, 2):
        m.optimize_parameters(step)
    raw = [o.clone() for o in m.test()]
    with m.ema_scope():
        avg = [o.clone() for o in m.test()]
    again = m.test()
    assert _all_equal(raw, again), "outside the scope the training weights answer, as before it"
    assert not any(torch.equal(x, y) for x, y in zip(raw, avg))
    m.save("2")
    assert sorted(os.listdir(tmp_path / "m")) == ["2_G.pth", "2_G_ema.pth"]
    sd, sd_ema = torch.load(tmp_path / "m" / "2_G.pth"), torch.load(tmp_path / "m" / "2_G_ema.pth")
    assert len(sd) == len(sd_ema) == 1332 and list(sd) == list(sd_ema)
    named = dict(m.netG.module.named_parameters())
    shadow = {n: e for (n, _), e in zip(m.netG.module.named_parameters(), m.weight_ema.shadow)}
    assert all(torch.equal(sd[n], p.detach().cpu()) and torch.equal(sd_ema[n], shadow[n].cpu()) for n, p in named.items())
    from bin_amd.models import create_model
    opt = _bin_opt(tmp_path / "fresh", "hip", str(tmp_path / "m" / "2_G_ema.pth"))
    opt["is_train"] = False
    fresh = _feed(create_model(opt))
    assert fresh.weight_ema is None
    assert _all_equal(avg, fresh.test()), "an ordinary checkpoint: a fresh model that loaded it gives the scope's outputs"
    # one more step, a second scope: different outputs again (the relayout cache and the streaming memo serve nothing stale)
    m.optimize_parameters(3)
    with m.ema_scope():
        avg3 = [o.clone() for o in m.test()]
    raw3 = m.test()
    assert not any(torch.equal(x, y) for x, y in zip(avg, avg3)) and not any(torch.equal(x, y) for x, y in zip(avg3, raw3))
    assert not any(torch.equal(x, y) for x, y in zip(raw, raw3))
    m.save("3")
    opt["path"]["pretrain_model_G"] = str(tmp_path / "m" / "3_G_ema.pth")
    assert _all_equal(avg3, _feed(create_model(opt)).test())


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_a_skipped_step_leaves_the_shadows_as_they_were(tmp_path, weights_file, optimizer):
    from bin_amd import _lib as L
    m = _model(tmp_path, optimizer, weights_file, ema_decay=0.9, skip_bad_steps=2)
    guard = m.grad_guard
    poison = {"on": False}
    real_apply = guard.apply

    def apply():
        if poison["on"]:
            p = list(m.netG.module.parameters())[3]
            p.grad.view(-1)[p.numel() // 2] = float("nan")   # an ordinary float store
        return real_apply()
    guard.apply = apply
    m.optimize_parameters(1)
    assert guard.last.flags == 0
    before = [e.clone() for e in m.weight_ema.shadow]
    versions = [e._version for e in m.weight_ema.shadow]
    assert not _all_equal(before, _params(m))
    poison["on"] = True
    m.optimize_parameters(2)
    assert guard.last.flags == L.GRAD_FLAG_NONFINITE and guard.last.skipped is True
    assert all(np.array_equal(_bits(x.cpu().numpy()), _bits(y.cpu().numpy())) for x, y in zip(before, m.weight_ema.shadow))
    assert [e._version for e in m.weight_ema.shadow] == versions
    poison["on"] = False
    m.optimize_parameters(3)
    assert guard.last.flags == 0 and not any(torch.equal(x, y) for x, y in zip(before, m.weight_ema.shadow))
    assert all(torch.isfinite(e).all() for e in m.weight_ema.shadow)


@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_save_and_resume(tmp_path, weights_file, optimizer, caplog):
    from bin_amd.models import create_model
    from bin_amd.options import options as option
    a = _model(tmp_path, optimizer, weights_file, ema_decay=0.9)
    for step in (1, 2, 3):
        a.optimize_parameters(step)
    a.save(3)
    a.save_training_state(0, 3)
    state = torch.load(tmp_path / "3.state", map_location="cpu", weights_only=False)
    assert set(state) == {"epoch", "iter", "schedulers", "optimizers"}, "`.state` files do not change"

    def resumed():
        opt = _bin_opt(tmp_path, optimizer, weights_file, ema_decay=0.9)
        opt["path"]["resume_state"] = str(tmp_path / "3.state")
        option.check_resume(opt, state["iter"])
        assert opt["path"]["pretrain_model_G"] == str(tmp_path / "3_G.pth")
        m = _feed(create_model(opt))
        with caplog.at_level(logging.WARNING, logger="base"):
            caplog.clear()
            m.resume_training(state)
        return m, [r.getMessage() for r in caplog.records if "ema_decay" in r.getMessage()]
    b, warned = resumed()
    assert not warned
    assert _all_equal(a.weight_ema.shadow, b.weight_ema.shadow) and _all_equal(_params(a), _params(b))
    for step in (4, 5):
        a.optimize_parameters(step)
        b.optimize_parameters(step)
    assert _all_equal(a.weight_ema.shadow, b.weight_ema.shadow) and _all_equal(_params(a), _params(b))
    assert _all_equal(_moments(a), _moments(b))
    del b
    os.remove(tmp_path / "3_G_ema.pth")
    c, warned = resumed()
    assert len(warned) == 1 and "3_G_ema.pth" in warned[0]
    assert _all_equal(c.weight_ema.shadow, _params(c)), "the shadows start from the loaded weights"


# ------------------------------------------------------------------------------------------------ 9. VideoBaseModel
def test_video_base_model_honours_the_option_with_two_groups(tmp_path):
    import videobase_cases as VC
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.optim import WeightEMA

    def model(**train):
        o = VC.opt(tmp_path, 3, "cb")
        o["gpu_ids"] = [0]
        o["train"].update(train)
        m = VideoBaseModel(o, netG=VC.StubVSR())
        m.feed_data(VC.batch())
        return m
    off = model()
    assert off.weight_ema is None
    with off.ema_scope():
        pass
    m = model(ema_decay=0.5)
    assert type(m.weight_ema) is WeightEMA and len(m.weight_ema.shadow) == 4
    assert [len(g["params"]) for g in m.optimizer_G.param_groups] == [2, 2]
    start = [e.cpu().numpy().reshape(-1) for e in m.weight_ema.shadow]
    steps = []
    for step in (3, 4, 5):                                   # step >= ft_tsa_only: both groups train
        m.optimize_parameters(step)
        steps.append([p.detach().cpu().numpy().reshape(-1) for p in m.netG.module.parameters()])
    assert not any(np.array_equal(a, b) for a, b in zip(start, steps[0])), "both groups moved"
    r64, bars = EC.walk_reference(start, steps, 0.5)
    EC.within("VideoBaseModel, 3 steps", [e.cpu().numpy().reshape(-1) for e in m.weight_ema.shadow], r64, bars)
    ids = [(p.data_ptr(), p._version) for p in m.netG.module.parameters()]
    with m.ema_scope():
        assert all(torch.equal(p.detach(), e) for p, e in zip(m.netG.module.parameters(), m.weight_ema.shadow))
    assert [(p.data_ptr(), p._version) for p in m.netG.module.parameters()] == ids
    m.save("5")
    assert {"5_G.pth", "5_G_ema.pth"} <= set(os.listdir(tmp_path))
    sd = torch.load(tmp_path / "5_G_ema.pth")
    assert all(torch.equal(sd[n], e.cpu()) for (n, _), e in zip(m.netG.module.named_parameters(), m.weight_ema.shadow))


# ------------------------------------------------------------------------------------------------ 10. the training script
def test_train_script_validates_and_saves_the_average(tmp_path):
    """python -m bin_amd.train on the shipped synthetic option file with ema_decay: 0.9, three steps, one validation pass."""
    y = open(os.path.join(REPO, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    y = y.replace("save_path: ./runs", f"save_path: {tmp_path}").replace("num_windows: 4000", "num_windows: 64")
    y = y.replace("n_workers: 3", "n_workers: 0").replace("niter: 2000", "niter: 4")
    y = y.replace("val_freq: 500", "val_freq: 2\n  val_max_batches: 2").replace("  # ema_decay: 0.999 ", "  ema_decay: 0.9 ")
    assert "\n  ema_decay: 0.9 " in y
    p = str(tmp_path / "syn.yml")
    open(p, "w").write(y)
    r = subprocess.run([sys.executable, "-m", "bin_amd.train", "-opt", p, "--max_iter", "3"], cwd=REPO, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exp = tmp_path / "experiments" / "synthetic_stage4"
    text = open(exp / [f for f in os.listdir(exp) if f.endswith(".log")][0]).read()
    lines = [ln for ln in text.splitlines() if "<val" in ln]
    print("\n".join(lines))
    assert len(lines) == 1 and "<val ema iter:" in lines[0] and "End of training." in text and "nan" not in lines[0].lower()
    raw = torch.load(exp / "models" / "latest_G.pth", weights_only=False)
    avg = torch.load(exp / "models" / "latest_G_ema.pth", weights_only=False)
    assert len(raw) == len(avg) == 1332 and list(raw) == list(avg)
    assert all(torch.isfinite(v).all() for v in avg.values())
    assert sum(not torch.equal(raw[k], avg[k]) for k in raw) > len(raw) // 2, "the two files hold different values"
