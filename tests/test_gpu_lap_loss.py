"""-m gpu: the criterion `pixel_criterion: cb+lap` on the device — libbinlap.so's forward and backward against the float64
restatement over the case table (lap_loss_cases.py), term independence, determinism, linearity in g, independence of what the
buffers held, the exact cases (x == y, a constant offset), the autograd node, one training step through
both wrappers, train.micro_batch, and that a `cb` run is what it was and loads nothing of the new library.  Host-side pins:
test_cpu_lap_loss.py.  Every comparison prints its figures on a line that starts with `[lap_loss]` before it asserts.

The bar (lap_loss_cases.bar), on every value and every gradient element, none excluded: |got - ref| <= 2^-23 |ref| + 2^-40 max|ref|:
one fp32 rounding of a double result with a factor 2 of slack, plus the round-off of the double arithmetic."""
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import lap_loss_cases as LC
from poison import BYTES, poisoned, same_bits

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S, MU, LEVELS = 64, 0.5, 5
CB_EPS = LC.EPS


def _device_case(i):
    terms = LC.case_terms(i)
    pairs = [(x.to(DEV), y.to(DEV)) for _, x, y, _, _ in terms]
    g = torch.tensor([t[3] for t in terms], dtype=torch.float32, device=DEV)
    return terms, pairs, g, [t[4] for t in terms]


def _same(a, b):
    return all(p is None and q is None or same_bits(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_value_and_gradients_against_float64(case):
    from bin_amd import ops
    i, planes, h, w, levels, T = case
    terms, pairs, g, need = _device_case(i)
    value = ops.lap_terms(pairs, levels, LC.EPS)
    grads = ops.lap_terms_grad(pairs, g, need, levels, LC.EPS)
    both = ops.lap_terms_grad(pairs, g, [(True, True)] * T, levels, LC.EPS)
    torch.cuda.synchronize()
    assert value.shape == (T,) and value.dtype == torch.float32 and len(grads) == T
    lines = []
    for t, ((kind, x, y, gt, nd), (v, rx, ry)) in enumerate(zip(terms, LC.case_reference(i))):
        fv = LC.worst_fraction(value[t].cpu(), v)
        gx, gy = grads[t]
        assert (gx is not None) == nd[0] and (gy is not None) == nd[1]
        assert all(o is None or (o.shape == x.shape and o.dtype == torch.float32) for o in (gx, gy))
        fr = [LC.worst_fraction(o.cpu(), r) for o, r in ((gx, rx), (gy, ry), (both[t][0], rx), (both[t][1], ry)) if o is not None]
        assert _same([o for o in (gx, gy)], [b if o is not None else None for o, b in zip((gx, gy), both[t])]), "one side alone is the same bits"
        lines.append((t, kind, fv, max(fr)))
    print(f"[lap_loss] table {LC.case_id(case)}: worst fraction of the bar: value {max(l[2] for l in lines):.3f}, gradient "
          f"{max(l[3] for l in lines):.3f}; per kind " +
          ", ".join(f"{k} {max(l[2] for l in lines if l[1] == k):.2f}/{max(l[3] for l in lines if l[1] == k):.2f}"
                    for k in dict.fromkeys(l[1] for l in lines)))
    for t, kind, fv, fg in lines:
        assert fv <= 1.0, (t, kind, fv)
        assert fg <= 1.0, (t, kind, fg)


# ------------------------------------------------------------------------------------------------ 2. the exact cases
@pytest.mark.parametrize("shape", [(2, 33, 47, 5), (1, LC.UH + 1, LC.UW + 1, 2), (1, 1, 1, 1)])
def test_equal_inputs_and_a_constant_offset_are_exact(shape):
    from bin_amd import ops
    planes, h, w, levels = shape
    x, y = (t.to(DEV) for t in LC.content("equal", (planes, h, w), 77))
    assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
    value = ops.lap_terms([(x, y)], levels, LC.EPS)
    (gx, gy), = ops.lap_terms_grad([(x, y)], torch.ones(1, device=DEV), [(True, True)], levels, LC.EPS)
    want = levels * LC.EPS ** 0.5
    print(f"[lap_loss] equal {shape}: lap {float(value):.9g} (L sqrt(eps) = {want:.9g}), max|gx| {float(gx.abs().max()):.3g}")
    assert abs(float(value) - want) <= 2.0 ** -23 * want and float(gx.abs().max()) == 0.0 and float(gy.abs().max()) == 0.0
    # a constant offset reaches the last band only: the value, and a gradient that is R^T ... R^T of a constant
    x, y = (t.to(DEV) for t in LC.content("offset", (planes, h, w), 78))
    value = ops.lap_terms([(x, y)], levels, LC.EPS)
    want = (levels - 1) * LC.EPS ** 0.5 + (LC.OFFSET ** 2 + LC.EPS) ** 0.5
    (gx, _), = ops.lap_terms_grad([(x, y)], torch.ones(1, device=DEV), [(True, False)], levels, LC.EPS)
    total = float(gx.double().sum())
    want_sum = -LC.OFFSET / (LC.OFFSET ** 2 + LC.EPS) ** 0.5           # R's rows sum to 1, so R^T keeps the sum of what it spreads
    print(f"[lap_loss] offset {shape}: lap {float(value):.9g} ({want:.9g}), sum gx {total:.9g} ({want_sum:.9g})")
    assert abs(float(value) - want) <= 2.0 ** -23 * want
    assert abs(total - want_sum) <= 2.0 ** -22 * abs(want_sum)


# ------------------------------------------------------------------------------------------------ 3. independence, determinism, g
@pytest.mark.parametrize("T", [17, 24])
def test_a_term_is_the_same_bits_alone_and_in_company_and_two_calls_agree(T):
    from bin_amd import ops
    i, _, _, _, levels, _ = next(c for c in LC.CASES if c[5] == T and c[4] >= 4)
    terms, pairs, g, need = _device_case(i)
    value, grads = ops.lap_terms(pairs, levels, LC.EPS), ops.lap_terms_grad(pairs, g, need, levels, LC.EPS)
    value2, grads2 = ops.lap_terms(pairs, levels, LC.EPS), ops.lap_terms_grad(pairs, g, need, levels, LC.EPS)
    assert same_bits(value, value2) and all(_same(a, b) for a, b in zip(grads, grads2))
    for t in range(T):
        v1 = ops.lap_terms(pairs[t:t + 1], levels, LC.EPS)
        one, = ops.lap_terms_grad(pairs[t:t + 1], g[t:t + 1], need[t:t + 1], levels, LC.EPS)
        assert same_bits(v1, value[t:t + 1]) and _same(one, grads[t]), t
    # more than one call's worth of terms: split into calls of 24, the same bits again
    many, n = pairs + pairs[:9], T + 9
    vn = ops.lap_terms(many, levels, LC.EPS)
    gn = ops.lap_terms_grad(many, torch.cat([g, g[:9]]), need + need[:9], levels, LC.EPS)
    assert vn.shape == (n,) and torch.equal(vn[:T], value) and torch.equal(vn[T:], value[:9])
    assert all(_same(gn[t], grads[t % T]) for t in range(n))


def test_the_gradient_is_linear_in_g_zero_included():
    from bin_amd import ops
    i, _, _, _, levels, T = next(c for c in LC.CASES if c[1:5] == (2, 33, 47, 5))
    terms, pairs, _, _ = _device_case(i)
    need = [(True, True)] * T
    one = ops.lap_terms_grad(pairs, torch.ones(T, device=DEV), need, levels, LC.EPS)
    g = torch.tensor([(0.0, 2.0, -0.5, -4.0)[t % 4] for t in range(T)], device=DEV)
    got = ops.lap_terms_grad(pairs, g, need, levels, LC.EPS)
    for t in range(T):
        s = float(g[t])
        assert torch.equal(got[t][0], s * one[t][0]) and torch.equal(got[t][1], s * one[t][1]), t      # powers of two scale exactly
        assert torch.equal(got[t][1], -got[t][0])
        if s == 0.0:
            assert float(got[t][0].abs().max()) == 0.0
    assert any(float(o[0].abs().max()) > 0 for o in one)


# ------------------------------------------------------------------------------------------------ 4. what the buffers held
def test_results_do_not_depend_on_what_outputs_and_workspace_held_and_guards_survive():
    from bin_amd import ops
    i, _, _, _, levels, T = next(c for c in LC.CASES if c[1:5] == (1, LC.UH + 1, LC.UW + 1, 2))    # several tiles and slots per plane
    j, _, _, _, levels_j, _ = next(c for c in LC.CASES if c[1:5] == (1, 17, 129, 4))
    runs = []
    for byte in BYTES:
        outs = []
        for k, lv in ((i, levels), (j, levels_j), (0, 1)):
            terms, pairs, g, need = _device_case(k)
            with poisoned(byte) as rec:                              # 256 guard bytes on each side of every allocation, checked on exit
                value = ops.lap_terms(pairs, lv, LC.EPS)
                grads = ops.lap_terms_grad(pairs, g, need, lv, LC.EPS)
                torch.cuda.synchronize()
            assert rec.count == 3 + sum(a + b for a, b in need), "the value, both workspaces and every gradient came from the patch"
            outs.append((value, grads))
        runs.append(outs)
    for outs in runs[1:]:
        for (value, grads), (value0, grads0) in zip(outs, runs[0]):
            assert same_bits(value, value0) and all(_same(a, b) for a, b in zip(grads, grads0))
    assert all(bool(torch.isfinite(v).all()) for v, _ in runs[-1])


# ------------------------------------------------------------------------------------------------ 5. through autograd
def _cb_grad64(x, y):
    d = x.double() - y.double()
    return d / (d * d + CB_EPS).sqrt() / d.numel()


def test_autograd_of_the_criterion_is_the_two_kernels_gradients_and_a_shared_tensor_gets_the_sum():
    from bin_amd import ops
    from bin_amd.models.loss import CharbonnierLapLoss, _MultiLapFn, _index_pairs
    x0, y0 = LC.content("noise", (6, 24, 40), 5)
    x = x0.reshape(2, 3, 24, 40).to(DEV).requires_grad_()
    y = y0.reshape(2, 3, 24, 40).to(DEV).requires_grad_()
    crit = CharbonnierLapLoss(MU, levels=4)
    loss = crit(x, y)
    gx, gy = torch.autograd.grad(loss, (x, y))
    v, lx, ly = LC.closed_form(x0, y0, 4)
    cb64 = ((x0.double() - y0.double()) ** 2 + CB_EPS).sqrt().mean()
    want = float(cb64 + MU * v)
    print(f"[lap_loss] autograd: loss {float(loss.detach()):.9g} float64 {want:.9g}; parts {[float(p) for p in crit.last_parts]} "
          f"float64 ({float(cb64):.9g}, {float(v):.9g})")
    assert abs(float(loss.detach()) - want) <= 2.0 ** -21 * want      # the cb mean in fp32 partial sums, the product, the addition
    assert LC.worst_fraction(crit.last_parts[1].cpu(), v) <= 1.0 and abs(float(crit.last_parts[0]) - float(cb64)) <= 2.0 ** -22 * float(cb64)
    # the kernels' own outputs, added as autograd adds them: the same bits
    cbx = ops.charbonnier_grad(x.detach(), y.detach(), torch.ones((), device=DEV), CB_EPS)
    (kx, ky), = ops.lap_terms_grad([(x.detach(), y.detach())], torch.tensor([MU], device=DEV), [(True, True)], 4, CB_EPS)
    assert torch.equal(gx, cbx + kx) and torch.equal(gy, -cbx + ky)
    assert LC.worst_fraction(kx.cpu(), MU * lx.reshape(kx.shape)) <= 1.0
    # a tensor in two terms gets the sum of its two buffers; a side that needs no gradient gets none
    a, b, c = (t.to(DEV).reshape(2, 3, 24, 40) for t in (x0, y0, LC.content("noise", (6, 24, 40), 6)[0]))
    a.requires_grad_()
    c.requires_grad_()
    uniq, idx = _index_pairs([(a, b), (c, a), (b, b.clone())])
    terms = _MultiLapFn.apply(4, CB_EPS, idx, *uniq)
    w = torch.tensor([1.0, -2.0, 3.0], device=DEV)
    ga, gc = torch.autograd.grad((terms * w).sum(), (a, c))
    (g0, _), (g1c, g1a) = ops.lap_terms_grad([(a.detach(), b), (c.detach(), a.detach())], w[:2].contiguous(), [(True, False), (True, True)], 4, CB_EPS)
    assert torch.equal(ga, g0 + g1a) and torch.equal(gc, g1c)


# ------------------------------------------------------------------------------------------------ the models
def _opt(tmp, model="bin", criterion="cb+lap", lr=1e-4, **train):
    opt = {"model": model, "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp)},
           "train": {"pixel_criterion": criterion, "lap_weight": MU if criterion == "cb+lap" else None, "pixel_weight": 1.0,
                     "weight_decay_G": 0, "ft_tsa_only": None, "optimizer": "torch", "lr_G": lr, "beta1": 0.9, "beta2": 0.99,
                     "lr_scheme": "MultiStepLR", "lr_steps": [100000], "restarts": None, "restart_weights": None, "lr_gamma": 0.5,
                     "clear_state": False}}
    opt["train"].update(train)
    return opt


def _batch(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    return {"LQs": torch.rand(n, 6, 3, S, S, generator=g), "GTenh": torch.rand(n, 6, 3, S, S, generator=g),
            "GTinp": torch.rand(n, 5, 3, S, S, generator=g)}


def _bin_model(tmp, n=1, **kw):
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    m = create_model(_opt(tmp, **kw))
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    m.feed_data(_batch(n))
    return m


def _pairs_of(m, outs):
    pairs = [(outs[i], gt) for i, gt in enumerate(m.get_info(mode=1)[1])]
    return pairs + [(outs[1], outs[7]), (outs[5], outs[9]), (outs[2], outs[8])]


def _loss64(pairs):
    """(loss, mean cb, mean lap, sum |term|) of the 17 pairs in float64."""
    cbs = [((x.double() - y.double()) ** 2 + CB_EPS).sqrt().mean() for x, y in pairs]
    laps = [LC.lap_ref(x, y, LEVELS) for x, y in pairs]
    terms = [c + MU * v for c, v in zip(cbs, laps)]
    return float(sum(terms) / len(terms)), float(sum(cbs) / len(cbs)), float(sum(laps) / len(laps)), float(sum(abs(t) for t in terms))


@functools.lru_cache(maxsize=None)
def _stepped():
    """One optimize_parameters step of bin_model at 1 x 64 x 64 under cb+lap, made once and shared: the model, its weights before."""
    from bin_amd import ops
    m = _bin_model(tempfile.gettempdir())
    before = [p.detach().clone() for p in m.netG.module.parameters()]
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    ops.check_status()
    return m, before


# ------------------------------------------------------------------------------------------------ 6. one step, both wrappers
def test_bin_model_step_under_the_criterion():
    m, before = _stepped()
    pairs = [(x.cpu(), y.cpu()) for x, y in _pairs_of(m, [t.detach() for t in m.Ft_p])]
    want, want_cb, want_lap, total = _loss64(pairs)
    bar = 17 * 2.0 ** -24 * total                                    # 17 fp32 terms, each rounded once, and their fp32 sum
    cb, lap = (float(p) for p in m.loss_parts)
    print(f"[lap_loss] bin_model step: loss {float(m.loss):.9g} float64 {want:.9g} bar {bar:.3g}; l_cb {cb:.9g} ({want_cb:.9g}) l_lap {lap:.9g} ({want_lap:.9g})")
    assert abs(float(m.loss) - want) <= bar and abs(cb - want_cb) <= bar and abs(lap - want_lap) <= bar
    assert m.loss_type == "cb+lap" and m.loss_part_names == ("l_cb", "l_lap") and len(m.loss_list) == 14
    assert not any(p.requires_grad for p in m.loss_parts) and m.cri_pix.levels == LEVELS
    moved = sum(1 for a, b in zip(before, m.netG.module.parameters()) if not torch.equal(a, b))
    print(f"[lap_loss] bin_model step: {moved} of {len(before)} parameters moved")
    assert moved > len(before) // 2, "parameters move"
    assert all(bool(torch.isfinite(p).all()) for p in m.netG.module.parameters())


def test_video_base_model_step_under_the_criterion(tmp_path):
    from bin_amd import ops
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.weights import reference_state_dict
    g = torch.Generator().manual_seed(17)
    data = {"LQs": torch.rand(1, 6, 3, S, S, generator=g), "GT": torch.rand(1, 14, 3, S, S, generator=g)}
    m = VideoBaseModel(_opt(tmp_path, model="video_base"))
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    m.feed_data(data)
    before = [p.detach().clone() for p in m.netG.module.parameters()]
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    ops.check_status()
    log = m.get_current_log()
    assert set(log) == {"total_loss", "l_pix", "lap_loss"}
    out, gt = m.fake_H.detach().cpu(), data["GT"]
    cb64 = float(((out.double() - gt.double()) ** 2 + CB_EPS).sqrt().mean())
    lap64 = float(LC.lap_ref(out, gt, LEVELS))
    want = cb64 + MU * lap64
    print(f"[lap_loss] VideoBaseModel step: total {log['total_loss']:.9g} float64 {want:.9g}; l_pix {log['l_pix']:.9g} ({cb64:.9g}) "
          f"lap_loss {log['lap_loss']:.9g} ({lap64:.9g})")
    assert abs(log["l_pix"] - cb64) <= 2.0 ** -22 * cb64 and abs(log["lap_loss"] - lap64) <= (2.0 ** -23 + 2.0 ** -40) * lap64
    assert abs(log["total_loss"] - want) <= 2.0 ** -21 * want
    assert sum(1 for a, b in zip(before, m.netG.module.parameters()) if not torch.equal(a, b)) > len(before) // 2, "parameters move"


# ------------------------------------------------------------------------------------------------ 7. micro-batches
def test_split_step_is_the_unsplit_step_under_the_criterion(tmp_path):
    """test_gpu_micro_batch.py's comparison and bars: outputs within 2e-5, gradients within 2e-4 relative per parameter, loss 2e-6."""
    whole, split = _bin_model(tmp_path, n=2, lr=0.0), _bin_model(tmp_path, n=2, lr=0.0, micro_batch=1)
    whole.optimize_parameters(1)
    split.optimize_parameters(1)
    torch.cuda.synchronize()

    def rel(a, b):
        scale = float(b.abs().max())
        return float((a - b).abs().max()) / scale if scale > 0 else float((a - b).abs().max())
    worst = max(rel(p.grad, q.grad) for p, q in zip(split.netG.module.parameters(), whole.netG.module.parameters()))
    d_out = max(float((a - b.detach()).abs().max()) for a, b in zip(split.Ft_p, whole.Ft_p))
    d_loss = abs(float(split.loss) - float(whole.loss))
    d_parts = max(abs(float(a) - float(b)) for a, b in zip(split.loss_parts, whole.loss_parts))
    print(f"[lap_loss] micro_batch 1 of 2: loss |d| {d_loss:.3g}, parts |d| {d_parts:.3g}, gradients worst relative {worst:.3g}, outputs max|d| {d_out:.3g}")
    assert not split.loss.requires_grad and all(t.grad_fn is None for t in split.Ft_p)
    assert d_out <= 2e-5 and worst <= 2e-4 and d_loss <= 2e-6 and d_parts <= 2e-6


# ------------------------------------------------------------------------------------------------ 8. cb is what it was
_CB_CHILD = r"""
import sys, tempfile, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_lap_loss as T
from bin_amd import _lib

def step(criterion):
    m = T._bin_model(tempfile.gettempdir(), criterion=criterion)
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    return m

fresh = step("cb")                                  # the process has seen nothing of the criterion yet
assert "binhip" in _lib._loaded and "binlap" not in _lib._loaded and "binssim" not in _lib._loaded, sorted(_lib._loaded)
lap = step("cb+lap")
assert "binlap" in _lib._loaded and lap.loss_parts is not None
again = step("cb")                                  # a cb step after a cb+lap step
assert fresh.loss_parts is None and again.loss_parts is None and again.loss_part_names is None
assert torch.equal(fresh.loss, again.loss) and all(torch.equal(a, b) for a, b in zip(fresh.loss_list, again.loss_list))
for (k, p), q in zip(fresh.netG.module.named_parameters(), again.netG.module.parameters()):
    assert torch.equal(p.grad, q.grad) and torch.equal(p, q), k
print("cb unchanged before and after a cb+lap step")
"""


def test_cb_steps_are_what_they_were_and_load_nothing_of_the_library():
    """In a process of its own (this one has loaded libbinlap.so long ago): a `cb` step in a fresh process state, which leaves
    libbinlap.so unloaded; then a cb+lap step; then a `cb` step again, bit for bit the first one."""
    run = subprocess.run([sys.executable, "-c", _CB_CHILD, REPO], capture_output=True, text=True, timeout=300)
    print("[lap_loss] " + run.stdout.strip()[-300:])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "cb unchanged" in run.stdout
