"""-m gpu: the criterion `pixel_criterion: cb+ssim` on the device — libbinssim.so's forward and backward against the float64
restatement over the case table (ssim_loss_cases.py), term independence, determinism, independence of what the buffers held, the
exact cases (x == y, all zeros), the autograd nodes, the fused multi_term_loss against the per-term loop, one training step through
both wrappers, train.micro_batch, and that a `cb` run is what it was and loads nothing of the new library.  Host-side pins:
test_cpu_ssim_loss.py.  Every comparison prints its figures on a line that starts with `[ssim_loss]` before it asserts.

The bars (ssim_loss_cases.py): value 2^-24 absolute, one fp32 rounding of a number of magnitude <= 1; gradient per element
2^-23 |ref| + 1e-9 max(max|ref|, 1 / (planes P)), one fp32 rounding with a factor 2 plus the slack for the order of the double sums.
Measured on the MI355X over the table: the value misses the reference by at most 0.494 of its bar and the gradient by at most
0.493 of its bar, the smooth and nearly flat kinds included (profiles/ssim_loss.md): one fp32 rounding of a double result."""
import functools
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import ssim_loss_cases as SC
from poison import BYTES, poisoned, same_bits

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
S, LAM = 64, 0.5
CB_EPS = 1e-6
CB_BAR = 2.0 ** -21             # relative, per element of a Charbonnier gradient d / sqrt(d^2 + eps) / n computed in fp32: the
                                # difference, its square, the sum, the reciprocal root, two products: <= 8 roundings of 2^-24
ADD = 2.0 ** -24                # one fp32 addition, relative to the larger operand


def _device_case(i):
    terms = SC.case_terms(i)
    pairs = [(x.to(DEV), y.to(DEV)) for _, x, y, _, _ in terms]
    g = torch.tensor([t[3] for t in terms], dtype=torch.float32, device=DEV)
    return terms, pairs, g, [t[4] for t in terms]


# ------------------------------------------------------------------------------------------------ 1. the table
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_value_and_gradients_against_float64(case):
    from bin_amd import ops
    i, h, w, planes, T = case
    terms, pairs, g, need = _device_case(i)
    value = ops.ssim_terms(pairs)
    grads = ops.ssim_terms_grad(pairs, g, need)
    torch.cuda.synchronize()
    assert value.shape == (T,) and value.dtype == torch.float32 and len(grads) == T
    worst_v, worst_g, lines = 0.0, 0.0, []
    for t, ((kind, x, y, gt, nd), (s, rx, ry)) in enumerate(zip(terms, SC.case_reference(i))):
        dv = abs(float(value[t].double().cpu() - s)) / SC.VALUE_BAR
        gx, gy = grads[t]
        assert (gx is not None) == nd[0] and (gy is not None) == nd[1]
        fr = [SC.worst_fraction(o.cpu(), r, planes, h, w) for o, r in ((gx, rx), (gy, ry)) if o is not None]
        assert all(o is None or (o.shape == x.shape and o.dtype == torch.float32) for o in (gx, gy))
        worst_v, worst_g = max(worst_v, dv), max(worst_g, max(fr))
        lines.append((t, kind, dv, max(fr)))
    print(f"[ssim_loss] table {SC.case_id(case)}: worst fraction of the bar: value {worst_v:.3f}, gradient {worst_g:.3f}; per kind " +
          ", ".join(f"{k} {max(l[2] for l in lines if l[1] == k):.2f}/{max(l[3] for l in lines if l[1] == k):.2f}"
                    for k in dict.fromkeys(l[1] for l in lines)))
    for t, kind, dv, fg in lines:
        assert dv <= 1.0, (t, kind, dv)
        assert fg <= 1.0, (t, kind, fg)


# ------------------------------------------------------------------------------------------------ 2, 3. independence, determinism
def test_a_term_is_the_same_bits_alone_and_among_seventeen_and_two_calls_agree():
    from bin_amd import ops
    i = next(c[0] for c in SC.CASES if c[4] == 17 and c[3] == 7)
    terms, pairs, g, need = _device_case(i)
    value, grads = ops.ssim_terms(pairs), ops.ssim_terms_grad(pairs, g, need)
    value2, grads2 = ops.ssim_terms(pairs), ops.ssim_terms_grad(pairs, g, need)
    assert same_bits(value, value2)
    for (a, b), (c, d) in zip(grads, grads2):
        assert all(p is None and q is None or same_bits(p, q) for p, q in ((a, c), (b, d)))
    for t in range(len(pairs)):
        v1 = ops.ssim_terms(pairs[t:t + 1])
        (gx, gy), = ops.ssim_terms_grad(pairs[t:t + 1], g[t:t + 1], need[t:t + 1])
        assert torch.equal(v1, value[t:t + 1]), t
        assert all(p is None and q is None or torch.equal(p, q) for p, q in ((gx, grads[t][0]), (gy, grads[t][1]))), t
    # more than one call's worth of terms: split into calls of 24, the same bits again
    many = pairs + pairs[:9]
    v26 = ops.ssim_terms(many)
    g26 = ops.ssim_terms_grad(many, torch.cat([g, g[:9]]), need + need[:9])
    assert v26.shape == (26,) and torch.equal(v26[:17], value) and torch.equal(v26[17:], value[:9])
    for t in range(26):
        assert all(p is None and q is None or torch.equal(p, q) for p, q in zip(g26[t], grads[t % 17])), t


# ------------------------------------------------------------------------------------------------ 4. what the buffers held
def test_results_do_not_depend_on_what_outputs_and_workspace_held_and_guards_survive():
    from bin_amd import ops
    i = next(c[0] for c in SC.CASES if c[2] - 10 > SC.FW)           # more than one forward tile per plane: several workspace slots
    terms, pairs, g, need = _device_case(i)
    runs = []
    for byte in BYTES:
        with poisoned(byte) as rec:                                  # 256 guard bytes on each side of every allocation, checked on exit
            value = ops.ssim_terms(pairs)
            grads = ops.ssim_terms_grad(pairs, g, need)
            torch.cuda.synchronize()
        assert rec.count == 2 + sum(a + b for a, b in need), "the value, the workspace and every gradient came from the patch"
        runs.append((value, grads))
    for value, grads in runs[1:]:
        assert same_bits(value, runs[0][0])
        for (a, b), (c, d) in zip(grads, runs[0][1]):
            assert all(p is None and q is None or same_bits(p, q) for p, q in ((a, c), (b, d)))
    assert bool(torch.isfinite(runs[-1][0]).all())


# ------------------------------------------------------------------------------------------------ 5, 6. the exact cases
@pytest.mark.parametrize("kind", ["equal", "zeros"])
@pytest.mark.parametrize("shape", [(3, SC.TH + 11, SC.TW + 1), (1, 11, 11), (2, SC.FH + 11, SC.FW + 11)])
def test_equal_and_zero_inputs_score_exactly_one(kind, shape):
    from bin_amd import ops
    planes, h, w = shape
    x, y = (t.to(DEV) for t in SC.content(kind, shape, 77))
    if kind == "equal":
        assert torch.equal(x, y) and x.data_ptr() != y.data_ptr()
    value = ops.ssim_terms([(x, y)])
    (gx, gy), = ops.ssim_terms_grad([(x, y)], torch.ones(1, device=DEV), [(True, True)])
    bar = 1e-9 / (planes * (h - 10) * (w - 10))                      # the element bar at ref = 0
    print(f"[ssim_loss] {kind} {shape}: ssim {float(value):.9g}, max|gx| {float(gx.abs().max()):.3g}, max|gy| {float(gy.abs().max()):.3g}, bar {bar:.3g}")
    assert float(value) == 1.0
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())
    assert float(gx.abs().max()) <= bar and float(gy.abs().max()) <= bar


def test_byte_offsets_past_two_to_the_32():
    """65 536 copies of one 181 x 181 plane: 2^31 - 458 752 elements per tensor, 8.6 GB, so the last planes lie past byte 2^32 and
    element 2^31 - 2^19.  Every plane's gradient must be the one plane's alone, bit for bit: with a power of two for the plane
    count, g / planes and 1 / (planes P) scale exactly.  The value is the one plane's within its bar (65 536 equal double partial
    sums per tile position, added in another order)."""
    from bin_amd import ops
    planes, h, w = 65536, 181, 181
    assert 2 ** 31 - 2 ** 19 <= planes * h * w <= 2 ** 31 - 1
    bx, by = (t.to(DEV) for t in SC.content("smooth", (1, h, w), 9))
    x, y = bx.expand(planes, h, w).contiguous(), by.expand(planes, h, w).contiguous()
    g = torch.tensor([-0.75], device=DEV)
    one_v = ops.ssim_terms([(bx, by)])
    (one_gx, _), = ops.ssim_terms_grad([(bx, by)], g / planes, [(True, False)])
    value = ops.ssim_terms([(x, y)])
    (gx, none), = ops.ssim_terms_grad([(x, y)], g, [(True, False)])
    torch.cuda.synchronize()
    same = bool((gx == one_gx).all())
    print(f"[ssim_loss] 2^31: ssim {float(value):.9g} one plane {float(one_v):.9g}; every plane's gradient equals the one plane's: {same}; "
          f"max|gx| {float(one_gx.abs().max()):.3g}")
    assert none is None and gx.shape == x.shape
    assert abs(float(value) - float(one_v)) <= SC.VALUE_BAR
    assert torch.equal(gx[0], one_gx[0]) and torch.equal(gx[planes // 2], one_gx[0]) and torch.equal(gx[-1], one_gx[0])
    assert same and float(one_gx.abs().max()) > 0


# ------------------------------------------------------------------------------------------------ 7. through autograd
def _cb_grad64(x, y):
    d = x.double() - y.double()
    return d / (d * d + CB_EPS).sqrt() / d.numel()


def test_autograd_of_the_criterion_is_the_two_kernels_gradients():
    from bin_amd import ops
    from bin_amd.models.loss import CharbonnierSsimLoss
    x0, y0 = SC.content("smooth", (6, 24, 40), 5)
    x = x0.reshape(2, 3, 24, 40).to(DEV).requires_grad_()
    y = y0.reshape(2, 3, 24, 40).to(DEV).requires_grad_()
    crit = CharbonnierSsimLoss(LAM)
    loss = crit(x, y)
    gx, gy = torch.autograd.grad(loss, (x, y))
    s, sx, sy = SC.ssim_ref_grads(x0, y0)
    cb64 = ((x0.double() - y0.double()) ** 2 + CB_EPS).sqrt().mean()
    want = float(cb64 + LAM * (1 - s))
    d_loss = abs(float(loss.detach()) - want)
    print(f"[ssim_loss] autograd: loss {float(loss.detach()):.9g} float64 {want:.9g} |d| {d_loss:.3g}; parts {[float(p) for p in crit.last_parts]}")
    assert d_loss <= 2.0 ** -21 * want + LAM * SC.VALUE_BAR          # the cb mean (fp32 partial sums: a few roundings), lambda x the value bar,
    #                                                                  1 - s, the product and the addition: one rounding each
    assert abs(float(crit.last_parts[1]) - float(1 - s)) <= 2 * SC.VALUE_BAR and abs(float(crit.last_parts[0]) - float(cb64)) <= 2.0 ** -22 * float(cb64)
    # the kernels' own outputs, added as autograd adds them: the same bits
    cbx = ops.charbonnier_grad(x.detach(), y.detach(), torch.ones((), device=DEV), CB_EPS)
    (kx, ky), = ops.ssim_terms_grad([(x.detach(), y.detach())], torch.tensor([-LAM], device=DEV), [(True, True)])
    assert torch.equal(gx, cbx + kx) and torch.equal(gy, -cbx + ky)
    # and float64: cb's own gradient plus -lambda x the SSIM gradient, within the two kernels' bars and the addition
    cb = _cb_grad64(x0, y0)
    for name, got, ref_cb, ref_s in (("x", gx, cb, -LAM * sx), ("y", gy, -cb, -LAM * sy)):
        ref = (ref_cb + ref_s).reshape(got.shape)
        bar = (CB_BAR * ref_cb.abs() + SC.grad_bar(ref_s, 6, 24, 40) + ADD * (ref_cb.abs() + ref_s.abs())).reshape(got.shape)
        frac = float(((got.double().cpu() - ref).abs() / bar).max())
        print(f"[ssim_loss] autograd d/d{name}: worst fraction of the bar {frac:.3f}")
        assert frac <= 1.0


# ------------------------------------------------------------------------------------------------ the models
def _opt(tmp, model="bin", criterion="cb+ssim", lr=1e-4, **train):
    opt = {"model": model, "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp)},
           "train": {"pixel_criterion": criterion, "ssim_weight": LAM if criterion == "cb+ssim" else None, "pixel_weight": 1.0,
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
    """(loss, mean cb, mean 1 - ssim, sum |term|) of the 17 pairs in float64."""
    cbs = [((x.double() - y.double()) ** 2 + CB_EPS).sqrt().mean() for x, y in pairs]
    ds = [1 - SC.ssim_ref(x, y) for x, y in pairs]
    terms = [c + LAM * d for c, d in zip(cbs, ds)]
    return float(sum(terms) / len(terms)), float(sum(cbs) / len(cbs)), float(sum(ds) / len(ds)), float(sum(abs(t) for t in terms))


@functools.lru_cache(maxsize=None)
def _stepped():
    """One optimize_parameters step of bin_model at 1 x 64 x 64 under cb+ssim, made once and shared: the model, its weights before."""
    from bin_amd import ops
    m = _bin_model(tempfile.gettempdir())
    before = [p.detach().clone() for p in m.netG.module.parameters()]
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    ops.check_status()
    return m, before


# ------------------------------------------------------------------------------------------------ 8. fused against the loop
def test_fused_multi_term_loss_against_the_per_term_loop():
    from bin_amd.models.loss import CharbonnierSsimLoss, multi_term_loss
    m, _ = _stepped()
    crit = CharbonnierSsimLoss(LAM)

    def run(fused):
        outs = [t.detach().clone().requires_grad_() for t in m.Ft_p]
        pairs = _pairs_of(m, outs)
        if fused:
            loss, terms = multi_term_loss(crit, pairs)
        else:
            terms = [crit(x, y) for x, y in pairs]
            loss = sum(terms) / len(terms)
        return loss.detach(), torch.stack([t.detach() for t in terms]), torch.autograd.grad(loss, outs)
    f_loss, f_terms, f_grads = run(True)
    parts = [float(p) for p in crit.last_parts]
    l_loss, l_terms, l_grads = run(False)
    cpu_pairs = _pairs_of(m, [t.detach().cpu() for t in m.Ft_p])
    cpu_pairs = [(x.cpu(), y.cpu()) for x, y in cpu_pairs]
    want, want_cb, want_d, total = _loss64(cpu_pairs)
    T = 17
    bar = T * 2.0 ** -24 * total
    print(f"[ssim_loss] fused loss {float(f_loss):.9g} loop {float(l_loss):.9g} float64 {want:.9g}; bar {bar:.3g}; parts {parts} float64 "
          f"({want_cb:.9g}, {want_d:.9g}); terms max|fused - loop| {float((f_terms - l_terms).abs().max()):.3g}")
    assert abs(float(f_loss) - float(l_loss)) <= bar and abs(float(f_loss) - want) <= bar and abs(float(l_loss) - want) <= bar
    assert abs(parts[0] - want_cb) <= bar and abs(parts[1] - want_d) <= bar
    assert float((f_terms - l_terms).abs().max()) <= 2.0 ** -23 * float(l_terms.abs().max())
    # gradients: per output the float64 sum of its terms' pieces; each piece within its kernel's bar, plus the fp32 additions
    g = float(torch.tensor(LAM, dtype=torch.float32) / T)
    ref = [torch.zeros(t.shape, dtype=torch.float64) for t in m.Ft_p]
    bars = [torch.zeros(t.shape, dtype=torch.float64) for t in m.Ft_p]
    sums = [torch.zeros(t.shape, dtype=torch.float64) for t in m.Ft_p]
    index = {id(t): k for k, t in enumerate(cpu_pairs[i][0] for i in range(14))}
    for x, y in cpu_pairs:
        _, sx, sy = SC.ssim_ref_grads(x, y)
        cb = _cb_grad64(x, y) / T
        for t, piece_cb, piece_s in ((x, cb, -g * sx), (y, -cb, -g * sy)):
            k = index.get(id(t))
            if k is None:
                continue
            piece_s = piece_s.reshape(t.shape)
            ref[k] += piece_cb + piece_s
            bars[k] += CB_BAR * piece_cb.abs() + SC.grad_bar(piece_s, x.numel() // (S * S), S, S)
            sums[k] += piece_cb.abs() + piece_s.abs()
    worst = {}
    for name, grads in (("fused", f_grads), ("loop", l_grads)):
        worst[name] = max(float(((got.double().cpu() - r).abs() / (b + 3 * ADD * s)).max()) for got, r, b, s in zip(grads, ref, bars, sums))
    twice = sum(1 for k in range(14) if sum(1 for x, y in cpu_pairs for t in (x, y) if index.get(id(t)) == k) == 2)
    print(f"[ssim_loss] fused against loop, gradients: worst fraction of the bar fused {worst['fused']:.3f} loop {worst['loop']:.3f}; "
          f"{twice} outputs sit in two terms")
    assert twice == 6
    assert worst["fused"] <= 1.0 and worst["loop"] <= 1.0


# ------------------------------------------------------------------------------------------------ 9. one step, both wrappers
def test_bin_model_step_under_the_criterion():
    m, before = _stepped()
    pairs = _pairs_of(m, [t.detach().cpu() for t in m.Ft_p])
    pairs = [(x.cpu(), y.cpu()) for x, y in pairs]
    want, want_cb, want_d, total = _loss64(pairs)
    bar = 17 * 2.0 ** -24 * total
    cb, d = (float(p) for p in m.loss_parts)
    print(f"[ssim_loss] bin_model step: loss {float(m.loss):.9g} float64 {want:.9g} bar {bar:.3g}; l_cb {cb:.9g} ({want_cb:.9g}) l_ssim {d:.9g} ({want_d:.9g})")
    assert abs(float(m.loss) - want) <= bar and abs(cb - want_cb) <= bar and abs(d - want_d) <= bar
    assert m.loss_type == "cb+ssim" and len(m.loss_list) == 14 and not any(p.requires_grad for p in m.loss_parts)
    moved = sum(1 for a, b in zip(before, m.netG.module.parameters()) if not torch.equal(a, b))
    print(f"[ssim_loss] bin_model step: {moved} of {len(before)} parameters moved")
    assert moved > len(before) // 2, "parameters move"
    assert all(bool(torch.isfinite(p).all()) for p in m.netG.module.parameters())
    m.train_AverageMeter()
    m.train_AverageMeter_update()                                    # (reads the status word: clean)
    inst, avg = m.get_current_log("train")
    assert abs(avg["Al"] - float(m.loss)) <= 1e-12 and set(inst) == {str(k) for k in range(14)}


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
    assert set(log) == {"total_loss", "l_pix", "ssim_loss"}
    out, gt = m.fake_H.detach().cpu(), data["GT"]
    cb64 = float(((out.double() - gt.double()) ** 2 + CB_EPS).sqrt().mean())
    d64 = float(1 - SC.ssim_ref(out, gt))
    want = cb64 + LAM * d64
    print(f"[ssim_loss] VideoBaseModel step: total {log['total_loss']:.9g} float64 {want:.9g}; l_pix {log['l_pix']:.9g} ({cb64:.9g}) "
          f"ssim_loss {log['ssim_loss']:.9g} ({d64:.9g})")
    assert abs(log["l_pix"] - cb64) <= 2.0 ** -22 * cb64 and abs(log["ssim_loss"] - d64) <= 2 * SC.VALUE_BAR
    assert abs(log["total_loss"] - want) <= 2.0 ** -22 * want + LAM * 2 * SC.VALUE_BAR
    assert sum(1 for a, b in zip(before, m.netG.module.parameters()) if not torch.equal(a, b)) > len(before) // 2, "parameters move"


# ------------------------------------------------------------------------------------------------ 10. micro-batches
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
    print(f"[ssim_loss] micro_batch 1 of 2: loss |d| {d_loss:.3g}, parts |d| {d_parts:.3g}, gradients worst relative {worst:.3g}, outputs max|d| {d_out:.3g}")
    assert not split.loss.requires_grad and all(t.grad_fn is None for t in split.Ft_p)
    assert d_out <= 2e-5 and worst <= 2e-4 and d_loss <= 2e-6 and d_parts <= 2e-6


# ------------------------------------------------------------------------------------------------ 11. cb is what it was
_CB_CHILD = r"""
import sys, tempfile, torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import test_gpu_ssim_loss as T
from bin_amd import _lib
from bin_amd.models import loss as LM

def parent_multi_term_loss(criterion, pairs):      # the function as it stood before cb+ssim existed
    import os
    kind = getattr(criterion, "kind", None)
    if os.environ.get("BIN_AMD_FUSED_LOSS", "1") == "0":
        kind = None
    x0 = pairs[0][0]
    fusable = (kind is not None and len(pairs) <= _lib.LOSS_MAX_TERMS
               and all(t.is_cuda and t.device == x0.device and t.shape == x0.shape for p in pairs for t in p))
    if not fusable:
        terms = [criterion(x, y) for x, y in pairs]
        return sum(terms) / len(terms), terms
    uniq, index = [], {}
    idx_pairs = []
    for x, y in pairs:
        ij = []
        for t in (x, y):
            if id(t) not in index:
                index[id(t)] = len(uniq)
                uniq.append(t)
            ij.append(index[id(t)])
        idx_pairs.append(tuple(ij))
    loss, terms = LM._MultiPixelLossFn.apply(kind, getattr(criterion, "eps", 0.0), tuple(idx_pairs), *uniq)
    return loss, list(terms.unbind(0))

def step():
    m = T._bin_model(tempfile.gettempdir(), criterion="cb")
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    return m

now = step()
product = LM.multi_term_loss
LM.multi_term_loss = parent_multi_term_loss
then = step()
LM.multi_term_loss = product
assert now.loss_parts is None and then.loss_parts is None
assert torch.equal(now.loss, then.loss) and all(torch.equal(a, b) for a, b in zip(now.loss_list, then.loss_list))
for (k, p), q in zip(now.netG.module.named_parameters(), then.netG.module.parameters()):
    assert torch.equal(p.grad, q.grad) and torch.equal(p, q), k
assert "binhip" in _lib._loaded and "binssim" not in _lib._loaded, sorted(_lib._loaded)
print("cb unchanged; loaded:", sorted(_lib._loaded))
"""


def test_cb_steps_are_what_they_were_and_load_nothing_of_the_library():
    """In a process of its own (this one has loaded libbinssim.so long ago): a `cb` step through today's multi_term_loss and one
    through the function as it stood before, bit for bit, and the set of loaded libraries afterwards."""
    run = subprocess.run([sys.executable, "-c", _CB_CHILD, REPO], capture_output=True, text=True, timeout=300)
    print("[ssim_loss] " + run.stdout.strip()[-300:])
    assert run.returncode == 0, run.stderr[-2000:]
    assert "cb unchanged" in run.stdout and "binssim" not in run.stdout
