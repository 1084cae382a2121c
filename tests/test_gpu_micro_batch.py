"""-m gpu: `train.micro_batch` through the real generator in f16x3 — which shapes the kernels see, the split step against the unsplit
step (loss, 14 terms, every gradient, the 14 outputs), identity when nothing is split, one optimizer / EMA / guard action per step, a
flagged step skipped as a whole, peak memory, two data-parallel ranks on one GPU, and VideoBaseModel.  Host-side pins:
test_cpu_micro_batch.py.  Every comparison prints its figures on a line that starts with `[micro_batch]` before it asserts.

The bars are those of the tests this feature borrows its reasons from: loss 2e-6 and terms 5e-6 absolute, gradients 2e-4 relative
(max|a - b| / max|b| per parameter: test_config3_step_8x256_batch_linearity_and_determinism holds "batch 8 = mean of eight batch 1"
to them: fp32-class kernels, another summation split), outputs 2e-5 (smoke()'s f16x3 bar), updated weights 2e-5
(test_training_step_matches_reference_golden's `after.*`).

The training schedule of bin_stage4 runs the pyramid's 17 RDN calls batched along N as four calls, one per weight set (5n, 6n, 4n and
2n images for a batch of n; BIN_AMD_FOUR_CALLS / `four_calls`); with `four_calls = False` it runs the 17 calls one by one on n
images each.  The shape test covers both: 17 K backwards on the chunk sizes, and 4 K backwards on their multiples."""
import functools
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, SEED = 4, 64, 3


def _opt(tmp, lr=0.0, criterion="cb", optimizer="torch", dist=False, **train):
    opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": dist,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp)},
           "train": {"pixel_criterion": criterion, "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "optimizer": optimizer,
                     "lr_G": lr, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    opt["train"].update(train)
    return opt


def _batch(n=B, size=S, seed=SEED):
    g = torch.Generator().manual_seed(seed)
    return {"LQs": torch.rand(n, 6, 3, size, size, generator=g), "GTenh": torch.rand(n, 6, 3, size, size, generator=g),
            "GTinp": torch.rand(n, 5, 3, size, size, generator=g)}


def _model(tmp, data=None, **kw):
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    m = create_model(_opt(tmp, **kw))
    m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
    m.feed_data(_batch() if data is None else data)
    return m


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.netG.module.named_parameters()}


def _params(m):
    return {k: p.detach().clone() for k, p in m.netG.module.named_parameters()}


def _rel(a, b):
    scale = float(b.abs().max())
    return float((a - b).abs().max()) / scale if scale > 0 else float((a - b).abs().max())


def _worst_rel(got, ref):
    return max(_rel(got[k], ref[k]) for k in ref)


@functools.lru_cache(maxsize=None)
def _whole(criterion, lr=0.0, optimizer="torch"):
    """The unsplit step on the shared batch: computed once per (criterion, lr, optimizer), shared, never written to."""
    m = _model(tempfile.gettempdir(), lr=lr, criterion=criterion, optimizer=optimizer)
    assert m.micro_batch is None
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    return {"loss": m.loss.detach().clone(), "loss_list": torch.stack([t.detach() for t in m.loss_list]),
            "grads": _grads(m), "Ft_p": [t.detach().clone() for t in m.Ft_p], "params": _params(m)}


# ------------------------------------------------------------------------------------------------ 1. shapes seen
@pytest.mark.parametrize("four_calls", [False, True], ids=["17_calls", "four_calls"])
@pytest.mark.parametrize("micro", [1, 2, 3])
def test_rdn_backwards_see_the_chunk_sizes_in_order(tmp_path, micro, four_calls):
    """One step of B = 4: the RDN backwards number 17 K on n = the chunk sizes in order (the schedule of 17 calls), 4 K on
    (2, 4, 6, 5) x the chunk sizes (the four-call schedule training runs by default).  Where the option is ignored every n belongs
    to the whole batch of 4."""
    from bin_amd.options.options import micro_batches
    m = _model(tmp_path, micro_batch=micro)
    net = m.netG.module
    net.four_calls = four_calls
    seen = []

    def hook(kind, module, dims, ws, info):
        if kind == "backward":
            seen.append(dims[0])
    for mod in net.rdn_modules():
        mod.debug_hook = hook
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    sizes = [n for _, n in micro_batches(B, micro)]
    K = len(sizes)
    assert sizes == {1: [1, 1, 1, 1], 2: [2, 2], 3: [3, 1]}[micro]
    print(f"[micro_batch] shapes micro {micro} four_calls {four_calls}: {len(seen)} RDN backwards, n = {seen}")
    if not four_calls:
        assert len(seen) == 17 * K
        assert seen == [n for n in sizes for _ in range(17)]
    else:
        assert len(seen) == 4 * K
        for k, n in enumerate(sizes):                        # model4, model3, model2, model1: 2n, 4n, 6n, 5n images
            assert sorted(seen[4 * k:4 * k + 4]) == [2 * n, 4 * n, 5 * n, 6 * n], (k, seen)
    assert tuple(m.Ft_p[0].shape) == (B, 3, S, S) and m.B1.shape[0] == B


# ------------------------------------------------------------------------------------------------ 2. same step
@pytest.mark.parametrize("criterion", ["cb", "l2"])
@pytest.mark.parametrize("micro", [1, 3])
def test_split_step_is_the_unsplit_step(tmp_path, criterion, micro):
    """Loss within 2e-6, the 14 terms within 5e-6, every parameter gradient within 2e-4 relative, the 14 outputs of the whole batch
    within 2e-5 of the unsplit step on a second model with the same weights and data.

    The l2 loss is a sum, 5909.92 on this batch (largest term 7402.62), where one fp32 ulp is 4.9e-4: the absolute bars lie below the
    spacing of the numbers it is stored in, so only the identical sum meets them.  A step that added up its chunks' fp32 losses (in
    double, rounded once) missed them by 1 - 2 ulps (9.8e-4 and 4.9e-4; terms 4.9e-4); the step therefore evaluates the criterion once
    more, without a graph, over the whole batch's outputs, as the unsplit step does.  Measured on the MI355X since: loss, terms and
    outputs bit-identical for both criteria and both splits; gradients within 5.9e-7 (cb) and 6.1e-7 (l2) relative."""
    ref = _whole(criterion)
    m = _model(tmp_path, criterion=criterion, micro_batch=micro)
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    d_loss = abs(float(m.loss) - float(ref["loss"]))
    d_terms = float((torch.stack(list(m.loss_list)) - ref["loss_list"]).abs().max())
    worst = _worst_rel(_grads(m), ref["grads"])
    d_out = max(float((a - b).abs().max()) for a, b in zip(m.Ft_p, ref["Ft_p"]))
    same_bits = all(torch.equal(a, b) for a, b in zip(m.Ft_p, ref["Ft_p"]))
    print(f"[micro_batch] same step {criterion} micro {micro}: loss {float(m.loss):.9g} whole {float(ref['loss']):.9g} |d| {d_loss:.3g}; "
          f"terms max|d| {d_terms:.3g} (largest term {float(ref['loss_list'].abs().max()):.6g}); gradients worst relative {worst:.3g}; "
          f"outputs max|d| {d_out:.3g}, bit-identical {same_bits}")
    assert len(m.Ft_p) == 14 and all(tuple(t.shape) == (B, 3, S, S) and t.grad_fn is None for t in m.Ft_p)
    assert len(m.loss_list) == 14 and not m.loss.requires_grad
    assert d_out <= 2e-5
    assert worst <= 2e-4
    assert d_loss <= 2e-6
    assert d_terms <= 5e-6


# ------------------------------------------------------------------------------------------------ 3. identity
@pytest.mark.parametrize("micro", [4, 8])
def test_micro_batch_at_or_above_the_batch_is_the_unsplit_step_bit_for_bit(tmp_path, micro):
    ref = _whole("cb", lr=1e-4)
    m = _model(tmp_path, lr=1e-4, micro_batch=micro)
    m.optimize_parameters(1)
    torch.cuda.synchronize()
    assert torch.equal(m.loss.detach(), ref["loss"])
    grads, params = _grads(m), _params(m)
    for k in ref["grads"]:
        assert torch.equal(grads[k], ref["grads"][k]), k
        assert torch.equal(params[k], ref["params"][k]), k


def test_split_step_is_deterministic(tmp_path):
    m = _model(tmp_path, micro_batch=1)
    m.optimize_parameters(1)
    loss, terms, grads, outs = m.loss.clone(), torch.stack(list(m.loss_list)), _grads(m), [t.clone() for t in m.Ft_p]
    m.optimize_parameters(2)
    torch.cuda.synchronize()
    assert torch.equal(m.loss, loss) and torch.equal(torch.stack(list(m.loss_list)), terms)
    again = _grads(m)
    for k in grads:
        assert torch.equal(grads[k], again[k]), k
    assert all(torch.equal(a, b) for a, b in zip(outs, m.Ft_p))


# ------------------------------------------------------------------------------------------------ 4. one optimizer step
@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_one_adam_step_one_ema_move_and_the_whole_batch_norm(tmp_path, optimizer):
    decay = 0.9
    train = {"ema_decay": decay, "grad_clip": 1e9}
    whole = _model(tmp_path, lr=1e-4, optimizer=optimizer, **train)
    split = _model(tmp_path, lr=1e-4, optimizer=optimizer, micro_batch=2, **train)
    start = _params(split)
    shadow0 = [e.clone() for e in split.weight_ema.shadow]   # (the average starts from the weights the model was built with)
    moves = []
    real = split.weight_ema.update
    split.weight_ema.update = lambda: (moves.append(1), real())[1]
    whole.optimize_parameters(1)
    split.optimize_parameters(1)
    torch.cuda.synchronize()
    steps = {float(split.optimizer_G.state[p]["step"]) for p in split.netG.module.parameters()}
    assert steps == {1.0} and len(split.optimizer_G.state) == 540, "Adam's step counter advanced by one"
    after, want = _params(split), _params(whole)
    d_w = max(float((after[k] - want[k]).abs().max()) for k in want)
    moved = max(float((after[k] - start[k]).abs().max()) for k in want)
    n_split, n_whole = split.grad_guard.last.norm, whole.grad_guard.last.norm
    d_e = 0.0                                                # in units of 2 fp32 ulps of the tensor's largest weight (at least of 1.0)
    for p, e, e0 in zip(split.weight_ema.params, split.weight_ema.shadow, shadow0):
        d = float((e - (e0 + (1.0 - decay) * (p.detach() - e0))).abs().max())
        d_e = max(d_e, d / (2.0 ** -22 * max(1.0, float(e0.abs().max()), float(p.detach().abs().max()))))
    print(f"[micro_batch] one step {optimizer}: weights max|split - whole| {d_w:.3g} (moved by {moved:.3g}); gradient norm split "
          f"{n_split:.9g} whole {n_whole:.9g}; EMA max|e - (e0 + (1 - d)(p - e0))| {d_e:.3g} x 2 ulp, update() calls {len(moves)}")
    assert moved > 1e-5, "the step was taken"
    assert d_w <= 2e-5
    assert len(moves) == 1 and d_e <= 1.0, "the average moved once, by one step's difference"
    assert split.grad_guard.last.coef == 1.0 and split.grad_guard.last.flags == 0
    assert abs(n_split - n_whole) <= 1e-4 * n_whole


# ------------------------------------------------------------------------------------------------ 5. skipped as a whole
@pytest.mark.parametrize("optimizer", ["torch", "hip"])
def test_a_nan_in_the_second_chunk_skips_the_whole_step(tmp_path, optimizer):
    """skip_bad_steps: 5, micro_batch: 2.  After one clean step (there is Adam state and a moved average to protect), a NaN in one
    sample of the second chunk's input: nothing is written — weights, Adam moments, step counters and the average are bit for bit
    what they were — although the first chunk's gradients were clean."""
    from bin_amd import ops
    m = _model(tmp_path, lr=1e-4, optimizer=optimizer, micro_batch=2, skip_bad_steps=5, ema_decay=0.9)
    params = list(m.netG.module.parameters())

    def snapshot():
        st = m.optimizer_G.state
        return ([p.detach().clone() for p in params], [st[p][k].clone() for p in params for k in ("exp_avg", "exp_avg_sq")],
                [float(st[p]["step"]) for p in params], [e.clone() for e in m.weight_ema.shadow])
    try:
        m.optimize_parameters(1)
        assert m.grad_guard.last.flags == 0 and m.grad_guard.last.skipped is False
        before = snapshot()
        assert set(before[2]) == {1.0}
        m.B5[2, 1, S // 2, S // 3] = float("nan")            # sample 2 = the first sample of the second chunk
        m.optimize_parameters(2)
        torch.cuda.synchronize()
        last = m.grad_guard.last
        print(f"[micro_batch] skipped step {optimizer}: flags {last.flags} norm {last.norm} skipped {last.skipped} consecutive {last.consecutive}")
        assert last.skipped is True and last.flags != 0 and last.consecutive == 1
        after = snapshot()
        for name, a, b in zip(("weights", "Adam moments", "step counters", "EMA"), before, after):
            if name == "step counters":
                assert a == b, name
            else:
                assert all(torch.equal(x, y) for x, y in zip(a, b)), name
        ops.check_status(m.device)                           # the guard cleared the saturation bit: this does not raise
    finally:
        ops.status_word(m.device).zero_()


# ------------------------------------------------------------------------------------------------ 6. memory
def test_split_step_peaks_below_the_unsplit_step(tmp_path):
    """B = 4 at 128 x 128 on ONE model (the step reads `micro_batch` each time): the peak of torch's allocator over a micro_batch: 1 step
    is strictly below the peak over the unsplit step.  The size of the gap is a measurement (profiles/micro_batch.md)."""
    import ctypes as C
    from bin_amd import _lib as L
    from bin_amd.rdn_plan import c_shape
    m = _model(tmp_path, data=_batch(B, 128, 5))
    peaks = {}
    for name, micro in (("warm split", 1), ("warm whole", None), ("split", 1), ("whole", None), ("split again", 1)):
        m.micro_batch = micro
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        m.optimize_parameters(1)
        torch.cuda.synchronize()
        peaks[name] = (torch.cuda.max_memory_allocated(), base)
    mod = m.netG.module.model.model1_1
    shape = c_shape(mod.kernel_weights(3).shape)
    ws = {n: L.lib().binhip_rdn_workspace_bytes(n, 128, 128, mod.N_INPUTS, 3, C.byref(shape)) for n in (1, 4)}
    print(f"[micro_batch] memory B 4 at 128x128: peak split {peaks['split'][0]} whole {peaks['whole'][0]} split again "
          f"{peaks['split again'][0]} bytes (allocated before the step: {peaks['split'][1]}, {peaks['whole'][1]}, {peaks['split again'][1]}); "
          f"17 x (binhip_rdn_workspace_bytes(N=4) - (N=1)) for the two-input RDN = {17 * (ws[4] - ws[1])}")
    assert peaks["split"][0] < peaks["whole"][0]
    assert peaks["split again"][0] < peaks["whole"][0]


# ------------------------------------------------------------------------------------------------ 7. data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q, tmp):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), BIN_AMD_DIST_BACKEND="gloo")
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from bin_amd.utils import dist_util
        data = _batch()
        m = _model(os.path.join(tmp, str(rank)), data={k: v[2 * rank:2 * rank + 2] for k, v in data.items()}, dist=True, micro_batch=1)
        m.broadcast_parameters()
        sync = m.grad_sync
        assert len(sync._buckets) == 4
        chunk = {"k": -1}
        forward = m.forward

        def counting_forward():
            chunk["k"] += 1
            return forward()
        m.forward = counting_forward
        early, slices = [], []
        reduce_slice, all_reduce = sync._reduce_slice, dist_util.all_reduce

        def spy_slice(start, end, overlap):
            if overlap:
                early.append((chunk["k"], start, end))
            return reduce_slice(start, end, overlap)

        def spy_all_reduce(t, op=None):
            start = (t.data_ptr() - sync.flat.data_ptr()) // 4
            slices.append((start, start + t.numel()))
            return all_reduce(t, op)
        sync._reduce_slice = spy_slice
        dist_util.all_reduce = spy_all_reduce
        m.optimize_parameters(1)
        torch.cuda.synchronize()
        count = np.zeros(sync.numel, dtype=np.int64)
        for a, b in slices:
            assert 0 <= a < b <= sync.numel
            count[a:b] += 1
        q.put((rank, float(m.loss), sync.flat.detach().cpu().numpy().copy(), chunk["k"] + 1, early, int(count.min()), int(count.max()),
               tuple(m.Ft_p[0].shape)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_reduce_every_slice_once_during_the_last_chunk(tmp_path):
    """Two ranks on one GPU over gloo, per-rank B = 2 in chunks of 1: both ranks end with the same gradients, the mean over the four
    samples (within 2e-4 relative of a one-process unsplit step on them); every element of the flat buffer went through exactly one
    all-reduce, and the four early bucket reduces were issued from the second (last) chunk's backward."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted((q.get(timeout=300) for _ in range(2)), key=lambda g: g[0])
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    ref = _whole("cb")
    for rank, loss, flat, chunks, early, cmin, cmax, shape in got:
        print(f"[micro_batch] rank {rank}: {chunks} chunks, early reduces (chunk, start, end) {early}, all-reduces per element {cmin}..{cmax}")
        assert chunks == 2 and shape == (2, 3, S, S)
        assert len(early) == 4 and {k for k, _, _ in early} == {1}, "the early bucket reduces belong to the last chunk"
        assert (cmin, cmax) == (1, 1), "every slice of the flat buffer was all-reduced exactly once"
    assert np.array_equal(got[0][2], got[1][2]), "both ranks hold the same gradients"
    assert abs(0.5 * (got[0][1] + got[1][1]) - float(ref["loss"])) <= 2e-6
    o, worst = 0, 0.0
    for name, g in ref["grads"].items():
        a, b = got[0][2][o:o + g.numel()], g.reshape(-1).cpu().numpy()
        o += g.numel()
        scale = float(np.abs(b).max())
        worst = max(worst, float(np.abs(a - b).max()) / scale if scale > 0 else float(np.abs(a - b).max()))
    assert o == got[0][2].size
    print(f"[micro_batch] two ranks x two chunks vs one unsplit step on the four samples: worst relative gradient difference {worst:.3g}")
    assert worst <= 2e-4


# ------------------------------------------------------------------------------------------------ 8. VideoBaseModel
def test_video_base_model_split_step_is_the_unsplit_step(tmp_path):
    from bin_amd.models.Video_base_model import VideoBaseModel
    from bin_amd.weights import reference_state_dict
    g = torch.Generator().manual_seed(17)
    data = {"LQs": torch.rand(2, 6, 3, S, S, generator=g), "GT": torch.rand(2, 14, 3, S, S, generator=g)}

    def model(**train):
        opt = _opt(tmp_path, **train)
        opt["model"] = "video_base"
        m = VideoBaseModel(opt)
        m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
        m.feed_data(data)
        return m
    whole, split = model(), model(micro_batch=1)
    seen = []
    for mod in split.netG.module.rdn_modules():
        mod.debug_hook = lambda kind, module, dims, ws, info: seen.append(dims[0]) if kind == "backward" else None
    whole.optimize_parameters(1)
    split.optimize_parameters(1)
    torch.cuda.synchronize()
    d_loss = abs(split.get_current_log()["l_pix"] - whole.get_current_log()["l_pix"])
    worst = _worst_rel(_grads(split), _grads(whole))
    d_out = float((split.fake_H - whole.fake_H.detach()).abs().max())
    print(f"[micro_batch] VideoBaseModel cb micro 1: l_pix |d| {d_loss:.3g}, gradients worst relative {worst:.3g}, outputs max|d| {d_out:.3g}, "
          f"RDN backwards on n = {seen}")
    assert sorted(seen) == sorted([2, 4, 5, 6] * 2), "two chunks of one sample"
    assert tuple(split.fake_H.shape) == (2, 14, 3, S, S) and split.fake_H.grad_fn is None and split.var_L.shape[0] == 2
    assert d_out <= 2e-5 and worst <= 2e-4 and d_loss <= 2e-6
