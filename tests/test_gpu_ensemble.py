"""GPU: the self-ensemble (bin_amd/ensemble.py) — binens_orient / binens_merge over the case table of ensemble_cases.py against the
numpy restatement bit for bit (adds in the same tree, a power-of-two scale: nothing to tolerate), both data paths, the guards, the
refusals; SelfEnsemble on the real generator against the composition by hand, batched against streamed, exact equivariance under
every element of the group, the oracle; interpolate_clip, `python -m bin_amd.test --self_ensemble`, `train.val_self_ensemble`.
A NaN is compared as a NaN, not by payload (the device and numpy sign the NaN of inf - inf differently).  CPU side:
test_cpu_ensemble.py."""
import functools
import logging
import os

import numpy as np
import pytest
import torch

import ensemble_cases as EC
from bin_amd import ensemble as E

pytestmark = pytest.mark.gpu

TOL_NET = {"f16x3": 2e-5, "f16": 1e-3}             # the bars tests/test_gpu_net.py holds the plain forward to


def _same(got, want):
    """Bit for bit, NaN for NaN."""
    got, want = np.asarray(got), np.asarray(want)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(EC.bits(got)[~nan], EC.bits(want)[~nan])


class _Arena:
    """One tensor of a case in a guarded device array at an offset of `off` floats from a 16-byte boundary."""

    def __init__(self, x, off, shape=None):
        shape = x.shape if shape is None else shape
        self.host, self.start = EC.arena(x if x is not None else np.zeros(shape, np.float32), off)
        self.buf = torch.from_numpy(self.host).cuda()
        self.n = int(np.prod(shape))
        self.view = self.buf[self.start:self.start + self.n].view(*shape)
        assert self.buf.data_ptr() % 16 == 0 and self.view.data_ptr() % 16 == 4 * off and self.view.is_contiguous()

    def read(self):
        a = self.buf.cpu().numpy()
        return a[self.start:self.start + self.n].reshape(self.view.shape), np.concatenate([a[:self.start], a[self.start + self.n:]])

    def untouched(self):
        return np.array_equal(EC.bits(self.buf.cpu().numpy()), EC.bits(self.host))


@functools.lru_cache(maxsize=None)
def _refs(tag):
    """(sources, merge reference, orient references) of a case: computed once, shared, never written to."""
    case = EC.CASE_BY_TAG.get(tag, EC.FULL_CASE)
    xs = EC.values(case, case.M)
    flips = EC.flips_of(case.M)
    return xs, EC.merge_ref32(xs, flips), EC.orient_ref(xs[0], flips)


def _run_merge(case, offs):
    from bin_amd import ops
    xs, want, _ = _refs(case.tag)
    src = [_Arena(x, offs[o % len(offs)]) for o, x in enumerate(xs)]
    dst = _Arena(None, offs[case.M % len(offs)], case.shape)
    out = ops.ens_merge([[a.view for a in src]], EC.flips_of(case.M), out=[dst.view])
    assert out[0] is dst.view
    torch.cuda.synchronize()
    got, rest = dst.read()
    assert (rest == EC.GUARD).all(), "a guard float around the destination was written"
    assert all(a.untouched() for a in src), "the sources and their guards are only read"
    return got, want


def _run_orient(case, offs):
    from bin_amd import ops
    xs, _, want = _refs(case.tag)
    src = _Arena(xs[0], offs[0])
    dst = [_Arena(None, offs[(1 + j) % len(offs)], case.shape) for j in range(case.M)]
    out = ops.ens_orient([src.view], [[a.view for a in dst]], [EC.flips_of(case.M)])
    assert all(o is a.view for o, a in zip(out[0], dst))
    torch.cuda.synchronize()
    got = []
    for a in dst:
        g, rest = a.read()
        assert (rest == EC.GUARD).all(), "a guard float around a destination was written"
        got.append(g)
    assert src.untouched()
    return got, want


# ------------------------------------------------------------------------------------------------ 1. the kernels over the case table
@pytest.mark.parametrize("tag", EC.TAGS)
def test_merge_case_table_bit_for_bit(tag):
    case = EC.CASE_BY_TAG[tag]
    got, want = _run_merge(case, case.offs)
    assert _same(got, want), tag
    if case.special:
        assert np.isnan(got).any() and np.isinf(got).any(), "inf and NaN propagate"
    r64 = EC.merge_ref64(_refs(tag)[0], EC.flips_of(case.M))
    ok = np.isfinite(r64)
    assert float(np.abs(got[ok] - r64[ok]).max(initial=0.0)) <= 3 * 2.0 ** -24 * 2.0, "and the tree is a mean: three roundings, |x| <= 2"


@pytest.mark.parametrize("tag", EC.TAGS)
def test_orient_case_table_bit_for_bit(tag):
    case = EC.CASE_BY_TAG[tag]
    got, want = _run_orient(case, case.offs)
    for j, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), (tag, j)


@pytest.mark.parametrize("tag", ["3x6x10_M4_aligned", "6x32x48_M8_aligned", "3x4x260_M2_aligned", "6x32x48_M4_inf_nan"])
def test_16_byte_and_4_byte_paths_give_the_same_bits(tag):
    """W % 4 == 0 (or 2, where only the 4 B path exists: the offsets then change nothing): all aligned takes float4s, any buffer off a
    16-byte boundary takes single floats."""
    case = EC.CASE_BY_TAG[tag]
    base_m, base_o = _run_merge(case, (0,))[0], _run_orient(case, (0,))[0]
    for offs in ((1,), (2,), (3,), (0, 0, 1), (0, 3, 0, 0)):
        assert _same(_run_merge(case, offs)[0], base_m), offs
        for g, w in zip(_run_orient(case, offs)[0], base_o):
            assert _same(g, w), offs


def test_full_size_frame_runs_once_both_kernels():
    """[3,768,1344] (a padded 720p frame), M = 8: 3.1e6 elements per tensor, the grid strides."""
    case = EC.FULL_CASE
    got, want = _run_merge(case, (0,))
    assert _same(got, want)
    got, want = _run_orient(case, (0,))
    assert all(_same(g, w) for g, w in zip(got, want))


def test_several_items_in_one_launch_and_fresh_outputs():
    from bin_amd import ops
    case = EC.CASE_BY_TAG["6x32x48_M4_aligned"]
    rng = np.random.Generator(np.random.PCG64(5))
    srcs = [[rng.uniform(-1, 2, size=case.shape).astype(np.float32) for _ in range(4)] for _ in range(14)]
    dev = [[torch.from_numpy(x).cuda() for x in row] for row in srcs]
    # a batch slice as a source: [2N] tensors whose halves are the operands
    big = torch.from_numpy(np.concatenate([srcs[0][0], srcs[0][1]])).cuda()
    dev[0][0], dev[0][1] = big[:6], big[6:]
    out = ops.ens_merge(dev, [0, 1, 2, 3])
    torch.cuda.synchronize()
    ptrs = {t.data_ptr() for row in dev for t in row}
    assert len(out) == 14 and all(o.data_ptr() not in ptrs for o in out)
    for o, row in zip(out, srcs):
        assert _same(o.cpu().numpy(), EC.merge_ref32(row, [0, 1, 2, 3]))
    frames = [torch.from_numpy(srcs[i][0]).cuda() for i in range(6)]
    flipped = ops.ens_orient(frames, None, [[1, 2, 3]] * 6)
    torch.cuda.synchronize()
    for i in range(6):
        for j, f in enumerate((1, 2, 3)):
            assert _same(flipped[i][j].cpu().numpy(), EC.flip_np(srcs[i][0], f))


# ------------------------------------------------------------------------------------------------ 2. refusals
def test_argument_errors_raise_and_launch_nothing():
    from bin_amd import _lib as L, ops
    x = [torch.full((1, 3, 4, 8), float(i), device="cuda") for i in range(16)]
    keep = [t.clone() for t in x]
    with pytest.raises(RuntimeError, match="ens_merge failed: bad argument"):           # M = 3
        ops.ens_merge([x[:3]], [0, 1, 2], out=[x[8]])
    with pytest.raises(RuntimeError, match="ens_merge failed: bad argument"):           # n = 15
        ops.ens_merge([[x[0], x[1]]] * 15, [0, 1], out=[torch.empty_like(x[0]) for _ in range(15)])
    with pytest.raises(RuntimeError, match="ens_merge failed: bad argument"):           # dst is src
        ops.ens_merge([[x[0], x[1]]], [0, 1], out=[x[1]])
    with pytest.raises(RuntimeError, match="ens_orient failed: bad argument"):
        ops.ens_orient([x[0]], [[x[1], x[0]]], [[1, 2]])
    with pytest.raises(RuntimeError, match="ens_orient failed: bad argument"):          # n = 7
        ops.ens_orient(x[:7], [[x[8 + i]] for i in range(7)], [[1]] * 7)
    stream = ops._stream()
    flips = (L.C.c_uint8 * 2)(0, 1)
    item = (L.BinEnsMerge * 1)()
    item[0].src[0], item[0].src[1], item[0].dst = x[0].data_ptr(), None, x[8].data_ptr()          # a null pointer
    with pytest.raises(RuntimeError, match="bad argument"):
        L.check(L.enslib().binens_merge(item, 1, 2, flips, 3, 4, 8, stream), "ens_merge")
    item[0].src[1] = x[1].data_ptr()
    with pytest.raises(RuntimeError, match="bad argument"):                                        # H = 0
        L.check(L.enslib().binens_merge(item, 1, 2, flips, 3, 0, 8, stream), "ens_merge")
    oitem = (L.BinEnsOrient * 1)()
    oitem[0].src, oitem[0].n_dst, oitem[0].dst[0], oitem[0].flip[0] = x[0].data_ptr(), 1, None, 1
    with pytest.raises(RuntimeError, match="bad argument"):
        L.check(L.enslib().binens_orient(oitem, 1, 3, 4, 8, stream), "ens_orient")
    oitem[0].dst[0] = x[9].data_ptr()
    with pytest.raises(RuntimeError, match="bad argument"):
        L.check(L.enslib().binens_orient(oitem, 1, 3, 0, 8, stream), "ens_orient")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(x, keep)), "nothing was launched"


# ------------------------------------------------------------------------------------------------ 3. the real generator
@functools.lru_cache(maxsize=None)
def _net(prec):
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval().set_precision(prec)


@functools.lru_cache(maxsize=None)
def _frames(shape):
    from bin_amd.weights import synthetic_frames
    n, _, h, w = shape
    return tuple(f.cuda() for f in synthetic_frames(1000 + h + w, n, h, w, 6))


@functools.lru_cache(maxsize=None)
def _composed(shape, group, prec="f16x3"):
    """The ensemble by hand (generator, torch.flip, SLOT_REVERSED, the tree): once per (shape, group), shared."""
    with torch.no_grad():
        return tuple(EC.by_hand(_net(prec), list(_frames(shape)), group))


SHAPES_NET = ((1, 3, 32, 48), (2, 3, 32, 32))       # not square: swapped axes show; N = 2: batch-slot indexing shows


@pytest.mark.parametrize("group", ["h", "hv", "ht", "hvt"])
@pytest.mark.parametrize("shape", SHAPES_NET, ids=["1x32x48", "2x32x32"])
def test_self_ensemble_equals_the_composition_by_hand_in_both_strategies(shape, group):
    net, frames, want = _net("f16x3"), list(_frames(shape)), _composed(shape, group)
    got = {s: E.SelfEnsemble(net, group, strategy=s)(frames) for s in ("streamed", "batched")}
    torch.cuda.synchronize()
    from bin_amd import ops
    ops.check_status()
    for s in ("streamed", "batched"):
        worst = max(float((a - b).abs().max()) for a, b in zip(got[s], want))
        print(f"[ensemble] {group} {shape} {s}: max |SelfEnsemble - by hand| = {worst:.3e}")
    for k in range(14):
        assert torch.equal(got["streamed"][k], want[k]), (group, k)
    for k in range(14):
        assert torch.equal(got["batched"][k], got["streamed"][k]), (group, k)
    with torch.no_grad():
        plain = net(*frames)
    assert not any(torch.equal(a, b) for a, b in zip(want, plain)), "the ensemble is not the plain forward"
    assert E.SelfEnsemble(net, group).strategy_for(frames[0]) == "batched", "a 32-pixel frame does not fill the chip"


# ------------------------------------------------------------------------------------------------ 4. exact equivariance
def _act(g, outs):
    """The group element g = (flip, reversed) acting on a 14-list of estimates."""
    flip, rev = g
    res = [None] * 14
    for k in range(14):
        res[E.SLOT_REVERSED[k] if rev else k] = EC.torch_flip(outs[k], flip)
    return res


@pytest.mark.parametrize("strategy", ["streamed", "batched"])
@pytest.mark.parametrize("shape,group", [((1, 3, 32, 48), "hvt"), ((2, 3, 32, 32), "hvt"), ((1, 3, 32, 48), "hv"), ((1, 3, 32, 48), "ht")],
                         ids=["1x32x48_hvt", "2x32x32_hvt", "1x32x48_hv", "1x32x48_ht"])
def test_ensemble_of_an_oriented_input_is_the_oriented_ensemble_bit_for_bit(shape, group, strategy):
    net, frames = _net("f16x3"), list(_frames(shape))
    ens = E.SelfEnsemble(net, group, strategy=strategy)
    base = ens(frames)
    for g in E.orientations(group)[1:]:
        flip, rev = g
        moved = [EC.torch_flip(f, flip).contiguous() for f in (frames[::-1] if rev else frames)]
        got, want = ens(moved), _act(g, base)
        for k in range(14):
            assert torch.equal(got[k], want[k]), (group, g, k)
    # and it is not a property of the plain forward: the generator (initialiser weights) is not equivariant
    flip, rev = E.orientations(group)[-1]
    moved = [EC.torch_flip(f, flip).contiguous() for f in (frames[::-1] if rev else frames)]
    with torch.no_grad():
        assert not any(torch.equal(a, b) for a, b in zip(net(*moved), _act((flip, rev), net(*frames))))


# ------------------------------------------------------------------------------------------------ 5. against the oracle
@functools.lru_cache(maxsize=None)
def _oracle_mean(shape, group):
    """float64 mean over the group of the un-oriented oracle outputs (the orientations ride along N in one oracle forward)."""
    from bin_amd.weights import canonical_weights
    from oracle import rdn_oracle as O
    canon = {k: torch.from_numpy(v) for k, v in canonical_weights(0).items()}
    frames = [f.cpu() for f in _frames(shape)]
    orient = E.orientations(group)
    n = shape[0]
    ins = [torch.cat([EC.torch_flip(frames[5 - j if rev else j], f) for f, rev in orient], 0) for j in range(6)]
    with torch.no_grad():
        outs = O.bin_stage4_forward(ins, canon)
    mean = []
    for k in range(14):
        leaves = [EC.torch_flip(outs[E.SLOT_REVERSED[k] if rev else k][o * n:(o + 1) * n], f).double() for o, (f, rev) in enumerate(orient)]
        mean.append(torch.stack(leaves).mean(0))
    return tuple(mean)


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_hvt_against_the_float64_mean_of_the_oracle(prec):
    """Every leaf is within the plain forward's bar of the oracle's, so their mean is, up to the tree's three roundings and the
    scale's none: bar = TOL_NET[prec] + 4 * 2^-24 * max|out|."""
    shape = (1, 3, 32, 48)
    ref = _oracle_mean(shape, "hvt")
    got = E.SelfEnsemble(_net(prec), "hvt")(list(_frames(shape)))
    from bin_amd import ops
    ops.check_status()
    mag = max(float(r.abs().max()) for r in ref)
    bar = TOL_NET[prec] + 4 * 2.0 ** -24 * mag
    errs = [float((g.cpu().double() - r).abs().max()) for g, r in zip(got, ref)]
    print(f"[ensemble] hvt vs oracle mean, {prec}: max err {max(errs):.3e}, bar {bar:.3e}, max|out| {mag:.3f}")
    assert max(errs) <= bar, (prec, errs)


# ------------------------------------------------------------------------------------------------ 6. the harness
def _u8_clip(T=5, hw=(64, 64), seed=9):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (T,) + hw + (3,), generator=g, dtype=torch.uint8)


def test_interpolate_clip_with_an_ensemble_equals_the_composition_per_window():
    from bin_amd import harness, ops
    from bin_amd.utils import util
    net, clip = _net("f16x3"), _u8_clip()
    T, h, w, _ = clip.shape
    pads = util.pad_sizes(h, w)
    l, r, t, b = pads
    got = harness.interpolate_clip(net, clip, ensemble="hv")
    assert sorted(got) == [0, 1, 2, 3]
    padded = [ops.u8_to_frame(clip[i].cuda(), pads) for i in range(T)]
    for i in range(T - 1):
        ids = harness.window_frame_ids(i, T)
        with torch.no_grad():
            want = EC.by_hand(net, [padded[j] for j in ids], "hv")
        for img, k in zip(got[i], (13, 8, 12)):
            assert img.shape == (h, w, 3) and img.dtype == np.uint8
            assert np.array_equal(img, ops.frame_to_u8(want[k], t, l, h, w).cpu().numpy()), (i, k)
    plain = harness.interpolate_clip(net, clip)
    assert any(not np.array_equal(a, b) for i in got for a, b in zip(got[i], plain[i]))
    for off in (None, "", "none"):
        same = harness.interpolate_clip(net, clip, ensemble=off)
        assert all(np.array_equal(a, b) for i in plain for a, b in zip(same[i], plain[i]))
    for bsz in (2, 8):                                   # windows batched along N under the ensemble: no bit changes
        batched = harness.interpolate_clip(net, clip, batch=bsz, ensemble="hv")
        assert all(np.array_equal(a, b) for i in got for a, b in zip(batched[i], got[i]))
    with pytest.raises(ValueError):
        harness.interpolate_clip(net, clip, ensemble="hq")


def test_streamed_ensemble_reuses_rdn_calls_in_every_orientation(monkeypatch):
    """With the four-call schedule off the harness streams: every orientation keeps its own oriented frames and memo, so after the
    first window every one of the M forwards repeats RDN calls of the window before (forward orientations slide forward, reversed
    ones backward: test_gpu_net.py's streaming test covers both); reuse on and off give the same images, and the batched strategy's.
    (The clip's clamped first and last windows name a frame several times, which the memo also folds: so the counts are bounded,
    not pinned.)"""
    from bin_amd import harness, rdn_plan
    net, clip = _net("f16x3"), _u8_clip(T=7)
    want = harness.interpolate_clip(net, clip, ensemble="hvt")         # the rule's own choice at this size: batched
    calls, per_forward = [], []
    real, real_forward = rdn_plan.rdn_forward, net._forward

    def counting(*a, **k):
        calls.append(1)
        return real(*a, **k)

    def forward(*a, **k):
        before = len(calls)
        out = real_forward(*a, **k)
        per_forward.append(len(calls) - before)
        return out
    monkeypatch.setattr(net, "four_calls_infer", "0")
    monkeypatch.setattr(rdn_plan, "rdn_forward", counting)
    monkeypatch.setattr(net, "_forward", forward)
    M, windows = 8, 6
    runs, counts = {}, {}
    for reuse in (True, False):
        per_forward.clear()
        runs[reuse] = harness.interpolate_clip(net, clip, reuse_stage1=reuse, ensemble="hvt")
        assert len(per_forward) == M * windows
        counts[reuse] = [per_forward[w * M:(w + 1) * M] for w in range(windows)]          # [window][orientation]
    print("[ensemble] RDN calls per window x orientation, reuse:", counts[True], "no reuse:", counts[False])
    assert all(c == 17 for row in counts[False] for c in row)
    for o in range(M):
        assert all(counts[True][w][o] <= 10 for w in range(1, windows)), (o, counts[True])
        assert sum(row[o] for row in counts[True]) < sum(row[o] for row in counts[False])
    for i in want:
        assert all(np.array_equal(a, b) for a, b in zip(runs[True][i], runs[False][i]))
        assert all(np.array_equal(a, b) for a, b in zip(runs[True][i], want[i]))


def test_cli_self_ensemble_writes_what_interpolate_clip_returns(tmp_path):
    from PIL import Image
    from bin_amd import harness
    from bin_amd import test as run_test
    from bin_amd.data import util as du
    from bin_amd.weights import reference_state_dict
    from host_fixtures import OPTION_YML
    rng = np.random.Generator(np.random.PCG64(3))
    root = tmp_path / "data" / "test_blur" / "c0"
    os.makedirs(root)
    for k in range(4):
        Image.fromarray(rng.integers(0, 256, (40, 56, 3), dtype=np.uint8)).save(str(root / f"{8 * k:05d}.png"))
    weights = str(tmp_path / "w.pth")
    torch.save(reference_state_dict(0), weights)
    yml = str(tmp_path / "opt.yml")
    open(yml, "w").write(OPTION_YML.replace("/tmp/bin_amd_runs", str(tmp_path)).replace("~/w/adobe_bin.pth", weights)
                         .replace("name: debug_host", "name: adobe_stage4"))
    names = sorted(os.listdir(root))
    frames = torch.from_numpy(np.stack([du.imread_u8(str(root / f)) for f in names]))
    want = harness.interpolate_clip(_net("f16x3"), frames, ensemble="hvt")
    for tag, extra in (("a", []), ("b", ["--batch", "2"]), ("c", ["--no_reuse", "--metrics", "device"])):
        out = str(tmp_path / f"out_{tag}")
        assert run_test.main(["--input_path", str(root.parent), "--output_path", out, "--opt", yml, "--precision", "f16x3",
                              "--self_ensemble", "hvt"] + extra) == 0
        res = os.path.join(out, "60fps_test_results", "adobe_stage4")
        read = lambda k: du.imread_u8(os.path.join(res, "c0", f"{k:05d}.png"))
        for i in range(3):
            interp, d0, d1 = want[i]
            assert np.array_equal(read(8 * i + 8), interp), (tag, i)
            if i == 0:
                assert np.array_equal(read(4), d0)
            if i < 2:
                assert np.array_equal(read(8 * i + 12), d1), (tag, i)
        log = [f for f in os.listdir(res) if f.endswith(".log")]
        assert "self-ensemble: group hvt, M = 8" in open(os.path.join(res, log[0])).read()


# ------------------------------------------------------------------------------------------------ 7. validation
def _model_opt(tmp, group=None):
    from bin_amd.options import options as option
    train = {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None, "lr_G": 1e-4,
             "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000], "restarts": None,
             "restart_weights": None, "lr_gamma": 0.5, "clear_state": False, "val_save_images": 0}
    if group is not None:
        train["val_self_ensemble"] = group
    return option.dict_to_nonedict({
        "model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
        "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2, "precision": "f16x3"},
        "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp), "val_images": str(tmp)},
        "train": train})


def test_val_self_ensemble_through_the_wrapper_and_validate(tmp_path, caplog):
    from bin_amd import train
    from bin_amd.data import create_dataset
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    ds = create_dataset({"mode": "synthetic_texture", "name": "v", "phase": "val", "LQ_size": [3, 32, 32], "num_windows": 1,
                         "seed": None, "max_speed": None})
    s = ds[0]
    batch = {"LQs": s["LQs"][None], "GTenh": s["GTenh"][None], "GTinp": s["GTinp"][None], "key": [s["key"].replace("/", "_")]}
    frames = [batch["LQs"][:, i].cuda().contiguous() for i in range(6)]
    log = logging.getLogger("test_ensemble")
    results = {}
    for group in (None, "flipx4"):
        m = create_model(_model_opt(tmp_path / str(group), group))
        m.netG.module.load_state_dict(reference_state_dict(0), strict=True)
        inner = m.netG.module
        with torch.no_grad():
            plain = inner.eval()(*frames)
            direct = plain if group is None else E.SelfEnsemble(inner, "hv")(frames)
            by_hand = plain if group is None else EC.by_hand(inner, frames, "hv")
            m.netG.train()
        m.feed_data(batch)
        out = m.test()
        assert len(out) == 14 and m.Ft_p is out and m.netG.training
        for a, b, c in zip(out, direct, by_hand):
            assert torch.equal(a, b) and torch.equal(a, c), group
        with caplog.at_level(logging.INFO, logger="test_ensemble"):
            caplog.clear()
            loss = train.validate(m, [batch], 5, m.opt, log)
        line = next(r.getMessage() for r in caplog.records if "<val" in r.getMessage())
        assert ("ens=hv" in line) == (group is not None), line
        for a, b in zip(m.Ft_p, direct):
            assert torch.equal(a, b)
        results[group] = (loss, [t.clone() for t in out])
    assert results[None][0] != results["flipx4"][0]
    assert not any(torch.equal(a, b) for a, b in zip(results[None][1], results["flipx4"][1]))
