"""CPU: `train.micro_batch` — the option parser, the split of a batch into chunks and their loss weights, the hold state of the
data-parallel reducer over gloo at world size 1, and the step's control flow through both wrappers with a toy generator.
The GPU side (the real generator, memory, two ranks) is tests/test_gpu_micro_batch.py."""
import os
import socket

import pytest
import torch

from bin_amd.options import options as option


def _opt(value):
    return {"train": {"micro_batch": value}}


# ------------------------------------------------------------------------------------------------ the option
def test_option_absent_or_null_is_off():
    assert option.micro_batch({}) is None
    assert option.micro_batch({"train": {}}) is None
    assert option.micro_batch({"train": None}) is None
    assert option.micro_batch(_opt(None)) is None
    assert option.micro_batch(option.dict_to_nonedict({"train": {"lr_G": 1e-4}})) is None


@pytest.mark.parametrize("value", [1, 2, 3, 8, 64, 10 ** 6])
def test_option_accepts_positive_integers(value):
    got = option.micro_batch(_opt(value))
    assert got == value and type(got) is int


@pytest.mark.parametrize("value", [0, -1, -8, 1.0, 2.5, float("nan"), float("inf"), True, False, "2", "", "all", [2], {"m": 2}])
def test_option_refuses_everything_else_and_names_the_value(value):
    with pytest.raises(ValueError) as e:
        option.micro_batch(_opt(value))
    assert str(e.value).startswith("train.micro_batch: ") and repr(value) in str(e.value)


def test_parse_reads_the_option_when_the_file_is_loaded(tmp_path):
    """A bad value stops the run at options.parse, and the three shipped files carry the key as a comment only."""
    import yaml
    shipped = os.path.join(os.path.dirname(option.__file__), "bin_stage4_synthetic.yml")
    for name in ("bin_stage4_adobe240.yml", "bin_stage4_y4m.yml", "bin_stage4_synthetic.yml"):
        text = open(os.path.join(os.path.dirname(option.__file__), name)).read()
        assert "micro_batch" in text and "micro_batch" not in (yaml.safe_load(text)["train"] or {}), name
    good = yaml.safe_load(open(shipped))
    good["path"]["save_path"] = str(tmp_path)
    env = os.environ.get("CUDA_VISIBLE_DEVICES")
    try:
        for value, ok in ((2, True), (0, False), ("2", False)):
            good["train"]["micro_batch"] = value
            path = tmp_path / f"o{value!r}.yml".replace("'", "_")
            path.write_text(yaml.safe_dump(good))
            if ok:
                assert option.micro_batch(option.parse(str(path))) == 2
            else:
                with pytest.raises(ValueError, match="train.micro_batch"):
                    option.parse(str(path))
    finally:
        if env is None:
            os.environ.pop("CUDA_VISIBLE_DEVICES", None)
        else:
            os.environ["CUDA_VISIBLE_DEVICES"] = env


# ------------------------------------------------------------------------------------------------ the split
SPLITS = {(4, 1): [1, 1, 1, 1], (4, 2): [2, 2], (4, 3): [3, 1], (4, 4): [4], (4, 8): [4], (1, 1): [1]}


@pytest.mark.parametrize("batch,m", sorted(SPLITS))
def test_chunks_are_contiguous_cover_the_batch_once_and_sum_to_it(batch, m):
    chunks = option.micro_batches(batch, m)
    assert [n for _, n in chunks] == SPLITS[(batch, m)]
    assert len(chunks) == -(-batch // min(m, batch))
    pos = 0
    for start, n in chunks:
        assert start == pos and n >= 1
        pos += n
    assert pos == batch == sum(n for _, n in chunks)
    covered = [0] * batch
    for start, n in chunks:
        for i in range(start, start + n):
            covered[i] += 1
    assert covered == [1] * batch
    assert all(n == m for _, n in chunks[:-1]) and chunks[-1][1] <= m


def test_no_option_is_one_chunk_and_bad_arguments_raise():
    assert option.micro_batches(8, None) == [(0, 8)]
    assert option.micro_batches(64, 8) == [(8 * k, 8) for k in range(8)]
    for batch, m in ((0, 1), (-2, 1), (4, 0), (4, -1)):
        with pytest.raises(ValueError):
            option.micro_batches(batch, m)


@pytest.mark.parametrize("batch,m", sorted(SPLITS) + [(64, 8), (7, 2), (5, 3)])
def test_loss_weights(batch, m):
    chunks = option.micro_batches(batch, m)
    mean = option.micro_batch_weights(chunks, "mean")
    assert mean == [n / batch for _, n in chunks] and abs(sum(mean) - 1.0) <= 1e-15
    assert option.micro_batch_weights(chunks, "sum") == [1.0] * len(chunks)
    for bad in (None, "none", "batchmean"):
        with pytest.raises(ValueError, match="train.micro_batch"):
            option.micro_batch_weights(chunks, bad)


def test_the_three_criteria_say_how_they_reduce():
    from bin_amd.models import loss
    from bin_amd.models.Video_base_model import _CbPair
    assert loss.CharbonnierLoss.reduction == "mean" and _CbPair().reduction == "mean"
    assert loss.L1SumLoss.reduction == "sum" and loss.L2SumLoss.reduction == "sum"


# ------------------------------------------------------------------------------------------------ the reducer
class _Toy(torch.nn.Module):
    """A watched RDN weight set (its parameters form one bucket) and a layer outside every bucket."""

    def __init__(self):
        super().__init__()
        from bin_amd.models.archs.RDN import RDN_residual_interp_2_input
        self.head = torch.nn.Linear(5, 3)
        self.rdn = RDN_residual_interp_2_input(96, 2, 4, 32)
        self.tail = torch.nn.Linear(3, 2)


@pytest.fixture
def gloo_world1():
    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    old = {k: os.environ.get(k) for k in ("MASTER_ADDR", "MASTER_PORT")}
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        yield dist
    finally:
        dist.destroy_process_group()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _reducer(monkeypatch):
    """(net, reducer, calls, count): every dist_util.all_reduce is recorded, counted per element of the flat buffer, and doubles what
    it reduces on top of the real world-1 collective, so that an element reduced twice (or never) shows in the values too."""
    from bin_amd.models.bin_model import FlatGradAllReduce
    from bin_amd.utils import dist_util
    torch.manual_seed(3)
    net = _Toy()
    sync = FlatGradAllReduce(net.parameters()).watch(net)
    sync.force_collective = True
    assert len(sync._buckets) == 1 and sync._held is False
    calls = []
    count = torch.zeros(sync.numel, dtype=torch.int64)
    real = dist_util.all_reduce

    def counting(t, op=None):
        start = (t.data_ptr() - sync.flat.data_ptr()) // 4
        assert 0 <= start and start + t.numel() <= sync.numel and t.is_contiguous()
        calls.append((start, start + t.numel()))
        count[start:start + t.numel()] += 1
        real(t, op)
        return t.mul_(2.0)
    monkeypatch.setattr(dist_util, "all_reduce", counting)
    return net, sync, calls, count


def _micro_batch(net, seed):
    """One "micro-batch": local gradients added into every .grad, then the watched set signals that its backward is complete."""
    g = torch.Generator().manual_seed(seed)
    local = [torch.randn(p.shape, generator=g) for p in net.parameters()]
    for p, q in zip(net.parameters(), local):
        p.grad.add_(q)
    net.rdn._grads_ready_cb()
    return torch.cat([q.reshape(-1) for q in local])


def test_reducer_held_reduces_nothing_then_every_element_exactly_once(gloo_world1, monkeypatch):
    net, sync, calls, count = _reducer(monkeypatch)
    _, b0, b1 = sync._buckets[0]
    assert 0 < b0 < b1 < sync.numel, "the bucket has parameters on both sides"
    sync.attach()
    total = torch.zeros(sync.numel)
    for k in range(3):                                   # three earlier micro-batches: held
        assert sync.hold(True) is sync
        total += _micro_batch(net, 10 + k)
        assert calls == [] and not count.any(), "no all-reduce while held"
        assert torch.equal(sync.flat, total) or torch.allclose(sync.flat, total, rtol=0, atol=1e-5)
    sync.hold(False)                                     # the last one: its finished bucket goes out early, as in an unsplit step
    total += _micro_batch(net, 13)
    assert calls == [(b0, b1)]
    with pytest.raises(RuntimeError, match="held"):
        sync.hold(True)()
    sync.hold(False)()
    assert sorted(calls) == [(0, b0), (b0, b1), (b1, sync.numel)]
    assert bool((count == 1).all()), "every element of the flat buffer was reduced exactly once"
    # world size 1: nothing is divided; the doubling all-reduce ran once over every element of the plain sum of the four micro-batches
    assert torch.allclose(sync.flat, 2.0 * total, rtol=1e-6, atol=1e-6)
    got = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.equal(got, sync.flat) and sync._views_intact()


def test_reducer_never_held_behaves_as_before_and_attach_releases(gloo_world1, monkeypatch):
    net, sync, calls, count = _reducer(monkeypatch)
    _, b0, b1 = sync._buckets[0]
    sync.attach()
    total = _micro_batch(net, 20)                        # a caller that never touches hold(): reduced at the first signal
    assert calls == [(b0, b1)]
    sync()
    assert bool((count == 1).all()) and torch.allclose(sync.flat, 2.0 * total, rtol=1e-6, atol=1e-6)
    sync.hold(True)
    sync.attach()                                        # a new step starts not held
    assert sync._held is False and float(sync.flat.abs().sum()) == 0.0


# ------------------------------------------------------------------------------------------------ the step, through both wrappers
class _ToyG(torch.nn.Module):
    """Six frames in, 14 frames out; records the batch size of every forward."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.conv = torch.nn.Conv2d(18, 42, 3, padding=1)
        self.seen, self.seen_training = [], []

    def forward(self, *frames):
        self.seen.append(int(frames[0].shape[0]))
        if torch.is_grad_enabled():
            self.seen_training.append(int(frames[0].shape[0]))
        return tuple(torch.tanh(self.conv(torch.cat(frames, 1))).split(3, 1))


class _Mean(torch.nn.Module):
    reduction = "mean"

    def forward(self, x, y):
        return ((x - y) ** 2 + 1e-6).sqrt().mean()


class _Sum(torch.nn.Module):
    reduction = "sum"

    def forward(self, x, y):
        return (x - y).abs().sum()


def _train_opt(tmp, model, **train):
    opt = {"model": model, "gpu_ids": None, "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp)},
           "train": {"pixel_criterion": "cb", "pixel_weight": 0.5, "weight_decay_G": 0, "ft_tsa_only": None,
                     "lr_G": 1e-3, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    opt["train"].update(train)
    return opt


def _data(B, S=8):
    g = torch.Generator().manual_seed(9)
    return {"LQs": torch.rand(B, 6, 3, S, S, generator=g), "GTenh": torch.rand(B, 6, 3, S, S, generator=g),
            "GTinp": torch.rand(B, 5, 3, S, S, generator=g)}


def _bin(tmp, cri, **train):
    from bin_amd.models.bin_model import bin_model
    m = bin_model(_train_opt(tmp, "bin", **train), netG=_ToyG(), cri_pix=cri)
    m.feed_data(_data(4))
    return m


@pytest.mark.parametrize("cri", [_Mean, _Sum])
@pytest.mark.parametrize("micro", [1, 2, 3])
def test_bin_model_step_in_chunks_is_the_whole_step(tmp_path, cri, micro):
    whole, split = _bin(tmp_path, cri()), _bin(tmp_path, cri(), micro_batch=micro)
    assert whole.micro_batch is None and split.micro_batch == micro
    fed = {nm: getattr(split, nm) for nm in split._BATCH_TENSORS}
    whole.optimize_parameters(1)
    split.optimize_parameters(1)
    assert whole.netG.module.seen == [4]
    assert split.netG.module.seen == [n for _, n in option.micro_batches(4, micro)]
    assert all(getattr(split, nm) is t for nm, t in fed.items()), "the fed tensors are back in place"
    whole_loss = float(whole.loss.detach())
    scale = abs(whole_loss)
    assert abs(float(split.loss) - whole_loss) <= 1e-5 * scale
    assert len(split.loss_list) == 14 and not split.loss.requires_grad and not any(t.requires_grad for t in split.loss_list)
    for a, b in zip(split.loss_list, whole.loss_list):
        assert abs(float(a) - float(b.detach())) <= 1e-5 * max(1.0, abs(float(b.detach())))
    assert len(split.Ft_p) == 14
    for a, b in zip(split.Ft_p, whole.Ft_p):
        assert a.shape == b.shape == (4, 3, 8, 8) and a.grad_fn is None and torch.allclose(a, b.detach(), rtol=0, atol=1e-6)
    for (name, p), q in zip(split.netG.module.named_parameters(), whole.netG.module.parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 1e-5 * float(q.grad.abs().max()), name
        assert torch.allclose(p, q, rtol=0, atol=1e-6), name      # ONE Adam step, of the same size
        assert float(split.optimizer_G.state[p]["step"]) == 1.0
    split.train_AverageMeter()
    split.train_AverageMeter_update()
    inst, avg = split.get_current_log("train")
    assert abs(avg["Al"] - whole_loss) <= 1e-5 * scale and len(split.get_current_visuals()["rlt"]) == 14


def test_bin_model_micro_batch_at_or_above_the_batch_is_the_unsplit_path(tmp_path):
    whole = _bin(tmp_path, _Mean())
    whole.optimize_parameters(1)
    for micro in (4, 8):
        m = _bin(tmp_path, _Mean(), micro_batch=micro)
        m.optimize_parameters(1)
        assert m.netG.module.seen == [4] and m.Ft_p[0].grad_fn is not None
        assert torch.equal(m.loss, whole.loss)
        for p, q in zip(m.netG.module.parameters(), whole.netG.module.parameters()):
            assert torch.equal(p.grad, q.grad) and torch.equal(p, q)


def test_bad_option_stops_the_model_being_built_and_a_silent_criterion_stops_the_step(tmp_path):
    from bin_amd.models.bin_model import bin_model
    with pytest.raises(ValueError, match="train.micro_batch: 0"):
        bin_model(_train_opt(tmp_path, "bin", micro_batch=0), netG=_ToyG(), cri_pix=_Mean())

    class Silent(torch.nn.Module):
        def forward(self, x, y):
            return (x - y).abs().mean()
    m = _bin(tmp_path, Silent(), micro_batch=2)
    before = [p.detach().clone() for p in m.netG.module.parameters()]
    with pytest.raises(ValueError, match="reduction"):
        m.optimize_parameters(1)
    assert all(torch.equal(a, p) for a, p in zip(before, m.netG.module.parameters())) and m.B1.shape[0] == 4


class _ToyStacked(torch.nn.Module):
    takes_stacked_frames = True

    def __init__(self):
        super().__init__()
        torch.manual_seed(6)
        self.conv = torch.nn.Conv2d(18, 42, 3, padding=1)
        self.seen = []

    def forward(self, x):
        b, n, c, h, w = x.shape
        self.seen.append(b)
        return torch.tanh(self.conv(x.reshape(b, n * c, h, w))).reshape(b, 14, c, h, w)


@pytest.mark.parametrize("kind", ["cb", "plain_sum"])
def test_video_base_model_step_in_chunks_is_the_whole_step(tmp_path, kind):
    from bin_amd.models.Video_base_model import VideoBaseModel
    g = torch.Generator().manual_seed(11)
    data = {"LQs": torch.rand(3, 6, 3, 8, 8, generator=g), "GT": torch.rand(3, 14, 3, 8, 8, generator=g)}

    def model(**train):
        cri = _Sum() if kind == "plain_sum" else None
        if cri is None:
            # the product's cb pair runs a HIP kernel: its CPU stand-in with the same return shape and the same attribute
            class Pair(_Mean):
                def forward(self, x, y):
                    return super().forward(x, y), None
            cri = Pair()
        m = VideoBaseModel(_train_opt(tmp_path, "video_base", **train), netG=_ToyStacked(), cri_pix=cri)
        m.feed_data(data)
        return m
    whole, split = model(), model(micro_batch=2)
    whole.optimize_parameters(1)
    split.optimize_parameters(1)
    assert whole.netG.module.seen == [3] and split.netG.module.seen == [2, 1]
    assert split.var_L.shape[0] == 3 and split.real_H.shape[0] == 3
    assert split.fake_H.shape == whole.fake_H.shape and split.fake_H.grad_fn is None
    assert torch.allclose(split.fake_H, whole.fake_H.detach(), rtol=0, atol=1e-6)
    a, b = split.get_current_log()["l_pix"], whole.get_current_log()["l_pix"]
    assert abs(a - b) <= 1e-5 * abs(b)
    for p, q in zip(split.netG.module.parameters(), whole.netG.module.parameters()):
        assert float((p.grad - q.grad).abs().max()) <= 1e-5 * float(q.grad.abs().max())
        assert float(split.optimizer_G.state[p]["step"]) == 1.0


# ------------------------------------------------------------------------------------------------ bin_amd.train
def test_train_script_names_the_split_once_and_trains_in_chunks(tmp_path, monkeypatch):
    """The shipped synthetic option file, shrunk, with its commented `#micro_batch:` line switched on: the log names the split once at
    start-up and every training forward sees one sample of the batch of two."""
    from bin_amd import train
    from bin_amd.models.bin_model import bin_model
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    y = open(os.path.join(os.path.dirname(option.__file__), "bin_stage4_synthetic.yml")).read()
    assert y.count("  #micro_batch: 2") == 1
    y = y.replace("  #micro_batch: 2", "  micro_batch: 1")
    y = y.replace("name: synthetic_stage4", "name: debug_synthetic").replace("save_path: ./runs", f"save_path: {tmp_path}")
    y = y.replace("LQ_size: [3, 128, 128]", "LQ_size: [3, 32, 32]").replace("num_windows: 4000", "num_windows: 12")
    y = y.replace("batch_size: 8", "batch_size: 2").replace("n_workers: 3", "n_workers: 0").replace("niter: 2000", "niter: 3")
    y = y.replace("val_freq: 500", "val_freq: 1000")
    path = str(tmp_path / "syn.yml")
    open(path, "w").write(y)
    nets = []

    def factory(opt):
        opt["gpu_ids"] = None
        nets.append(_ToyG())
        return bin_model(opt, netG=nets[0], cri_pix=_Mean())
    assert train.main(["-opt", path], model_factory=factory) == 0
    exp = tmp_path / "experiments" / "debug_synthetic"
    text = open(exp / [f for f in os.listdir(exp) if f.endswith(".log")][0]).read()
    assert text.count("micro_batch 1: 2 forward/backward passes per step") == 1
    assert nets[0].seen_training == [1] * 6, "three steps of two chunks (validation runs its own forwards without a graph)"
