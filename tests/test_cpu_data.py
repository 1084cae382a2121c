"""CPU host-logic tests of the rows SURVEY.md §8f marks "next": data pipeline + sampler (N2), option parsing /
training loop / checkpoints (N4) and the single-tensor wrapper (row a17), against tests/golden/g7_host.json
(generated from the reference by tests/golden/make_golden_host.py)."""
import json
import os
import random
import socket
import sys

import numpy as np
import pytest
import torch

from conftest import REPO
from host_fixtures import OPTION_HOME, OPTION_YML, make_adobe_tree

G7 = json.load(open(os.path.join(REPO, "tests", "golden", "g7_host.json")))


# ------------------------------------------------------------------ sampler
def test_dist_iter_sampler_matches_reference():
    from bin_amd.data.data_sampler import DistIterSampler
    for c in G7["sampler"]:
        n, world, rank, ratio, epoch = c["case"]
        s = DistIterSampler(list(range(n)), world, rank, ratio)
        s.set_epoch(epoch)
        assert len(s) == c["len"]
        assert list(iter(s)) == c["indices"]
    with pytest.raises(RuntimeError):
        DistIterSampler([0, 1])                        # no process group, no explicit rank/world


def test_sampler_ranks_partition_the_epoch():
    from bin_amd.data.data_sampler import DistIterSampler
    parts = []
    for r in range(4):
        s = DistIterSampler(list(range(10)), 4, r, ratio=6)
        s.set_epoch(2)
        parts.append(list(iter(s)))
    flat = sorted(v for p in parts for v in p)
    assert len(flat) == 60 and all(flat.count(v) == 6 for v in range(10))


# ------------------------------------------------------------------ dataset
@pytest.fixture(scope="module")
def adobe(tmp_path_factory):
    return make_adobe_tree(str(tmp_path_factory.mktemp("adobe")))


def test_window_list_matches_reference(adobe):
    from bin_amd.data.BIN_dataset import make_window_list
    kept, rest = make_window_list(adobe, mode="train", shuffle=False)
    assert rest == []
    rel = lambda p: os.path.relpath(p, adobe)
    mine = sorted(([[rel(p) for p in w[0]], [rel(p) for p in w[1]], [rel(p) for p in w[2]], w[3]] for w in kept),
                  key=lambda w: w[3])
    assert mine == G7["windows"]
    # clipA: 9 blurry frames -> 4 windows, the one touching the unlisted last frame is dropped; clipB: 7 -> 2
    assert [w[3] for w in mine] == ["clipA_00016", "clipA_00024", "clipA_00032", "clipB_00000", "clipB_00008"]
    random.seed(3)
    a, b = make_window_list(adobe, mode="train", split=60)
    assert len(a) == 3 and len(b) == 2 and sorted(w[3] for w in a + b) == [w[3] for w in mine]


def test_loader_draws_match_reference(adobe):
    from bin_amd.data.BIN_dataset import make_window_list, load_window, BINDataset
    kept, _ = make_window_list(adobe, mode="train", shuffle=False)
    win = sorted(kept, key=lambda w: w[3])[1]
    for ref in G7["loader"]:
        random.seed(ref["seed"])
        LQs, GTenh, GTinp, key = load_window(win, input_frame_size=(3, 64, 96))
        arrs = [np.stack(x, 0) for x in (LQs, GTenh, GTinp)]
        assert key == ref["key"]
        assert [list(a.shape) for a in arrs] == ref["shapes"]
        for a, s, f, l in zip(arrs, ref["sums"], ref["first"], ref["last"]):
            assert a.dtype == np.float32
            assert float(a.astype(np.float64).sum()) == s                  # same crop, flip and order, bit for bit
            assert a[0, 0, 0, :].astype(float).tolist() == f and a[-1, -1, -1, :].astype(float).tolist() == l
    # the facade keeps the reference's name and argument order
    random.seed(1)
    again = BINDataset.Adobe_BIN_loader(win, (3, 64, 96))
    random.seed(1)
    assert np.array_equal(np.stack(again[0]), np.stack(load_window(win, (3, 64, 96))[0]))


def test_dataset_items_and_loader(adobe):
    from bin_amd.data import create_dataset, create_dataloader
    random.seed(0)
    ds = create_dataset({"mode": "BIN", "name": "train", "dataroot_GT": adobe, "dataroot_LQ": adobe,
                         "LQ_size": [3, 32, 48], "data_type": "img", "phase": "train"})
    assert len(ds) == 5
    item = ds[0]
    assert item["LQs"].shape == (6, 3, 32, 48) and item["GTenh"].shape == (6, 3, 32, 48)
    assert item["GTinp"].shape == (5, 3, 32, 48) and item["LQs"].dtype == torch.float32
    assert 0.0 <= float(item["LQs"].min()) and float(item["LQs"].max()) <= 1.0
    loader = create_dataloader(ds, {"phase": "train", "batch_size": 2, "n_workers": 0}, {"dist": False, "gpu_ids": [0]})
    batches = list(loader)
    assert len(batches) == 2 and batches[0]["LQs"].shape == (2, 6, 3, 32, 48)       # drop_last
    val = create_dataloader(ds, {"phase": "val"}, {"dist": False}, vscode_debug=True)
    assert len(list(val)) == 5
    with pytest.raises(NotImplementedError):
        create_dataset({"mode": "REDS", "name": "x"})


def test_image_io_helpers(tmp_path):
    from bin_amd.data import util as du
    from bin_amd.utils import util
    g = np.random.Generator(np.random.PCG64(0))
    bgr = g.integers(0, 256, (9, 7, 3), dtype=np.uint8)
    p = str(tmp_path / "a.png")
    util.save_img(bgr, p)
    assert np.array_equal(du.imread_u8(p), bgr)                              # BGR in, BGR out, like cv2
    f = du.read_img(p)
    assert f.dtype == np.float32 and np.allclose(f, bgr / 255.0)
    grey = g.integers(0, 256, (5, 4, 1), dtype=np.uint8)
    util.save_img(grey, str(tmp_path / "g.png"))
    assert du.read_img(str(tmp_path / "g.png")).shape == (5, 4, 1)
    seq = du.read_img_seq([p, p])
    assert seq.shape == (2, 3, 9, 7) and torch.allclose(seq[0], torch.from_numpy(bgr[:, :, ::-1].copy()).permute(2, 0, 1) / 255.0)
    assert du.is_image_file("x.PNG") and not du.is_image_file("x.txt")
    paths, sizes = du.get_image_paths("img", str(tmp_path))
    assert [os.path.basename(q) for q in paths] == ["a.png", "g.png"] and sizes is None
    random.seed(4)
    draws = [random.random() < 0.5 for _ in range(3)]
    random.seed(4)
    out = du.augment([bgr], hflip=True, rot=True)[0]
    want = bgr[:, ::-1] if draws[0] else bgr
    want = want[::-1] if draws[1] else want
    want = want.transpose(1, 0, 2) if draws[2] else want
    assert np.array_equal(out, want)


# ------------------------------------------------------------------ options
def _norm(o):
    return json.loads(json.dumps(o))


def test_options_parse_matches_reference(tmp_path, monkeypatch):
    from bin_amd.options import options as option
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    monkeypatch.setenv("HOME", OPTION_HOME)
    yml = tmp_path / "o.yml"
    yml.write_text(OPTION_YML)
    assert _norm(option.parse(str(yml), is_train=True)) == G7["options_train"]
    assert os.environ["CUDA_VISIBLE_DEVICES"] == "0"
    t = option.parse(str(yml), is_train=False)
    assert _norm(t) == G7["options_test"]
    assert option.dict2str(_norm(t)) == G7["dict2str"]
    nd = option.dict_to_nonedict(t)
    assert nd["train"]["T_period"] is None and nd["nope"] is None and nd["train"]["lr_steps"] == [4, 8]
    # one process per GPU: the launcher owns device visibility
    monkeypatch.setenv("WORLD_SIZE", "8")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "3")
    option.parse(str(yml), is_train=True)
    assert os.environ["CUDA_VISIBLE_DEVICES"] == "3"


def test_check_resume():
    from bin_amd.options import options as option
    opt = {"model": "bin", "path": {"resume_state": "/x/5.state", "models": "/m", "pretrain_model_G": "/w.pth"}}
    option.check_resume(opt, 5)
    assert opt["path"]["pretrain_model_G"] == os.path.join("/m", "5_G.pth")
    opt = {"model": "bin", "path": {"resume_state": None, "models": "/m", "pretrain_model_G": "/w.pth"}}
    option.check_resume(opt, 5)
    assert opt["path"]["pretrain_model_G"] == "/w.pth"


# ------------------------------------------------------------------ wrappers on a tiny stand-in generator
class TinyNet(torch.nn.Module):
    """6 frames -> 14 frames, pointwise (1x1 conv of the frame mix): fast on CPU, exact under tiling."""

    def __init__(self):
        super().__init__()
        self.mix = torch.nn.Conv2d(18, 42, 1)
        self.prev_state = self.hidden_state = None

    def forward(self, *frames):
        y = self.mix(torch.cat(frames, 1))
        return tuple(y[:, 3 * i:3 * i + 3] for i in range(14))


class _Cb(torch.nn.Module):
    def forward(self, x, y):
        return torch.sqrt((x - y) ** 2 + 1e-6).mean()


def _vopt(tmp):
    return {"model": "video_base", "gpu_ids": None, "is_train": True, "dist": False,
            "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
            "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp)},
            "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "lr_G": 1e-3, "beta1": 0.9, "beta2": 0.99,
                      "lr_scheme": "MultiStepLR", "lr_steps": [100], "lr_gamma": 0.5}}


def test_video_base_model_surface(tmp_path):
    from bin_amd.models.Video_base_model import VideoBaseModel
    torch.manual_seed(0)
    m = VideoBaseModel(_vopt(tmp_path), netG=TinyNet(), cri_pix=_Cb())
    data = {"LQs": torch.rand(2, 6, 3, 40, 56), "GT": torch.rand(2, 14, 3, 40, 56)}
    m.feed_data(data)
    before = float(m.get_loss()) if hasattr(m, "fake_H") else None
    losses = []
    for step in range(1, 6):
        m.optimize_parameters(step)
        losses.append(m.get_current_log()["l_pix"])
    assert before is None and losses[-1] < losses[0]
    m.test()
    full = m.fake_H.clone()
    assert full.shape == (2, 14, 3, 40, 56)
    m.test_stitch(tile_hw=(16, 32), halo=8)                  # ragged: 40 = 2.5 tiles, 56 = 1.75 tiles
    assert m.fake_H.shape == full.shape and torch.allclose(m.fake_H, full, atol=1e-6)
    vis = m.get_current_visuals(save=True, name="v", save_path=str(tmp_path))
    assert vis["LQ"].shape == (6, 3, 40, 56) and vis["rlt"].shape == (14, 3, 40, 56) and vis["GT"].shape == (14, 3, 40, 56)
    assert (tmp_path / "v.png").exists()
    m.save(7)
    m2 = VideoBaseModel({**_vopt(tmp_path), "path": {**_vopt(tmp_path)["path"],
                                                       "pretrain_model_G": str(tmp_path / "7_G.pth")}},
                        netG=TinyNet(), cri_pix=_Cb())
    for a, b in zip(m.netG.parameters(), m2.netG.parameters()):
        assert torch.equal(a, b)
    from bin_amd.models import _wrappers
    assert _wrappers()["video_base"] is VideoBaseModel


def test_video_base_model_stitch_geometry_matches_the_reference(tmp_path):
    """Row a17's only non-trivial logic, pinned (round 4): fixture g12_stitch is the REFERENCE's VideoBaseModel.test_stitch
    (Video_base_model.py:189-280; imported with the one missing loss name injected, tests/golden/make_golden_stitch.py) on a
    seeded 960x540 two-frame input over the stand-in x4 generator of tests/stitch_cases.py.  bin_amd's stitcher with the
    reference's hard-wired geometry as ARGUMENTS — 320x180 tiles, 32-px halo, scale 4 — makes the same 9 generator calls on the
    same crops and assembles the same [1,3,2160,3840] image, bit for bit (SHA-256 of the whole tensor)."""
    import hashlib
    import stitch_cases as SC
    from conftest import load_golden
    from bin_amd.models.Video_base_model import VideoBaseModel
    g = load_golden("g12_stitch")
    calls = []

    class Recording(SC.StubSR):
        def forward(self, x):
            calls.append(tuple(x.shape))
            return super().forward(x)

    opt = {**_vopt(tmp_path), "is_train": False}
    m = VideoBaseModel(opt, netG=Recording().eval())
    m.feed_data({"LQs": SC.frame()}, need_GT=False)
    with torch.no_grad():
        m.test_stitch(tile_hw=SC.TILE_HW, halo=SC.HALO, scale=SC.SCALE)
    y = m.fake_H
    assert tuple(y.shape) == (1, 3, SC.LR_H * SC.SCALE, SC.LR_W * SC.SCALE)
    assert len(calls) == int(g["n_calls"]) and set(calls) == {tuple(int(v) for v in g["crop_shape"])}
    for k, v in SC.sample(y).items():
        assert np.array_equal(v.numpy(), g[k]), k
    assert hashlib.sha256(y.contiguous().numpy().tobytes()).digest() == bytes(g["sha256"])
    # a different halo or a shifted interior would NOT reproduce it (the stand-in's blur and crop ramp see to that)
    with torch.no_grad():
        m.test_stitch(tile_hw=SC.TILE_HW, halo=SC.HALO // 2, scale=SC.SCALE)
    assert not np.array_equal(SC.sample(m.fake_H)["seam_rows"].numpy(), g["seam_rows"])


# ------------------------------------------------------------------ the training loop (bin_amd.train) on CPU
def _train_yml(tmp, adobe, resume=None, niter=6):
    y = OPTION_YML.replace("~/data/adobe", adobe).replace("/tmp/bin_amd_runs", str(tmp))
    y = y.replace("pretrain_model_G: ~/w/adobe_bin.pth", "pretrain_model_G: ~")
    y = y.replace("mode: BIN_mc", "mode: BIN").replace("/data/val.lmdb", adobe).replace("/data/val", adobe)
    y = y.replace("name: test", "name: train")             # validate on the same tiny tree
    y = y.replace("save_checkpoint_freq: !!float 5000", "save_checkpoint_freq: 3")
    y = y.replace("print_freq: 100", "print_freq: 2").replace("val_freq: !!float 5e3", "val_freq: 4")
    y = y.replace("niter: 6", f"niter: {niter}\n  val_max_batches: 1\n  val_save_images: 1")
    if resume:
        y = y.replace("resume_state: ~", f"resume_state: {resume}")
    p = os.path.join(str(tmp), "train.yml" if not resume else "resume.yml")
    open(p, "w").write(y)
    return p


def _tiny_factory(opt):
    from bin_amd.models.bin_model import bin_model
    torch.manual_seed(11)
    opt["gpu_ids"] = None                                   # BaseModel: no gpu ids -> cpu (reference base_model.py:11)
    return bin_model(opt, netG=TinyNet(), cri_pix=_Cb())


def test_train_loop_checkpoints_and_resume(tmp_path, adobe, monkeypatch):
    from bin_amd import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    assert train.main(["-opt", _train_yml(tmp_path, adobe)], model_factory=_tiny_factory) == 0
    exp = tmp_path / "experiments" / "debug_host"          # 'debug' in the name: freqs forced to 1 by parse()
    models = sorted(os.listdir(exp / "models"))
    assert "latest_G.pth" in models and "6_G.pth" in models and "3_G.pth" in models
    assert (exp / "training_state" / "3.state").exists()
    logs = [f for f in os.listdir(exp) if f.endswith(".log")]
    text = open(exp / logs[0]).read()
    assert "<epoch:" in text and "<val iter:" in text and "End of training." in text
    assert any(f.startswith("rlt_") for f in os.listdir(exp / "val_images" / "1"))
    # resume from iteration 3: continues at 4, ends at 6, the LR follows MultiStepLR([4, 8]) from the restored state
    state = torch.load(exp / "training_state" / "3.state", weights_only=False)
    assert state["iter"] == 3
    assert train.main(["-opt", _train_yml(tmp_path, adobe, resume=str(exp / "training_state" / "3.state"))],
                      model_factory=_tiny_factory) == 0
    logs2 = sorted(f for f in os.listdir(exp) if f.endswith(".log"))
    text2 = "".join(open(exp / f).read() for f in logs2)
    assert "Resuming training from epoch" in text2 and "iter:       4" in text2.replace("iter:       4,", "iter:       4")
    final = torch.load(exp / "models" / "6_G.pth", weights_only=False)
    assert set(final) == set(TinyNet().state_dict())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dist_worker(rank, world, port, yml, q):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    import test_cpu_data as T
    from bin_amd import train
    captured = {}

    def factory(opt):
        captured["m"] = T._tiny_factory(opt)
        return captured["m"]

    probe = {}
    rc = train.main(["-opt", yml, "--launcher", "pytorch", "--max_iter", "3"], model_factory=factory, probe=probe)
    q.put((rank, rc, [p.detach().double().sum().item() for p in captured["m"].netG.parameters()], probe))
    torch.distributed.destroy_process_group()


def test_train_loop_world2_gloo(tmp_path, adobe):
    import torch.multiprocessing as mp
    yml = _train_yml(tmp_path, adobe)
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dist_worker, args=(r, 2, port, yml, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert got[0][1] == 0 and got[1][1] == 0
    assert got[0][2] == got[1][2]                            # ranks hold identical parameters after 3 DP steps
    # the ranks seed differently for augmentation (seed + rank) but must build the SAME shuffled window list, or the
    # sampler's disjoint index shares would overlap / skip windows: union of the shares == ratio x dataset
    pa, pb = got[0][3], got[1][3]
    assert pa["windows"] == pb["windows"] and len(pa["windows"]) > 0
    n, ratio = len(pa["windows"]), pa["ratio"]
    union = sorted(pa["share"] + pb["share"])
    want = sorted(list(range(n)) * ratio)
    assert len(union) >= len(want) and len(union) - len(want) < 2           # rounded up to a multiple of the world size
    from collections import Counter
    cu, cw = Counter(union), Counter(want)
    assert all(cu[i] >= cw[i] for i in range(n)) and sum((cu - cw).values()) == len(union) - len(want)


def test_train_loop_reduce_lr_on_plateau(tmp_path, adobe, monkeypatch):
    """The reference's own option file uses lr_scheme: ReduceLROnPlateau (factor 0.2, patience 1): the loop must step
    that scheduler with the validation loss (and never through update_learning_rate, which has no metric)."""
    from bin_amd import train
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    yml = _train_yml(tmp_path, adobe, niter=6)
    y = open(yml).read().replace("lr_scheme: MultiStepLR", "lr_scheme: ReduceLROnPlateau\n  factor: 0.2\n  patience: 0")
    open(yml, "w").write(y)
    captured = {}

    def factory(opt):
        captured["m"] = _tiny_factory(opt)
        # a criterion that grows every call: the validation loss never improves -> the plateau scheduler must fire
        captured["m"].cri_pix = _Growing()
        return captured["m"]

    assert train.main(["-opt", yml], model_factory=factory) == 0
    lr = captured["m"].get_current_learning_rate()[0]
    assert lr < 1e-4 * 0.21                              # reduced at least once from lr_G = 1e-4


class _Growing(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.k = 0

    def forward(self, x, y):
        self.k += 1
        return torch.sqrt((x - y) ** 2 + 1e-6).mean() * (1.0 + 0.5 * self.k)


def test_folder_runner_window_and_file_naming(tmp_path):
    """bin_amd.test host logic (reference test.py:236-312): clips in sorted order, one window per frame but the last;
    window `index` of a clip whose frame file is <num>.png writes <num+8> (interpolated), <num+4> and — except for the
    clip's last window — <num+12> (deblurred); the six input frames are index + [-2..3] clamped to the clip."""
    from bin_amd import harness
    from bin_amd import test as run_test
    for clip, first, n in (("b_clip", 40, 4), ("a_clip", 0, 3)):
        d = tmp_path / clip
        d.mkdir()
        for k in range(n):
            (d / f"{first + 8 * k:05d}.png").write_bytes(b"")
        (d / "notes.txt").write_text("not a frame")
    wins = run_test.list_windows(str(tmp_path))
    assert [(c, i) for c, _, i in wins] == [("a_clip", 0), ("a_clip", 1), ("b_clip", 0), ("b_clip", 1), ("b_clip", 2)]
    frames_b = wins[2][1]
    assert frames_b == ["00040.png", "00048.png", "00056.png", "00064.png"]
    assert run_test.output_names(frames_b, 0) == ("00048.png", "00044.png", "00052.png")
    assert run_test.output_names(frames_b, 1) == ("00056.png", "00052.png", "00060.png")
    assert run_test.output_names(frames_b, 2) == ("00064.png", "00060.png", None)          # last window: no second deblur
    assert harness.window_frame_ids(0, 4) == [0, 0, 0, 1, 2, 3]
    assert harness.window_frame_ids(2, 4) == [0, 1, 2, 3, 3, 3]
    assert harness.window_frame_ids(5, 12) == [3, 4, 5, 6, 7, 8]
    args = run_test.parse_args(["--input_path", "i", "--output_path", "o", "--opt", "x.yml", "--batch", "4"])
    assert args.batch == 4 and args.gt_path is None and args.time_step == 0.5 and args.launcher == "none"


@pytest.mark.parametrize("case", ["cb_pair", "cb_pair_ft", "cb_plain_noschedule", "l1_plain_noschedule_ft", "l2_plain_noschedule"])
def test_video_base_model_training_step_matches_the_reference(tmp_path, case):
    """Row a17's training step, pinned (round 5): fixture g13_videobase_step is the REFERENCE's VideoBaseModel run whole —
    `__init__` (criterion, Adam groups incl. `ft_tsa_only`, scheduler), `feed_data`, `optimize_parameters` :134-158 /
    `optimize_parameters_without_schudlue` :161-181, `update_learning_rate`, `get_current_log`, `test` — over the single-tensor
    stand-in generator of tests/videobase_cases.py (tests/golden/make_golden_videobase_step.py: the one missing loss name
    injected, `define_G` pointed at the stub).  bin_amd's class over the same generator, options and batch reproduces every
    step's logged loss, the rates each step ran with, every parameter after every step, and `test()`'s output."""
    import videobase_cases as VC
    from conftest import load_golden
    from bin_amd.models.Video_base_model import VideoBaseModel
    g = load_golden("g13_videobase_step")
    ft, crit, method, pair = VC.CASES[case]
    # (the product's criteria are HIP kernels and refuse CPU tensors: here the criterion is the plain-torch statement of the
    #  same formula, so this test pins the wrapper's own logic; tests/test_gpu_train.py runs the same fixture on the device
    #  with the product's criteria)
    cri = {"cb": _Cb(), "l1": torch.nn.L1Loss(reduction="sum"), "l2": torch.nn.MSELoss(reduction="sum")}[crit]
    m = VideoBaseModel(VC.opt(tmp_path, ft, crit), netG=VC.StubVSR(), cri_pix=VC.PairCriterion(cri) if pair else cri)
    assert [len(grp["params"]) for grp in m.optimizer_G.param_groups] == g[f"{case}/groups"].tolist()
    data = VC.batch()
    for step in range(1, VC.STEPS + 1):
        m.feed_data(data)
        getattr(m, method)(step)
        assert [grp["lr"] for grp in m.optimizer_G.param_groups] == pytest.approx(g[f"{case}/s{step}/lr_used"].tolist(), rel=1e-12, abs=0)
        m.update_learning_rate(step, warmup_iter=-1)
        log = m.get_current_log()
        assert list(log) == ["l_pix"]
        assert log["l_pix"] == pytest.approx(float(g[f"{case}/s{step}/l_pix"]), rel=2e-6)
        assert m.get_current_learning_rate() == pytest.approx(g[f"{case}/s{step}/lr_next"].tolist(), rel=1e-12, abs=0)
        for n, p in m.netG.module.named_parameters():
            want = g[f"{case}/s{step}/{n}"]
            assert np.abs(p.detach().numpy() - want).max() <= 2e-6 * max(1.0, np.abs(want).max()), (step, n)
    m.feed_data(data, need_GT=False)
    m.test()
    assert m.netG.training
    assert float(m.fake_H.double().mean()) == pytest.approx(float(g[f"{case}/test_mean"]), abs=1e-6)
    if f"{case}/test" in g.files:
        assert np.abs(m.fake_H.numpy() - g[f"{case}/test"]).max() <= 1e-5


def test_striped_png_writer_decodes_to_the_same_pixels(tmp_path):
    """util.png_bytes_striped (the folder runner's PNG writer since round 5: DEFLATE in independent bands stitched into one zlib
    stream, 'Up' row filter): a standard PNG — Pillow decodes it to exactly the pixels handed in, for any band count, with and
    without a pool, on ragged sizes; and `imread_u8` reads the written file back."""
    import io
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    from bin_amd.data import util as data_util
    from bin_amd.utils import util
    g = np.random.Generator(np.random.PCG64(5))
    pool = ThreadPoolExecutor(3)
    for shape in ((1, 1, 3), (5, 7, 3), (64, 96, 3), (33, 130, 3)):
        img = g.integers(0, 256, shape, dtype=np.uint8)
        smooth = (np.add.outer(np.arange(shape[0]), np.arange(shape[1]))[:, :, None] * np.array([1, 2, 3]) % 256).astype(np.uint8)
        for a in (img, smooth):
            for strips, p in ((1, None), (4, None), (4, pool), (1000, pool)):
                b = util.png_bytes_striped(a, p, strips)
                back = np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))[:, :, ::-1]
                assert np.array_equal(back, a), (shape, strips)
    path = str(tmp_path / "x.png")
    util.save_png_striped(img, path, pool, 4)
    assert np.array_equal(data_util.imread_u8(path), img)
    with pytest.raises(ValueError):
        util.png_bytes_striped(np.zeros((4, 4), dtype=np.uint8))
    pool.shutdown()


def test_synthetic_moving_texture_clips_have_the_dataset_structure():
    """bin_amd.data.synthetic: the dict feed_data takes (BIN_dataset.py:170-183 shapes), deterministic in (seed, index), values in
    [0, 1], a blurry frame = the exposure mean of its sharp neighbourhood (smoother than, and close to, the sharp frame at its instant),
    and the in-between sharp frame lies between its neighbours in time (uniform motion)."""
    import torch
    from bin_amd.data.synthetic import moving_texture_batch, moving_texture_clip
    d = moving_texture_batch(3, 10, 2, 48)
    assert d["LQs"].shape == (2, 6, 3, 48, 48) and d["GTenh"].shape == (2, 6, 3, 48, 48) and d["GTinp"].shape == (2, 5, 3, 48, 48)
    assert all(v.dtype == torch.float32 and 0.0 <= float(v.min()) and float(v.max()) <= 1.0 for v in d.values())
    again = moving_texture_clip(3, 11, 48)
    assert torch.equal(again[0], d["LQs"][1]) and torch.equal(again[2], d["GTinp"][1])
    assert not torch.equal(d["LQs"][0], d["LQs"][1])

    def roughness(x):
        return float((x[..., 1:, :] - x[..., :-1, :]).abs().mean() + (x[..., :, 1:] - x[..., :, :-1]).abs().mean())
    lq, enh, inp = moving_texture_clip(3, 10, 48, max_speed=3.0)
    assert roughness(lq) < roughness(enh)                                   # motion blur removes detail
    assert float((lq - enh).abs().mean()) < 0.5 * float((enh[0] - enh[5]).abs().mean())      # ... but stays at its instant
    mid = 0.5 * (enh[2] + enh[3])
    assert float((inp[2] - mid).abs().mean()) < float((inp[2] - enh[2]).abs().mean())       # I6 is nearer the mean of I5, I7 than I5


def test_train_script_on_the_synthetic_dataset_option_file(tmp_path, monkeypatch):
    """`mode: synthetic_texture` (bin_amd extension): the shipped options/bin_stage4_synthetic.yml — shrunk to a few tiny windows — goes
    through option parsing, create_dataset / create_dataloader, the training loop, validation and checkpointing with nothing on disk."""
    from bin_amd import train
    from bin_amd.data import create_dataset
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "")
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    y = open(os.path.join(here, "bin_amd", "options", "bin_stage4_synthetic.yml")).read()
    y = y.replace("name: synthetic_stage4", "name: debug_synthetic").replace("save_path: ./runs", f"save_path: {tmp_path}")
    y = y.replace("LQ_size: [3, 128, 128]", "LQ_size: [3, 32, 32]").replace("num_windows: 4000", "num_windows: 12")
    y = y.replace("batch_size: 8", "batch_size: 2").replace("n_workers: 3", "n_workers: 0").replace("niter: 2000", "niter: 4")
    y = y.replace("val_freq: 500", "val_freq: 2\n  val_max_batches: 2")
    p = str(tmp_path / "syn.yml")
    open(p, "w").write(y)
    assert train.main(["-opt", p], model_factory=_tiny_factory) == 0
    exp = tmp_path / "experiments" / "debug_synthetic"
    assert (exp / "models" / "latest_G.pth").exists()
    text = open(exp / [f for f in os.listdir(exp) if f.endswith(".log")][0]).read()
    assert "SyntheticTextureDataset" in text and "<val iter:" in text and "End of training." in text
    ds = create_dataset({"mode": "synthetic_texture", "name": "v", "phase": "val", "LQ_size": [3, 32, 32], "num_windows": 3, "seed": None, "max_speed": None})
    tr = create_dataset({"mode": "synthetic_texture", "name": "t", "phase": "train", "LQ_size": [3, 32, 32], "num_windows": 3, "seed": None, "max_speed": None})
    assert len(ds) == 3 and ds[1]["key"] == "synthetic/000001" and ds[1]["LQs"].shape == (6, 3, 32, 32)
    assert not torch.equal(ds[0]["LQs"], tr[0]["LQs"])                          # validation draws from its own stream
    with pytest.raises(ValueError):
        create_dataset({"mode": "synthetic_texture", "name": "x", "phase": "train", "LQ_size": [3, 32, 48], "num_windows": 3, "seed": None, "max_speed": None})
