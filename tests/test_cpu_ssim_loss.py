"""CPU: the criterion `pixel_criterion: cb+ssim` without a device — the closed-form gradient of include/binssim.h against float64
autograd over the case table (ssim_loss_cases.py), the bookkeeping of libbinssim.so and of the third, open-ended library table,
every refusal of its entry points (they come before any HIP call, so made-up addresses are never followed), the option
`train.ssim_weight`, both wrappers' control flow with a toy generator and a CPU stand-in of the criterion, and which branch
multi_term_loss takes."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import ssim_loss_cases as SC
from conftest import REPO

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]
NAME = "binssim"
WANT = ["binssim_version", "binssim_workspace_bytes", "binssim_forward", "binssim_backward"]


# ------------------------------------------------------------------------------------------------ 1. the closed form
@pytest.mark.parametrize("case", SC.CASES, ids=SC.case_id)
def test_closed_form_equals_autograd_in_float64(case):
    worst = 0.0
    for (kind, x, y, g, need), (s, gx, gy) in zip(SC.case_terms(case[0]), SC.case_reference(case[0])):
        s2, gx2, gy2 = SC.closed_form(x, y)
        d = max(abs(float(s - s2)), float((gx / g - gx2).abs().max()), float((gy / g - gy2).abs().max()))
        worst = max(worst, d)
        assert d <= 1e-13, (kind, d)
        assert gx2.shape == x.shape and gy2.dtype == torch.float64
    print(f"[ssim_loss] closed form {SC.case_id(case)}: max|closed - autograd| {worst:.3g}")


def test_table_covers_the_tile_edges_every_kind_and_every_gradient_request():
    hs, ws = {c[1] for c in SC.CASES}, {c[2] for c in SC.CASES}
    assert set(SC.HS) <= hs and set(SC.WS) <= ws
    assert SC.HS == (11, 12, SC.TH - 1, SC.TH, SC.TH + 1, SC.TH + 10, SC.TH + 11, 2 * SC.TH + 5)
    assert SC.WS == (11, 12, SC.TW - 1, SC.TW, SC.TW + 1, SC.TW + 10, SC.TW + 11, 2 * SC.TW + 5)
    assert {c[3] for c in SC.CASES} == {1, 3, 7} and {c[4] for c in SC.CASES} == {1, 2, 17, 24}
    assert any(c[2] - 10 > SC.FW for c in SC.CASES) and any(c[1] - 10 > SC.FH for c in SC.CASES), "more than one forward tile"
    seen = {(SC.term_kind(c, t), SC.term_need(t)) for c in SC.CASES for t in range(c[4])}
    assert seen == {(k, n) for k in SC.KINDS for n in SC.NEEDS}
    x, y = SC.content("smooth", (3, 69, 69), 1)
    assert 0.98 <= float(SC.ssim_ref(x, y)) <= 0.999
    x, y = SC.content("flat", (1, 33, 33), 2)
    assert float((x - 0.5).abs().max()) <= 1e-3 + 1e-7
    x, y = SC.content("equal", (1, 12, 12), 3)
    assert torch.equal(x, y) and float(SC.ssim_ref(x, y)) == 1.0


# ------------------------------------------------------------------------------------------------ 2. the library's bookkeeping
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_header_binding_and_dynamic_symbols_agree():
    from bin_amd import _lib, build
    assert NAME in [row.name for row in build.ADDON_LIBRARIES] and NAME in _lib._ADDON_LIBRARIES
    assert list(build.ADDON_BY_NAME) == [row.name for row in build.ADDON_LIBRARIES] == list(_lib._ADDON_LIBRARIES)
    assert NAME not in build.BY_NAME and NAME not in build.EXTRA_BY_NAME and NAME not in _lib._LIBRARIES and NAME not in _lib._EXTRA_LIBRARIES
    assert len(build.LIBRARIES) == 11 and [row.name for row in build.EXTRA_LIBRARIES] == ["binexpose"]
    lib = build.ADDON_BY_NAME[NAME]
    assert build.row(NAME) is lib and build.row("binexpose") is build.EXTRA_BY_NAME["binexpose"] and build.row("binhip") is build.LIBRARIES[0]
    hdr = open(lib.header).read()
    declared = build.abi_symbols(NAME)
    assert lib.sources == ["binssim.hip"] and lib.subdir == "extra" and lib.purpose and "\n" not in lib.purpose
    assert lib.path == os.path.join(build.CSRC, "extra", "libbinssim.so") and lib.header == os.path.join(REPO, "include", "binssim.h")
    assert declared == WANT
    assert set(_lib.exported_symbols(NAME)) == set(declared) == _defined(lib.path)
    assert set(re.findall(rf"\b({NAME}_[a-z0-9_]+)\s*\(", hdr)) == set(declared)
    assert all(m.startswith("BINSSIM_") for m in re.findall(r"#\s*define\s+(\w+)", hdr))
    assert "#pragma once" in hdr
    assert re.findall(r'(?m)^\s*#\s*include\s+"(\w+\.h)"', hdr) == [], "no other project header"
    assert re.findall(r"(?m)^\s*#\s*(?:if|ifdef|ifndef|elif)\b\s*(.*)$", hdr) == ["__cplusplus", "__cplusplus"]
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", hdr).group(1))
    assert _lib.library(NAME).binssim_version() == macro("BINSSIM_VERSION") == _lib._ADDON_LIBRARIES[NAME][1] == _lib.SSIM_VERSION == 100
    assert (macro("BINSSIM_E_ARG"), macro("BINSSIM_E_SHAPE"), macro("BINSSIM_E_WORKSPACE")) == \
        (_lib.SSIM_E_ARG, _lib.SSIM_E_SHAPE, _lib.SSIM_E_WORKSPACE) == (-1, -2, -3)
    assert macro("BINSSIM_MAX_TERMS") == _lib.SSIM_MAX_TERMS == 24
    assert (macro("BINSSIM_FWD_TILE_H"), macro("BINSSIM_FWD_TILE_W")) == _lib.SSIM_FWD_TILE
    assert (macro("BINSSIM_BWD_TILE_H"), macro("BINSSIM_BWD_TILE_W")) == _lib.SSIM_BWD_TILE
    assert C.sizeof(_lib.BinSsimTerms) == 4 * 24 * 8 + 8
    assert _lib.ssimlib() is _lib.library(NAME)
    assert "binssim.hip" not in os.listdir(build.CSRC) and os.path.exists(os.path.join(build.CSRC, "extra", "binssim.hip"))
    built = ["bin_amd/csrc/extra/libbinssim.so", "bin_amd/csrc/extra/binhip_exports.binssim.map", "bin_amd/csrc/extra/binssim.o"]
    ignored = subprocess.run(["git", "check-ignore"] + built, cwd=REPO, capture_output=True, text=True)
    if ignored.returncode != 128:                                 # (128: not a git checkout)
        assert len(ignored.stdout.split()) == len(built), "the built files stay out of git"


def test_version_gate_and_a_missing_library(monkeypatch, tmp_path):
    from bin_amd import _lib, build
    monkeypatch.setattr(_lib, "_loaded", {})
    assert _lib.library(NAME) is _lib.library(NAME), "loaded once"
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setitem(_lib._ADDON_LIBRARIES, NAME, (_lib._SSIM_SIGNATURES, 101))
    with pytest.raises(RuntimeError, match=r"libbinssim\.so is version 100, this binding is for 101"):
        _lib.library(NAME)
    monkeypatch.setitem(_lib._ADDON_LIBRARIES, NAME, (_lib._SSIM_SIGNATURES, 100))
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setattr(build, "CSRC", str(tmp_path))
    with pytest.raises(RuntimeError, match=r"HIP library \S*libbinssim\.so not built.*no CPU fallback"):
        _lib.library(NAME)


def test_plans_core_links_eleven_extra_is_one_row_and_the_addon_plan_has_the_core_flags():
    from bin_amd import build
    compiles, links = build.build_plan()
    assert len(links) == 11 and not any(NAME in " ".join(c) for c in compiles + [l[2] for l in links])
    assert len(build.build_plan(table=build.EXTRA_LIBRARIES)[1]) == 1
    compiles, links = build.build_plan(table=build.ADDON_LIBRARIES)
    extra = os.path.join(build.CSRC, "extra")
    at = [row.name for row in build.ADDON_LIBRARIES].index(NAME)
    cmd, (vmap, names, link) = compiles[at], links[at]
    hipcc = build.build_plan()[0][0][0]
    assert cmd == [hipcc] + FLAGS + ["-c", os.path.join(extra, "binssim.hip"), "-o", os.path.join(extra, "binssim.o")]
    assert vmap == os.path.join(extra, "binhip_exports.binssim.map") and names == build.abi_symbols(NAME) == WANT
    assert link == [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}", "-o",
                    os.path.join(extra, "libbinssim.so"), os.path.join(extra, "binssim.o")]
    core = build.build_plan()
    assert cmd[1:6] == core[0][0][1:6] == FLAGS and link[1:5] == core[1][1][2][1:5], "the same flags as the core rows"


def test_build_library_without_a_table_builds_all_three(monkeypatch):
    from bin_amd import build
    ran = []

    class P:
        def __init__(self, cmd):
            ran.append(cmd)

        def wait(self):
            return 0
    monkeypatch.setattr(build.subprocess, "Popen", P)
    monkeypatch.setattr(build.subprocess, "check_call", lambda cmd: ran.append(cmd))
    written = []
    real_open = open

    def fake_open(path, mode="r", *a, **k):
        if "w" in mode:
            written.append(path)
            return real_open(os.devnull, mode)
        return real_open(path, mode, *a, **k)
    monkeypatch.setattr("builtins.open", fake_open)
    build.build_library(force=True, verbose=False)
    outs = [cmd[cmd.index("-o") + 1] for cmd in ran if "-shared" in cmd]
    assert outs == [row.path for row in build.LIBRARIES + build.EXTRA_LIBRARIES + build.ADDON_LIBRARIES]
    assert len(written) == len(outs)


def test_a_build_is_stale_when_the_library_is_missing_or_older_than_its_source_or_header(monkeypatch):
    from bin_amd import build
    lib = build.ADDON_BY_NAME[NAME]
    times, missing = {}, set()
    monkeypatch.setattr(os.path, "getmtime", lambda p: times.get(p, 100.0))
    monkeypatch.setattr(os.path, "exists", lambda p: p not in missing)
    fresh = {row.path: 200.0 for row in build.LIBRARIES + build.EXTRA_LIBRARIES + build.ADDON_LIBRARIES}
    times.update(fresh)
    assert build._stale() is False
    for newer in (os.path.join(build.CSRC, "extra", "binssim.hip"), lib.header):
        times.update(fresh)
        times.update({lib.path: 150.0, newer: 160.0})
        assert build._stale() is True, newer
        times[newer] = 100.0
        assert build._stale() is False
    missing.add(lib.path)
    assert build._stale() is True


def test_driver_loads_the_addon_table_and_checks_its_symbols(monkeypatch):
    import inspect
    import __graft_entry__ as entry
    from bin_amd import _lib, build
    assert NAME not in entry.load_libraries() and NAME not in entry.load_libraries(build.EXTRA_LIBRARIES)
    loaded = entry.load_libraries(build.ADDON_LIBRARIES)
    assert NAME in loaded and loaded[NAME] is _lib.library(NAME)
    assert "load_libraries(ADDON_LIBRARIES)" in inspect.getsource(entry.build)
    real = _lib.exported_symbols
    monkeypatch.setattr(_lib, "exported_symbols", lambda n="binhip": real(n) + (["binssim_absent"] if n == NAME else []))
    with pytest.raises(RuntimeError, match=r"libbinssim\.so is missing symbols: \['binssim_absent'\]"):
        entry.load_libraries(build.ADDON_LIBRARIES)


# ------------------------------------------------------------------------------------------------ 3. refusals
X, Y, GX, GY, WS, OUT, G = 0x100000, 0x200000, 0x300000, 0x400000, 0x8000000, 0x700000, 0x600000
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3


def _terms(n=2, **fields):
    """n terms with made-up, well separated addresses (1 MiB apart per kind, 16 KiB apart per term: a 3 x 24 x 40 fp32 stack is
    11 520 bytes); `fields`: name -> {term: address}."""
    from bin_amd import _lib
    t = _lib.BinSsimTerms()
    t.n_terms = n
    for i in range(min(max(n, 0), 24)):
        t.x[i], t.y[i], t.gx[i], t.gy[i] = X + 0x4000 * i, Y + 0x4000 * i, GX + 0x4000 * i, GY + 0x4000 * i
    for name, changes in fields.items():
        for i, v in changes.items():
            getattr(t, name)[i] = v
    return t


def test_workspace_query():
    from bin_amd import _lib
    q = _lib.library(NAME).binssim_workspace_bytes
    fh, fw = _lib.SSIM_FWD_TILE
    assert q(1, 1, 11, 11) == 8 and q(24, 1, 11, 11) == 8 * 24
    assert q(2, 3, fh + 10, fw + 10) == 8 * 2 * 3 and q(2, 3, fh + 11, fw + 10) == 8 * 2 * 3 * 2 and q(2, 3, fh + 11, fw + 11) == 8 * 2 * 3 * 4
    assert q(17, 24, 256, 256) == 8 * 17 * 24 * 16 * 3
    for bad in ((0, 1, 11, 11), (25, 1, 11, 11), (-1, 1, 11, 11), (1, 0, 11, 11), (1, -1, 11, 11), (1, 1, 10, 11), (1, 1, 11, 10),
                (1, 2 ** 15, 2 ** 8, 2 ** 8), (1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), (1, 1, -(2 ** 31), 11)):
        assert q(*bad) == 0, bad
    assert q(1, 2 ** 15 - 1, 2 ** 8, 2 ** 8) > 0 and q(1, 1, 2 ** 15, 2 ** 16 - 1) > 0


def test_forward_refusals_return_their_code_without_a_device():
    from bin_amd import _lib
    lib = _lib.library(NAME)
    taps = (C.c_double * 11)()
    nb = lib.binssim_workspace_bytes(2, 3, 24, 40)

    def call(terms=None, planes=3, H=24, W=40, taps=taps, ws=WS, ws_bytes=nb, ssim=OUT):
        return lib.binssim_forward(C.byref(terms if terms is not None else _terms()), planes, H, W, taps, ws, ws_bytes, ssim, None)

    assert lib.binssim_forward(None, 3, 24, 40, taps, WS, nb, OUT, None) == E_ARG
    assert call(taps=None) == E_ARG and call(ws=None) == E_ARG and call(ssim=None) == E_ARG
    for n in (0, -1, 25, 2 ** 31 - 1):
        assert call(_terms(n)) == E_ARG, n
    assert call(_terms(x={1: None})) == E_ARG and call(_terms(y={0: None})) == E_ARG
    assert call(_terms(x={2: None}), H=10) == E_SHAPE, "an entry past n_terms is ignored"
    assert call(_terms(x={0: X + 2})) == E_ARG and call(_terms(y={1: Y + 1})) == E_ARG
    assert call(ssim=OUT + 2) == E_ARG and call(ws=WS + 4) == E_ARG
    # the shape
    for kw in (dict(planes=0), dict(planes=-1), dict(H=10), dict(W=10), dict(H=-5), dict(planes=2 ** 15, H=256, W=256),
               dict(planes=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)):
        assert call(**kw) == E_SHAPE, kw
    assert call(_terms(x={0: None}), planes=0) == E_ARG, "a null pointer is named first"
    # overlaps: an output that is also an input, the outputs on each other
    stack = 4 * 3 * 24 * 40
    assert call(ssim=X) == E_ARG and call(ssim=X + stack - 4) == E_ARG and call(ssim=Y + 0x4000 + 8) == E_ARG
    assert call(ssim=X - 4) == E_ARG and call(ssim=X - 8, ws_bytes=0) == E_WORKSPACE, "one element before an input touches nothing"
    assert call(ws=Y) == E_ARG and call(ws=X + 0x4000 - 8) == E_ARG and call(ws=OUT) == E_ARG and call(ssim=WS + 8) == E_ARG
    # the workspace
    assert call(ws_bytes=nb - 1) == E_WORKSPACE and call(ws_bytes=0) == E_WORKSPACE
    assert call(H=2 * 24, ws_bytes=nb) == E_WORKSPACE


def test_backward_refusals_return_their_code_without_a_device():
    from bin_amd import _lib
    lib = _lib.library(NAME)
    taps = (C.c_double * 11)()

    def call(terms=None, planes=3, H=24, W=40, taps=taps, g=G):
        return lib.binssim_backward(C.byref(terms if terms is not None else _terms()), planes, H, W, taps, g, None)

    assert lib.binssim_backward(None, 3, 24, 40, taps, G, None) == E_ARG
    assert call(taps=None) == E_ARG and call(g=None) == E_ARG and call(g=G + 2) == E_ARG
    for n in (0, -1, 25):
        assert call(_terms(n)) == E_ARG, n
    assert call(_terms(x={1: None})) == E_ARG and call(_terms(y={0: None})) == E_ARG
    assert call(_terms(gx={1: None}, gy={1: None})) == E_ARG, "a term with neither gradient"
    assert call(_terms(x={1: X + 0x4001})) == E_ARG and call(_terms(gx={0: GX + 2})) == E_ARG and call(_terms(gy={1: GY + 0x4003})) == E_ARG
    for kw in (dict(planes=0), dict(H=10), dict(W=10), dict(planes=2 ** 15, H=256, W=256)):
        assert call(**kw) == E_SHAPE, kw
    assert call(_terms(gx={0: None}, gy={0: None}), H=10) == E_ARG, "the terms are named before the shape"
    stack = 4 * 3 * 24 * 40
    # an output that is also an input: its own term's, another term's, by one element at either end, and g
    assert call(_terms(gx={0: X})) == E_ARG and call(_terms(gy={0: Y + 0x4000})) == E_ARG
    assert call(_terms(gx={1: X + stack - 4})) == E_ARG and call(_terms(gx={1: X - stack + 4})) == E_ARG
    assert call(_terms(gy={1: G})) == E_ARG and call(_terms(gy={1: G + 4})) == E_ARG and call(_terms(gy={1: G - stack + 4})) == E_ARG
    # an output named twice
    assert call(_terms(gy={0: GX})) == E_ARG and call(_terms(gx={1: GX})) == E_ARG and call(_terms(gy={1: GX + stack - 4})) == E_ARG


# ------------------------------------------------------------------------------------------------ 4. the option
def _opt(criterion, **train):
    return {"train": dict({"pixel_criterion": criterion}, **train)}


def test_ssim_weight_accept_and_refuse_table():
    from bin_amd.options.options import ssim_weight
    assert ssim_weight(_opt("cb+ssim", ssim_weight=0.5)) == 0.5 and ssim_weight(_opt("cb+ssim", ssim_weight=2)) == 2.0
    assert isinstance(ssim_weight(_opt("cb+ssim", ssim_weight=1)), float)
    for criterion in ("cb", "l1", "l2", None):
        assert ssim_weight(_opt(criterion)) is None and ssim_weight(_opt(criterion, ssim_weight=None)) is None
        with pytest.raises(ValueError, match=r"^train\.ssim_weight: 0\.5 is set, but train\.pixel_criterion is"):
            ssim_weight(_opt(criterion, ssim_weight=0.5))
    assert ssim_weight({}) is None and ssim_weight({"train": None}) is None
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: pixel_criterion: cb\+ssim needs it"):
        ssim_weight(_opt("cb+ssim"))
    for bad in (0, 0.0, -0.1, float("inf"), float("nan"), True, False, "0.5", [0.5], "1e-1"):
        with pytest.raises(ValueError, match=r"^train\.ssim_weight:"):
            ssim_weight(_opt("cb+ssim", ssim_weight=bad))


def test_shipped_option_files_carry_the_commented_lines_and_parse_checks_the_weight(tmp_path):
    from bin_amd.options import options
    folder = os.path.join(REPO, "bin_amd", "options")
    for name in ("bin_stage4_adobe240.yml", "bin_stage4_synthetic.yml", "bin_stage4_y4m.yml"):
        text = open(os.path.join(folder, name)).read()
        assert re.search(r"(?m)^\s*#\s*pixel_criterion: cb\+ssim", text) and re.search(r"(?m)^\s*#\s*ssim_weight:", text), name
        assert re.search(r"(?m)^\s*pixel_criterion: cb\b", text), name
        bad = str(tmp_path / name)
        with open(bad, "w") as f:
            f.write(re.sub(r"(?m)^(\s*)pixel_criterion: cb\b.*$", r"\1pixel_criterion: cb+ssim", text))
        with pytest.raises(ValueError, match=r"^train\.ssim_weight: pixel_criterion: cb\+ssim needs it"):
            options.parse(bad, is_train=True)


# ------------------------------------------------------------------------------------------------ 5. the wrappers
class _CpuCbSsim(torch.nn.Module):
    """CPU stand-in of CharbonnierSsimLoss: the same attributes and return, from the float64 restatement."""
    reduction = "mean"

    def __init__(self, ssim_weight, eps=1e-6):
        super().__init__()
        self.ssim_weight, self.eps, self.last_parts = ssim_weight, eps, None

    def forward(self, x, y):
        cb = ((x - y) ** 2 + self.eps).sqrt().mean()
        d = (1.0 - SC.ssim_ref(x, y)).float()
        self.last_parts = (cb.detach(), d.detach())
        return cb + self.ssim_weight * d


class _CpuPair(torch.nn.Module):
    def __init__(self, inner):
        super().__init__()
        self.inner, self.reduction = inner, inner.reduction

    def forward(self, x, y):
        return self.inner(x, y), self.inner.last_parts


class _ToyG(torch.nn.Module):
    def __init__(self):
        super().__init__()
        torch.manual_seed(5)
        self.conv = torch.nn.Conv2d(18, 42, 3, padding=1)

    def forward(self, *frames):
        return tuple(torch.sigmoid(self.conv(torch.cat(frames, 1))).split(3, 1))


def _train_opt(tmp, model, **train):
    opt = {"model": model, "gpu_ids": None, "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp), "training_state": str(tmp)},
           "train": {"pixel_criterion": "cb+ssim", "ssim_weight": 0.5, "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None,
                     "lr_G": 1e-3, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [100000],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    opt["train"].update(train)
    return opt


def _data(B, S=16):
    g = torch.Generator().manual_seed(9)
    return {"LQs": torch.rand(B, 6, 3, S, S, generator=g), "GTenh": torch.rand(B, 6, 3, S, S, generator=g),
            "GTinp": torch.rand(B, 5, 3, S, S, generator=g)}


@pytest.mark.parametrize("micro", [None, 1])
def test_bin_model_accepts_the_criterion_and_keeps_the_parts(tmp_path, micro):
    from bin_amd.models.bin_model import bin_model
    from bin_amd.models.loss import CharbonnierSsimLoss
    m = bin_model(_train_opt(tmp_path, "bin", micro_batch=micro), netG=_ToyG(), cri_pix=_CpuCbSsim(0.5))
    assert m.loss_type == "cb+ssim" and m.loss_parts is None
    m.feed_data(_data(2))
    before = [p.detach().clone() for p in m.netG.parameters()]
    m.optimize_parameters(1)
    cb, d = m.loss_parts
    assert not cb.requires_grad and not d.requires_grad and cb.dim() == d.dim() == 0
    assert abs(float(m.loss.detach()) - (float(cb) + 0.5 * float(d))) <= 1e-6
    pairs = [(m.Ft_p[i], gt) for i, gt in enumerate(m.get_info(mode=1)[1])]
    pairs += [(m.Ft_p[1], m.Ft_p[7]), (m.Ft_p[5], m.Ft_p[9]), (m.Ft_p[2], m.Ft_p[8])]
    want_d = sum(1.0 - float(SC.ssim_ref(x.detach(), y.detach())) for x, y in pairs) / 17
    assert abs(float(d) - want_d) <= 1e-6 and len(m.loss_list) == 14
    assert any(not torch.equal(a, b) for a, b in zip(before, m.netG.parameters())), "parameters move"
    # the product criterion is what the option builds when none is injected; its weight comes from the option
    built = bin_model(_train_opt(tmp_path, "bin", ssim_weight=0.25), netG=_ToyG())
    assert isinstance(built.cri_pix, CharbonnierSsimLoss) and built.cri_pix.ssim_weight == 0.25 and built.cri_pix.reduction == "mean"
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: pixel_criterion: cb\+ssim needs it"):
        bin_model(_train_opt(tmp_path, "bin", ssim_weight=None), netG=_ToyG())
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: 0\.5 is set, but"):
        bin_model(_train_opt(tmp_path, "bin", pixel_criterion="cb"), netG=_ToyG())
    plain = bin_model(_train_opt(tmp_path, "bin", pixel_criterion="cb", ssim_weight=None), netG=_ToyG(),
                      cri_pix=lambda x, y: ((x - y) ** 2 + 1e-6).sqrt().mean())
    plain.feed_data(_data(2))
    plain.optimize_parameters(1)
    assert plain.loss_parts is None
    with pytest.raises(NotImplementedError, match=r"Loss type \[cb\+msssim\] is not recognized"):
        bin_model(_train_opt(tmp_path, "bin", pixel_criterion="cb+msssim", ssim_weight=None), netG=_ToyG())


@pytest.mark.parametrize("micro", [None, 1])
def test_video_base_model_accepts_the_criterion_and_fills_the_log(tmp_path, micro):
    import videobase_cases as VC
    from bin_amd.models.Video_base_model import VideoBaseModel, _CbSsimPair
    opt = _train_opt(tmp_path, "video_base", micro_batch=micro, pixel_weight=0.5)
    m = VideoBaseModel(opt, netG=VC.StubVSR(), cri_pix=_CpuPair(_CpuCbSsim(0.5)))
    m.feed_data(VC.batch())
    before = [p.detach().clone() for p in m.netG.parameters()]
    m.optimize_parameters(1)
    log = m.get_current_log()
    assert set(log) == {"total_loss", "l_pix", "ssim_loss"} and all(isinstance(v, float) for v in log.values())
    assert abs(log["total_loss"] - 0.5 * (log["l_pix"] + 0.5 * log["ssim_loss"])) <= 1e-6
    want = 1.0 - float(SC.ssim_ref(m.fake_H.detach(), m.real_H))
    assert abs(log["ssim_loss"] - want) <= 1e-6
    assert any(not torch.equal(a, b) for a, b in zip(before, m.netG.parameters())), "parameters move"
    built = VideoBaseModel(_train_opt(tmp_path, "video_base", ssim_weight=0.25), netG=VC.StubVSR())
    assert isinstance(built.cri_pix, _CbSsimPair) and built.cri_pix.ssim_weight == 0.25 and built.cri_pix.reduction == "mean"
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: pixel_criterion: cb\+ssim needs it"):
        VideoBaseModel(_train_opt(tmp_path, "video_base", ssim_weight=None), netG=VC.StubVSR())
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: 0\.5 is set, but"):
        VideoBaseModel(_train_opt(tmp_path, "video_base", pixel_criterion="l1"), netG=VC.StubVSR())


def test_train_log_line_names_the_parts_when_present():
    import inspect
    from bin_amd import train
    src = inspect.getsource(train)
    assert 'getattr(model, "loss_parts", None)' in src and "l_cb %.4e  l_ssim %.4e" in src


def test_criterion_refuses_a_bad_weight_and_has_no_cpu_path():
    from bin_amd.models.loss import CharbonnierSsimLoss
    for bad in (0, -1.0, float("nan"), float("inf"), True, "0.5", None):
        with pytest.raises(ValueError, match="ssim_weight"):
            CharbonnierSsimLoss(bad)
    crit = CharbonnierSsimLoss(0.5)
    assert crit.eps == 1e-6 and crit.reduction == "mean" and not hasattr(crit, "kind")
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_ops_refuse_with_the_cause():
    from bin_amd import ops
    a = torch.zeros(2, 3, 16, 16)
    for what, pairs in (("non-empty", []), ("no CPU path", [(a, a)])):
        with pytest.raises((ValueError, RuntimeError), match=what):
            ops.ssim_terms(pairs)


# ------------------------------------------------------------------------------------------------ 6. the routing
def test_multi_term_loss_routes_by_ssim_weight_and_everything_else_as_before(monkeypatch):
    from bin_amd import _lib
    from bin_amd.models import loss as LM
    calls = []

    class FakeCb:
        @staticmethod
        def apply(kind, eps, idx_pairs, *uniq):
            calls.append(("cb", kind, eps, idx_pairs, len(uniq)))
            T = len(idx_pairs)
            return torch.tensor(3.0), torch.arange(T, dtype=torch.float32)

    class FakeSsim:
        @staticmethod
        def apply(idx_pairs, *uniq):
            calls.append(("ssim", idx_pairs, len(uniq)))
            return torch.full((len(idx_pairs),), 0.75)

    monkeypatch.setattr(LM, "_MultiPixelLossFn", FakeCb)
    monkeypatch.setattr(LM, "_MultiSsimFn", FakeSsim)
    a, b, c = (torch.rand(1, 3, 12, 12) for _ in range(3))
    pairs = [(a, b), (a, c), (b, c)]
    crit = LM.CharbonnierSsimLoss(0.5, eps=1e-3)
    # CPU tensors: the per-term loop (which raises in the product criterion: no CPU path)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LM.multi_term_loss(crit, pairs)
    assert calls == []
    monkeypatch.setattr(LM, "_one_shape_on_device", lambda pairs: True)
    loss, terms = LM.multi_term_loss(crit, pairs)
    want_pairs = ((0, 1), (0, 2), (1, 2))
    assert calls == [("cb", _lib.LOSS_CHARBONNIER, 1e-3, want_pairs, 3), ("ssim", want_pairs, 3)]
    assert float(loss) == 3.0 + 0.5 * 0.25 and [float(t) for t in terms] == [0.125, 1.125, 2.125]
    assert [float(p) for p in crit.last_parts] == [3.0, 0.25]
    # a criterion of the module without ssim_weight: the one node, as before; last_parts is not touched
    del calls[:]
    cb = LM.CharbonnierLoss()
    loss, terms = LM.multi_term_loss(cb, pairs)
    assert calls == [("cb", _lib.LOSS_CHARBONNIER, 1e-6, want_pairs, 3)] and float(loss) == 3.0 and not hasattr(cb, "last_parts")
    # an injected criterion, the switch, too many pairs: the loop
    del calls[:]
    loss, terms = LM.multi_term_loss(lambda x, y: (x - y).abs().mean(), pairs)
    assert calls == [] and len(terms) == 3 and abs(float(loss) - float(sum(terms) / 3)) == 0.0
    stand_in = _CpuCbSsim(0.5)
    monkeypatch.setenv("BIN_AMD_FUSED_LOSS", "0")
    loss, terms = LM.multi_term_loss(stand_in, pairs)
    assert calls == [] and len(terms) == 3
    cbs = [((x - y) ** 2 + 1e-6).sqrt().mean() for x, y in pairs]
    assert abs(float(stand_in.last_parts[0]) - float(sum(cbs) / 3)) <= 1e-7
    monkeypatch.delenv("BIN_AMD_FUSED_LOSS")
    loss, terms = LM.multi_term_loss(stand_in, [(a, b)] * 25)
    assert calls == [] and len(terms) == 25
