"""CPU: the criterion `pixel_criterion: cb+lap` without a device — the closed-form gradient of include/binlap.h against float64
autograd over the case table (lap_loss_cases.py) and the properties of the two operators, the bookkeeping of libbinlap.so and of its
row in the open-ended library table, every refusal of its entry points (they come before any HIP call, so made-up addresses are
never followed), the options `train.lap_weight` and `train.lap_levels`, both wrappers' control flow with a toy generator and a CPU
stand-in of the criterion, and which branch multi_term_loss takes."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import lap_loss_cases as LC
from conftest import REPO

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]
NAME = "binlap"
WANT = ["binlap_version", "binlap_forward_workspace_bytes", "binlap_backward_workspace_bytes", "binlap_forward", "binlap_backward"]


# ------------------------------------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("case", LC.CASES, ids=LC.case_id)
def test_closed_form_equals_autograd_in_float64(case):
    i, planes, h, w, levels, T = case
    worst = 0.0
    for kind, x, y, g, need in LC.case_terms(i)[:5]:
        xd, yd = x.double().requires_grad_(), y.double().requires_grad_()
        v = LC.lap_ref(xd, yd, levels)
        ax, ay = torch.autograd.grad(v, (xd, yd))
        v2, gx, gy = LC.closed_form(x, y, levels)
        scale = float(ax.abs().max())
        d = max(float((gx - ax).abs().max()), float((gy - ay).abs().max()))
        worst = max(worst, d / scale if scale else d)
        assert abs(float(v) - float(v2)) <= 1e-15 * float(v) and gx.shape == x.shape and gy.dtype == torch.float64
        assert d <= 1e-12 * scale, (kind, d, scale)
    print(f"[lap_loss] closed form {LC.case_id(case)}: max|closed - autograd| / max|grad| {worst:.3g}")


def test_rows_of_both_operators_sum_to_one_at_every_size():
    for n in list(range(1, 40)) + [47, 64, 129]:
        r, e = LC.reduce_matrix(n), LC.expand_matrix(n)
        m = (n + 1) // 2
        assert r.shape == (m, n) and e.shape == (n, m)
        assert float((r.sum(1) - 1).abs().max()) == 0.0 and float((e.sum(1) - 1).abs().max()) == 0.0, n
    e = LC.expand_matrix(8)
    assert e[4].tolist() == [0, 0.125, 0.75, 0.125] and e[3].tolist() == [0, 0.5, 0.5, 0] and e[0].tolist() == [0.875, 0.125, 0, 0]
    r = LC.reduce_matrix(7)
    assert r[1].tolist() == [1 / 16, 4 / 16, 6 / 16, 4 / 16, 1 / 16, 0, 0] and r[0].tolist() == [11 / 16, 4 / 16, 1 / 16, 0, 0, 0, 0]
    assert r[3].tolist() == [0, 0, 0, 0, 1 / 16, 4 / 16, 11 / 16]


def test_one_level_is_the_charbonnier_mean_equal_inputs_and_a_constant_offset():
    x, y = LC.content("noise", (2, 9, 13), 1)
    cb = ((x.double() - y.double()) ** 2 + LC.EPS).sqrt().mean()
    v, gx, gy = LC.closed_form(x, y, 1)
    d = x.double() - y.double()
    assert float(v) == float(cb) and torch.equal(gx, d / (d * d + LC.EPS).sqrt() / d.numel()) and torch.equal(gy, -gx)
    for shape, levels in (((2, 33, 47), 5), ((1, 16, 16), 5), ((3, 5, 7), 2)):
        x, y = LC.content("equal", shape, 2)
        v, gx, gy = LC.closed_form(x, y, levels)
        assert abs(float(v) - levels * LC.EPS ** 0.5) <= 1e-17 and float(gx.abs().max()) == 0.0 and float(gy.abs().max()) == 0.0
        x, y = LC.content("offset", shape, 3)
        bs = LC.bands(x.double() - y.double(), levels)
        assert all(float(b.abs().max()) == 0.0 for b in bs[:-1]) and bool((bs[-1] == -LC.OFFSET).all())
        v = LC.lap_ref(x, y, levels)
        assert abs(float(v) - ((levels - 1) * LC.EPS ** 0.5 + (LC.OFFSET ** 2 + LC.EPS) ** 0.5)) <= 1e-15


def test_table_covers_the_issue_shapes_the_tile_edges_every_kind_and_every_gradient_request():
    shapes = {c[1:5] for c in LC.CASES}
    assert {(1, 1, 1, 1), (2, 4, 4, 2), (3, 5, 7, 2), (2, 33, 47, 5), (1, 32, 32, 5), (1, 17, 129, 4), (24, 16, 16, 3), (24, 64, 64, 5)} <= shapes
    assert {(1, LC.UH, LC.UW, 2), (1, LC.UH + 1, LC.UW + 1, 2), (1, 2 * LC.DH, 2 * LC.DW, 2), (1, 2 * LC.DH + 1, 2 * LC.DW + 1, 2)} <= shapes
    assert {1, 17, 24} <= {c[5] for c in LC.CASES}
    assert all(min(h, w) >= 2 ** (levels - 1) for _, _, h, w, levels, _ in LC.CASES)
    seen = {(LC.term_kind(c, t), LC.term_need(t)) for c in LC.CASES for t in range(c[5])}
    assert seen == {(k, n) for k in LC.KINDS for n in LC.NEEDS}
    x, y = LC.content("near", (1, 8, 8), 4)
    assert 0 < float((y - x).abs().max()) <= 1.01e-4
    x, y = LC.content("edge", (2, 4, 16), 5)
    assert torch.equal(y[0, 0, 3:], x[0, 0, :-3]) and not torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 2. the library's bookkeeping
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_header_binding_and_dynamic_symbols_agree():
    from bin_amd import _lib, build
    names = [row.name for row in build.ADDON_LIBRARIES]
    assert names[names.index("binssim") + 1] == NAME, "the row comes after binssim"
    assert list(build.ADDON_BY_NAME) == names == list(_lib._ADDON_LIBRARIES)
    assert NAME not in build.BY_NAME and NAME not in build.EXTRA_BY_NAME and NAME not in _lib._LIBRARIES and NAME not in _lib._EXTRA_LIBRARIES
    assert len(build.LIBRARIES) == 11 and [row.name for row in build.EXTRA_LIBRARIES] == ["binexpose"]
    lib = build.ADDON_BY_NAME[NAME]
    assert build.row(NAME) is lib
    hdr = open(lib.header).read()
    declared = build.abi_symbols(NAME)
    assert lib.sources == ["binlap.hip"] and lib.subdir == "extra" and lib.purpose and "\n" not in lib.purpose
    assert lib.path == os.path.join(build.CSRC, "extra", "libbinlap.so") and lib.header == os.path.join(REPO, "include", "binlap.h")
    assert declared == WANT
    assert set(_lib.exported_symbols(NAME)) == set(declared) == _defined(lib.path)
    assert set(re.findall(rf"\b({NAME}_[a-z0-9_]+)\s*\(", hdr)) == set(declared)
    assert all(m.startswith("BINLAP_") for m in re.findall(r"#\s*define\s+(\w+)", hdr))
    assert "#pragma once" in hdr
    assert re.findall(r'(?m)^\s*#\s*include\s+"(\w+\.h)"', hdr) == [], "no other project header"
    assert re.findall(r"(?m)^\s*#\s*(?:if|ifdef|ifndef|elif)\b\s*(.*)$", hdr) == ["__cplusplus", "__cplusplus"]
    macro = lambda name: int(re.search(rf"#define\s+{name}\s+\(?(-?\d+)\)?", hdr).group(1))
    assert _lib.library(NAME).binlap_version() == macro("BINLAP_VERSION") == _lib._ADDON_LIBRARIES[NAME][1] == _lib.LAP_VERSION == 100
    assert (macro("BINLAP_E_ARG"), macro("BINLAP_E_SHAPE"), macro("BINLAP_E_WORKSPACE")) == \
        (_lib.LAP_E_ARG, _lib.LAP_E_SHAPE, _lib.LAP_E_WORKSPACE) == (-1, -2, -3)
    assert macro("BINLAP_MAX_TERMS") == _lib.LAP_MAX_TERMS == 24 and macro("BINLAP_MAX_LEVELS") == _lib.LAP_MAX_LEVELS == 8
    assert (macro("BINLAP_DOWN_TILE_H"), macro("BINLAP_DOWN_TILE_W")) == _lib.LAP_DOWN_TILE
    assert (macro("BINLAP_UP_TILE_H"), macro("BINLAP_UP_TILE_W")) == _lib.LAP_UP_TILE
    assert C.sizeof(_lib.BinLapTerms) == 4 * 24 * 8 + 8
    assert _lib.laplib() is _lib.library(NAME)
    # the header's parameter lists against the binding's signatures: how many, and which are integers, doubles, sizes and pointers
    kinds = {C.c_int: "int", C.c_double: "double", C.c_size_t: "size_t", C.c_void_p: "ptr"}
    for sym, (res, args) in _lib._LAP_SIGNATURES.items():
        m = re.search(rf"BINLAP_API\s+(\w+)\s+{sym}\s*\(([^)]*)\)", hdr)
        params = [p.strip() for p in m.group(2).split(",")] if m.group(2).strip() != "void" else []
        want = ["ptr" if "*" in p else p.split()[0] for p in params]
        assert [kinds.get(a, "ptr") for a in args] == want, sym
        assert {C.c_int: "int", C.c_size_t: "size_t"}[res] == m.group(1), sym
    assert "binlap.hip" not in os.listdir(build.CSRC) and os.path.exists(os.path.join(build.CSRC, "extra", "binlap.hip"))
    built = ["bin_amd/csrc/extra/libbinlap.so", "bin_amd/csrc/extra/binhip_exports.binlap.map", "bin_amd/csrc/extra/binlap.o"]
    ignored = subprocess.run(["git", "check-ignore"] + built, cwd=REPO, capture_output=True, text=True)
    if ignored.returncode != 128:                                 # (128: not a git checkout)
        assert len(ignored.stdout.split()) == len(built), "the built files stay out of git"


def test_version_gate_and_a_missing_library(monkeypatch, tmp_path):
    from bin_amd import _lib, build
    monkeypatch.setattr(_lib, "_loaded", {})
    assert _lib.library(NAME) is _lib.library(NAME), "loaded once"
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setitem(_lib._ADDON_LIBRARIES, NAME, (_lib._LAP_SIGNATURES, 101))
    with pytest.raises(RuntimeError, match=r"libbinlap\.so is version 100, this binding is for 101"):
        _lib.library(NAME)
    monkeypatch.setitem(_lib._ADDON_LIBRARIES, NAME, (_lib._LAP_SIGNATURES, 100))
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setattr(build, "CSRC", str(tmp_path))
    with pytest.raises(RuntimeError, match=r"HIP library \S*libbinlap\.so not built.*no CPU fallback"):
        _lib.library(NAME)


def test_the_addon_plan_compiles_one_source_into_the_library_with_the_core_flags():
    from bin_amd import build
    compiles, links = build.build_plan()
    assert len(links) == 11 and not any(NAME in " ".join(c) for c in compiles + [l[2] for l in links])
    compiles, links = build.build_plan(table=build.ADDON_LIBRARIES)
    assert len(compiles) == len(links) == len(build.ADDON_LIBRARIES)
    extra = os.path.join(build.CSRC, "extra")
    at = [row.name for row in build.ADDON_LIBRARIES].index(NAME)
    cmd, (vmap, names, link) = compiles[at], links[at]
    hipcc = build.build_plan()[0][0][0]
    assert cmd == [hipcc] + FLAGS + ["-c", os.path.join(extra, "binlap.hip"), "-o", os.path.join(extra, "binlap.o")]
    assert vmap == os.path.join(extra, "binhip_exports.binlap.map") and names == build.abi_symbols(NAME) == WANT
    assert link == [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}", "-o",
                    os.path.join(extra, "libbinlap.so"), os.path.join(extra, "binlap.o")]
    assert sum(1 for c in compiles if "binlap.hip" in c[-3]) == 1


def test_driver_loads_the_row_and_checks_its_symbols(monkeypatch):
    import __graft_entry__ as entry
    from bin_amd import _lib, build
    assert NAME not in entry.load_libraries() and NAME not in entry.load_libraries(build.EXTRA_LIBRARIES)
    loaded = entry.load_libraries(build.ADDON_LIBRARIES)
    assert list(loaded) == [row.name for row in build.ADDON_LIBRARIES] and loaded[NAME] is _lib.library(NAME)
    real = _lib.exported_symbols
    monkeypatch.setattr(_lib, "exported_symbols", lambda n="binhip": real(n) + (["binlap_absent"] if n == NAME else []))
    with pytest.raises(RuntimeError, match=r"libbinlap\.so is missing symbols: \['binlap_absent'\]"):
        entry.load_libraries(build.ADDON_LIBRARIES)


# ------------------------------------------------------------------------------------------------ 3. refusals
X, Y, GX, GY, WS, OUT, G = 0x100000, 0x200000, 0x300000, 0x400000, 0x8000000, 0x700000, 0x600000
E_ARG, E_SHAPE, E_WORKSPACE = -1, -2, -3
EPS = 1e-6


def _terms(n=2, **fields):
    """n terms with made-up, well separated addresses (1 MiB apart per kind, 16 KiB apart per term: a 3 x 24 x 40 fp32 stack is
    11 520 bytes); `fields`: name -> {term: address}."""
    from bin_amd import _lib
    t = _lib.BinLapTerms()
    t.n_terms = n
    for i in range(min(max(n, 0), 24)):
        t.x[i], t.y[i], t.gx[i], t.gy[i] = X + 0x4000 * i, Y + 0x4000 * i, GX + 0x4000 * i, GY + 0x4000 * i
    for name, changes in fields.items():
        for i, v in changes.items():
            getattr(t, name)[i] = v
    return t


def _level_sizes(n, levels):
    out = [n]
    for _ in range(levels - 1):
        out.append((out[-1] + 1) // 2)
    return out


def _want_bytes(T, planes, H, W, levels):
    hs, ws = _level_sizes(H, levels), _level_sizes(W, levels)
    from bin_amd import _lib
    uh, uw = _lib.LAP_UP_TILE
    coarse = sum(T * planes * h * w for h, w in list(zip(hs, ws))[1:])
    slots = sum(T * planes * -(-h // uh) * -(-w // uw) for h, w in zip(hs, ws))
    return 8 * (coarse + slots), 8 * max(2 * coarse, 1)


BAD_GEOMETRY = ((0, 1, 16, 16, 5), (25, 1, 16, 16, 5), (-1, 1, 16, 16, 5), (1, 0, 16, 16, 5), (1, -1, 16, 16, 5), (1, 1, 15, 16, 5),
                (1, 1, 16, 15, 5), (1, 1, 16, 16, 0), (1, 1, 16, 16, 9), (1, 1, 16, 16, -1), (1, 1, 127, 128, 8), (1, 1, 0, 1, 1),
                (1, 2 ** 15, 2 ** 8, 2 ** 8, 1), (1, 2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 1), (1, 1, -(2 ** 31), 16, 1))


def test_workspace_queries_count_the_pyramid_and_the_tiles_and_are_zero_where_the_calls_refuse():
    from bin_amd import _lib
    lib = _lib.library(NAME)
    fq, bq = lib.binlap_forward_workspace_bytes, lib.binlap_backward_workspace_bytes
    uh, uw = _lib.LAP_UP_TILE
    assert fq(1, 1, 1, 1, 1) == 8 and bq(1, 1, 1, 1, 1) == 8, "one slot; one pad double so that 0 always means a refusal"
    assert fq(24, 3, uh, uw, 1) == 8 * 24 * 3 and fq(2, 3, uh + 1, uw, 1) == 8 * 2 * 3 * 2 and fq(2, 3, uh + 1, uw + 1, 1) == 8 * 2 * 3 * 4
    for args in ((1, 1, 1, 1, 1), (2, 3, 5, 7, 2), (2, 2, 33, 47, 5), (17, 24, 256, 256, 5), (24, 1, 17, 129, 4), (1, 1, 128, 128, 8),
                 (3, 2, uh + 1, uw + 1, 2)):
        assert (fq(*args), bq(*args)) == _want_bytes(*args), args
    for bad in BAD_GEOMETRY:
        assert fq(*bad) == 0 and bq(*bad) == 0, bad
    assert fq(1, 2 ** 15 - 1, 2 ** 8, 2 ** 8, 1) > 0 and bq(1, 1, 2 ** 15, 2 ** 16 - 1, 8) > 0


def test_forward_refusals_return_their_code_without_a_device():
    from bin_amd import _lib
    lib = _lib.library(NAME)
    nb = lib.binlap_forward_workspace_bytes(2, 3, 24, 40, 4)

    def call(terms=None, planes=3, H=24, W=40, levels=4, eps=EPS, ws=WS, ws_bytes=nb, lap=OUT):
        return lib.binlap_forward(C.byref(terms if terms is not None else _terms()), planes, H, W, levels, eps, ws, ws_bytes, lap, None)

    assert lib.binlap_forward(None, 3, 24, 40, 4, EPS, WS, nb, OUT, None) == E_ARG
    assert call(ws=None) == E_ARG and call(lap=None) == E_ARG
    for n in (0, -1, 25, 2 ** 31 - 1):
        assert call(_terms(n)) == E_ARG, n
    assert call(_terms(x={1: None})) == E_ARG and call(_terms(y={0: None})) == E_ARG
    assert call(_terms(x={2: None}), H=7) == E_SHAPE, "an entry past n_terms is ignored"
    assert call(_terms(x={0: X + 2})) == E_ARG and call(_terms(y={1: Y + 1})) == E_ARG
    assert call(lap=OUT + 2) == E_ARG and call(ws=WS + 4) == E_ARG
    # levels and eps
    for levels in (0, -1, 9, 2 ** 31 - 1):
        assert call(levels=levels) == E_ARG, levels
    for eps in (0.0, -1e-6, float("inf"), float("nan"), -0.0):
        assert call(eps=eps) == E_ARG, eps
    assert call(levels=9, H=0) == E_ARG and call(eps=0.0, planes=0) == E_ARG, "a bad value is named before the shape"
    assert call(_terms(x={0: None}), levels=0) == E_ARG and call(ws=None, levels=0, planes=0) == E_ARG
    # the shape
    for kw in (dict(planes=0), dict(planes=-1), dict(H=7), dict(W=7), dict(H=-5), dict(levels=6), dict(levels=6, W=64), dict(planes=2 ** 15, H=256, W=256),
               dict(planes=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)):
        assert call(**kw) == E_SHAPE, kw
    assert call(H=8, W=8, ws_bytes=0) == E_WORKSPACE and call(levels=1, H=1, W=1, ws_bytes=0) == E_WORKSPACE, "the smallest plane of a level count"
    # overlaps: an output that is also an input, the outputs on each other
    stack = 4 * 3 * 24 * 40
    assert call(lap=X) == E_ARG and call(lap=X + stack - 4) == E_ARG and call(lap=Y + 0x4000 + 8) == E_ARG
    assert call(lap=X - 4) == E_ARG and call(lap=X - 8, ws_bytes=0) == E_WORKSPACE, "one element before an input touches nothing"
    assert call(ws=Y) == E_ARG and call(ws=X + 0x4000 - 8) == E_ARG and call(lap=WS + 8) == E_ARG and call(lap=WS + nb - 4) == E_ARG
    assert call(ws=X - nb + 8) == E_ARG and call(ws=OUT - nb + 8) == E_ARG
    assert call(planes=0, lap=X) == E_SHAPE, "the shape is named before an overlap"
    # the workspace
    assert call(ws_bytes=nb - 1) == E_WORKSPACE and call(ws_bytes=0) == E_WORKSPACE
    assert call(H=2 * 24, ws_bytes=nb) == E_WORKSPACE and call(lap=X, ws_bytes=0) == E_ARG, "an overlap is named before the workspace"


def test_backward_refusals_return_their_code_without_a_device():
    from bin_amd import _lib
    lib = _lib.library(NAME)
    nb = lib.binlap_backward_workspace_bytes(2, 3, 24, 40, 4)

    def call(terms=None, planes=3, H=24, W=40, levels=4, eps=EPS, g=G, ws=WS, ws_bytes=nb):
        return lib.binlap_backward(C.byref(terms if terms is not None else _terms()), planes, H, W, levels, eps, g, ws, ws_bytes, None)

    assert lib.binlap_backward(None, 3, 24, 40, 4, EPS, G, WS, nb, None) == E_ARG
    assert call(g=None) == E_ARG and call(g=G + 2) == E_ARG and call(ws=None) == E_ARG and call(ws=WS + 4) == E_ARG
    for n in (0, -1, 25):
        assert call(_terms(n)) == E_ARG, n
    assert call(_terms(x={1: None})) == E_ARG and call(_terms(y={0: None})) == E_ARG
    assert call(_terms(gx={1: None}, gy={1: None})) == E_ARG, "a term with neither gradient"
    assert call(_terms(gx={1: None}), ws_bytes=0) == E_WORKSPACE and call(_terms(gy={0: None}), ws_bytes=0) == E_WORKSPACE, "one of them is enough"
    assert call(_terms(x={1: X + 0x4001})) == E_ARG and call(_terms(gx={0: GX + 2})) == E_ARG and call(_terms(gy={1: GY + 0x4003})) == E_ARG
    for levels in (0, -1, 9):
        assert call(levels=levels) == E_ARG, levels
    for eps in (0.0, -1e-6, float("inf"), float("nan")):
        assert call(eps=eps) == E_ARG, eps
    assert call(levels=9, H=0) == E_ARG and call(eps=0.0, planes=0) == E_ARG, "a bad value is named before the shape"
    for kw in (dict(planes=0), dict(H=7), dict(W=7), dict(levels=6), dict(planes=2 ** 15, H=256, W=256)):
        assert call(**kw) == E_SHAPE, kw
    assert call(_terms(gx={0: None}, gy={0: None}), H=7) == E_ARG, "the terms are named before the shape"
    stack = 4 * 3 * 24 * 40
    # an output that is also an input: its own term's, another term's, by one element at either end, and g
    assert call(_terms(gx={0: X})) == E_ARG and call(_terms(gy={0: Y + 0x4000})) == E_ARG
    assert call(_terms(gx={1: X + stack - 4})) == E_ARG and call(_terms(gx={1: X - stack + 4})) == E_ARG
    assert call(_terms(gy={1: G})) == E_ARG and call(_terms(gy={1: G + 4})) == E_ARG and call(_terms(gy={1: G - stack + 4})) == E_ARG
    # an output named twice
    assert call(_terms(gy={0: GX})) == E_ARG and call(_terms(gx={1: GX})) == E_ARG and call(_terms(gy={1: GX + stack - 4})) == E_ARG
    # the used workspace on an output, an input or g
    assert call(ws=GX) == E_ARG and call(ws=GY + 0x4000 + stack - 8) == E_ARG and call(ws=X) == E_ARG and call(ws=Y - nb + 8) == E_ARG
    assert call(ws=G) == E_ARG and call(ws=G - nb + 8) == E_ARG
    assert call(ws=X, planes=0) == E_SHAPE, "the shape is named before an overlap"
    # the workspace
    assert call(ws_bytes=nb - 1) == E_WORKSPACE and call(ws_bytes=0) == E_WORKSPACE and call(W=44) == E_WORKSPACE
    assert call(ws=X, ws_bytes=0) == E_ARG, "an overlap is named before the workspace"
    assert call(levels=1, ws_bytes=7) == E_WORKSPACE and call(levels=1, H=1, W=1, ws_bytes=0) == E_WORKSPACE, "one level still takes its pad double"
    for bad in BAD_GEOMETRY:                                         # the queries are 0 exactly where the calls refuse these arguments
        T, planes, H, W, levels = bad
        assert call(_terms(T), planes, H, W, levels) in (E_ARG, E_SHAPE), bad
        assert lib.binlap_forward(C.byref(_terms(T)), planes, H, W, levels, EPS, WS, 1 << 40, OUT, None) in (E_ARG, E_SHAPE), bad


# ------------------------------------------------------------------------------------------------ 4. the options
def _opt(criterion, **train):
    return {"train": dict({"pixel_criterion": criterion}, **train)}


def test_lap_weight_accept_and_refuse_table():
    from bin_amd.options.options import lap_weight, ssim_weight
    assert lap_weight(_opt("cb+lap", lap_weight=0.5)) == 0.5 and lap_weight(_opt("cb+lap", lap_weight=2)) == 2.0
    assert isinstance(lap_weight(_opt("cb+lap", lap_weight=1)), float)
    for criterion in ("cb", "l1", "l2", "cb+ssim", None):
        assert lap_weight(_opt(criterion)) is None and lap_weight(_opt(criterion, lap_weight=None)) is None
        with pytest.raises(ValueError, match=r"^train\.lap_weight: 0\.5 is set, but train\.pixel_criterion is"):
            lap_weight(_opt(criterion, lap_weight=0.5))
    assert lap_weight({}) is None and lap_weight({"train": None}) is None
    with pytest.raises(ValueError, match=r"^train\.lap_weight: pixel_criterion: cb\+lap needs it"):
        lap_weight(_opt("cb+lap"))
    for bad in (0, 0.0, -0.1, float("inf"), float("nan"), True, False, "0.5", [0.5], "1e-1"):
        with pytest.raises(ValueError, match=r"^train\.lap_weight:"):
            lap_weight(_opt("cb+lap", lap_weight=bad))
    assert ssim_weight(_opt("cb+lap", lap_weight=0.5)) is None
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: 0\.1 is set, but train\.pixel_criterion is 'cb\+lap'"):
        ssim_weight(_opt("cb+lap", lap_weight=0.5, ssim_weight=0.1))


def test_lap_levels_accept_and_refuse_table():
    from bin_amd.options.options import lap_levels
    assert lap_levels(_opt("cb+lap")) == 5 and lap_levels(_opt("cb+lap", lap_levels=None)) == 5
    for ok in range(1, 9):
        assert lap_levels(_opt("cb+lap", lap_levels=ok)) == ok
    for bad in (0, 9, -1, 2.0, 5.5, True, False, "5", [5], float("nan")):
        with pytest.raises(ValueError, match=r"^train\.lap_levels:"):
            lap_levels(_opt("cb+lap", lap_levels=bad))
    for criterion in ("cb", "l1", "l2", "cb+ssim", None):
        assert lap_levels(_opt(criterion)) is None
        with pytest.raises(ValueError, match=r"^train\.lap_levels: 4 is set, but train\.pixel_criterion is"):
            lap_levels(_opt(criterion, lap_levels=4))
    assert lap_levels({}) is None and lap_levels({"train": None}) is None


def test_shipped_option_files_carry_the_commented_lines_and_parse_checks_the_options(tmp_path):
    from bin_amd.options import options
    folder = os.path.join(REPO, "bin_amd", "options")
    for name in ("bin_stage4_adobe240.yml", "bin_stage4_synthetic.yml", "bin_stage4_y4m.yml"):
        text = open(os.path.join(folder, name)).read()
        for key in (r"pixel_criterion: cb\+lap", "lap_weight:", "lap_levels:"):
            assert re.search(rf"(?m)^\s*#\s*{key}", text), (name, key)
        assert re.search(r"(?m)^\s*pixel_criterion: cb\b(?!\+)", text), name
        assert text.index("#ssim_weight:") < text.index("#pixel_criterion: cb+lap") < text.index("#lap_weight:") < text.index("#lap_levels:")
        bad = str(tmp_path / name)
        with open(bad, "w") as f:
            f.write(re.sub(r"(?m)^(\s*)pixel_criterion: cb\b.*$", r"\1pixel_criterion: cb+lap", text))
        with pytest.raises(ValueError, match=r"^train\.lap_weight: pixel_criterion: cb\+lap needs it"):
            options.parse(bad, is_train=True)
        with open(bad, "w") as f:
            f.write(re.sub(r"(?m)^(\s*)pixel_criterion: cb\b.*$", r"\1pixel_criterion: cb+lap\n\1lap_weight: 0.5\n\1lap_levels: 9", text))
        with pytest.raises(ValueError, match=r"^train\.lap_levels: 9 is not an integer 1 \.\. 8"):
            options.parse(bad, is_train=True)


# ------------------------------------------------------------------------------------------------ 5. the wrappers
class _CpuCbLap(torch.nn.Module):
    """CPU stand-in of CharbonnierLapLoss: the same attributes and return, from the float64 restatement."""
    reduction = "mean"

    def __init__(self, lap_weight, levels=3, eps=1e-6):
        super().__init__()
        self.lap_weight, self.levels, self.eps, self.last_parts = lap_weight, levels, eps, None

    def forward(self, x, y):
        cb = ((x - y) ** 2 + self.eps).sqrt().mean()
        lap = LC.lap_ref(x, y, self.levels, self.eps).float()
        self.last_parts = (cb.detach(), lap.detach())
        return cb + self.lap_weight * lap


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
           "train": {"pixel_criterion": "cb+lap", "lap_weight": 0.5, "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None,
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
    from bin_amd.models.loss import CharbonnierLapLoss
    m = bin_model(_train_opt(tmp_path, "bin", micro_batch=micro), netG=_ToyG(), cri_pix=_CpuCbLap(0.5))
    assert m.loss_type == "cb+lap" and m.loss_parts is None and m.loss_part_names == ("l_cb", "l_lap")
    m.feed_data(_data(2))
    before = [p.detach().clone() for p in m.netG.parameters()]
    m.optimize_parameters(1)
    cb, lap = m.loss_parts
    assert not cb.requires_grad and not lap.requires_grad and cb.dim() == lap.dim() == 0
    assert abs(float(m.loss.detach()) - (float(cb) + 0.5 * float(lap))) <= 1e-6
    pairs = [(m.Ft_p[i], gt) for i, gt in enumerate(m.get_info(mode=1)[1])]
    pairs += [(m.Ft_p[1], m.Ft_p[7]), (m.Ft_p[5], m.Ft_p[9]), (m.Ft_p[2], m.Ft_p[8])]
    want = sum(float(LC.lap_ref(x.detach(), y.detach(), 3)) for x, y in pairs) / 17
    assert abs(float(lap) - want) <= 1e-6 and len(m.loss_list) == 14
    assert any(not torch.equal(a, b) for a, b in zip(before, m.netG.parameters())), "parameters move"
    # the product criterion is what the option builds when none is injected; its weight and level count come from the options
    built = bin_model(_train_opt(tmp_path, "bin", lap_weight=0.25), netG=_ToyG())
    assert isinstance(built.cri_pix, CharbonnierLapLoss) and built.cri_pix.lap_weight == 0.25 and built.cri_pix.levels == 5
    assert built.cri_pix.reduction == "mean" and built.cri_pix.eps == 1e-6
    assert bin_model(_train_opt(tmp_path, "bin", lap_levels=3), netG=_ToyG()).cri_pix.levels == 3
    with pytest.raises(ValueError, match=r"^train\.lap_weight: pixel_criterion: cb\+lap needs it"):
        bin_model(_train_opt(tmp_path, "bin", lap_weight=None), netG=_ToyG())
    with pytest.raises(ValueError, match=r"^train\.lap_weight: 0\.5 is set, but"):
        bin_model(_train_opt(tmp_path, "bin", pixel_criterion="cb"), netG=_ToyG())
    with pytest.raises(ValueError, match=r"^train\.ssim_weight: 0\.1 is set, but"):
        bin_model(_train_opt(tmp_path, "bin", ssim_weight=0.1), netG=_ToyG())
    plain = bin_model(_train_opt(tmp_path, "bin", pixel_criterion="cb", lap_weight=None), netG=_ToyG(),
                      cri_pix=lambda x, y: ((x - y) ** 2 + 1e-6).sqrt().mean())
    plain.feed_data(_data(2))
    plain.optimize_parameters(1)
    assert plain.loss_parts is None and plain.loss_part_names is None
    ssim = bin_model(_train_opt(tmp_path, "bin", pixel_criterion="cb+ssim", lap_weight=None, ssim_weight=0.5), netG=_ToyG())
    assert ssim.loss_part_names == ("l_cb", "l_ssim")


@pytest.mark.parametrize("micro", [None, 1])
def test_video_base_model_accepts_the_criterion_and_fills_the_log(tmp_path, micro):
    import videobase_cases as VC
    from bin_amd.models.Video_base_model import VideoBaseModel, _CbLapPair
    opt = _train_opt(tmp_path, "video_base", micro_batch=micro, pixel_weight=0.5)
    m = VideoBaseModel(opt, netG=VC.StubVSR(), cri_pix=_CpuPair(_CpuCbLap(0.5)))
    m.feed_data(VC.batch())
    before = [p.detach().clone() for p in m.netG.parameters()]
    m.optimize_parameters(1)
    log = m.get_current_log()
    assert set(log) == {"total_loss", "l_pix", "lap_loss"} and all(isinstance(v, float) for v in log.values())
    assert abs(log["total_loss"] - 0.5 * (log["l_pix"] + 0.5 * log["lap_loss"])) <= 1e-6
    want = float(LC.lap_ref(m.fake_H.detach(), m.real_H, 3))
    assert abs(log["lap_loss"] - want) <= 1e-6
    assert any(not torch.equal(a, b) for a, b in zip(before, m.netG.parameters())), "parameters move"
    built = VideoBaseModel(_train_opt(tmp_path, "video_base", lap_weight=0.25, lap_levels=4), netG=VC.StubVSR())
    assert isinstance(built.cri_pix, _CbLapPair) and built.cri_pix.lap_weight == 0.25 and built.cri_pix.levels == 4
    assert built.cri_pix.reduction == "mean"
    with pytest.raises(ValueError, match=r"^train\.lap_weight: pixel_criterion: cb\+lap needs it"):
        VideoBaseModel(_train_opt(tmp_path, "video_base", lap_weight=None), netG=VC.StubVSR())
    with pytest.raises(ValueError, match=r"^train\.lap_weight: 0\.5 is set, but"):
        VideoBaseModel(_train_opt(tmp_path, "video_base", pixel_criterion="l1"), netG=VC.StubVSR())


def test_train_log_line_names_the_parts_the_model_holds():
    import inspect
    from bin_amd import train
    src = inspect.getsource(train)
    assert 'getattr(model, "loss_part_names", None)' in src and "l_cb %.4e  l_lap %.4e" in src and "l_cb %.4e  l_ssim %.4e" in src


def test_criterion_refuses_bad_arguments_and_has_no_cpu_path():
    from bin_amd.models.loss import CharbonnierLapLoss
    for bad in (0, -1.0, float("nan"), float("inf"), True, "0.5", None):
        with pytest.raises(ValueError, match="lap_weight"):
            CharbonnierLapLoss(bad)
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="levels"):
            CharbonnierLapLoss(0.5, bad)
    crit = CharbonnierLapLoss(0.5)
    assert crit.eps == 1e-6 and crit.levels == 5 and crit.reduction == "mean" and not hasattr(crit, "kind") and not hasattr(crit, "ssim_weight")
    with pytest.raises(RuntimeError, match="no CPU path"):
        crit(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))


def test_ops_refuse_with_the_cause():
    from bin_amd import ops
    a = torch.zeros(2, 3, 16, 16)
    for what, pairs in (("non-empty", []), ("no CPU path", [(a, a)])):
        with pytest.raises((ValueError, RuntimeError), match=what):
            ops.lap_terms(pairs, 5, 1e-6)
        with pytest.raises((ValueError, RuntimeError), match=what):
            ops.lap_terms_grad(pairs, torch.ones(len(pairs)), [(True, True)] * len(pairs), 5, 1e-6)
    for levels in (0, 9, True, 2.0):
        with pytest.raises(ValueError, match="levels"):
            ops.lap_terms([(a, a)], levels, 1e-6)
    for eps in (0.0, -1.0, float("nan"), float("inf"), "1e-6"):
        with pytest.raises(ValueError, match="eps"):
            ops.lap_terms([(a, a)], 5, eps)


# ------------------------------------------------------------------------------------------------ 6. the routing
def test_multi_term_loss_routes_by_lap_weight_and_everything_else_as_before(monkeypatch):
    from bin_amd import _lib
    from bin_amd.models import loss as LM
    calls = []

    class FakeCb:
        @staticmethod
        def apply(kind, eps, idx_pairs, *uniq):
            calls.append(("cb", kind, eps, idx_pairs, len(uniq)))
            return torch.tensor(3.0), torch.arange(len(idx_pairs), dtype=torch.float32)

    class FakeSsim:
        @staticmethod
        def apply(idx_pairs, *uniq):
            calls.append(("ssim", idx_pairs, len(uniq)))
            return torch.full((len(idx_pairs),), 0.75)

    class FakeLap:
        @staticmethod
        def apply(levels, eps, idx_pairs, *uniq):
            calls.append(("lap", levels, eps, idx_pairs, len(uniq)))
            return torch.full((len(idx_pairs),), 0.25)

    monkeypatch.setattr(LM, "_MultiPixelLossFn", FakeCb)
    monkeypatch.setattr(LM, "_MultiSsimFn", FakeSsim)
    monkeypatch.setattr(LM, "_MultiLapFn", FakeLap)
    a, b, c = (torch.rand(1, 3, 16, 16) for _ in range(3))
    pairs = [(a, b), (a, c), (b, c)]
    crit = LM.CharbonnierLapLoss(0.5, levels=4, eps=1e-3)
    # CPU tensors: the per-term loop (which raises in the product criterion: no CPU path)
    with pytest.raises(RuntimeError, match="no CPU path"):
        LM.multi_term_loss(crit, pairs)
    assert calls == []
    monkeypatch.setattr(LM, "_one_shape_on_device", lambda pairs: True)
    loss, terms = LM.multi_term_loss(crit, pairs)
    want_pairs = ((0, 1), (0, 2), (1, 2))
    assert calls == [("cb", _lib.LOSS_CHARBONNIER, 1e-3, want_pairs, 3), ("lap", 4, 1e-3, want_pairs, 3)]
    assert float(loss) == 3.0 + 0.5 * 0.25 and [float(t) for t in terms] == [0.125, 1.125, 2.125]
    assert [float(p) for p in crit.last_parts] == [3.0, 0.25]
    # cb and cb+ssim: routed as before
    del calls[:]
    cb = LM.CharbonnierLoss()
    loss, terms = LM.multi_term_loss(cb, pairs)
    assert calls == [("cb", _lib.LOSS_CHARBONNIER, 1e-6, want_pairs, 3)] and float(loss) == 3.0 and not hasattr(cb, "last_parts")
    del calls[:]
    ssim = LM.CharbonnierSsimLoss(0.5, eps=1e-3)
    loss, terms = LM.multi_term_loss(ssim, pairs)
    assert calls == [("cb", _lib.LOSS_CHARBONNIER, 1e-3, want_pairs, 3), ("ssim", want_pairs, 3)] and float(loss) == 3.0 + 0.5 * 0.25
    # an injected criterion, the switch, too many pairs: the loop, and the parts are the means of the terms' parts
    del calls[:]
    loss, terms = LM.multi_term_loss(lambda x, y: (x - y).abs().mean(), pairs)
    assert calls == [] and len(terms) == 3 and abs(float(loss) - float(sum(terms) / 3)) == 0.0
    stand_in = _CpuCbLap(0.5)
    monkeypatch.setenv("BIN_AMD_FUSED_LOSS", "0")
    loss, terms = LM.multi_term_loss(stand_in, pairs)
    assert calls == [] and len(terms) == 3
    laps = [LC.lap_ref(x, y, 3) for x, y in pairs]
    assert abs(float(stand_in.last_parts[1]) - float(sum(laps) / 3)) <= 1e-6
    monkeypatch.delenv("BIN_AMD_FUSED_LOSS")
    loss, terms = LM.multi_term_loss(stand_in, [(a, b)] * 25)
    assert calls == [] and len(terms) == 25
