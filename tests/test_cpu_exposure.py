"""CPU: the exposure path (dataset options `blur_gamma` / `blur_noise`, bin_amd/data/exposure.py, libbinexpose.so) without a
device: the curve tables and their validity rules, the option refusals, the numpy host twin against the plain-integer restatement
of include/binexpose.h (exposure_cases.py) and against the real-number formula in float64, the statistics of the noise integer, the
bookkeeping of the extra library table, binexpose_gather's refusals, that nothing of it is touched when the options are absent, and
tools/make_blur_folder.py --gamma."""
import ctypes as C
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import exposure_cases as EC
from conftest import REPO

GAMMAS = (1.0, 1.8, 2.2, 2.4, "srgb")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]


def _u32(values):
    return np.ascontiguousarray(values, dtype=np.uint32)


def _check(lin, mid, sig):
    from bin_amd import _lib
    lin, mid, sig = _u32(lin), _u32(mid), _u32(sig)
    return _lib.library("binexpose").binexpose_check_curve(lin.ctypes.data, mid.ctypes.data, sig.ctypes.data)


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize("gamma", GAMMAS)
def test_tables_are_valid_equal_the_restatement_and_decode_every_code(gamma):
    from bin_amd.data import exposure as X
    for noise in (None, (0.004, 0.0004), (0.1, 0.01), (0.0, 0.0)):
        lin, mid, sig = EC.tables(gamma, noise)
        assert EC.curve_is_valid(lin, mid, sig)
        assert [EC.decode(mid, lin[v]) for v in range(256)] == list(range(256))
        t = X.curve_tables(gamma, noise)
        assert t.dtype == np.uint32 and t.tolist() == [lin, mid, sig] and not t.flags.writeable
        assert X.decode(t[1], t[0]).tolist() == list(range(256))
        assert _check(lin, mid, sig) == 0
        assert (max(sig) == 0) == (noise in (None, (0.0, 0.0))) and max(sig) < 2 ** 23
    assert EC.tables(gamma)[0][255] == EC.ONE and X.curve_tables(gamma) is X.curve_tables(gamma)


def test_check_curve_refuses_each_broken_rule_by_its_own_mutation():
    from bin_amd.data import exposure as X
    lin, mid, sig = EC.tables(2.2, (0.01, 0.002))
    assert _check(lin, mid, sig) == 0
    mutants = {}
    m = list(lin); m[100] = m[99] - 1; mutants["a decreasing LIN"] = (m, mid, sig)
    m = list(mid); m[100] = m[99]; mutants["a repeated MID"] = (lin, m, sig)
    m = list(lin); m[100] = mid[101]; mutants["LIN[c] >= MID[c + 1]"] = (m, mid, sig)
    m = list(lin); m[255] = EC.ONE + 1; mutants["LIN[255] > ONE"] = (m, mid, sig)
    m = list(sig); m[7] = 2 ** 23; mutants["SIG >= 2^23"] = (lin, mid, m)
    m = list(lin); m[0] = 1; mutants["LIN[0] != 0"] = (m, mid, sig)
    m = list(lin); m[100] = mid[100] - 1; mutants["LIN[c] < MID[c]"] = (m, mid, sig)
    for name, (a, b, c) in mutants.items():
        assert not EC.curve_is_valid(a, b, c), name
        assert _check(a, b, c) == -1, name
        with pytest.raises(ValueError, match="does not hold"):
            X.check_tables(np.array([a, b, c], dtype=np.uint32))
    # the edges of each rule are legal
    m = list(lin); m[100] = m[99]
    assert _check(m, mid, sig) == (0 if m[100] >= mid[100] else -1)
    m = list(sig); m[7] = 2 ** 23 - 1
    assert _check(lin, mid, m) == 0
    from bin_amd import _lib
    ok = _u32(lin)
    fn = _lib.library("binexpose").binexpose_check_curve
    assert fn(None, ok.ctypes.data, ok.ctypes.data) == fn(ok.ctypes.data, None, ok.ctypes.data) == fn(ok.ctypes.data, ok.ctypes.data, None) == -1


# ------------------------------------------------------------------------------------------------ options
def test_option_refusals_name_the_option():
    from bin_amd.data import exposure as X
    for bad in (0.9, 2.5, True, False, "rec709", "", [2.2], float("nan")):
        with pytest.raises(ValueError, match="^blur_gamma:"):
            X.parse_blur_gamma(bad)
    assert X.parse_blur_gamma(None) is None and X.parse_blur_gamma(1) == 1.0 and X.parse_blur_gamma(2.4) == 2.4
    assert X.parse_blur_gamma("srgb") == X.parse_blur_gamma("sRGB") == "srgb"
    for bad in ([-0.001, 0], [0, -1e-9], [0.11, 0], [0, 0.011], [0.01], [0.01, 0.001, 0], 0.01, "0.01,0.001", [True, 0], [0.01, None],
                [float("nan"), 0]):
        with pytest.raises(ValueError, match="^blur_noise:"):
            X.parse_blur_noise(bad)
    assert X.parse_blur_noise(None) is None and X.parse_blur_noise([0.1, 0.01]) == (0.1, 0.01) and X.parse_blur_noise((0, 0)) == (0.0, 0.0)
    with pytest.raises(ValueError, match="^blur_gamma: needs `blur_window`"):
        X.parse_options({"blur_gamma": 2.2}, None)
    with pytest.raises(ValueError, match="^blur_noise: needs `blur_window`"):
        X.parse_options({"blur_noise": [0.01, 0.001]}, None)
    with pytest.raises(ValueError, match="^blur_noise: needs `blur_gamma`"):
        X.parse_options({"blur_noise": [0.01, 0.001]}, 11)
    assert X.parse_options({}, 11) is None and X.parse_options({}, None) is None
    assert X.parse_options({"blur_gamma": 1.0}, 11) == X.Exposure(1.0, None)
    assert X.parse_options({"blur_gamma": "srgb", "blur_noise": [0.004, 0.0004]}, (7, 11)) == X.Exposure("srgb", (0.004, 0.0004))


def test_datasets_refuse_the_options_without_blur_window(tmp_path):
    from bin_amd.data import create_dataset
    root = str(tmp_path)
    for sub in ("train", "train_blur", "train_list"):
        os.makedirs(os.path.join(root, sub))
    base = {"mode": "BIN", "name": "train", "dataroot_GT": root, "dataroot_LQ": root, "LQ_size": [3, 8, 8], "phase": "train"}
    for name, value in (("blur_gamma", 2.2), ("blur_noise", [0.01, 0.001])):
        with pytest.raises(ValueError, match=f"^{name}: needs `blur_window`"):
            create_dataset(dict(base, **{name: value}))
    with pytest.raises(ValueError, match="^blur_gamma:"):
        create_dataset(dict(base, blur_window=11, blur_gamma=2.5))


# ------------------------------------------------------------------------------------------------ the host twin
def test_philox_known_answer_and_the_numpy_philox():
    from bin_amd.data import exposure as X
    assert EC.philox4x32_10((0, 0, 0, 0), (0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    g = random.Random(4)
    cs = [[g.getrandbits(32) for _ in range(50)] for _ in range(4)]
    ks = [[g.getrandbits(32) for _ in range(50)] for _ in range(2)]
    got = X.philox4x32(cs, ks)
    for i in range(50):
        assert tuple(int(w[i]) for w in got) == EC.philox4x32_10([c[i] for c in cs], [k[i] for k in ks])


@pytest.mark.parametrize("case", EC.CASES)
def test_expose_average_equals_the_restatement(case):
    """Per sample and blurry slot: the exposure's frames cropped and flipped as the loader does, then expose_average."""
    from bin_amd.data import exposure as X
    hw, crop, gamma, noise, content = EC.split(case)
    rows, codes = EC.reference(case)
    frames, t = EC.arena(content, hw), X.curve_tables(gamma, noise)
    for b, row in enumerate(rows.tolist()):
        y0, x0, flip, h, k0, k1 = row[EC.N_SLOTS:]
        for s in range(EC.N_BLUR):
            stack = frames[row[s] - h:row[s] + h + 1, y0:y0 + crop[0], x0:x0 + crop[1]]
            got = X.expose_average(stack[:, :, ::-1] if flip else stack, t, (k0, k1), s)
            assert got.dtype == np.uint8 and np.array_equal(got[:, :, ::-1].transpose(2, 0, 1), codes[s, b]), (b, s)
    if content in ("zeros", "full") and noise is None:
        assert (codes == (0 if content == "zeros" else 255)).all()


@pytest.mark.parametrize("gamma", [2.2, "srgb"])
@pytest.mark.parametrize("length", [3, 11, 33])
def test_against_the_real_number_formula_in_float64(gamma, length):
    """round(255 enc(mean(dec(v / 255)))) in float64.  Elements whose float64 value lies within 0.01 of a half-integer are left
    out (their share at most 2.5 %); of the rest not one may differ."""
    from bin_amd.data import exposure as X
    n = 200_000
    g = np.random.Generator(np.random.PCG64(length))
    base = g.integers(0, 256, n)
    kinds = {"uniform": g.integers(0, 256, (length, n)), "shadows": g.integers(0, 12, (length, n)),
             "jitter": np.clip(base[None, :] + g.integers(-20, 21, (length, n)), 0, 255)}
    dec = np.array([EC.dec(gamma, v / 255) for v in range(256)])
    if gamma == "srgb":
        enc = lambda x: np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.maximum(x, 1e-30) ** (1 / 2.4) - 0.055)
    else:
        enc = lambda x: x ** (1.0 / gamma)
    t = X.curve_tables(gamma)
    for kind, codes in kinds.items():
        real = 255.0 * enc(dec[codes].mean(axis=0))
        near = np.abs(real - np.floor(real) - 0.5) < 0.01
        got = X.expose_average(codes.astype(np.uint8)[:, None, :, None], t)[0, :, 0]
        share, wrong = near.mean(), int((got[~near] != np.rint(real[~near])).sum())
        print(f"gamma {gamma} L {length} {kind}: {100 * share:.2f} % within 0.01 of a half-integer, {wrong} of the rest differ")
        assert share <= 0.025, (kind, share)
        assert wrong == 0, (kind, wrong)


@pytest.mark.parametrize("k", [0, 128, 255])
def test_noise_integer_on_a_flat_field(k):
    """12 288 samples of n in linear bin k: mean within 4 standard errors of 0, deviation within 3 % of sigma * ONE (about 4.7
    standard errors of a sample deviation at that count, plus the rounding of SIG)."""
    from bin_amd.data import exposure as X
    read, shot = 0.01, 0.002
    sig = X.curve_tables(2.2, (read, shot))[2]
    m = np.full((64, 64, 3), (k << 16) + 0x8000, np.int64)
    n = X.noise_field(sig, m, (0x1234ABCD, 77 + k), 2, (2, 1, 0)).astype(np.float64)
    assert n.size == 12288
    sigma = np.sqrt(read * read + shot * (k + 0.5) / 256) * EC.ONE
    print(f"bin {k}: mean {n.mean():.1f} (standard error {sigma / np.sqrt(n.size):.1f}), deviation {n.std():.1f} of {sigma:.1f}")
    assert abs(n.mean()) <= 4 * sigma / np.sqrt(n.size)
    assert abs(n.std() / sigma - 1) <= 0.03
    # the field is the restatement's, element for element
    lin, mid, sg = EC.tables(2.2, (read, shot))
    for y, x, j in ((0, 0, 0), (63, 63, 2), (5, 40, 1)):
        assert int(n[y, x, j]) == EC.noise_int(sg, int(m[y, x, j]), x, y, 2, (2, 1, 0)[j], (0x1234ABCD, 77 + k))


def test_sample_key_draws_only_in_training_and_only_with_noise():
    from bin_amd.data import exposure as X
    random.seed(3)
    before = random.getstate()
    assert X.sample_key(X.Exposure(2.2, None), True, 5) == (0, 0) and random.getstate() == before
    assert X.sample_key(X.Exposure(2.2, (0.01, 0.001)), False, 5) == (0x9E3779B9, 5) and random.getstate() == before
    k0, k1 = X.sample_key(X.Exposure(2.2, (0.01, 0.001)), True, 5)
    random.setstate(before)
    r = random.getrandbits(64)
    assert (k0, k1) == (r & 0xFFFFFFFF, r >> 32)


# ------------------------------------------------------------------------------------------------ the library's bookkeeping
def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def test_header_binding_and_dynamic_symbols_agree():
    from bin_amd import _lib, build
    name, want = "binexpose", ["binexpose_version", "binexpose_check_curve", "binexpose_gather"]
    assert [row.name for row in build.EXTRA_LIBRARIES] == [name] and list(_lib._EXTRA_LIBRARIES) == [name]
    assert name not in build.BY_NAME and name not in _lib._LIBRARIES and len(build.LIBRARIES) == 11
    lib = build.EXTRA_BY_NAME[name]
    hdr = open(lib.header).read()
    declared = build.abi_symbols(name)
    assert lib.sources == ["binexpose.hip"] and lib.subdir == "extra" and lib.purpose and "\n" not in lib.purpose
    assert lib.path == os.path.join(build.CSRC, "extra", "libbinexpose.so") and lib.header == os.path.join(REPO, "include", "binexpose.h")
    assert declared == want
    assert set(_lib.exported_symbols(name)) == set(declared) == _defined(lib.path)
    assert set(re.findall(rf"\b({name}_[a-z0-9_]+)\s*\(", hdr)) == set(declared)
    assert all(m.startswith("BINEXPOSE_") for m in re.findall(r"#\s*define\s+(\w+)", hdr))
    assert re.findall(r'(?m)^\s*#\s*include\s+"(\w+\.h)"', hdr) == [], "no other project header"
    assert re.findall(r"(?m)^\s*#\s*(?:if|ifdef|ifndef|elif)\b\s*(.*)$", hdr) == ["__cplusplus", "__cplusplus"]
    version = int(re.search(r"#define\s+BINEXPOSE_VERSION\s+(\d+)", hdr).group(1))
    assert _lib.library(name).binexpose_version() == version == _lib._EXTRA_LIBRARIES[name][1] == 100
    assert (int(re.search(r"#define\s+BINEXPOSE_E_ARG\s+\((-\d+)\)", hdr).group(1)),
            int(re.search(r"#define\s+BINEXPOSE_E_SHAPE\s+\((-\d+)\)", hdr).group(1))) == (_lib.EXPOSE_E_ARG, _lib.EXPOSE_E_SHAPE) == (-1, -2)
    # the source is one folder down: the top level of bin_amd/csrc/ holds the eleven core libraries' sources only
    assert "binexpose.hip" not in os.listdir(build.CSRC) and os.path.exists(os.path.join(build.CSRC, "extra", "binexpose.hip"))
    built = ["bin_amd/csrc/extra/libbinexpose.so", "bin_amd/csrc/extra/binhip_exports.binexpose.map", "bin_amd/csrc/extra/binexpose.o"]
    ignored = subprocess.run(["git", "check-ignore"] + built, cwd=REPO, capture_output=True, text=True)
    if ignored.returncode != 128:                                 # (128: not a git checkout)
        assert len(ignored.stdout.split()) == len(built), "the built files stay out of git"
    # the shared window load is one header, included by both sources
    for src in ("binhip_data.hip", os.path.join("extra", "binexpose.hip")):
        text = open(os.path.join(build.CSRC, src)).read()
        assert "binhip_gather_load.h" in text and "void gw_load12" not in text


def test_plans_core_links_eleven_and_the_extra_plan_has_the_core_flags():
    from bin_amd import build
    compiles, links = build.build_plan()
    assert len(links) == 11 and not any("binexpose" in " ".join(c) for c in compiles + [l[2] for l in links])
    compiles, links = build.build_plan(table=build.EXTRA_LIBRARIES)
    extra = os.path.join(build.CSRC, "extra")
    (cmd,), ((vmap, names, link),) = compiles, links
    hipcc = build.build_plan()[0][0][0]
    assert cmd == [hipcc] + FLAGS + ["-c", os.path.join(extra, "binexpose.hip"), "-o", os.path.join(extra, "binexpose.o")]
    assert vmap == os.path.join(extra, "binhip_exports.binexpose.map") and names == build.abi_symbols("binexpose")
    assert link == [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}", "-o",
                    os.path.join(extra, "libbinexpose.so"), os.path.join(extra, "binexpose.o")]
    core = build.build_plan()
    assert cmd[1:6] == core[0][0][1:6] == FLAGS and link[1:5] == core[1][1][2][1:5], "the same flags as the core rows"
    assert link[5].startswith("-Wl,--version-script=") and core[1][1][2][5].startswith("-Wl,--version-script=") and link[5] != core[1][1][2][5]


def test_a_build_is_stale_when_the_extra_library_is_missing_or_older_than_its_source(monkeypatch):
    from bin_amd import build
    lib = build.EXTRA_BY_NAME["binexpose"]
    times, missing = {}, set()
    monkeypatch.setattr(os.path, "getmtime", lambda p: times.get(p, 100.0))
    monkeypatch.setattr(os.path, "exists", lambda p: p not in missing)
    fresh = {row.path: 200.0 for row in build.LIBRARIES + build.EXTRA_LIBRARIES}
    times.update(fresh)
    assert build._stale() is False
    for newer in (os.path.join(build.CSRC, "extra", "binexpose.hip"), lib.header, os.path.join(build.CSRC, "binhip_gather_load.h")):
        times.update(fresh)
        times.update({lib.path: 150.0, newer: 160.0})
        assert build._stale() is True, newer
        times[newer] = 100.0
        assert build._stale() is False
    missing.add(lib.path)
    assert build._stale() is True


def test_driver_loads_the_extra_table_and_checks_its_symbols(monkeypatch):
    import __graft_entry__ as entry
    from bin_amd import _lib, build
    assert "binexpose" not in entry.load_libraries()
    loaded = entry.load_libraries(build.EXTRA_LIBRARIES)
    assert list(loaded) == ["binexpose"] and loaded["binexpose"] is _lib.library("binexpose")
    real = _lib.exported_symbols
    monkeypatch.setattr(_lib, "exported_symbols", lambda n="binhip": real(n) + (["binexpose_absent"] if n == "binexpose" else []))
    with pytest.raises(RuntimeError, match=r"libbinexpose\.so is missing symbols: \['binexpose_absent'\]"):
        entry.load_libraries(build.EXTRA_LIBRARIES)
    monkeypatch.setattr(_lib, "exported_symbols", real)
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setitem(_lib._EXTRA_LIBRARIES, "binexpose", (_lib._EXPOSE_SIGNATURES, 101))
    with pytest.raises(RuntimeError, match=r"libbinexpose\.so is version 100, this binding is for 101"):
        _lib.library("binexpose")


# ------------------------------------------------------------------------------------------------ refusals of the entry point
def test_gather_refusals_return_their_code_without_a_device():
    """Every refusal comes before any HIP call, so it needs no GPU: the pointers are never followed."""
    from bin_amd import _lib
    fn = _lib.library("binexpose").binexpose_gather
    p = C.c_void_p(0x1000)
    good = dict(frames=p, n_frames=40, H=24, W=36, table=p, n=3, n_slots=17, n_blur=6, ch=8, cw=16, curve=p, out=p, stream=None)

    def call(**kw):
        a = dict(good, **kw)
        return fn(a["frames"], a["n_frames"], a["H"], a["W"], a["table"], a["n"], a["n_slots"], a["n_blur"], a["ch"], a["cw"], a["curve"],
                  a["out"], a["stream"])

    for ptr in ("frames", "table", "curve", "out"):
        assert call(**{ptr: None}) == -1, ptr                                     # BINEXPOSE_E_ARG
    for size in ("n_frames", "H", "W", "n", "ch", "cw", "n_slots"):
        for v in (0, -1):
            assert call(**{size: v}) == -2, (size, v)                             # BINEXPOSE_E_SHAPE
    assert call(n_slots=33) == -2
    assert call(ch=25) == -2 and call(cw=37) == -2                                # crop larger than the frame
    assert call(n_blur=-1) == -2 and call(n_blur=18) == -2
    big = 2 ** 31 - 1
    assert call(n=big) == -2                                                      # 17 * n alone is beyond 2^31 - 1
    assert call(n_slots=1, n_blur=1, n=2 ** 20, H=2 ** 12, ch=2 ** 12, W=4, cw=4) == -2      # 2^32 items
    assert call(n_slots=32, n_blur=0, n=big, H=big, W=big, ch=big, cw=big) == -2  # the product of the four passes 2^63
    assert call(frames=None, n=0) == -1                                           # a null pointer is named first


# ------------------------------------------------------------------------------------------------ absent options
@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return EC.make_toy_tree(str(tmp_path_factory.mktemp("toy")), clips=(("clipA", 1, 64),))


def _dataset(root, **extra):
    from bin_amd.data import create_dataset
    random.seed(0)
    return create_dataset(dict({"mode": "BIN", "name": "train", "dataroot_GT": root, "dataroot_LQ": root, "LQ_size": [3, 16, 24],
                                "data_type": "img", "phase": "train", "blur_window": 5}, **extra))


class _FakeCache:
    shape, frames, clip_ranges = (64, 352, 640, 3), object(), None

    def table(self, windows, draws, halves=None, keys=None):
        return ("table", len(windows), halves, keys)


def test_absent_options_never_touch_the_module(toy, monkeypatch):
    import bin_amd.data
    from bin_amd import ops
    from bin_amd.data.device_cache import DeviceWindowLoader
    monkeypatch.delitem(sys.modules, "bin_amd.data.exposure", raising=False)
    monkeypatch.delattr(bin_amd.data, "exposure", raising=False)
    calls = []
    monkeypatch.setattr(ops, "gather_windows_blur", lambda frames, table, crop, n_blur, clips=None:
                        calls.append(("blur", table)) or torch.zeros((17, table[1], 3) + tuple(crop)))
    monkeypatch.setattr(ops, "gather_windows_exposed", lambda *a, **k: calls.append(("exposed",)))
    monkeypatch.setattr(ops, "exposure_curve", lambda *a, **k: calls.append(("curve",)))
    ds = _dataset(toy)
    assert ds.exposure is None and len(ds) == 1
    random.seed(9)
    sample = ds[0]
    after_host = random.getstate()
    assert sample["LQs"].shape == (6, 3, 16, 24)
    dev = DeviceWindowLoader(ds, 1, cache=_FakeCache())
    random.seed(9)
    batch = next(iter(dev))
    assert random.getstate() == after_host, "the draws of an existing configuration are untouched"
    assert batch["LQs"].shape == (1, 6, 3, 16, 24)
    assert calls == [("blur", ("table", 1, [2], None))]
    assert "bin_amd.data.exposure" not in sys.modules


def test_set_options_draw_the_key_after_the_exposure_and_call_the_exposed_gather(toy, monkeypatch):
    """The device loader's side without a device: which ops function is called, with which table columns and draws."""
    from bin_amd import ops
    from bin_amd.data import exposure as X
    from bin_amd.data.BIN_dataset import draw_blur_half, draw_window_aug
    from bin_amd.data.device_cache import DeviceWindowLoader
    calls = []
    monkeypatch.setattr(ops, "gather_windows_blur", lambda *a, **k: calls.append(("blur",)))
    monkeypatch.setattr(ops, "gather_windows_exposed", lambda frames, table, crop, n_blur, curve, clips=None:
                        calls.append(("exposed", table, curve)) or torch.zeros((17, table[1], 3) + tuple(crop)))
    for phase, noise in (("train", [0.01, 0.002]), ("val", [0.01, 0.002]), ("train", None)):
        ds = _dataset(toy, blur_window=[3, 5], blur_gamma="srgb", blur_noise=noise, phase=phase)
        assert ds.exposure == X.Exposure("srgb", None if noise is None else (0.01, 0.002))
        del calls[:]
        random.seed(21)
        next(iter(DeviceWindowLoader(ds, 1, cache=_FakeCache())))
        after = random.getstate()
        random.seed(21)
        draw_window_aug((3, 16, 24))
        h = draw_blur_half((3, 5))
        r = random.getrandbits(64) if phase == "train" and noise is not None else None
        assert random.getstate() == after
        key = (0, 0) if noise is None else (r & 0xFFFFFFFF, r >> 32) if phase == "train" else (0x9E3779B9, 0)
        (what, table, curve), = calls
        assert what == "exposed" and table == ("table", 1, [h], [key])
        assert np.array_equal(curve, X.curve_tables("srgb", ds.exposure.noise))


def test_window_table_carries_the_key_bits():
    from bin_amd.data.device_cache import window_table
    paths = [f"p{i}" for i in range(17)]
    index = {p: i for i, p in enumerate(paths)}
    win = [paths[0:6], paths[6:12], paths[12:17], "k"]
    rows = window_table([win, win], [(False, 1, 2, True), (True, 3, 4, False)], index, [5, 0], [(0xFFFFFFFF, 7), (1, 0x80000000)])
    assert rows.dtype == np.int32 and rows.shape == (2, 23)
    assert rows[:, 17:21].tolist() == [[1, 2, 1, 5], [3, 4, 0, 0]]
    assert rows[:, 21:].view(np.uint32).tolist() == [[0xFFFFFFFF, 7], [1, 0x80000000]]
    assert np.array_equal(rows[:, :21], window_table([win, win], [(False, 1, 2, True), (True, 3, 4, False)], index, [5, 0]))


# ------------------------------------------------------------------------------------------------ the tool
def test_make_blur_folder_gamma_writes_expose_average_and_without_it_todays_bytes(tmp_path):
    from bin_amd.data import exposure as X
    from bin_amd.data.BIN_dataset import blur_average
    from bin_amd.data.util import imread_u8
    clips = (("clipA", 1, 24), ("clipB", 3, 26), ("clipC", 0, 33))                # one, one and two blurry centres
    roots = [EC.make_toy_tree(str(tmp_path / name), mode="test", clips=clips, hw=(6, 9)) for name in ("plain", "gamma", "noisy")]
    tool = os.path.join(REPO, "tools", "make_blur_folder.py")
    sys.path.insert(0, os.path.dirname(tool))
    try:
        import make_blur_folder as T
    finally:
        sys.path.pop(0)
    T.make_blur_folder(roots[0], "test", 5)
    subprocess.run([sys.executable, tool, "--root", roots[1], "--mode", "test", "--window", "5", "--gamma", "2.2"], check=True,
                   capture_output=True)                                           # the command line once; the rest in this process
    assert (T.parse_gamma_flag("srgb"), T.parse_gamma_flag("2.2"), T.parse_noise_flag("0.01,0.002")) == ("srgb", 2.2, [0.01, 0.002])
    T.make_blur_folder(roots[2], "test", 5, T.parse_gamma_flag("srgb"), T.parse_noise_flag("0.01,0.002"), 9)
    count = 0
    for clip, first, n in clips:
        for c in [first + 16 + 8 * i for i in range(n // 8 - 2)]:
            stack = [imread_u8(os.path.join(roots[0], "test", clip, f"{k:05d}.png")) for k in range(c - 2, c + 3)]
            name = os.path.join("test_blur", clip, f"{c:05d}.png")
            assert np.array_equal(imread_u8(os.path.join(roots[0], name)), blur_average(stack))
            assert np.array_equal(imread_u8(os.path.join(roots[1], name)), X.expose_average(stack, X.curve_tables(2.2)))
            noisy = X.expose_average(stack, X.curve_tables("srgb", (0.01, 0.002)), (9, count))
            assert np.array_equal(imread_u8(os.path.join(roots[2], name)), noisy)
            assert not np.array_equal(noisy, X.expose_average(stack, X.curve_tables("srgb")))
            count += 1
    assert count == 4
    with pytest.raises(ValueError, match="^blur_noise: needs `blur_gamma`"):
        T.make_blur_folder(str(tmp_path / "none"), "test", 5, None, [0.01, 0.002])
    with pytest.raises(ValueError, match="--noise"):
        T.parse_noise_flag("a,b")
