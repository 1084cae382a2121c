"""CPU: the bookkeeping every shared object of bin_amd/build.py's table shares — header, binding and dynamic symbols agree, the
version gate, what the product build and the timeline side build compile and link (build.build_plan), when a build is stale, and
that the driver's build() loads all of them.  What is particular to one library stays in that library's own test file."""
import os
import re
import subprocess

import pytest

from bin_amd import _lib, build
from conftest import REPO

# name -> (sources, entry points in header order); binhip's entry points are counted against BINHIP_ABI_EXPORTS instead
EXPECTED = {
    "binhip": (build.SOURCES, None),
    "binopt": (["binopt_adam.hip"], ["binopt_version", "binopt_adam_step"]),
    "bingrad": (["bingrad_norm.hip"], ["bingrad_version", "bingrad_norm_workspace_bytes", "bingrad_norm", "bingrad_scale"]),
    "binema": (["binema_step.hip"], ["binema_version", "binema_step"]),
    "binens": (["binens.hip"], ["binens_version", "binens_orient", "binens_merge"]),
    "binyuv": (["binyuv.hip"], ["binyuv_version", "binyuv_to_frame", "binyuv_from_frame"]),
    "binscene": (["binscene.hip"], ["binscene_version", "binscene_luma_stats"]),
    "binchain": (["binchain.hip"], ["binchain_version", "binchain_reframe"]),
    "binrate": (["binrate.hip"], ["binrate_version", "binrate_blend_to_yuv"]),
    "binscore": (["binscore.hip"], ["binscore_version", "binscore_workspace_bytes", "binscore_planes"]),
    "binclip": (["binclip.hip"], ["binclip_version", "binclip_yuv_to_bgr"]),
}
NAMES = list(EXPECTED)
SMALL_VERSION = 100                                           # what every <NAME>_VERSION but binhip's is today
INCLUDES = {"binrate": ["binyuv.h"], "binclip": ["binyuv.h"]}   # the project headers a header includes; the others include none
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"]


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.strip()}


def _macro(hdr, name):
    return int(re.search(rf"#define\s+{name}\s+(\d+)", hdr).group(1))


# ------------------------------------------------------------------------------------------------ the table
def test_table_is_the_eleven_in_build_order_and_every_source_belongs_to_exactly_one():
    assert [lib.name for lib in build.LIBRARIES] == NAMES and list(build.BY_NAME) == NAMES
    assert (build.SOURCES, build.HEADER, build.LIB_PATH) == (build.LIBRARIES[0].sources, build.LIBRARIES[0].header, build.LIBRARIES[0].path)
    owned = [s for lib in build.LIBRARIES for s in lib.sources]
    assert len(owned) == len(set(owned)), "no source file belongs to two libraries"
    assert sorted(owned) == sorted(f for f in os.listdir(build.CSRC) if f.endswith(".hip")), "every .hip belongs to a library"
    assert len(build.SOURCES) == 13 and all(lib.purpose and "\n" not in lib.purpose for lib in build.LIBRARIES)
    assert list(_lib._LIBRARIES) == NAMES and _lib.LIB_PATH == build.LIB_PATH


# ------------------------------------------------------------------------------------------------ one library at a time
@pytest.mark.parametrize("name", NAMES)
def test_header_binding_and_dynamic_symbols_agree(name):
    """Each library's dynamic symbols are exactly its header's declarations, the binding's and nothing else; nothing of it shows in
    a library that came before it."""
    lib, (sources, want) = build.BY_NAME[name], EXPECTED[name]
    hdr = open(lib.header).read()
    declared = build.abi_symbols(name)
    assert lib.sources == sources
    assert (os.path.basename(lib.path), os.path.basename(lib.header)) == (f"lib{name}.so", f"{name}.h")
    assert declared and len(declared) == len(set(declared))
    assert declared == want if want else len(declared) == _macro(hdr, "BINHIP_ABI_EXPORTS")
    assert set(_lib.exported_symbols(name)) == set(declared) == _defined(lib.path)
    assert set(re.findall(rf"\b({name}_[a-z0-9_]+)\s*\(", hdr)) == set(declared)
    assert all(m.startswith(name.upper() + "_") for m in re.findall(r"#\s*define\s+(\w+)", hdr))
    assert re.findall(r'(?m)^\s*#\s*include\s+"(\w+\.h)"', hdr) == INCLUDES.get(name, [])
    for later in NAMES[NAMES.index(name) + 1:]:
        assert later not in hdr.lower(), f"{name}.h mentions {later}"
    # the version gate
    loaded, version = _lib.library(name), _lib._LIBRARIES[name][1]
    assert getattr(loaded, name + "_version")() == _macro(hdr, name.upper() + "_VERSION")
    if name != "binhip":
        switches = re.findall(r"(?m)^\s*#\s*(?:if|ifdef|ifndef|elif)\b\s*(.*)$", hdr)
        assert switches == ["__cplusplus", "__cplusplus"], "#pragma once: no include-guard macro, no switches"
        assert getattr(loaded, name + "_version")() == version == SMALL_VERSION
    built = [f"bin_amd/csrc/lib{name}.so", "bin_amd/csrc/binhip_exports.map" if name == "binhip" else f"bin_amd/csrc/binhip_exports.{name}.map"]
    built += ["bin_amd/csrc/" + s.replace(".hip", ".o") for s in lib.sources]
    ignored = subprocess.run(["git", "check-ignore"] + built, cwd=REPO, capture_output=True, text=True)
    if ignored.returncode != 128:                                 # (128: not a git checkout)
        assert len(ignored.stdout.split()) == len(built), "the built files stay out of git"


@pytest.mark.parametrize("name", NAMES)
def test_loader_refuses_another_version_and_a_missing_library(name, monkeypatch, tmp_path):
    signatures, version = _lib._LIBRARIES[name]
    monkeypatch.setattr(_lib, "_loaded", {})
    assert _lib.library(name) is _lib.library(name), "loaded once"
    assert (version is None) == (name == "binhip")
    if version is not None:
        monkeypatch.setattr(_lib, "_loaded", {})
        monkeypatch.setitem(_lib._LIBRARIES, name, (signatures, version + 1))
        with pytest.raises(RuntimeError, match=rf"lib{name}\.so is version {version}, this binding is for {version + 1}"):
            _lib.library(name)
        monkeypatch.setitem(_lib._LIBRARIES, name, (signatures, version))
    monkeypatch.setattr(_lib, "_loaded", {})
    monkeypatch.setenv("BIN_AMD_LIB", str(tmp_path / "absent.so"))    # honoured for binhip only; the hint names the built path
    if name != "binhip":
        assert _lib.library(name) is _lib._loaded.pop(name)
        monkeypatch.setattr(build, "CSRC", str(tmp_path))             # where Library.path looks
    with pytest.raises(RuntimeError, match=rf"HIP library \S*lib{name}\.so not built.*no CPU fallback"):
        _lib.library(name)


# ------------------------------------------------------------------------------------------------ the plans
def test_product_plan_compiles_every_source_once_and_links_eleven_libraries():
    compiles, links = build.build_plan()
    hipcc = compiles[0][0]
    sources = [s for lib in build.LIBRARIES for s in lib.sources]
    assert len(compiles) == len(sources) and len(links) == 11
    for cmd, s in zip(compiles, sources):
        obj = os.path.join(build.CSRC, s.replace(".hip", ".o"))
        assert cmd == [hipcc] + FLAGS + ["-c", os.path.join(build.CSRC, s), "-o", obj]
    for (vmap, names, cmd), lib in zip(links, build.LIBRARIES):
        assert vmap == os.path.join(build.CSRC, "binhip_exports.map" if lib.name == "binhip" else f"binhip_exports.{lib.name}.map")
        objs = [os.path.join(build.CSRC, s.replace(".hip", ".o")) for s in lib.sources]
        assert cmd == [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}", "-o", lib.path] + objs
        assert names == build.abi_symbols(lib.name)
    assert len({vmap for vmap, _, _ in links}) == 11, "each library its own version script"


def test_side_build_plan_makes_libbinhip_alone_with_tagged_objects_and_the_timeline_setter(tmp_path):
    out = str(tmp_path / "side" / "libbinhip_timeline.so")
    compiles, links = build.build_plan(("BINHIP_TIMELINE=1",), out)
    side = os.path.dirname(out)
    objs = [os.path.join(side, s.replace(".hip", ".libbinhip_timeline.o")) for s in build.SOURCES]
    assert [cmd[1:] for cmd in compiles] == [FLAGS + ["-DBINHIP_TIMELINE=1", "-c", os.path.join(build.CSRC, s), "-o", o]
                                             for s, o in zip(build.SOURCES, objs)] and len(compiles) == 13
    (vmap, names, cmd), = links
    assert vmap == os.path.join(side, "binhip_exports.libbinhip_timeline.map")
    assert cmd[1:] == ["--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}", "-o", out] + objs
    assert names == build.abi_symbols() + ["binhip_set_timeline"] and "binhip_set_timeline" not in build.build_plan()[1][0][1]
    text = " ".join(" ".join(c) for c in compiles + [cmd] + [names])
    assert not any(other in text for other in NAMES[1:]), "nothing of the other ten"
    assert not os.path.exists(side), "a plan writes nothing"


@pytest.mark.parametrize("name", NAMES)
def test_a_build_is_stale_when_any_library_is_missing_or_older_than_a_source_or_its_header(name, monkeypatch):
    lib = build.BY_NAME[name]
    times, missing = {}, set()
    monkeypatch.setattr(os.path, "getmtime", lambda p: times.get(p, 100.0))
    monkeypatch.setattr(os.path, "exists", lambda p: p not in missing)
    fresh = {row.path: 200.0 for row in build.LIBRARIES}
    times.update(fresh)
    assert build._stale() is False
    for newer in (os.path.join(build.CSRC, lib.sources[-1]), lib.header):
        times.update(fresh)
        times.update({lib.path: 150.0, newer: 160.0})
        assert build._stale() is True, newer
        times[newer] = 100.0
        assert build._stale() is False
    missing.add(lib.path)
    assert build._stale() is True


# ------------------------------------------------------------------------------------------------ the driver
def test_driver_loads_every_library_and_checks_every_bound_symbol(monkeypatch):
    import __graft_entry__ as entry
    loaded = entry.load_libraries()
    assert list(loaded) == NAMES and all(loaded[n] is _lib.library(n) for n in NAMES)
    real = _lib.exported_symbols
    for name in NAMES:
        monkeypatch.setattr(_lib, "exported_symbols", lambda n="binhip": real(n) + ([name + "_absent"] if n == name else []))
        with pytest.raises(RuntimeError, match=rf"lib{name}\.so is missing symbols: \['{name}_absent'\]"):
            entry.load_libraries()
