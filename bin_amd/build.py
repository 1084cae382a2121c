"""Build recipe for the project's shared objects (hand-written HIP for gfx950, each behind a flat C ABI — include/<name>.h).

`hipcc --offload-arch=gfx950` cross-compiles without a GPU, so this runs in the build container; the
resulting .so files stay in-tree (git-ignored) and travel to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")


class Library(NamedTuple):
    """One shared object: bin_amd/csrc/lib<name>.so, made from `sources`, exporting exactly what include/<name>.h declares
    <NAME>_API.  Each is a library of its own, so that no other library's interface changes with it.  `subdir`: the folder under
    bin_amd/csrc/ that holds its sources and receives what is built from them (the core table's rows have none)."""
    name: str
    sources: list
    purpose: str
    subdir: str = ""

    @property
    def header(self):
        return os.path.join(os.path.dirname(HERE), "include", self.name + ".h")

    @property
    def path(self):
        return os.path.join(CSRC, self.subdir, f"lib{self.name}.so")


# every shared object, in build order: what drives the compile, the version script, the link and the binding (bin_amd/_lib.py)
LIBRARIES = (
    Library("binhip", ["binhip_conv.hip", "binhip_relayout.hip", "binhip_conv_x3.hip", "binhip_fused.hip", "binhip_fused_x3.hip",
                       "binhip_wgrad.hip", "binhip_layout.hip", "binhip_convlstm.hip", "binhip_loss.hip", "binhip_upnet_bwd.hip",
                       "binhip_plan.hip", "binhip_metrics.hip", "binhip_data.hip"],
            "the network: convolutions, ConvLSTM, losses, the RDN plans, metrics and the training batches"),
    Library("binopt", ["binopt_adam.hip"], "the optimizer: the multi-tensor Adam step (train.optimizer: hip)"),
    Library("bingrad", ["bingrad_norm.hip"], "the gradient guard: the global gradient norm, the clip and the bad-step flags"),
    Library("binema", ["binema_step.hip"], "the weight average: the exponential moving average of the weights (train.ema_decay)"),
    Library("binens", ["binens.hip"], "the self-ensemble: the orient and merge kernels of bin_amd/ensemble.py"),
    Library("binyuv", ["binyuv.hip"], "video: 8-bit planar YUV <-> padded fp32 frame, the kernels of bin_amd/video.py"),
    Library("binscene", ["binscene.hip"], "scenes: luma histogram and SAD of a frame pair, the kernel of bin_amd/scene.py"),
    Library("binchain", ["binchain.hip"],
            "chained passes: the fp32 hand-off between interpolation passes, the kernel of bin_amd/chain.py (--factor 4 | 8)"),
    Library("binrate", ["binrate.hip"],
            "frame rates: two fp32 frames mixed and converted to planar YUV in one launch, the kernel of bin_amd/rate.py (--output_rate)"),
    Library("binscore", ["binscore.hip"],
            "scores: the per-plane scores of one YUV payload against another, the kernel of bin_amd/score.py (--gt_video)"),
    Library("binclip", ["binclip.hip"],
            "clips: the Y4M payloads of a clip -> the uint8 BGR frames of the device frame cache (dataset mode BIN_video)"),
)
BY_NAME = {lib.name: lib for lib in LIBRARIES}
# the libraries beside the core table: the same rows, built, linked and bound by the same machinery, their sources one folder down
EXTRA_LIBRARIES = (
    Library("binexpose", ["binexpose.hip"],
            "exposures: the training batches with blurry inputs averaged in linear light, with sensor noise (blur_gamma, blur_noise)",
            "extra"),
)
EXTRA_BY_NAME = {lib.name: lib for lib in EXTRA_LIBRARIES}
# the open-ended table: a library added after those two joins it here (the same rows and machinery again), so neither of them moves
ADDON_LIBRARIES = (
    Library("binssim", ["binssim.hip"],
            "the structural term of the training criterion: SSIM of fp32 frames and its gradient, in double (pixel_criterion: cb+ssim)",
            "extra"),
    Library("binlap", ["binlap.hip"],
            "the multi-scale term of the training criterion: the Laplacian-pyramid loss of fp32 frames and its gradient, in double "
            "(pixel_criterion: cb+lap)",
            "extra"),
    Library("bincrop", ["bincrop.hip"],
            "crops: a batch's crops of the YUV payloads of a byte arena -> uint8 BGR, the per-batch decode of a device frame cache kept "
            "in YUV (device_cache_format: yuv)",
            "extra"),
)
ADDON_BY_NAME = {lib.name: lib for lib in ADDON_LIBRARIES}
SOURCES, HEADER, LIB_PATH = BY_NAME["binhip"].sources, BY_NAME["binhip"].header, BY_NAME["binhip"].path


def _declared(header, macro, prefix):
    """The entry points `header` declares (every `macro` declaration of a `prefix`_ name), in header order."""
    import re
    with open(header) as f:
        return re.findall(rf"(?m)^{macro}\s+[\w\s\*]+?\b({prefix}_\w+)\s*\(", f.read())


def abi_symbols(name="binhip"):
    """The entry points include/<name>.h declares (every <NAME>_API declaration), in header order."""
    return _declared(row(name).header, name.upper() + "_API", name)


def row(name):
    """The Library row of `name`, of any of the three tables."""
    for table in (BY_NAME, EXTRA_BY_NAME):
        if name in table:
            return table[name]
    return ADDON_BY_NAME[name]


def _stale():
    rows = LIBRARIES + EXTRA_LIBRARIES + ADDON_LIBRARIES
    libs = [lib.path for lib in rows]
    if not all(os.path.exists(p) for p in libs):
        return True
    t = min(os.path.getmtime(p) for p in libs)
    dirs = [CSRC] + sorted({os.path.join(CSRC, lib.subdir) for lib in rows if lib.subdir})
    deps = [os.path.join(d, f) for d in dirs for f in os.listdir(d) if f.endswith((".hip", ".h"))]
    deps += [lib.header for lib in rows]
    return any(os.path.getmtime(d) > t for d in deps)


def build_plan(defines=(), out=None, table=LIBRARIES):
    """What build_library(defines=, out=) runs for the rows of `table`, without running it: the compile commands (one hipcc per
    source), and per library to link its (version-script path, exported names, link command)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = CSRC if out is None else os.path.dirname(os.path.abspath(out))
    tag = "" if out is None else "." + os.path.splitext(os.path.basename(out))[0]
    libraries = [(lib, lib.path) for lib in table] if out is None else [(BY_NAME["binhip"], out)]
    compiles, links = [], []
    for lib, path in libraries:
        objs = [os.path.join(objdir, lib.subdir, src.replace(".hip", tag + ".o")) for src in lib.sources]
        for src, obj in zip(lib.sources, objs):
            compiles.append([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"] +
                            [f"-D{d}" for d in defines] + ["-c", os.path.join(CSRC, lib.subdir, src), "-o", obj])
        # Dynamic symbols = exactly the entry points the library's header declares (sources are compiled -fvisibility=hidden; the
        # version script also makes the host-side kernel handles hipcc emits with default visibility local).
        vmap = os.path.join(objdir, lib.subdir, "binhip_exports" + tag + ".map" if lib.name == "binhip" else f"binhip_exports.{lib.name}.map")
        names = abi_symbols(lib.name)
        if lib.name == "binhip" and any(d.startswith("BINHIP_TIMELINE") for d in defines):
            names.append("binhip_set_timeline")
        # -z defs: a kernel template the host pass silently failed to instantiate shows up as an undefined symbol HERE, not at dlopen
        links.append((vmap, names, [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}",
                                    "-o", path] + objs))
    return compiles, links


def build_library(force=False, verbose=True, defines=(), out=None, table=None):
    """Compile every HIP source for gfx950 into every library of `table`: of all three tables, LIBRARIES, EXTRA_LIBRARIES and
    ADDON_LIBRARIES, when none is given (bin_amd/csrc/lib<name>.so, bin_amd/csrc/extra/lib<name>.so).

    `defines` / `out`: the instrumentation side build of tools/wg_timeline.py (defines=("BINHIP_TIMELINE=1",), out=<path>:
    per-workgroup time stamps, which the product library does not contain): libbinhip.so alone, under another name.  The
    sources are compiled in parallel (one hipcc per file)."""
    if out is None and not force and not _stale():
        return LIB_PATH
    tables = [table] if table is not None else [LIBRARIES] if out is not None else [LIBRARIES, EXTRA_LIBRARIES, ADDON_LIBRARIES]
    compiles, links = [], []
    for rows in tables:
        c, l = build_plan(defines, out, rows)
        compiles += c
        links += l
    os.makedirs(CSRC if out is None else os.path.dirname(os.path.abspath(out)), exist_ok=True)
    procs = []
    for cmd in compiles:
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    for vmap, names, cmd in links:
        with open(vmap, "w") as f:
            f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in names) + "  local: *;\n};\n")
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return out or LIB_PATH


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB_PATH)
