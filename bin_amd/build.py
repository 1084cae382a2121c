"""Build recipe for libbinhip.so (hand-written HIP for gfx950, flat C ABI — include/binhip.h).

`hipcc --offload-arch=gfx950` cross-compiles without a GPU, so this runs in the build container; the
resulting .so stays in-tree (git-ignored) and travels to the GPU box with the repo snapshot.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["binhip_conv.hip", "binhip_relayout.hip", "binhip_conv_x3.hip", "binhip_fused.hip", "binhip_fused_x3.hip", "binhip_wgrad.hip", "binhip_layout.hip",
           "binhip_convlstm.hip", "binhip_loss.hip", "binhip_upnet_bwd.hip", "binhip_plan.hip", "binhip_metrics.hip", "binhip_data.hip"]
LIB_PATH = os.path.join(CSRC, "libbinhip.so")
# the optimizer library (include/binopt.h): a shared object of its own, so that libbinhip.so's interface does not change with it
OPT_SOURCES = ["binopt_adam.hip"]
OPT_LIB_PATH = os.path.join(CSRC, "libbinopt.so")
OPT_HEADER = os.path.join(os.path.dirname(HERE), "include", "binopt.h")
# the gradient-guard library (include/bingrad.h): the global gradient norm, the clip and the bad-step flags; a third shared object, for
# the same reason
GRAD_SOURCES = ["bingrad_norm.hip"]
GRAD_LIB_PATH = os.path.join(CSRC, "libbingrad.so")
GRAD_HEADER = os.path.join(os.path.dirname(HERE), "include", "bingrad.h")
# the weight-average library (include/binema.h): the exponential moving average of the weights (train.ema_decay); a fourth shared
# object, for the same reason
EMA_SOURCES = ["binema_step.hip"]
EMA_LIB_PATH = os.path.join(CSRC, "libbinema.so")
EMA_HEADER = os.path.join(os.path.dirname(HERE), "include", "binema.h")
# the self-ensemble library (include/binens.h): the orient and merge kernels of bin_amd/ensemble.py; a fifth shared object, for the
# same reason
ENS_SOURCES = ["binens.hip"]
ENS_LIB_PATH = os.path.join(CSRC, "libbinens.so")
ENS_HEADER = os.path.join(os.path.dirname(HERE), "include", "binens.h")


# the video library (include/binyuv.h): 8-bit planar YUV <-> padded fp32 frame, the kernels of bin_amd/video.py; a sixth shared object,
# for the same reason
YUV_SOURCES = ["binyuv.hip"]
YUV_LIB_PATH = os.path.join(CSRC, "libbinyuv.so")
YUV_HEADER = os.path.join(os.path.dirname(HERE), "include", "binyuv.h")

# the scene library (include/binscene.h): luma histogram and SAD of a frame pair, the kernel of bin_amd/scene.py; a seventh shared
# object, for the same reason
SCENE_SOURCES = ["binscene.hip"]
SCENE_LIB_PATH = os.path.join(CSRC, "libbinscene.so")
SCENE_HEADER = os.path.join(os.path.dirname(HERE), "include", "binscene.h")

# the chain library (include/binchain.h): the fp32 hand-off between chained interpolation passes, the kernel of bin_amd/chain.py
# (--factor 4 | 8); an eighth shared object, for the same reason
CHAIN_SOURCES = ["binchain.hip"]
CHAIN_LIB_PATH = os.path.join(CSRC, "libbinchain.so")
CHAIN_HEADER = os.path.join(os.path.dirname(HERE), "include", "binchain.h")

# the rate library (include/binrate.h): two fp32 frames mixed and converted to planar YUV in one launch, the kernel of
# bin_amd/rate.py (--output_rate); a ninth shared object, for the same reason
RATE_SOURCES = ["binrate.hip"]
RATE_LIB_PATH = os.path.join(CSRC, "libbinrate.so")
RATE_HEADER = os.path.join(os.path.dirname(HERE), "include", "binrate.h")

# the score library (include/binscore.h): the per-plane scores of one YUV payload against another, the kernel of bin_amd/score.py
# (--gt_video); a tenth shared object, for the same reason
SCORE_SOURCES = ["binscore.hip"]
SCORE_LIB_PATH = os.path.join(CSRC, "libbinscore.so")
SCORE_HEADER = os.path.join(os.path.dirname(HERE), "include", "binscore.h")

# the clip library (include/binclip.h): the Y4M payloads of a clip -> the uint8 BGR frames of the device frame cache, the kernel of
# bin_amd/data/video_dataset.py (dataset mode BIN_video); an eleventh shared object, for the same reason
CLIP_SOURCES = ["binclip.hip"]
CLIP_LIB_PATH = os.path.join(CSRC, "libbinclip.so")
CLIP_HEADER = os.path.join(os.path.dirname(HERE), "include", "binclip.h")

HEADER = os.path.join(os.path.dirname(HERE), "include", "binhip.h")
# (name, sources, header, path) of every shared object: what drives the compile, the version script and the link
LIBRARIES = (("binhip", SOURCES, HEADER, LIB_PATH), ("binopt", OPT_SOURCES, OPT_HEADER, OPT_LIB_PATH),
             ("bingrad", GRAD_SOURCES, GRAD_HEADER, GRAD_LIB_PATH), ("binema", EMA_SOURCES, EMA_HEADER, EMA_LIB_PATH),
             ("binens", ENS_SOURCES, ENS_HEADER, ENS_LIB_PATH))
# the libraries of the input / output side (same tuple layout), built and checked for staleness with the ones above
IO_LIBRARIES = (("binyuv", YUV_SOURCES, YUV_HEADER, YUV_LIB_PATH),)
# the libraries that measure frames without changing them (same tuple layout), built and checked likewise
ANALYSIS_LIBRARIES = (("binscene", SCENE_SOURCES, SCENE_HEADER, SCENE_LIB_PATH),)
PRODUCT_LIBRARIES = LIBRARIES + IO_LIBRARIES + ANALYSIS_LIBRARIES
# the libraries of the chained passes (same tuple layout); ALL_LIBRARIES is what the product build makes and checks for staleness
CHAIN_LIBRARIES = (("binchain", CHAIN_SOURCES, CHAIN_HEADER, CHAIN_LIB_PATH),)
ALL_LIBRARIES = PRODUCT_LIBRARIES + CHAIN_LIBRARIES
# the libraries of the frame-rate resampler (same tuple layout), built and checked for staleness with ALL_LIBRARIES
RATE_LIBRARIES = (("binrate", RATE_SOURCES, RATE_HEADER, RATE_LIB_PATH),)
# the libraries that score a video run against its ground truth (same tuple layout), built and checked for staleness with them
SCORE_LIBRARIES = (("binscore", SCORE_SOURCES, SCORE_HEADER, SCORE_LIB_PATH),)
# the libraries that fill the training frame cache from video (same tuple layout), built and checked for staleness with them
CLIP_LIBRARIES = (("binclip", CLIP_SOURCES, CLIP_HEADER, CLIP_LIB_PATH),)


def _declared(header, macro, prefix):
    """The entry points `header` declares (every `macro` declaration of a `prefix`_ name), in header order."""
    import re
    with open(header) as f:
        return re.findall(rf"(?m)^{macro}\s+[\w\s\*]+?\b({prefix}_\w+)\s*\(", f.read())


def abi_symbols():
    """The entry points include/binhip.h declares (every BINHIP_API declaration), in header order."""
    return _declared(HEADER, "BINHIP_API", "binhip")


def opt_abi_symbols():
    """The entry points include/binopt.h declares (every BINOPT_API declaration), in header order."""
    return _declared(OPT_HEADER, "BINOPT_API", "binopt")


def grad_abi_symbols():
    """The entry points include/bingrad.h declares (every BINGRAD_API declaration), in header order."""
    return _declared(GRAD_HEADER, "BINGRAD_API", "bingrad")


def ema_abi_symbols():
    """The entry points include/binema.h declares (every BINEMA_API declaration), in header order."""
    return _declared(EMA_HEADER, "BINEMA_API", "binema")


def ens_abi_symbols():
    """The entry points include/binens.h declares (every BINENS_API declaration), in header order."""
    return _declared(ENS_HEADER, "BINENS_API", "binens")


def yuv_abi_symbols():
    """The entry points include/binyuv.h declares (every BINYUV_API declaration), in header order."""
    return _declared(YUV_HEADER, "BINYUV_API", "binyuv")


def scene_abi_symbols():
    """The entry points include/binscene.h declares (every BINSCENE_API declaration), in header order."""
    return _declared(SCENE_HEADER, "BINSCENE_API", "binscene")


def chain_abi_symbols():
    """The entry points include/binchain.h declares (every BINCHAIN_API declaration), in header order."""
    return _declared(CHAIN_HEADER, "BINCHAIN_API", "binchain")


def rate_abi_symbols():
    """The entry points include/binrate.h declares (every BINRATE_API declaration), in header order."""
    return _declared(RATE_HEADER, "BINRATE_API", "binrate")


def score_abi_symbols():
    """The entry points include/binscore.h declares (every BINSCORE_API declaration), in header order."""
    return _declared(SCORE_HEADER, "BINSCORE_API", "binscore")


def clip_abi_symbols():
    """The entry points include/binclip.h declares (every BINCLIP_API declaration), in header order."""
    return _declared(CLIP_HEADER, "BINCLIP_API", "binclip")


def _stale():
    libs = [path for _, _, _, path in ALL_LIBRARIES + RATE_LIBRARIES + SCORE_LIBRARIES + CLIP_LIBRARIES]
    if not all(os.path.exists(p) for p in libs):
        return True
    t = min(os.path.getmtime(p) for p in libs)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    deps += [header for _, _, header, _ in ALL_LIBRARIES + RATE_LIBRARIES + SCORE_LIBRARIES + CLIP_LIBRARIES]
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=True, defines=(), out=None):
    """Compile every HIP source for gfx950 into bin_amd/csrc/libbinhip.so (and, for the product build, the optimizer
    library bin_amd/csrc/libbinopt.so, the gradient-guard library bin_amd/csrc/libbingrad.so, the weight-average library
    bin_amd/csrc/libbinema.so, the self-ensemble library bin_amd/csrc/libbinens.so, the video library
    bin_amd/csrc/libbinyuv.so, the scene library bin_amd/csrc/libbinscene.so, the chain library bin_amd/csrc/libbinchain.so, the
    rate library bin_amd/csrc/libbinrate.so, the score library bin_amd/csrc/libbinscore.so and the clip library
    bin_amd/csrc/libbinclip.so beside it).

    `defines` / `out`: the instrumentation side build of tools/wg_timeline.py (defines=("BINHIP_TIMELINE=1",), out=<path>:
    per-workgroup time stamps, which the product library does not contain): libbinhip.so alone, under another name.  The
    sources are compiled in parallel (one hipcc per file)."""
    if out is None and not force and not _stale():
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = CSRC if out is None else os.path.dirname(os.path.abspath(out))
    os.makedirs(objdir, exist_ok=True)
    tag = "" if out is None else "." + os.path.splitext(os.path.basename(out))[0]
    libraries = ALL_LIBRARIES + RATE_LIBRARIES + SCORE_LIBRARIES + CLIP_LIBRARIES if out is None else (("binhip", SOURCES, HEADER, out),)
    procs, objs = [], {}
    for name, sources, _, _ in libraries:
        for src in sources:
            obj = os.path.join(objdir, src.replace(".hip", tag + ".o"))
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden"] + [f"-D{d}" for d in defines] + \
                  ["-c", os.path.join(CSRC, src), "-o", obj]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((cmd, subprocess.Popen(cmd)))
            objs.setdefault(name, []).append(obj)
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    for name, _, header, path in libraries:
        # Dynamic symbols = exactly the entry points the library's header declares (sources are compiled -fvisibility=hidden; the
        # version script also makes the host-side kernel handles hipcc emits with default visibility local).
        vmap = os.path.join(objdir, "binhip_exports" + tag + ".map" if name == "binhip" else f"binhip_exports.{name}.map")
        names = _declared(header, name.upper() + "_API", name)
        if name == "binhip" and any(d.startswith("BINHIP_TIMELINE") for d in defines):
            names.append("binhip_set_timeline")
        with open(vmap, "w") as f:
            f.write("{\n  global:\n" + "".join(f"    {n};\n" for n in names) + "  local: *;\n};\n")
        # -z defs: a kernel template the host pass silently failed to instantiate shows up as an undefined symbol HERE, not at dlopen
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-z,defs", f"-Wl,--version-script={vmap}",
               "-o", path] + objs[name]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return out or LIB_PATH


if __name__ == "__main__":
    build_library(force="--force" in sys.argv)
    print(LIB_PATH)
