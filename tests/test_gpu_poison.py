"""-m gpu: no result of an entry point depends on what its buffers held before the call, and no entry point writes outside the buffers
it is given.  Instrument: tests/poison.py (shown to be sensitive on the host by tests/test_cpu_poison.py).

Every case makes the same call three times on identical inputs, under `poisoned(byte)` for byte in poison.BYTES = (0x00, 0x47, 0xFF) with
the cached workspaces dropped (so that they are allocated again under the patch, guard bands included) or filled with the byte.  Across
the three runs every output must be the same bits (torch.equal on an integer view: NaNs compare too), the 0x00 run must be finite, the
status word clean after each run, at least one allocation must have gone through the patched names (two for rdn_forward: workspace and
output), and all guard bands must still hold 0xA5 when the context closes.  No tolerance and no reference: the float64 checks of the same
calls live in the other test files.  Each case prints its number of poisoned allocations and their bytes.

Not seen by this instrument: out-of-bounds READS (they leave no trace unless the value reaches a result) and writes further than
poison.GUARD = 256 bytes from a buffer.

Integer, flag and accumulated regions of the scratch buffers, read from the kernels and launchers BEFORE the first run (a poisoned word
used as an index, counter or flag before it is written would send a kernel out of bounds or into a spin):

  region                                   written by (same call, before any read)                 read by
  ---------------------------------------  ------------------------------------------------------  -----------------------------------
  RDB3 sync words: 32 reserved + 2 flag    hipMemsetAsync over all 32 + 2 T words in               conv_x3_rdbs_kernel's neighbour
  words per tile, behind the planes of     binhip_rdn_forward when PLAN_RDB3 applies (nterms 3,    waits: `!= epoch`, a BOUNDED spin
  rdn_plan.workspace (uint32)              stage-4 shape); phase p of tile t then stores epoch     (RDB3_SPIN_LIMIT -> STATUS_SYNC_
                                           = block + 1; untouched (and unread) otherwise           TIMEOUT), never an index
  BinSceneRecord (uint64 SAD + 64 uint32   hipMemsetAsync of the 264 bytes in                      the host, after the call; the kernel
  bins) of ops.luma_stats                  binscene_luma_stats, then atomicAdd per block           only adds
  ScorePartial slots (int64 sse, sad;      score_tile_kernel: one slot per workgroup, all eight    image_score_final_kernel /
  double g11[3], u7[3]) of ops._score_ws,  fields stored by plain stores (no accumulation)         binscore's final kernel: sums in a
  image_scores' and frame_scores' ws                                                               fixed order, no indexing by content
  raw [n, 4] int64 of image / frame        the final kernel writes the whole BinImageScore         torch copies into the float64 result
  scores
  wgrad partials (fp32) of the backward    bh_wgrad_partials: every split of every layer slot      bh_wgrad_reduce_batch (sums, scaled
  workspace and conv2d_bwd_weight's ws     (tests/test_gpu_wgrad.py pins this separately)          by inv_scale)
  sc[2] + 1024 amax partials (fp32) of     binhip_grad_scale: partials by the first launch, sc by  every gradient-plane store and the
  the backward workspace                   the second                                              wgrad reduce (values, not indices)
  up_dwr [n, 9, 12, 25, G0] and up_dbr     torch.zeros in autograd.py (state of the call, NOT      upnet_ring_wgrad_kernel writes the
  (accumulated over images on the host)    scratch): the 12 (variant, sub-pixel) pairs with ring   other 12 pairs; up_dwr.sum(0) reads
                                           pixels are written, the other 24 stay zero              all 36
  dw / db of _ConvLstmFn.backward          torch.zeros_like (state)                                binhip_convlstm_bwd accumulates
  grad-norm workspace (double partials)    bingrad_norm's first pass, one slot per workgroup       its final pass (fixed order)
  loss partials (fp32)                     the first launch of binhip_pixel_loss_fwd /             the second launch
                                           binhip_multi_loss_fwd, one per workgroup
  status words, grad record                torch.zeros at creation: state, left alone by poison_caches

There is no device-side counter, ticket or pointer in any scratch buffer (the only atomics in the sources are the status-word ORs, the
scene record's adds and LDS reductions), and every table of indices (gather_windows, the multi-tensor rows) is built on the host.  So
every entry point below runs under all three bytes."""
import ctypes as C
import zlib

import numpy as np
import pytest
import torch

import conv_cases as cc
from backward_cases import SET_FOR_K, restrict
from poison import BYTES, bits, poison_caches, poisoned

pytestmark = pytest.mark.gpu

PREFIX = {2: "model1.", 3: "model2.", 5: "model3."}


def _seed(*key):
    return zlib.crc32(repr(key).encode())


def _flat(res, prefix=""):
    """{name: tensor} of a nested result (tensors, CP planes, None, lists / tuples / dicts of those)."""
    from bin_amd import ops
    out = {}
    if res is None:
        return out
    if isinstance(res, torch.Tensor):
        out[prefix or "out"] = res
    elif isinstance(res, ops.CP):
        out[prefix + ".hi"] = res.hi
        if res.lo is not None:
            out[prefix + ".lo"] = res.lo
    elif isinstance(res, dict):
        for k, v in res.items():
            out.update(_flat(v, f"{prefix}.{k}" if prefix else str(k)))
    elif isinstance(res, (list, tuple)):
        for i, v in enumerate(res):
            out.update(_flat(v, f"{prefix}[{i}]"))
    else:
        raise TypeError(type(res))
    return out


def three_runs(label, call, min_count=1, owners=(), fill_caches=False, before=None, finite=True):
    """The check of the module docstring on `call()` (a nested result of device tensors).  `before(byte)`: run ahead of each poisoned
    call, outside the patch (the workspace-reuse case's larger call); `fill_caches`: fill the cached workspaces instead of dropping
    them.  Returns the 0x00 run's outputs on the host as integer views."""
    from bin_amd import ops
    runs, stats = [], []
    ops.check_status()
    for b in BYTES:
        if before is not None:
            before(b)
        torch.cuda.synchronize()
        filled = poison_caches(b, owners, release=not fill_caches)
        torch.cuda.synchronize()
        with poisoned(b) as rec:
            res = _flat(call())
            torch.cuda.synchronize()
        ops.check_status()
        runs.append({k: bits(v).cpu() for k, v in res.items()})
        if finite and b == 0:
            bad = [k for k, v in res.items() if v.dtype.is_floating_point and not bool(torch.isfinite(v).all())]
            assert not bad, f"{label}: the baseline run is not finite in {bad}"
        stats.append((rec.count, rec.nbytes, filled))
        del res, rec
    print(f"[poison] {label}: " + ", ".join(f"0x{b:02X}: {c} allocations, {n} bytes poisoned (+{f} cached)" for b, (c, n, f) in zip(BYTES, stats)))
    assert all(c >= min_count for c, _, _ in stats), (label, stats)
    assert runs[0], f"{label}: no outputs"
    for b, r in zip(BYTES[1:], runs[1:]):
        assert r.keys() == runs[0].keys()
        diff = [k for k in r if r[k].shape != runs[0][k].shape or not torch.equal(r[k], runs[0][k])]
        assert not diff, f"{label}: outputs differ between fill bytes 0x00 and 0x{b:02X} (they depend on uninitialised memory): {diff[:12]}"
    return runs[0]


def _frames(k, n, H, W, salt=0):
    gen = torch.Generator().manual_seed(_seed("poison", k, n, H, W, salt))
    ins = [torch.rand(n, 3, H, W, generator=gen) for _ in range(k)]
    gout = torch.randn(n, 3, H, W, generator=gen) * 1e-3
    return ins, gout


# ------------------------------------------------------------------------------------------------ 1. RDN forward
def _plan_flags():
    from bin_amd import _lib as L
    return {"0": 0, "no_fuse": L.PLAN_NO_FUSE, "keep_acts": L.PLAN_KEEP_ACTS, "rdb3": L.PLAN_RDB3, "fused_upnet": L.PLAN_FUSED_UPNET,
            "fused_upnet_fold": L.PLAN_FUSED_UPNET | L.PLAN_UPNET_FOLD}


FLAG_NAMES = ("0", "no_fuse", "keep_acts", "rdb3", "fused_upnet", "fused_upnet_fold")
FWD_SHAPES = ((2, 34, 66), (1, 2, 2))


@pytest.mark.parametrize("flag", FLAG_NAMES)
@pytest.mark.parametrize("nterms", [3, 1])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_rdn_forward(k, nterms, flag, canon_gpu):
    """rdn_forward without ws= and out=: the cached workspace (dropped, so allocated under the patch), the output and the kernel-layout
    weights of a fresh RdnWeights all start poisoned."""
    from bin_amd.rdn_plan import RdnWeights, rdn_forward
    flags = _plan_flags()[flag]
    for n, H, W in FWD_SHAPES:
        ins = [t.cuda() for t in _frames(k, n, H, W)[0]]

        def call():
            wts = RdnWeights(canon_gpu, k, nterms, prefix=PREFIX[k])
            return rdn_forward(wts, ins, flags=flags)
        three_runs(f"rdn_forward k={k} nterms={nterms} {flag} {n}x{H}x{W}", call, min_count=2)


@pytest.mark.parametrize("flag", ["0", "fused_upnet"])
@pytest.mark.parametrize("nterms", [3, 1])
def test_rdn_forward_into_the_callers_buffers(nterms, flag, canon_gpu):
    """ws= of exactly binhip_rdn_workspace_bytes and out=, both poisoned and guarded.  What the plan documents as untouched still holds
    the poison: the sync words without PLAN_RDB3, and with the fused UPNet the U planes (UPNet.0's shuffled output, never produced)."""
    from bin_amd import _lib as L
    from bin_amd.rdn_plan import STAGE4_SHAPE, RdnWeights, c_shape, rdn_forward
    k, (n, H, W) = 3, FWD_SHAPES[0]
    flags = _plan_flags()[flag]
    ins = [t.cuda() for t in _frames(k, n, H, W)[0]]
    lib = L.lib()
    shape = c_shape(STAGE4_SHAPE)
    nbytes = lib.binhip_rdn_workspace_bytes(n, H, W, k, nterms, C.byref(shape))
    lay = (C.c_int64 * L.RDN_LAYOUT_WORDS)()
    assert lib.binhip_rdn_workspace_layout(n, H, W, k, nterms, C.byref(shape), lay, L.RDN_LAYOUT_WORDS) == 0
    u_off, u_size = int(lay[13]), int(lay[14]) * (2 if nterms == 3 else 1)            # fp16 elements from the 256-byte aligned base
    wts = RdnWeights(canon_gpu, k, nterms, prefix=PREFIX[k])
    seen = []

    def call():
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        out = torch.empty((n, 3, H, W), dtype=torch.float32, device="cuda")
        y = rdn_forward(wts, ins, out=out, ws=ws, flags=flags)
        assert y is out
        base = (-ws.data_ptr()) % 256                                   # the library rounds the workspace up to 256 bytes
        end = 2 * (u_off + u_size)
        seen.append({"sync": ws[base + (end + 255) // 256 * 256:].cpu(), "u": ws[base + 2 * u_off: base + end].cpu()})
        return out
    three_runs(f"rdn_forward ws= out= nterms={nterms} {flag}", call, min_count=2)
    for b, s in zip(BYTES, seen):
        assert s["sync"].numel() >= 4 * 32 and bool((s["sync"] == b).all()), f"0x{b:02X}: the sync words were written without PLAN_RDB3"
        if flag == "fused_upnet":
            assert s["u"].numel() == 2 * u_size and bool((s["u"] == b).all()), f"0x{b:02X}: the U planes were written under the fused UPNet"
        elif b:
            assert not bool((s["u"] == b).all()), f"0x{b:02X}: the two-layer UPNet left its U planes unwritten"


def test_workspace_reuse_after_a_larger_call(canon_gpu):
    """One call at (1, 66, 130), then the cached workspace is filled with the byte and the probe at (2, 12, 14) runs in it: what the
    probe sees is poison where the larger call's planes lay."""
    from bin_amd import rdn_plan
    from bin_amd.rdn_plan import RdnWeights, rdn_forward
    k = 3
    for nterms in (3, 1):
        wts = RdnWeights(canon_gpu, k, nterms, prefix=PREFIX[k])
        big = [t.cuda() for t in _frames(k, 1, 66, 130)[0]]
        probe = [t.cuda() for t in _frames(k, 2, 12, 14)[0]]
        rdn_plan.release_workspaces()
        sizes = []

        def before(b):
            rdn_forward(wts, big)
            sizes.append(sum(t.numel() for t in rdn_plan._workspaces.values()))

        def call():
            y = rdn_forward(wts, probe)
            assert sum(t.numel() for t in rdn_plan._workspaces.values()) == sizes[-1], "the probe did not reuse the larger workspace"
            return y
        three_runs(f"workspace reuse nterms={nterms}", call, before=before, fill_caches=True)
        rdn_plan.release_workspaces()


# ------------------------------------------------------------------------------------------------ 2. RDN training
TRAIN_SHAPES = ((2, 12, 14), (1, 22, 38))


def _module(canon_cpu, k, mode, shape=None, weights=None):
    from bin_amd.models.archs import RDN as A
    from bin_amd.weights import rdn_param_shapes
    cls = {2: A.RDN_residual_interp_2_input, 3: A.RDN_residual_interp_2_1_input, 5: A.RDN_residual_interp_4_1_input}[k]
    if shape is None:
        mod = cls(G0=96, D=12)
        mod.load_state_dict({n: canon_cpu[f"{SET_FOR_K[k]}.{n}"] for n in rdn_param_shapes(k)})
    else:
        G0, D, Cc, G = shape
        mod = cls(G0=G0, D=D, C=Cc, G=G)
        mod.load_state_dict({nm: torch.from_numpy(v) for nm, v in weights.items()}, strict=True)
    mod = mod.cuda()
    mod.precision = "f16x3"
    mod.backward_precision = "f16" if mode == "mixed" else None
    return mod


def _train_call(make_module, ins, gout):
    """Forward and backward through a FRESH module (its kernel-layout weights are then built under the patch): the output, every
    parameter gradient and every frame gradient."""
    def call():
        mod = make_module()
        xs = [t.cuda().requires_grad_(True) for t in ins]
        y = mod(*xs)
        y.backward(gout.cuda())
        g = {n: p.grad for n, p in mod.named_parameters()}
        assert all(v is not None for v in g.values()) and all(x.grad is not None for x in xs)
        g.update({f"in{i}": x.grad for i, x in enumerate(xs)})
        g["y"] = y.detach()
        return g
    return call


@pytest.mark.parametrize("kind", ["full", "ring"])
@pytest.mark.parametrize("mode", ["f16x3", "mixed", "two_layer"])
@pytest.mark.parametrize("k", [2, 5])
def test_rdn_training(k, mode, kind, canon_cpu, monkeypatch):
    """All 132 parameter gradients and every frame gradient.  kind "ring": the upstream gradient restricted to the full-resolution border
    ring, so that the 24 (variant, sub-pixel) pairs of up_dwr that upnet_ring_wgrad_kernel leaves alone are what the operator's
    gradient consists of next to the 12 it writes."""
    if mode == "two_layer":
        monkeypatch.setenv("BIN_AMD_FUSED_UPNET_TRAIN", "0")
    else:
        monkeypatch.delenv("BIN_AMD_FUSED_UPNET_TRAIN", raising=False)
    for n, H, W in TRAIN_SHAPES:
        ins, gout = _frames(k, n, H, W)
        if kind == "ring":
            gout = restrict(gout, "ring")
        got = three_runs(f"rdn training k={k} {mode} {kind} {n}x{H}x{W}", _train_call(lambda: _module(canon_cpu, k, mode), ins, gout),
                         min_count=2)
        assert len(got) == 132 + k + 1
        assert bool(got["UPNet.2.weight"].any()) and bool(got["SFENet1.weight"].any())


# ------------------------------------------------------------------------------------------------ 3. general configurations
def _config_cases():
    """The SWEEP entry with the smallest G0 (then the smallest G and C), the one with the smallest G at the LARGEST G0 (so that the two
    differ), and the D = 20 corner."""
    from rdn_config_cases import CORNERS, SWEEP
    a = min(SWEEP, key=lambda t: (SWEEP[t][1][0], SWEEP[t][1][3], SWEEP[t][1][2]))
    b = min(SWEEP, key=lambda t: (SWEEP[t][1][3], -SWEEP[t][1][0], SWEEP[t][1][2]))
    assert a != b
    return {a: SWEEP[a], b: SWEEP[b], "d20_g032_c1_g32": CORNERS["d20_g032_c1_g32"][:5]}


@pytest.mark.parametrize("which", [0, 1, 2])
def test_general_configurations(which):
    from bin_amd.weights import general_rdn_weights
    tag, (k, shape, n, H, W) = list(_config_cases().items())[which]
    weights = general_rdn_weights(0, k, shape)
    ins, gout = _frames(k, n, H, W)
    for prec in ("f16x3", "f16"):
        def fwd():
            mod = _module(None, k, "f16x3", shape, weights)
            mod.precision = prec
            with torch.no_grad():
                return mod(*[t.cuda() for t in ins])
        three_runs(f"config {tag} {shape} forward {prec}", fwd, min_count=2)
    three_runs(f"config {tag} {shape} backward f16x3", _train_call(lambda: _module(None, k, "f16x3", shape, weights), ins, gout), min_count=2)


# ------------------------------------------------------------------------------------------------ 4. per-op convolutions and the tail
CONV_SHAPES = ((1, 17, 33), (2, 18, 44))
CONV_EVEN_SHAPES = ((1, 18, 34), (2, 18, 44))


@pytest.mark.parametrize("nterms", cc.NTERMS)
@pytest.mark.parametrize("tag", cc.TAGS)
def test_conv_case(tag, nterms):
    """Every dispatcher row of conv_cases.CASES with its output planes allocated by the wrapper (poisoned), not zero-filled.  The stores
    cover whole chunks (och_limit = ceil(cout / 16)), so the planes are compared in full: a pad lane of the last chunk is a function of
    the zero weight rows and zero bias the relayout wrote, not of what the buffer held."""
    case = cc.BY_TAG[tag]
    for shape in (CONV_EVEN_SHAPES if case.opts.get("y_unshuf") else CONV_SHAPES):
        opnd = cc.white_noise_operands(case, shape)
        three_runs(f"conv {tag} nterms={nterms} {shape}", lambda: cc.call_library(case, nterms, shape, opnd, zero_fill=False)[0])


@pytest.mark.parametrize("nterms", cc.NTERMS)
def test_gff0_backward_data_leaves_the_gap_planes_alone(nterms):
    """conv2d_bwd_data with y_cpg / y_group_stride into the caller's poisoned, guarded planes: 12 groups of 6 chunks with one gap plane
    between groups (as tests/test_gpu_conv_float64.py lays them out); the gap planes still hold the poison byte afterwards."""
    import conv_ref_cases as rc
    from bin_amd import ops
    case = cc.BY_TAG[rc.SCATTER_TAG]
    cpg, ngroups = rc.SCATTER_CPG, rc.SCATTER_GROUPS
    shape = CONV_SHAPES[1]
    n, h, w = shape
    opnd = cc.white_noise_operands(case, shape)
    data = [g * (cpg + 1) + i for g in range(ngroups) for i in range(cpg)]
    gaps = [g * (cpg + 1) + cpg for g in range(ngroups)]
    seen = []

    def call():
        out = ops.CP.empty(ngroups * (cpg + 1), n, h, w, nterms, torch.device("cuda"))
        y = cc.call_library(case, nterms, shape, opnd, out=out, y_cpg=cpg, y_group_stride=(cpg + 1) * n * h * w * 16)[0]["y"]
        seen.append([p[gaps].view(torch.uint8).cpu() for p in (y.hi, y.lo) if p is not None])
        return {"hi": y.hi[data], "lo": None if y.lo is None else y.lo[data]}
    three_runs(f"gff0 scatter nterms={nterms}", call)
    for b, planes in zip(BYTES, seen):
        assert all(bool((p == b).all()) for p in planes), f"0x{b:02X}: a gap plane was written"


@pytest.mark.parametrize("nterms", cc.NTERMS)
@pytest.mark.parametrize("tag", ["p3_32", "p5_sfe1_24", "p1_96_lff"])
def test_conv_leaves_the_planes_beyond_cout_alone(tag, nterms):
    """The caller's poisoned, guarded output planes with one chunk more than ceil(cout / 16): the stores stop at och_limit, so the
    extra plane still holds the poison byte (BLK's layout relies on it: the next conv's planes lie right behind)."""
    from bin_amd import ops
    case = cc.BY_TAG[tag]
    nch = cc.chunks(case.cout)
    shape = CONV_SHAPES[1]
    n, h, w = shape
    opnd = cc.white_noise_operands(case, shape)
    seen = []

    def call():
        out = ops.CP.empty(nch + 1, n, h, w, nterms, torch.device("cuda"), case.cout)
        y = cc.call_library(case, nterms, shape, opnd, out=out)[0]["y"]
        seen.append([p[nch].view(torch.uint8).cpu() for p in (y.hi, y.lo) if p is not None])
        return y.sub(0, nch)
    three_runs(f"conv {tag} nterms={nterms}, one plane beyond cout", call)
    for b, planes in zip(BYTES, seen):
        assert all(bool((p == b).all()) for p in planes), f"0x{b:02X}: a plane beyond cout was written"


@pytest.mark.parametrize("nterms", cc.NTERMS)
def test_wgrad_and_tail_into_the_callers_buffers(nterms):
    """ops.conv2d_bwd_weight with workspace= of exactly binhip_wgrad_workspace_bytes and out=, and ops.rdb_tail with out=: all poisoned
    and guarded by the caller."""
    from bin_amd import _lib as L, ops
    n, h, w = CONV_SHAPES[1]
    gen = torch.Generator().manual_seed(_seed("wgrad", nterms))
    x = torch.randn(n, 96, h, w, generator=gen).cuda()
    gy = torch.randn(n, 32, h, w, generator=gen).cuda()
    need = L.lib().binhip_wgrad_workspace_bytes(3, n, h, w, 6, 32)

    def wgrad():
        xp, gp = ops.nchw_to_planes(x, nterms), ops.nchw_to_planes(gy, nterms)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        dw = torch.empty((32, 96, 3, 3), dtype=torch.float32, device="cuda")
        db = torch.empty((32,), dtype=torch.float32, device="cuda")
        return ops.conv2d_bwd_weight(xp, gp, 32, 96, 3, nterms, out=(dw, db), workspace=ws)
    three_runs(f"conv2d_bwd_weight workspace= out= nterms={nterms}", wgrad, min_count=5)
    three_runs(f"conv2d_bwd_weight nterms={nterms}",
               lambda: ops.conv2d_bwd_weight(ops.nchw_to_planes(x, nterms), ops.nchw_to_planes(gy, nterms), 32, 96, 3, nterms), min_count=5)
    case = cc.BY_TAG["tail_o3"]
    opnd = cc.white_noise_operands(case, (n, h, w))
    three_runs(f"rdb_tail out= nterms={nterms}",
               lambda: cc.call_library(case, nterms, (n, h, w), opnd, out=ops.CP.empty(6, n, h, w, nterms, torch.device("cuda"), 96))[0])


# ------------------------------------------------------------------------------------------------ 5. layout
@pytest.mark.parametrize("nterms", [3, 1])
def test_layout_kernels(nterms):
    from bin_amd import _lib as L, ops
    n, h, w = 2, 6, 10
    gen = torch.Generator().manual_seed(_seed("layout", nterms))
    for c in (24, 36, 60):
        x = torch.randn(n, c, h, w, generator=gen).cuda()
        got = three_runs(f"nchw_to_planes C={c} nterms={nterms}", lambda: ops.nchw_to_planes(x, nterms))
        for name, p in got.items():
            pad = p.view(-1, n, h, w, 16)[-1, ..., c % 16:]
            assert pad.numel() > 0 and bool((pad == 0).all()), f"nchw_to_planes C={c}: pad lanes of {name} are not zero"
        xp = ops.nchw_to_planes(x, nterms)
        three_runs(f"planes_to_nchw C={c} nterms={nterms}", lambda: ops.planes_to_nchw(xp, c))
    for k in (2, 3, 5):
        imgs = [torch.rand(n, 3, h, w, generator=gen).cuda() for _ in range(k)]
        got = three_runs(f"pack_inputs k={k} nterms={nterms}", lambda: ops.pack_inputs(imgs, nterms))
        lanes = (12 * k) % 16
        if lanes:
            for name, p in got.items():
                assert bool((p.view(-1, n, h // 2, w // 2, 16)[-1, ..., lanes:] == 0).all()), f"pack_inputs k={k}: pad lanes of {name}"
        # unpack_input_grads: the packed gradient planes back to k frame gradients (+ gout / k), outputs from torch.empty
        gp = ops.nchw_to_planes(torch.randn(n, ((12 * k + 31) // 32) * 32, h // 2, w // 2, generator=gen).cuda() * 8, nterms)
        gout = torch.randn(n, 3, h, w, generator=gen).cuda()
        sc = torch.tensor([128.0, 1.0 / 128.0], device="cuda")

        def unpack():
            outs = [torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda") for _ in range(k)]
            arr = (C.c_void_p * k)(*[o.data_ptr() for o in outs])
            L.check(L.lib().binhip_unpack_input_grads(ops._ptr(gp.hi), ops._ptr(gp.lo), ops._ptr(gout), ops._ptr(sc), k, n, h, w, arr,
                                                      ops._stream()), "unpack_input_grads")
            return outs
        three_runs(f"unpack_input_grads k={k} nterms={nterms}", unpack, min_count=k)
    src = ops.nchw_to_planes(torch.randn(n, 48, 2 * h, 2 * w, generator=gen).cuda(), nterms)

    def unshuffle():
        y = ops.CP.empty(12, n, h, w, nterms, torch.device("cuda"))
        L.check(L.lib().binhip_unshuffle_planes(ops._ptr(src.hi), ops._ptr(src.lo), n, h, w, 3, ops._ptr(y.hi), ops._ptr(y.lo), ops._stream()),
                "unshuffle_planes")
        return y
    three_runs(f"unshuffle_planes nterms={nterms}", unshuffle)
    if nterms == 3:
        xu = torch.randn(3, 17, 18, 30, generator=gen).cuda()
        for r in (2, 3):
            three_runs(f"pixel_unshuffle r={r}", lambda: ops.pixel_unshuffle(xu, r))


# ------------------------------------------------------------------------------------------------ 6. ConvLSTM
LSTM_SHAPES = ((2, 9, 65), (1, 16, 128))


@pytest.mark.parametrize("state", [False, True], ids=["nostate", "state"])
@pytest.mark.parametrize("nhw", LSTM_SHAPES, ids=["%dx%dx%d" % s for s in LSTM_SHAPES])
def test_convlstm(nhw, state):
    import lstm_cases as LC
    from bin_amd import autograd as ag, ops
    n, h, w = nhw
    case = LC.CASE_BY_TAG[LC._tag(n, h, w, state, 1.0, "moderate", "full")]
    inp = {k: (None if v is None else v.cuda()) for k, v in LC.make_inputs(case).items()}
    st = [inp["c0"], inp["h0"]] if state else None

    def cell():
        hn, (cn, _) = ops.convlstm_cell(inp["x"], st, inp["w"], inp["b"], case.fb)
        return {"h": hn, "c": cn}
    three_runs(f"convlstm_cell {case.tag}", cell, min_count=2)

    def apply():
        leaves = {k: inp[k].clone().requires_grad_(True) for k in ("x", "w", "b") + (("c0", "h0") if state else ())}
        hn, (cn, _) = ag.convlstm_apply(leaves["x"], [leaves["c0"], leaves["h0"]] if state else None, leaves["w"], leaves["b"], case.fb)
        torch.autograd.backward([hn, cn], [inp["gh"], inp["gc"]])
        out = {"h": hn.detach(), "c": cn.detach()}
        out.update({"g_" + k: v.grad for k, v in leaves.items()})
        return out
    three_runs(f"convlstm_apply {case.tag}", apply, min_count=3)


@pytest.mark.parametrize("hidden", [3, 16])
def test_lstm_gates(hidden):
    import lstm_cases as LC
    from bin_amd import ops
    gates, cp, gh, gc = (t.cuda() for t in LC.make_gates(hidden, "moderate"))
    for with_state in (False, True):
        c_prev = cp if with_state else None
        three_runs(f"lstm_gates hidden={hidden} state={with_state}", lambda: ops.lstm_gates(gates, c_prev, 1.0, hidden), min_count=2)
        three_runs(f"lstm_gates_grad hidden={hidden} state={with_state}",
                   lambda: ops.lstm_gates_grad(gates, c_prev, gh, gc, 1.0, hidden, with_state), min_count=1)


# ------------------------------------------------------------------------------------------------ 7. losses
@pytest.mark.parametrize("numel", [257, 1024 * 256 + 1])
def test_losses(numel):
    import loss_cases as LS
    from bin_amd import _lib as L, ops
    assert LS.FWD_CAP + 1 == 1024 * 256 + 1
    x, y = (t.cuda() for t in LS.make_xy(numel))
    gl = torch.tensor(LS.GLOSS, device="cuda")
    for kind in LS.KINDS:
        kid = LS.KIND_ID[kind]
        three_runs(f"pixel_loss {kind} numel={numel}", lambda: ops.pixel_loss(kid, x, y), min_count=2)
        three_runs(f"pixel_loss_grad {kind} numel={numel}", lambda: ops.pixel_loss_grad(kid, x, y, gl))
    ts = [t.cuda() for t in LS.make_multi(numel)]
    pairs, idx = LS.multi_pairs(17, ts)
    three_runs(f"multi_pixel_loss T=17 numel={numel}", lambda: ops.multi_pixel_loss(L.LOSS_CHARBONNIER, pairs), min_count=3)
    used = sorted({i for p in idx for i in p})
    wanted = [(ts[i], [(t, 1.0 if a == i else -1.0) for t, (a, b_) in enumerate(idx) if i in (a, b_)]) for i in used]

    def multi_grads():                   # (one launch writes at most BINHIP_LOSS_MAX_TERMS gradients)
        return [o for k0 in range(0, len(wanted), L.LOSS_MAX_TERMS)
                for o in ops.multi_pixel_loss_grad(L.LOSS_CHARBONNIER, pairs, gl, wanted[k0:k0 + L.LOSS_MAX_TERMS])]
    three_runs(f"multi_pixel_loss_grad T=17 numel={numel}", multi_grads, min_count=len(used))
    g = (torch.randn(1, 1, 1, numel, generator=torch.Generator().manual_seed(numel)) * 3e-4).cuda()
    for nterms in (3, 1):
        three_runs(f"grad_scale + scaled planes numel={numel} nterms={nterms}", lambda: ops.grad_planes(g, nterms), min_count=3)


# ------------------------------------------------------------------------------------------------ 8. scores
SCORE_SHAPES = ((12, 300), (17, 247))


@pytest.mark.parametrize("hw", SCORE_SHAPES, ids=["%dx%d" % s for s in SCORE_SHAPES])
def test_scores(hw):
    from bin_amd import ops
    h, w = hw
    rng = np.random.Generator(np.random.PCG64(_seed("scores", h, w)))
    a = torch.from_numpy(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)).cuda()
    b = torch.from_numpy(rng.integers(0, 256, (2, h, w, 3), dtype=np.uint8)).cuda()
    three_runs(f"image_scores {h}x{w}", lambda: ops.image_scores(a, b), min_count=3)
    xs = [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).cuda() for _ in range(3)]
    ys = [torch.from_numpy(rng.random((3, h, w), dtype=np.float32)).cuda() for _ in range(3)]
    three_runs(f"frame_scores {h}x{w}", lambda: ops.frame_scores(xs, ys), min_count=3)
    for chroma in (420, 444):
        nb = ops.yuv_frame_bytes(h, w, chroma)[0]
        pa = torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)).cuda()
        pb = torch.from_numpy(rng.integers(0, 256, nb, dtype=np.uint8)).cuda()
        # dropped: the workspace and the record are allocated under the patch; filled: the cached workspace starts poisoned
        three_runs(f"payload_scores {h}x{w} {chroma}", lambda: ops.payload_scores(pa, pb, h, w, chroma), min_count=2)
        three_runs(f"payload_scores {h}x{w} {chroma}, cached workspace", lambda: ops.payload_scores(pa, pb, h, w, chroma),
                   fill_caches=True)
        assert ops._score_ws
    cur = torch.from_numpy(rng.integers(0, 256, h * w, dtype=np.uint8)).cuda()
    prev = torch.from_numpy(rng.integers(0, 256, h * w, dtype=np.uint8)).cuda()
    three_runs(f"luma_stats {h}x{w}", lambda: ops.luma_stats(cur, prev, h, w))
    three_runs(f"luma_stats {h}x{w}, no previous plane", lambda: ops.luma_stats(cur, None, h, w))


# ------------------------------------------------------------------------------------------------ 9. video
def test_video_kernels():
    import video_cases as VC
    from bin_amd import _lib as L, ops
    h, w = 33, 130
    rng = np.random.Generator(np.random.PCG64(_seed("video")))
    img = torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).cuda()
    frame = torch.from_numpy(rng.random((1, 3, h + 5, w + 7), dtype=np.float32) * 1.2 - 0.1).cuda()
    other = torch.from_numpy(rng.random((1, 3, h + 5, w + 7), dtype=np.float32) * 1.2 - 0.1).cuda()
    three_runs("u8_to_frame", lambda: ops.u8_to_frame(img, (3, 5, 2, 7)))
    three_runs("frame_to_u8", lambda: ops.frame_to_u8(frame, 2, 3, h, w))
    for chroma in VC.CHROMAS:
        fmt = (chroma, "bt709", "limited")
        pay = torch.from_numpy(VC.random_payload(h, w, chroma, 3)).cuda()
        three_runs(f"yuv_to_frame {chroma}", lambda: ops.yuv_to_frame(pay, h, w, fmt, (1, 2, 3, 0)))
        three_runs(f"frame_to_yuv {chroma}", lambda: ops.frame_to_yuv(frame, 2, 3, h, w, fmt))
        three_runs(f"blend_to_yuv {chroma}", lambda: ops.blend_to_yuv(frame, other, 0.2, 2, 3, h, w, fmt))
        pays = torch.from_numpy(np.stack([VC.random_payload(h, w, chroma, s) for s in (4, 5, 6)])).cuda()
        three_runs(f"yuv_to_bgr {chroma}", lambda: ops.yuv_to_bgr(pays, h, w, fmt))
    batch = torch.from_numpy(rng.random((2, 3, h + 5, w + 7), dtype=np.float32) * 1.4 - 0.2).cuda()
    three_runs("reframe", lambda: ops.reframe([batch, batch.flip(0).contiguous()], 2, 3, h, w, (3, 5, 2, 7)), min_count=2)
    srcs = [torch.from_numpy(rng.random((1, 3, h, w), dtype=np.float32)).cuda() for _ in range(2)]
    flips = [[0, L.ENS_FLIP_W, L.ENS_FLIP_H, L.ENS_FLIP_W | L.ENS_FLIP_H]] * 2
    three_runs("ens_orient", lambda: ops.ens_orient(srcs, None, flips), min_count=8)
    outs = ops.ens_orient(srcs, None, flips)
    three_runs("ens_merge", lambda: ops.ens_merge(outs, flips[0]), min_count=2)


@pytest.mark.parametrize("cw", [5, 256])
def test_gather_windows(cw):
    from bin_amd import ops
    nf, H, W, ch = 9, 40, 300, 7
    rng = np.random.Generator(np.random.PCG64(_seed("gather", cw)))
    arena = torch.from_numpy(rng.integers(0, 256, (nf, H, W, 3), dtype=np.uint8)).cuda()
    n, slots = 3, 4
    tab = np.zeros((n, slots + 3), dtype=np.int32)
    tab[:, :slots] = rng.integers(2, nf - 2, (n, slots))
    tab[:, slots] = rng.integers(0, H - ch + 1, n)
    tab[:, slots + 1] = rng.integers(0, W - cw + 1, n)
    tab[:, slots + 2] = [0, 1, 1]
    three_runs(f"gather_windows cw={cw}", lambda: ops.gather_windows(arena, tab, (ch, cw)))
    tabb = np.concatenate([tab, np.array([[0], [1], [2]], dtype=np.int32)], axis=1)
    three_runs(f"gather_windows_blur cw={cw}", lambda: ops.gather_windows_blur(arena, tabb, (ch, cw), 2))


# ------------------------------------------------------------------------------------------------ 10. optimiser side
def test_optimiser_side():
    """One binopt Adam step, one EMA step and one grad-norm + scale over rows of 1, 2047 and 4097 elements at misaligned offsets
    (optim_cases' arenas, whose sentinels between the rows must survive); the grad-norm workspace starts poisoned."""
    import optim_cases as OC
    from bin_amd import ops
    from bin_amd.optim import GradGuard
    rows = OC._rows((1, 2047, 4097))
    assert any(any(r.offs) for r in rows)
    rng = np.random.Generator(np.random.PCG64(7))
    vals = {k: [(rng.standard_normal(r.numel) * s).astype(np.float32) for r in rows] for k, s in (("p", 0.1), ("g", 1e-2), ("m", 1e-3), ("e", 0.1))}
    vals["v"] = [np.abs(rng.standard_normal(r.numel) * 1e-4).astype(np.float32) for r in rows]
    kind = {"p": 0, "g": 1, "m": 2, "v": 3, "e": 0}

    def call():
        ar = {k: torch.from_numpy(OC.arena(rows, kind[k], vals[k])).cuda() for k in vals}
        view = {k: [ar[k][s:s + r.numel] for s, r in zip(OC.layout(rows, kind[k])[0], rows)] for k in vals}
        params = [torch.nn.Parameter(p) for p in view["p"]]
        for q, g in zip(params, view["g"]):
            q.grad = g
        guard = GradGuard(params, max_norm=0.05)
        assert guard.apply() is True
        assert guard._workspace is not None
        ops.adam_step([(p, g, m, v, 2e-4, 1.0) for p, g, m, v in zip(view["p"], view["g"], view["m"], view["v"])], 0.9, 0.99, 1e-8, 1e-2)
        table = ops.ema_rows(len(rows))
        for i, (e, p) in enumerate(zip(view["e"], view["p"])):
            ops.ema_row(table, i, e, p)
        ops.ema_launch(table, len(rows), torch.device("cuda", torch.cuda.current_device()), 0.999)
        out = dict(ar)
        out["record"] = guard._record
        return out
    got = three_runs("adam + ema + grad-norm and scale", call)
    for k in ("p", "g", "m", "v", "e"):
        _, blank = OC.split(rows, kind[k], got[k].view(torch.float32).numpy())
        assert np.array_equal(blank.view(np.uint32), np.full(blank.shape, OC.GUARD, np.float32).view(np.uint32)), f"{k}: a sentinel between rows changed"
    coef = np.frombuffer(got["record"].numpy().tobytes(), dtype=np.float32)[3]
    assert 0.0 < float(coef) < 1.0, "the clip did not engage: grad_scale was not exercised"


# ------------------------------------------------------------------------------------------------ 11. whole generator, training step
@pytest.mark.parametrize("streams", ["default", "multi"])
@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_whole_generator(prec, streams, monkeypatch):
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict, synthetic_frames
    if streams == "multi":
        monkeypatch.setenv("BIN_AMD_STREAMS", "3")
    else:
        monkeypatch.delenv("BIN_AMD_STREAMS", raising=False)
    frames = [f.cuda() for f in synthetic_frames(1234, 1, 64, 64, 6)]
    sd = reference_state_dict(0)

    def call():
        net = bin_stage4_lstm()
        net.load_state_dict(sd, strict=True)
        net = net.cuda().eval()
        net.set_precision(prec)
        with torch.no_grad():
            return list(net(*frames))
    got = three_runs(f"bin_stage4_lstm 64x64 {prec} streams={streams}", call, min_count=2)
    assert len(got) == 14


def test_training_step(tmp_path):
    """One bin_model.optimize_parameters step with the training settings of options/bin_stage4_synthetic.yml on a batch of 2 crops of
    64 x 64 of the synthetic moving-texture task: the loss, its 17 terms and every .grad."""
    from bin_amd.data.synthetic import moving_texture_batch
    from bin_amd.models import create_model
    from bin_amd.weights import reference_state_dict
    opt = {"model": "bin", "gpu_ids": [0], "is_train": True, "dist": False,
           "network_G": {"which_model_G": "bin_stage4", "nframes": 6, "version": 2},
           "path": {"pretrain_model_G": None, "strict_load": True, "models": str(tmp_path), "training_state": str(tmp_path)},
           "train": {"pixel_criterion": "cb", "pixel_weight": 1.0, "weight_decay_G": 0, "ft_tsa_only": None,
                     "lr_G": 2e-4, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "lr_steps": [1500],
                     "restarts": None, "restart_weights": None, "lr_gamma": 0.5, "clear_state": False}}
    batch = moving_texture_batch(0, 0, 2, 64)
    sd = reference_state_dict(0)

    def call():
        m = create_model(opt)
        m.netG.module.load_state_dict(sd, strict=True)
        m.feed_data(batch)
        m.optimize_parameters(1)
        out = {"loss": torch.as_tensor(m.loss).detach(), "terms": torch.stack([l.detach() for l in m.loss_list])}
        out.update({"grad." + n: p.grad for n, p in m.netG.module.named_parameters() if p.grad is not None})
        out.update({"after." + n: p.detach() for n, p in m.netG.module.named_parameters()})
        return out
    got = three_runs("optimize_parameters batch 2 crop 64", call, min_count=2)
    assert sum(k.startswith("grad.") for k in got) > 500


# ------------------------------------------------------------------------------------------------ 12. self-ensemble and the video harness
def _fresh_net(prec="f16x3"):
    from bin_amd.models.archs.RDN import bin_stage4_lstm
    from bin_amd.weights import reference_state_dict
    net = bin_stage4_lstm()
    net.load_state_dict(reference_state_dict(0), strict=True)
    return net.cuda().eval().set_precision(prec)


@pytest.mark.parametrize("strategy", ["batched", "streamed"])
def test_self_ensemble(strategy):
    """SelfEnsemble over the flips of W and H: the batched strategy's six [M N, 3, H, W] inputs come from torch.empty and are filled by
    one ens_orient launch; both strategies end in ens_merge's fresh outputs."""
    from bin_amd.ensemble import SelfEnsemble
    from bin_amd.weights import synthetic_frames
    frames = [f.cuda() for f in synthetic_frames(77, 1, 32, 32, 6)]
    got = three_runs(f"SelfEnsemble hv {strategy}", lambda: SelfEnsemble(_fresh_net(), "hv", strategy=strategy)(frames), min_count=14)
    assert len(got) == 14


def test_video_harness():
    """harness.interpolate_video at twice the frame rate and at 60 from 24 frames per second (the blend), scored against a ground truth
    (the per-frame score records and the cached score workspace start poisoned; records of frames without a truth are never read), and
    harness.luma_records (one [T, 264] buffer of scene records)."""
    import rate_cases as RC
    from bin_amd import harness
    header, payloads = RC.clip_at((24, 1), T=5)
    payloads = torch.from_numpy(payloads)

    def video(**kw):
        def call():
            out, rows = harness.interpolate_video(_fresh_net(), payloads, header, gt=payloads, **kw)
            assert len(rows) == 5
            return {"out": out, "rows": torch.tensor([[float(v) for v in r[:2] + r[3:]] for r in rows], dtype=torch.float64)}
        return call
    three_runs("interpolate_video factor 2 with scores", video(factor=2), min_count=3)
    three_runs("interpolate_video 24 -> 60 fps with scores", video(rate=(60, 1)), min_count=3)

    def luma():
        recs = harness.luma_records(payloads, header, device="cuda")
        return torch.tensor([[sad] + [int(v) for v in hist] for sad, hist in recs], dtype=torch.int64)
    three_runs("luma_records", luma)
