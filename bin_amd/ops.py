"""Thin torch-tensor wrappers over the libbinhip C ABI (include/binhip.h).

PyTorch is plumbing here (device memory, streams); every computation is a hand-written HIP kernel.
Activations between layers are "chunk planes" (CP): fp16 [C/16][N][H][W][16], optionally hi+lo.
"""
import ctypes as C
import functools
import os

import torch

from . import _lib as L


def _stream(device=None):
    """The caller's current stream ON `device` (default: the current device).  Library calls launch on the current
    HIP device, so entry points that take tensors run under `on_device(t)`."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def on_device(t):
    """Context that makes `t`'s device current (a no-op when it already is): kernels launch on the CURRENT device and
    on its stream, so a tensor living on another GPU of the same process must switch first."""
    return torch.cuda.device(t.device)


_status = {}


def status_word(device):
    """Per-device uint32 status word the kernels OR into (include/binhip.h BINHIP_STATUS_*)."""
    key = _device_key(device)
    w = _status.get(key)
    if w is None:
        w = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", key))
        _status[key] = w
    return w


def _device_key(device):
    device = torch.device(device)
    return device.index if device.index is not None else torch.cuda.current_device()


def check_status(device=None, reset=True):
    """Raise if any kernel since the last check reported a problem in its device status word: a stored value outside
    the fp16 range (or a NaN), a neighbour-flag timeout of the three-phase dense-block launch, or any bit this host
    code does not know.  Reads the device word, i.e. synchronises: call it where the host syncs anyway (after a step,
    before images leave the device).  `device=None` checks every device that has a word; a device without an index
    means the current one (as in `status_word`)."""
    keys = list(_status) if device is None else [_device_key(device)]
    for k in keys:
        w = _status.get(k)
        if w is None:
            continue
        v = int(w.item()) & 0xFFFFFFFF
        if not v:
            continue
        if reset:
            w.zero_()
        if v & L.STATUS_SYNC_TIMEOUT:
            raise RuntimeError(
                "bin_amd: dense-block launch on cuda:%d timed out waiting for a neighbour tile (BINHIP_STATUS_SYNC_TIMEOUT): "
                "a tile was computed from inputs that may not have been published; results since the last check are "
                "invalid" % k)
        if v & L.STATUS_SATURATED:
            raise RuntimeError(
                "bin_amd: fp16 range exceeded on cuda:%d — an activation / gradient left +-65504 (or was NaN) and was "
                "saturated; results since the last check are not those of the fp32 reference (include/binhip.h, "
                "'Dynamic range')" % k)
        raise RuntimeError("bin_amd: unknown status bits 0x%x on cuda:%d (library newer than this host code?)" % (v, k))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("bin_amd: tensors must live on a HIP device (there is no CPU path; "
                               "the CPU restatement lives in oracle/ and is test-only)")


def chunks(c):
    return (c + 15) // 16


class CP:
    """A chunk-plane tensor: `hi` (and `lo` when split) are fp16 [nchunks, N, H, W, 16]."""

    def __init__(self, hi, lo, channels):
        self.hi, self.lo, self.channels = hi, lo, channels

    @property
    def shape(self):
        return tuple(self.hi.shape)

    @staticmethod
    def empty(nchunks, n, h, w, nterms, device, channels=None):
        hi = torch.empty((nchunks, n, h, w, 16), dtype=torch.float16, device=device)
        lo = torch.empty_like(hi) if nterms == 3 else None
        return CP(hi, lo, channels if channels is not None else nchunks * 16)

    def sub(self, c0, nch):
        return CP(self.hi[c0:c0 + nch], self.lo[c0:c0 + nch] if self.lo is not None else None, nch * 16)


def nchw_to_planes(x, nterms=1):
    _need_cuda(x)
    x = x.contiguous().float()
    n, c, h, w = x.shape
    y = CP.empty(chunks(c), n, h, w, nterms, x.device, c)
    L.check(L.lib().binhip_nchw_to_planes(_ptr(x), n, c, h, w, _ptr(y.hi), _ptr(y.lo), _ptr(status_word(x.device)),
                                          _stream()), "nchw_to_planes")
    return y


def planes_to_nchw(cp, channels=None):
    c = channels if channels is not None else cp.channels
    _, n, h, w, _ = cp.hi.shape
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=cp.hi.device)
    L.check(L.lib().binhip_planes_to_nchw(_ptr(cp.hi), _ptr(cp.lo), n, c, h, w, _ptr(y), _stream()), "planes_to_nchw")
    return y


def pack_inputs(images, nterms=1):
    """K1: pixel_reshuffle(cat(images), 2) -> CP at half resolution (reference RDN.py:107-132)."""
    _need_cuda(*images)
    images = [im.contiguous().float() for im in images]
    n, c, h, w = images[0].shape
    assert c == 3 and h % 2 == 0 and w % 2 == 0
    k = len(images)
    y = CP.empty(chunks(12 * k), n, h // 2, w // 2, nterms, images[0].device, 12 * k)
    arr = (C.c_void_p * k)(*[im.data_ptr() for im in images])
    L.check(L.lib().binhip_pack_inputs(arr, k, n, h, w, _ptr(y.hi), _ptr(y.lo), _ptr(status_word(images[0].device)),
                                       _stream()), "pack_inputs")
    return y


def relayout_item(kind, srcs, bias, w_hi, w_lo, bias_out, cout, cin, ks, rows_pad, cin_chunks, cout_block, shuffle_or_group,
                  shape=None):
    """One BinRelayoutItem (include/binhip.h).  `srcs`: the fp32 OIHW source tensor(s); the caller keeps them alive until
    relayout_batch() has enqueued the launch."""
    it = L.BinRelayoutItem()
    w = it.w
    for i, t in enumerate(srcs):
        w[i] = t.data_ptr() if t is not None else None
    it.bias = bias.data_ptr() if bias is not None else None
    it.w_hi, it.w_lo = w_hi.data_ptr(), (w_lo.data_ptr() if w_lo is not None else None)
    it.bias_out = bias_out.data_ptr()
    it.kind, it.cout, it.cin, it.ksize, it.rows_pad = kind, cout, cin, ks, rows_pad
    it.cin_chunks, it.cout_block, it.shuffle_or_group = cin_chunks, cout_block, shuffle_or_group
    if shape is not None:                  # RDB_GATHER of a block other than bin_stage4's
        sh = it.shape
        sh.G0, sh.D, sh.C, sh.G = shape
    return it


def relayout_batch(items):
    """Enqueue the relayouts of `items` (list of BinRelayoutItem) in as few launches as the library needs.
    BIN_AMD_RELAYOUT_BATCH=0 (A/B switch of tools/): one launch per item, as before round 3."""
    if not items:
        return
    lib = L.lib()
    if os.environ.get("BIN_AMD_RELAYOUT_BATCH", "1") == "0":
        for it in items:
            L.check(lib.binhip_weights_relayout_batch(C.byref(it), 1, _stream()), "weights_relayout_batch")
        return
    arr = (L.BinRelayoutItem * len(items))(*items)
    L.check(lib.binhip_weights_relayout_batch(arr, len(items), _stream()), "weights_relayout_batch")


def _source(t):
    """A relayout source: on the device, as a contiguous fp32 tensor outside autograd — `t` itself when it already is one (a weight
    set hands each source to several relayouts: this is on its construction's critical path, which is host time)."""
    if t.is_cuda and t.dtype is torch.float32 and t.is_contiguous() and not t.requires_grad:
        return t
    _need_cuda(t)
    return t.detach().contiguous().float()


# The library's answers about a layout are pure functions of a few small integers; a weight set asks them for each of its 66 + 66
# layers after every optimizer step, where a ctypes call costs as much as an allocation
@functools.lru_cache(maxsize=None)
def _plane_elems(rows_pad, cin_chunks, ks):
    return L.lib().binhip_weights_bytes(rows_pad, cin_chunks, ks) // 2


@functools.lru_cache(maxsize=None)
def _cout_block(ks, cout_pad, nterms):
    return L.lib().binhip_conv_cout_block(ks, cout_pad, nterms)


def alloc_weights(rows_pad, cin_chunks, ks, nterms, device):
    """(w_hi, w_lo or None, bias): the uninitialised kernel-layout buffers of one relayout (include/binhip.h)."""
    n = _plane_elems(rows_pad, cin_chunks, ks)
    return (torch.empty(n, dtype=torch.float16, device=device),
            torch.empty(n, dtype=torch.float16, device=device) if nterms == 3 else None,
            torch.empty(rows_pad, dtype=torch.float32, device=device))


class _KernelWeights:
    """What the three kinds of kernel-layout weights share: the geometry the convolution launch reads (ks, nterms, cout, cout_pad,
    cin_chunks, cout_block), the buffers, and one launch route.  `defer`: a list that receives the relayout item instead of
    launching it (RdnWeights / RdnDgradWeights batch the layers of a weight set); `_src` then keeps the sources alive."""

    def _relayout(self, kind, srcs, bias, cout, cin, shuffle_or_group, defer, shape=None):
        srcs = [_source(w) for w in srcs]
        bias = _source(bias) if bias is not None else None
        self.cout_block = _cout_block(self.ks, self.cout_pad, self.nterms)
        self.w_hi, self.w_lo, self.bias = alloc_weights(self.cout_pad, self.cin_chunks, self.ks, self.nterms, srcs[0].device)
        item = relayout_item(kind, srcs, bias, self.w_hi, self.w_lo, self.bias, cout, cin, self.ks, self.cout_pad, self.cin_chunks,
                             self.cout_block, shuffle_or_group, shape)
        if defer is None:
            relayout_batch([item])
        else:
            self._src = (srcs, bias)
            defer.append(item)


class ConvWeights(_KernelWeights):
    """Kernel-layout weights of one convolution (see binhip_weights_relayout)."""

    def __init__(self, weight, bias, nterms=1, shuffle=False, cout_pad=None, cin_chunks=None, defer=None):
        cout, cin, ks, _ = weight.shape
        self.cout, self.cin, self.ks, self.nterms, self.shuffle = cout, cin, ks, nterms, shuffle
        self.cout_pad = cout_pad if cout_pad is not None else ((cout + 31) // 32) * 32
        self.cin_chunks = cin_chunks if cin_chunks is not None else chunks(cin)
        self._relayout(L.RELAYOUT_FWD, [weight], bias, cout, cin, 1 if shuffle else 0, defer)


def conv2d(x, cw, relu=False, residual=None, out=None, epilogue=L.EPI_PLANES, images=None, x_cpg=0,
           x_group_stride=0, cin_chunks=None):
    """One fused convolution launch.  x: CP (its first `cin_chunks` planes are read);
    PLANES/SHUFFLE return a CP, FINAL returns fp32 NCHW."""
    nch, n, h, w, _ = x.hi.shape
    d = L.BinConvDesc()
    d.N, d.H, d.W, d.ksize = n, h, w, cw.ks
    d.cin_chunks = cin_chunks if cin_chunks is not None else cw.cin_chunks
    d.cout, d.cout_pad, d.nterms, d.epilogue, d.relu = cw.cout, cw.cout_pad, cw.nterms, epilogue, int(relu)
    d.x_cpg, d.x_group_stride = x_cpg, x_group_stride
    d.n_images = len(images) if images else 0
    # BINHIP_CONV_HALF_LAST_CHUNK: a 5x5 layer whose last chunk holds <= 8 real channels (x from nchw_to_planes / pack_inputs and
    # the relayouted weights are zero there) may spend that chunk's K on tap pairs
    if cw.ks == 5 and 1 <= cw.cin % 16 <= 8 and d.cin_chunks == cw.cin_chunks:
        d.reserved = L.CONV_HALF_LAST_CHUNK
    dev = x.hi.device
    d.status = status_word(dev).data_ptr()
    y_f32, arr = None, None
    if epilogue == L.EPI_PLANES:
        if out is None:
            out = CP.empty(chunks(cw.cout), n, h, w, cw.nterms, dev, cw.cout)
    elif epilogue == L.EPI_SHUFFLE:
        if out is None:
            out = CP.empty(chunks(cw.cout // 4), n, 2 * h, 2 * w, cw.nterms, dev, cw.cout // 4)
    else:
        y_f32 = torch.empty((n, cw.cout, h, w), dtype=torch.float32, device=dev)
        if images:
            images = [im.contiguous().float() for im in images]
            arr = (C.c_void_p * len(images))(*[im.data_ptr() for im in images])
    rc = L.lib().binhip_conv2d_fwd(
        C.byref(d), _ptr(x.hi), _ptr(x.lo), _ptr(cw.w_hi), _ptr(cw.w_lo), _ptr(cw.bias),
        _ptr(residual.hi) if residual is not None else C.c_void_p(0),
        _ptr(residual.lo) if residual is not None else C.c_void_p(0),
        _ptr(out.hi) if out is not None else C.c_void_p(0),
        _ptr(out.lo) if out is not None else C.c_void_p(0),
        _ptr(y_f32), arr, _stream())
    L.check(rc, "conv2d_fwd")
    return out if epilogue in (L.EPI_PLANES, L.EPI_SHUFFLE) else y_f32


def convlstm_cell(x, state, weight, bias, forget_bias=1.0):
    """ConvLSTMCell.forward (reference RDN.py:50-95).  Returns (h', [c', h'])."""
    _need_cuda(x, weight)
    x = x.contiguous().float()
    n, c, h, w = x.shape
    assert c == 3 and tuple(weight.shape) == (12, 6, 3, 3)
    cn = torch.empty_like(x)
    hn = torch.empty_like(x)
    cp = state[0].contiguous().float() if state is not None else None
    hp = state[1].contiguous().float() if state is not None else None
    L.check(L.lib().binhip_convlstm_fwd(_ptr(x), _ptr(cp), _ptr(hp), _ptr(weight.detach().contiguous().float()),
                                        _ptr(bias.detach().contiguous().float()), float(forget_bias), n, h, w,
                                        _ptr(cn), _ptr(hn), _stream()), "convlstm_fwd")
    return hn, [cn, hn]


def pixel_loss(kind, x, y, eps=1e-6):
    """One of bin_model's pixel criteria (L.LOSS_*), forward only: Charbonnier mean, L1 sum, L2 sum."""
    _need_cuda(x, y)
    x = x.contiguous().float()
    y = y.contiguous().float()
    lib = L.lib()
    part = torch.empty(lib.binhip_charbonnier_partials(x.numel()), dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    with on_device(x):
        L.check(lib.binhip_pixel_loss_fwd(kind, _ptr(x), _ptr(y), x.numel(), float(eps), _ptr(part), _ptr(loss), _stream()),
                "pixel_loss_fwd")
    return loss


def pixel_loss_grad(kind, x, y, gloss, eps=1e-6):
    x = x.contiguous().float()
    y = y.contiguous().float()
    gx = torch.empty_like(x)
    g = gloss.reshape(1).contiguous().float()
    with on_device(x):
        L.check(L.lib().binhip_pixel_loss_bwd(kind, _ptr(x), _ptr(y), x.numel(), float(eps), _ptr(g), _ptr(gx),
                                              C.c_void_p(0), _stream()), "pixel_loss_bwd")
    return gx


def multi_pixel_loss(kind, pairs, eps=1e-6):
    """All terms of bin_model.get_loss in two launches (binhip_multi_loss_fwd): `pairs` = [(x, y)] contiguous fp32 device tensors
    of one size.  Returns (loss = sum(terms) / T as Python's sum(list) / len(list) computes it, terms [T])."""
    xs = [p[0] for p in pairs] + [p[1] for p in pairs]
    _need_cuda(*xs)
    n = pairs[0][0].numel()
    T = len(pairs)
    if T > L.LOSS_MAX_TERMS or any(t.numel() != n or t.dtype != torch.float32 or not t.is_contiguous() for t in xs):
        raise ValueError("multi_pixel_loss: up to %d pairs of contiguous fp32 tensors of one size" % L.LOSS_MAX_TERMS)
    lib = L.lib()
    dev = pairs[0][0].device
    t = L.BinLossTerms()
    t.n_terms = T
    for i, (x, y) in enumerate(pairs):
        t.x[i], t.y[i] = x.data_ptr(), y.data_ptr()
    part = torch.empty(T * lib.binhip_charbonnier_partials(n), dtype=torch.float32, device=dev)
    terms = torch.empty(T, dtype=torch.float32, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev)
    with on_device(pairs[0][0]):
        L.check(lib.binhip_multi_loss_fwd(kind, C.byref(t), n, float(eps), _ptr(part), _ptr(terms), _ptr(loss), _stream()),
                "multi_loss_fwd")
    return loss, terms


def multi_pixel_loss_grad(kind, pairs, gloss, wanted, eps=1e-6):
    """Gradients of that loss in one launch (binhip_multi_loss_bwd).  `wanted`: [(like, [(term, sign), ...])] — one entry per
    tensor that needs a gradient, with the (at most two) terms it appears in; returns the gradient tensors in that order."""
    n = pairs[0][0].numel()
    t = L.BinLossTerms()
    t.n_terms = len(pairs)
    for i, (x, y) in enumerate(pairs):
        t.x[i], t.y[i] = x.data_ptr(), y.data_ptr()
    g = L.BinLossGrads()
    g.n_out = len(wanted)
    outs = []
    for k, (like, where) in enumerate(wanted):
        if not 1 <= len(where) <= 2:
            raise ValueError("multi_pixel_loss_grad: a tensor may appear in one or two terms")
        o = torch.empty_like(like)
        outs.append(o)
        g.out[k] = o.data_ptr()
        g.term_a[k], g.sign_a[k] = where[0]
        g.term_b[k], g.sign_b[k] = where[1] if len(where) == 2 else (-1, 0.0)
    gl = gloss.reshape(1).contiguous().float()
    with on_device(pairs[0][0]):
        L.check(L.lib().binhip_multi_loss_bwd(kind, C.byref(t), n, float(eps), _ptr(gl), C.byref(g), _stream()), "multi_loss_bwd")
    return outs


def charbonnier(x, y, eps=1e-6):
    """mean(sqrt((x-y)^2 + eps)) (reference loss.py:137-141), forward only."""
    return pixel_loss(L.LOSS_CHARBONNIER, x, y, eps)


def charbonnier_grad(x, y, gloss, eps=1e-6):
    return pixel_loss_grad(L.LOSS_CHARBONNIER, x, y, gloss, eps)


_SSIM_TAPS = None


def _ssim_taps():
    global _SSIM_TAPS
    if _SSIM_TAPS is None:
        from .utils.util import _gauss_taps
        _SSIM_TAPS = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    return _SSIM_TAPS


def _ssim_geometry(what, pairs):
    """(planes, H, W) of the pairs of ssim_terms / ssim_terms_grad, which are checked here: tensors of one shape, at least 3-D with
    the last two dimensions H, W, contiguous fp32 on one device."""
    pairs = list(pairs)
    if not pairs or any(len(p) != 2 for p in pairs):
        raise ValueError(f"{what}: a non-empty sequence of (x, y) pairs")
    first = pairs[0][0]
    _need_cuda(*[t for p in pairs for t in p])
    for t in (t for p in pairs for t in p):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: float32 tensors, got {t.dtype}")
        if t.dim() < 3:
            raise ValueError(f"{what}: tensors of at least 3 dimensions [..., H, W], got {tuple(t.shape)}")
        if t.shape != first.shape or t.device != first.device:
            raise ValueError(f"{what}: tensors of one shape on one device, got {tuple(t.shape)} on {t.device} next to "
                             f"{tuple(first.shape)} on {first.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: contiguous tensors, got strides {t.stride()} for shape {tuple(t.shape)}")
    h, w = first.shape[-2:]
    planes = first.numel() // (h * w) if h * w else 0
    if h < 11 or w < 11 or planes < 1 or first.numel() > 2 ** 31 - 1:
        raise ValueError(f"{what}: planes of at least 11 x 11 pixels and at most 2^31 - 1 elements per tensor, got {tuple(first.shape)}")
    return pairs, planes, h, w


def ssim_terms(pairs):
    """ssim(x, y) of every (x, y) of `pairs` as an fp32 device tensor [T] (binssim_forward, include/binssim.h): the mean over all
    planes and all valid 11 x 11 Gaussian windows (sigma 1.5, C1 = 0.01^2, C2 = 0.03^2, data range 1), in double, rounded once.
    One call of two launches per SSIM_MAX_TERMS pairs, on the current stream, no host sync."""
    pairs, planes, h, w = _ssim_geometry("ssim_terms", pairs)
    lib = L.ssimlib()
    dev = pairs[0][0].device
    out = torch.empty(len(pairs), dtype=torch.float32, device=dev)
    with on_device(pairs[0][0]):
        for i0 in range(0, len(pairs), L.SSIM_MAX_TERMS):
            part = pairs[i0:i0 + L.SSIM_MAX_TERMS]
            t = L.BinSsimTerms()
            t.n_terms = len(part)
            for i, (x, y) in enumerate(part):
                t.x[i], t.y[i] = x.data_ptr(), y.data_ptr()
            nb = lib.binssim_workspace_bytes(len(part), planes, h, w)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            L.check(lib.binssim_forward(C.byref(t), planes, h, w, _ssim_taps(), _ptr(ws), nb, _ptr(out[i0:i0 + len(part)]), _stream()),
                    "ssim_forward")
    return out


def ssim_terms_grad(pairs, g, need):
    """The gradients of `sum_t g[t] * ssim(x_t, y_t)` (binssim_backward): `g` an fp32 device tensor [T], `need` per term
    (want_gx, want_gy), at least one of them.  Returns per term (gx | None, gy | None), fresh tensors shaped like the inputs.  One
    launch per SSIM_MAX_TERMS pairs, on the current stream, no host sync."""
    pairs, planes, h, w = _ssim_geometry("ssim_terms_grad", pairs)
    need = [(bool(a), bool(b)) for a, b in need]
    if len(need) != len(pairs) or not all(a or b for a, b in need):
        raise ValueError(f"ssim_terms_grad: `need` names at least one side of each of the {len(pairs)} terms, got {need}")
    dev = pairs[0][0].device
    if g.dtype != torch.float32 or g.shape != (len(pairs),) or g.device != dev:
        raise ValueError(f"ssim_terms_grad: g is a float32 tensor [{len(pairs)}] on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
    g = g.contiguous()
    lib = L.ssimlib()
    outs = []
    with on_device(pairs[0][0]):
        for i0 in range(0, len(pairs), L.SSIM_MAX_TERMS):
            part = pairs[i0:i0 + L.SSIM_MAX_TERMS]
            t = L.BinSsimTerms()
            t.n_terms = len(part)
            for i, ((x, y), (wx, wy)) in enumerate(zip(part, need[i0:i0 + len(part)])):
                gx = torch.empty_like(x) if wx else None
                gy = torch.empty_like(y) if wy else None
                t.x[i], t.y[i] = x.data_ptr(), y.data_ptr()
                t.gx[i], t.gy[i] = gx.data_ptr() if wx else None, gy.data_ptr() if wy else None
                outs.append((gx, gy))
            L.check(lib.binssim_backward(C.byref(t), planes, h, w, _ssim_taps(), _ptr(g[i0:i0 + len(part)]), _stream()), "ssim_backward")
    return outs


def _lap_geometry(what, pairs, levels, eps):
    """(pairs, planes, H, W, levels, eps) of lap_terms / lap_terms_grad, which are checked here: tensors of one shape, at least 3-D
    with the last two dimensions H, W of at least 2^(levels - 1) pixels, contiguous fp32 on one device; levels an int 1 .. 8, eps a
    finite number > 0."""
    pairs = list(pairs)
    if not pairs or any(len(p) != 2 for p in pairs):
        raise ValueError(f"{what}: a non-empty sequence of (x, y) pairs")
    if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= L.LAP_MAX_LEVELS:
        raise ValueError(f"{what}: levels {levels!r} is not an integer 1 .. {L.LAP_MAX_LEVELS}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 < float(eps) < float("inf"):
        raise ValueError(f"{what}: eps {eps!r} is not a finite number > 0")
    first = pairs[0][0]
    _need_cuda(*[t for p in pairs for t in p])
    for t in (t for p in pairs for t in p):
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: float32 tensors, got {t.dtype}")
        if t.dim() < 3:
            raise ValueError(f"{what}: tensors of at least 3 dimensions [..., H, W], got {tuple(t.shape)}")
        if t.shape != first.shape or t.device != first.device:
            raise ValueError(f"{what}: tensors of one shape on one device, got {tuple(t.shape)} on {t.device} next to "
                             f"{tuple(first.shape)} on {first.device}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: contiguous tensors, got strides {t.stride()} for shape {tuple(t.shape)}")
    h, w = first.shape[-2:]
    planes = first.numel() // (h * w) if h * w else 0
    least = 1 << (levels - 1)
    if h < least or w < least or planes < 1 or first.numel() > 2 ** 31 - 1:
        raise ValueError(f"{what}: planes of at least {least} x {least} pixels for {levels} levels and at most 2^31 - 1 elements per "
                         f"tensor, got {tuple(first.shape)}")
    return pairs, planes, h, w, levels, float(eps)


def lap_terms(pairs, levels=5, eps=1e-6):
    """lap(x, y) of every (x, y) of `pairs` as an fp32 device tensor [T] (binlap_forward, include/binlap.h): the sum over `levels`
    Laplacian-pyramid bands of x - y of the mean of sqrt(b^2 + eps), in double, rounded once.  One call of 2 * levels launches per
    LAP_MAX_TERMS pairs, on the current stream, no host sync."""
    pairs, planes, h, w, levels, eps = _lap_geometry("lap_terms", pairs, levels, eps)
    lib = L.laplib()
    dev = pairs[0][0].device
    out = torch.empty(len(pairs), dtype=torch.float32, device=dev)
    with on_device(pairs[0][0]):
        for i0 in range(0, len(pairs), L.LAP_MAX_TERMS):
            part = pairs[i0:i0 + L.LAP_MAX_TERMS]
            t = L.BinLapTerms()
            t.n_terms = len(part)
            for i, (x, y) in enumerate(part):
                t.x[i], t.y[i] = x.data_ptr(), y.data_ptr()
            nb = lib.binlap_forward_workspace_bytes(len(part), planes, h, w, levels)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            L.check(lib.binlap_forward(C.byref(t), planes, h, w, levels, eps, _ptr(ws), nb, _ptr(out[i0:i0 + len(part)]), _stream()),
                    "lap_forward")
    return out


def lap_terms_grad(pairs, g, wants, levels=5, eps=1e-6):
    """The gradients of `sum_t g[t] * lap(x_t, y_t)` (binlap_backward): `g` an fp32 device tensor [T], `wants` per term
    (want_gx, want_gy), at least one of them.  Returns per term (gx | None, gy | None), fresh tensors shaped like the inputs.  One
    call of 3 * levels - 2 launches per LAP_MAX_TERMS pairs, on the current stream, no host sync."""
    pairs, planes, h, w, levels, eps = _lap_geometry("lap_terms_grad", pairs, levels, eps)
    wants = [(bool(a), bool(b)) for a, b in wants]
    if len(wants) != len(pairs) or not all(a or b for a, b in wants):
        raise ValueError(f"lap_terms_grad: `wants` names at least one side of each of the {len(pairs)} terms, got {wants}")
    dev = pairs[0][0].device
    if g.dtype != torch.float32 or g.shape != (len(pairs),) or g.device != dev:
        raise ValueError(f"lap_terms_grad: g is a float32 tensor [{len(pairs)}] on {dev}, got {g.dtype} {tuple(g.shape)} on {g.device}")
    g = g.contiguous()
    lib = L.laplib()
    outs = []
    with on_device(pairs[0][0]):
        for i0 in range(0, len(pairs), L.LAP_MAX_TERMS):
            part = pairs[i0:i0 + L.LAP_MAX_TERMS]
            t = L.BinLapTerms()
            t.n_terms = len(part)
            for i, ((x, y), (wx, wy)) in enumerate(zip(part, wants[i0:i0 + len(part)])):
                gx = torch.empty_like(x) if wx else None
                gy = torch.empty_like(y) if wy else None
                t.x[i], t.y[i] = x.data_ptr(), y.data_ptr()
                t.gx[i], t.gy[i] = gx.data_ptr() if wx else None, gy.data_ptr() if wy else None
                outs.append((gx, gy))
            nb = lib.binlap_backward_workspace_bytes(len(part), planes, h, w, levels)
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            L.check(lib.binlap_backward(C.byref(t), planes, h, w, levels, eps, _ptr(g[i0:i0 + len(part)]), _ptr(ws), nb, _stream()),
                    "lap_backward")
    return outs


# --------------------------------------------------------------------------------------------- backward ops
class DgradWeights(_KernelWeights):
    """Backward-data weights of one convolution (binhip_weights_relayout_dgrad)."""

    def __init__(self, weight, nterms=1, shuffle=False, defer=None):
        cout, cin, ks, _ = weight.shape
        self.ks, self.nterms = ks, nterms
        self.cout = cin                                   # the dgrad conv's outputs = original inputs
        self.cout_pad = L.lib().binhip_dgrad_rows_pad(ks, cin)
        self.cin_chunks = chunks(cout)
        self._relayout(L.RELAYOUT_DGRAD, [weight], None, cout, cin, 1 if shuffle else 0, defer)


class RdbGatherWeights(_KernelWeights):
    """Backward-data weights of ONE concat group of a residual dense block (G0, C, G) in gather form
    (binhip_weights_relayout_rdb_gather, include/binhip.h): group g = 0 produces the gradient of the block's G0 input
    channels, g >= 1 that of conv g-1's G outputs, each as one forward-shaped 3x3 conv over the stacked output
    gradients of convs g..C-1.  `weights`: the block's C OIHW fp32 conv weights (bin_stage4: four, (96, 4, 32))."""

    def __init__(self, weights, group, nterms=1, defer=None):
        (G, G0, _, _), C_ = weights[0].shape, len(weights)
        self.ks, self.nterms = 3, nterms
        self.cout = self.cout_pad = G0 if group == 0 else G
        self.cin_chunks = (C_ - group) * G // 16
        self._relayout(L.RELAYOUT_RDB_GATHER, weights, None, G, G0 + G * group, group, defer, shape=(G0, 0, C_, G))


def rdb_tail(blk, cw3, cwl, out=None, store_o3=False):
    """Fused tail of a residual dense block (binhip_rdb_tail_fwd): o3 = relu(conv3x3(blk[0:192])), y = LFF(cat(blk[0:192],
    o3)) + blk[0:96].  blk: 14-chunk CP (planes 12, 13 receive o3 when store_o3); returns the 6-chunk output CP."""
    _, n, h, w, _ = blk.hi.shape
    nt = cw3.nterms
    if out is None:
        out = CP.empty(6, n, h, w, nt, blk.hi.device, 96)
    L.check(L.lib().binhip_rdb_tail_fwd(n, h, w, nt, _ptr(blk.hi), _ptr(blk.lo), _ptr(cw3.w_hi), _ptr(cw3.w_lo),
                                        _ptr(cw3.bias), _ptr(cwl.w_hi), _ptr(cwl.w_lo), _ptr(cwl.bias), _ptr(out.hi),
                                        _ptr(out.lo), 1 if store_o3 else 0, _ptr(status_word(blk.hi.device)), _stream()),
            "rdb_tail_fwd")
    return out


def conv2d_bwd_data(gy, dw, res=None, res_chunks=0, acc=None, mask=None, mask_from=0, out=None, y_unshuf=0, y_cpg=0,
                    y_group_stride=0):
    """gx = [mask](conv_{W'}(gy) [+ res] [+ acc]) on chunk planes (binhip_conv2d_bwd_data).  `y_unshuf` > 0: the result leaves
    through an inverse PixelShuffle(2) — 4 * y_unshuf planes at half resolution (BinConvDesc.reserved).  `y_cpg` /
    `y_group_stride` (fp16 elements): output chunk i goes to group i // y_cpg of `out`, which the caller then supplies (as are res,
    acc and mask, which are indexed like the output)."""
    if y_cpg > 0 and out is None:
        raise ValueError("bin_amd: conv2d_bwd_data with y_cpg needs the grouped `out` buffer")
    _, n, h, w, _ = gy.hi.shape
    d = L.BinConvDesc()
    d.N, d.H, d.W, d.ksize = n, h, w, dw.ks
    d.cin_chunks, d.cout, d.cout_pad, d.nterms = dw.cin_chunks, dw.cout, dw.cout_pad, dw.nterms
    d.epilogue, d.relu, d.x_cpg, d.x_group_stride, d.n_images = L.EPI_PLANES, 0, 0, 0, 0
    d.status = status_word(gy.hi.device).data_ptr()
    d.reserved = int(y_unshuf)
    if out is None:
        out = (CP.empty(4 * y_unshuf, n, h // 2, w // 2, dw.nterms, gy.hi.device) if y_unshuf
               else CP.empty(chunks(dw.cout), n, h, w, dw.nterms, gy.hi.device, dw.cout))
    z = C.c_void_p(0)
    rc = L.lib().binhip_conv2d_bwd_data(
        C.byref(d), _ptr(gy.hi), _ptr(gy.lo), _ptr(dw.w_hi), _ptr(dw.w_lo), _ptr(dw.bias),
        _ptr(res.hi) if res is not None else z, _ptr(res.lo) if res is not None else z, res_chunks,
        _ptr(acc.hi) if acc is not None else z, _ptr(acc.lo) if acc is not None else z,
        _ptr(mask.hi) if mask is not None else z, mask_from, int(y_cpg), int(y_group_stride), _ptr(out.hi), _ptr(out.lo), _stream())
    L.check(rc, "conv2d_bwd_data")
    return out


def conv2d_bwd_weight(x, gy, cout, cin, ks, nterms, inv_scale=None, shuffle=False, accumulate=False, x_cpg=0,
                      x_group_stride=0, out=None, workspace=None):
    """(dW [cout,cin,ks,ks], db [cout]) fp32 from saved input planes x and gradient planes gy.  `accumulate`: add to `out` instead of
    overwriting it.  `x_cpg` / `x_group_stride` (fp16 elements): input chunk i lives in group i // x_cpg of x (BinConvDesc).  `out`: the
    caller's contiguous fp32 (dw, db), views into larger buffers included.  `workspace`: the caller's uint8 buffer of at least
    binhip_wgrad_workspace_bytes() bytes (a shorter one is the library's BINHIP_E_WORKSPACE)."""
    n, h, w = gy.hi.shape[1:4]
    lib = L.lib()
    d = L.BinConvDesc()
    d.N, d.H, d.W, d.ksize = n, h, w, ks
    d.cin_chunks, d.cout, d.cout_pad, d.nterms = chunks(cin), cout, 0, nterms
    d.epilogue, d.relu, d.x_cpg, d.x_group_stride, d.n_images = 0, 0, int(x_cpg), int(x_group_stride), 0
    dev = x.hi.device
    ws = workspace
    if ws is None:
        ws = torch.empty(lib.binhip_wgrad_workspace_bytes(ks, n, h, w, chunks(cin), cout), dtype=torch.uint8, device=dev)
    if out is None:
        if accumulate:
            raise ValueError("bin_amd: conv2d_bwd_weight(accumulate=True) needs out=(dw, db) to add to")
        dw = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=dev)
        db = torch.empty((cout,), dtype=torch.float32, device=dev)
    else:
        dw, db = out
        _need_cuda(dw, db)
        if (dw.dtype != torch.float32 or db.dtype != torch.float32 or tuple(dw.shape) != (cout, cin, ks, ks)
                or tuple(db.shape) != (cout,) or not dw.is_contiguous() or not db.is_contiguous()):
            raise ValueError("bin_amd: conv2d_bwd_weight out= must be contiguous fp32 (dw [cout,cin,ks,ks], db [cout])")
    L.check(lib.binhip_conv2d_bwd_weight(C.byref(d), _ptr(x.hi), _ptr(x.lo), _ptr(gy.hi), _ptr(gy.lo),
                                         _ptr(inv_scale), _ptr(ws), ws.numel() * ws.element_size(), _ptr(dw), _ptr(db), cin,
                                         1 if shuffle else 0, 1 if accumulate else 0, _stream()), "conv2d_bwd_weight")
    return dw, db


def grad_planes(g, nterms):
    """fp32 NCHW gradient -> chunk planes stored times a power-of-two scale that maps max|g| into (8, 16] (fp16 range), plus
    the device pair [scale, 1 / scale] (binhip_grad_scale + binhip_nchw_to_planes_scaled)."""
    _need_cuda(g)
    g = g.contiguous().float()
    n, c, h, w = g.shape
    lib = L.lib()
    part = torch.empty(lib.binhip_charbonnier_partials(g.numel()), dtype=torch.float32, device=g.device)
    sc = torch.empty(2, dtype=torch.float32, device=g.device)
    y = CP.empty(chunks(c), n, h, w, nterms, g.device, c)
    with on_device(g):
        L.check(lib.binhip_grad_scale(_ptr(g), g.numel(), 16.0, _ptr(part), _ptr(sc), _stream()), "grad_scale")
        L.check(lib.binhip_nchw_to_planes_scaled(_ptr(g), n, c, h, w, _ptr(sc), _ptr(y.hi), _ptr(y.lo),
                                                 _ptr(status_word(g.device)), _stream()), "nchw_to_planes_scaled")
    return y, sc


def lstm_gates(gates, c_prev, forget_bias, hidden):
    """(c', h') from the gates conv output [N, 4*hidden, H, W] of a ConvLSTM cell of any size (reference RDN.py:74-82)."""
    _need_cuda(gates)
    gates = gates.contiguous().float()
    n, c4, h, w = gates.shape
    assert c4 == 4 * hidden
    cn = torch.empty((n, hidden, h, w), dtype=torch.float32, device=gates.device)
    hn = torch.empty_like(cn)
    cp = c_prev.contiguous().float() if c_prev is not None else None
    with on_device(gates):
        L.check(L.lib().binhip_lstm_gates_fwd(_ptr(gates), _ptr(cp), float(forget_bias), n, hidden, h, w, _ptr(cn), _ptr(hn),
                                              _stream()), "lstm_gates_fwd")
    return cn, hn


def lstm_gates_grad(gates, c_prev, g_h, g_c, forget_bias, hidden, need_cprev):
    gates = gates.contiguous()                      # the kernel indexes plain NCHW
    n, _, h, w = gates.shape
    dg = torch.empty(gates.shape, dtype=gates.dtype, device=gates.device)
    gcp = torch.empty((n, hidden, h, w), dtype=torch.float32, device=gates.device) if need_cprev else None
    cp = c_prev.contiguous().float() if c_prev is not None else None
    gh = g_h.contiguous().float() if g_h is not None else None
    gc = g_c.contiguous().float() if g_c is not None else None
    with on_device(gates):
        L.check(L.lib().binhip_lstm_gates_bwd(_ptr(gates), _ptr(cp), _ptr(gh), _ptr(gc), float(forget_bias), n, hidden, h, w,
                                              _ptr(dg), _ptr(gcp), _stream()), "lstm_gates_bwd")
    return dg, gcp


# --------------------------------------------------------------------------------------------- harness glue (N1)
def u8_to_frame(img_u8, pads):
    """HWC BGR uint8 device tensor -> padded fp32 [1,3,Hp,Wp] RGB frame (read_image + ReplicationPad2d)."""
    _need_cuda(img_u8)
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3
    img_u8 = img_u8.contiguous()
    h, w, _ = img_u8.shape
    l, r, t, b = pads
    out = torch.empty((1, 3, h + t + b, w + l + r), dtype=torch.float32, device=img_u8.device)
    L.check(L.lib().binhip_u8_to_frame(_ptr(img_u8), h, w, l, r, t, b, _ptr(out), _stream()), "u8_to_frame")
    return out


def frame_to_u8(frame, top, left, h, w):
    """fp32 [1,3,Hp,Wp] (or [3,Hp,Wp]) RGB -> cropped HWC BGR uint8 (tensor2img + crop)."""
    _need_cuda(frame)
    f = frame.reshape(3, frame.shape[-2], frame.shape[-1]).contiguous().float()
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=f.device)
    L.check(L.lib().binhip_frame_to_u8(_ptr(f), f.shape[1], f.shape[2], top, left, h, w, _ptr(out), _stream()), "frame_to_u8")
    return out


# --------------------------------------------------------------------------------------------- video glue (libbinyuv.so)
_YUV_MATRIX = {"bt601": L.YUV_MATRIX_BT601, "bt709": L.YUV_MATRIX_BT709}
_YUV_RANGE = {"limited": L.YUV_RANGE_LIMITED, "full": L.YUV_RANGE_FULL}


def yuv_format(fmt):
    """BinYuvFormat of (chroma, matrix, range) = (420 | 444, "bt601" | "bt709", "limited" | "full")."""
    chroma, matrix, rng = fmt
    if chroma not in (420, 444) or matrix not in _YUV_MATRIX or rng not in _YUV_RANGE:
        raise ValueError(f"bin_amd: unknown YUV format {fmt!r}: (420 | 444, bt601 | bt709, limited | full)")
    return L.BinYuvFormat(int(chroma), _YUV_MATRIX[matrix], _YUV_RANGE[rng])


def yuv_frame_bytes(h, w, chroma):
    """(bytes of a frame's payload, chroma rows, chroma columns) of an h x w picture."""
    ch, cw = (h, w) if chroma == 444 else ((h + 1) // 2, (w + 1) // 2)
    return h * w + 2 * ch * cw, ch, cw


def _yuv_planes(payload, h, w, chroma):
    """Addresses of the Y, U and V planes: of one contiguous uint8 payload, or of a (y, u, v) triple of tensors."""
    n, ch, cw = yuv_frame_bytes(h, w, chroma)
    if isinstance(payload, (tuple, list)):
        if len(payload) != 3:
            raise ValueError("bin_amd: a YUV payload is one uint8 tensor or a (y, u, v) triple")
        _need_cuda(*payload)
        for t, size in zip(payload, (h * w, ch * cw, ch * cw)):
            if t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != size:
                raise ValueError(f"bin_amd: a plane of a {w}x{h} {chroma} frame is a contiguous uint8 tensor of {size} bytes")
        return tuple(C.c_void_p(t.data_ptr()) for t in payload)
    _need_cuda(payload)
    if payload.dtype != torch.uint8 or payload.dim() != 1 or not payload.is_contiguous() or payload.numel() != n:
        raise ValueError(f"bin_amd: the payload of a {w}x{h} {chroma} frame is a contiguous uint8 tensor of [{n}] bytes "
                         f"(got {payload.dtype} {tuple(payload.shape)})")
    p = payload.data_ptr()
    return C.c_void_p(p), C.c_void_p(p + h * w), C.c_void_p(p + h * w + ch * cw)


def yuv_to_frame(payload_u8, h, w, fmt, pads):
    """A Y4M frame payload (uint8 [frame_bytes]: the Y, U and V planes; or a (y, u, v) triple of plane tensors) on the device ->
    padded fp32 [1,3,Hp,Wp] RGB frame, the tensor u8_to_frame gives (include/binyuv.h).  fmt: (chroma, matrix, range)."""
    f = yuv_format(fmt)
    if h < 1 or w < 1 or len(pads) != 4 or min(pads) < 0:
        raise ValueError(f"bin_amd: yuv_to_frame needs a positive size and four non-negative pads (got {h}x{w}, {pads})")
    y, u, v = _yuv_planes(payload_u8, h, w, fmt[0])
    l, r, t, b = pads
    first = payload_u8[0] if isinstance(payload_u8, (tuple, list)) else payload_u8
    out = torch.empty((1, 3, h + t + b, w + l + r), dtype=torch.float32, device=first.device)
    with on_device(first):
        L.check(L.yuvlib().binyuv_to_frame(y, u, v, h, w, C.byref(f), l, r, t, b, _ptr(out), _stream()), "yuv_to_frame")
    return out


def _crop_to_payload(name, frames, top, left, h, w, chroma, out):
    """What frame_to_yuv and blend_to_yuv check and prepare alike: `frames` ([1,3,Hp,Wp] or [3,Hp,Wp], of one shape on one device) as
    contiguous fp32 [3,Hp,Wp] tensors, the crop checked against them, and the payload (`out`, or a fresh one) with its plane addresses.
    Returns (frames, Hp, Wp, out, (y, u, v))."""
    _need_cuda(*frames)
    count = "one [1,3,Hp,Wp] frame" if len(frames) == 1 else "two [1,3,Hp,Wp] frames"
    for x in frames:
        if x.dim() not in (3, 4) or x.numel() != 3 * x.shape[-2] * x.shape[-1]:
            raise ValueError(f"bin_amd: {name} takes {count} (got {tuple(x.shape)})")
    if any(x.shape[-2:] != frames[0].shape[-2:] or x.device != frames[0].device for x in frames):
        raise ValueError(f"bin_amd: {name} takes {count} of one shape on one device (got {', '.join(str(tuple(x.shape)) for x in frames)})")
    frames = [x.reshape(3, x.shape[-2], x.shape[-1]).contiguous().float() for x in frames]
    hp, wp = frames[0].shape[1], frames[0].shape[2]
    if h < 1 or w < 1 or top < 0 or left < 0 or top + h > hp or left + w > wp:
        raise ValueError(f"bin_amd: crop ({top}, {left}, {h}, {w}) leaves the {hp}x{wp} frame")
    if out is None:
        out = torch.empty(yuv_frame_bytes(h, w, chroma)[0], dtype=torch.uint8, device=frames[0].device)
    return frames, hp, wp, out, _yuv_planes(out, h, w, chroma)


def frame_to_yuv(frame, top, left, h, w, fmt, out=None):
    """fp32 [1,3,Hp,Wp] (or [3,Hp,Wp]) RGB -> the Y4M payload of its crop (uint8 [frame_bytes], into `out` when given; `out` may
    also be a (y, u, v) triple of plane tensors).  Float all the way: one rounding, so yuv_to_frame -> frame_to_yuv is exact."""
    f = yuv_format(fmt)
    (x,), hp, wp, out, (y, u, v) = _crop_to_payload("frame_to_yuv", [frame], top, left, h, w, fmt[0], out)
    with on_device(x):
        L.check(L.yuvlib().binyuv_from_frame(_ptr(x), hp, wp, top, left, h, w, C.byref(f), y, u, v, _stream()), "frame_to_yuv")
    return out


# --------------------------------------------------------------------------------------------- clip glue (libbinclip.so)
def yuv_to_bgr(payloads, h, w, fmt, out=None):
    """The Y4M payloads of n frames (device uint8 [n, stride], stride >= frame_bytes, each row contiguous: frame i is the first
    frame_bytes bytes of row i, the rest of a row is never read) -> uint8 [n, h, w, 3] HWC BGR, the frames of the device frame cache
    (into `out` when given: a contiguous uint8 [n, h, w, 3], e.g. arena[i:j]).  One launch; per frame the bytes of
    frame_to_u8(yuv_to_frame(payload, pads 0)) (include/binclip.h).  fmt: (chroma, matrix, range)."""
    f = yuv_format(fmt)
    if h < 1 or w < 1:
        raise ValueError(f"bin_amd: yuv_to_bgr needs a positive size (got {h}x{w})")
    need = yuv_frame_bytes(h, w, fmt[0])[0]
    if payloads.dtype != torch.uint8 or payloads.dim() != 2 or payloads.shape[0] < 1 or payloads.shape[1] < need or \
            (payloads.shape[1] > 1 and payloads.stride(1) != 1) or (payloads.shape[0] > 1 and payloads.stride(0) < payloads.shape[1]):
        raise ValueError(f"bin_amd: the payloads of {w}x{h} {fmt[0]} frames are a uint8 tensor [n, stride >= {need}] with contiguous rows "
                         f"(got {payloads.dtype} {tuple(payloads.shape)}, strides {tuple(payloads.stride())})")
    n = payloads.shape[0]
    stride = payloads.stride(0) if n > 1 else payloads.shape[1]
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (n, h, w, 3) or not out.is_contiguous() or out.device != payloads.device):
        raise ValueError(f"bin_amd: yuv_to_bgr fills a contiguous uint8 [{n}, {h}, {w}, 3] on the payloads' device "
                         f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
    _need_cuda(payloads, out)
    if out is None:
        out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=payloads.device)
    with on_device(payloads):
        L.check(L.cliplib().binclip_yuv_to_bgr(_ptr(payloads), n, stride, h, w, C.byref(f), _ptr(out), _stream()), "yuv_to_bgr")
    return out


# --------------------------------------------------------------------------------------------- crop glue (libbincrop.so)
CROP_ROW_FIELDS = ("offset", "H", "W", "y0", "x0", "format")


def yuv_format_index(fmt):
    """The format index of a crop row: 2 * matrix + range of (chroma, matrix, range) (include/bincrop.h)."""
    f = yuv_format(fmt)
    return 2 * f.matrix + f.range


def yuv_crops_to_bgr(arena_u8, rows_host, crop, chroma, out=None):
    """Crops of YUV frames that lie in a byte arena -> uint8 [n_rows, ch, cw, 3] HWC BGR in one launch (bincrop_yuv_crops_to_bgr,
    libbincrop.so): per row the bytes yuv_to_bgr gives the crop of that frame.  `arena_u8`: contiguous uint8 [bytes] device tensor;
    `rows_host`: integer [n_rows, 6] on the HOST, per decoded frame (payload offset, H, W, y0, x0, format index: yuv_format_index);
    `crop`: (ch, cw); `chroma`: 420 | 444, of every row.  The table is checked here (the kernel only clamps): every payload inside the
    arena, every crop inside its frame, every format index known; a ValueError names the row and what is wrong with it.  It is
    uploaded through pinned memory without a host sync and the kernel launched on the current stream.  `out`: a contiguous uint8
    [n_rows, ch, cw, 3] on the arena's device to fill."""
    import numpy as np
    if arena_u8.dtype != torch.uint8 or arena_u8.dim() != 1 or arena_u8.numel() < 1 or not arena_u8.is_contiguous():
        raise ValueError(f"yuv_crops_to_bgr: the arena must be a contiguous uint8 [bytes] tensor, got {arena_u8.dtype} {tuple(arena_u8.shape)}")
    if chroma not in (420, 444):
        raise ValueError(f"yuv_crops_to_bgr: unknown chroma {chroma!r}: 420 | 444")
    ch, cw = (int(v) for v in crop)
    if ch < 1 or cw < 1:
        raise ValueError(f"yuv_crops_to_bgr: a crop of {ch}x{cw}")
    tab = np.asarray(rows_host.numpy() if torch.is_tensor(rows_host) else rows_host)
    if tab.ndim != 2 or tab.shape[0] < 1 or tab.shape[1] != len(CROP_ROW_FIELDS) or tab.dtype.kind not in "iu":
        raise ValueError(f"yuv_crops_to_bgr: rows must be an integer [n_rows, {len(CROP_ROW_FIELDS)}] table "
                         f"({', '.join(CROP_ROW_FIELDS)}), got {tab.dtype} {tab.shape}")
    tab = tab.astype(np.int64)
    off, h, w, y0, x0, fmt = (tab[:, i] for i in range(6))
    nbytes = arena_u8.numel()

    def refuse(bad, what):
        if bad.any():
            r = int(np.argmax(bad))
            raise ValueError(f"yuv_crops_to_bgr: row {r}: {what} (offset {off[r]}, {w[r]}x{h[r]} frame, crop {cw}x{ch} at "
                             f"({y0[r]}, {x0[r]}), format {fmt[r]})")
    refuse((h < 1) | (w < 1) | (h > 2 ** 31 - 1) | (w > 2 ** 31 - 1), "the frame size is not positive")
    c_h, c_w = (h, w) if chroma == 444 else ((h + 1) // 2, (w + 1) // 2)
    frame_bytes = h * w + 2 * c_h * c_w
    refuse((off < 0) | (off > nbytes - frame_bytes), f"the payload leaves the arena of {nbytes} bytes")
    refuse((y0 < 0) | (x0 < 0) | (y0 > h - ch) | (x0 > w - cw), "the crop leaves the frame")
    refuse((fmt < 0) | (fmt >= L.CROP_FORMATS), f"the format index is outside [0, {L.CROP_FORMATS})")
    n = tab.shape[0]
    if out is not None and (out.dtype != torch.uint8 or tuple(out.shape) != (n, ch, cw, 3) or not out.is_contiguous() or
                            out.device != arena_u8.device):
        raise ValueError(f"yuv_crops_to_bgr: fills a contiguous uint8 [{n}, {ch}, {cw}, 3] on the arena's device "
                         f"(got {out.dtype} {tuple(out.shape)} on {out.device})")
    _need_cuda(arena_u8, out)
    words = np.zeros((n, 8), dtype=np.int32)                 # BinCropRow: int64 offset, then H, W, y0, x0, format, reserved
    words[:, :2] = off.astype("<i8").view(np.int32).reshape(n, 2)
    words[:, 2:7] = tab[:, 1:6]
    dev = arena_u8.device
    with on_device(arena_u8):
        table = torch.from_numpy(words).pin_memory().to(dev, non_blocking=True)
        if out is None:
            out = torch.empty((n, ch, cw, 3), dtype=torch.uint8, device=dev)
        L.check(L.croplib().bincrop_yuv_crops_to_bgr(_ptr(arena_u8), nbytes, _ptr(table), n, ch, cw, int(chroma), _ptr(out), _stream()),
                "yuv_crops_to_bgr")
    return out


# --------------------------------------------------------------------------------------------- rate glue (libbinrate.so)
def blend_to_yuv(a, b, w, top, left, h, w_, fmt, out=None):
    """Two fp32 [1,3,Hp,Wp] (or [3,Hp,Wp]) RGB frames of one shape -> the Y4M payload of the crop of a + w (b - a), 0 <= w < 1, on
    clamped values (include/binrate.h): one launch, frame_to_yuv's conversion and its `out`.  w == 0 and `b is a` give
    frame_to_yuv(a)'s bytes."""
    f = yuv_format(fmt)
    (a, b), hp, wp, out, (y, u, v) = _crop_to_payload("blend_to_yuv", [a, b], top, left, h, w_, fmt[0], out)
    w = float(w)
    if not 0.0 <= w < 1.0:
        raise ValueError(f"bin_amd: blend_to_yuv takes a weight in [0, 1) (got {w})")
    with on_device(a):
        L.check(L.ratelib().binrate_blend_to_yuv(_ptr(a), _ptr(b), w, hp, wp, top, left, h, w_, C.byref(f), y, u, v, _stream()),
                "blend_to_yuv")
    return out


# --------------------------------------------------------------------------------------------- records (scene and score glue)
def _record_out(out, nbytes, what, inputs, device):
    """The device record a kernel fills: `out` when it is one (a contiguous uint8 [nbytes] on `device`), a fresh one when None."""
    if out is None:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() != nbytes or out.device != device:
        raise ValueError(f"bin_amd: a {what} record is a contiguous uint8 tensor of [{nbytes}] bytes on the {inputs}' device "
                         f"(got {out.dtype} {tuple(out.shape)})")
    return out


def _read_record(record, struct, what, reader):
    """A downloaded record (a uint8 tensor or array of the struct's size, or its bytes) as the ctypes `struct`."""
    import numpy as np
    if isinstance(record, torch.Tensor):
        if record.is_cuda:
            raise ValueError(f"bin_amd: {reader} reads a downloaded record (record.cpu())")
        record = record.numpy()
    raw = bytes(memoryview(np.ascontiguousarray(record)).cast("B"))
    if len(raw) != C.sizeof(struct):
        raise ValueError(f"bin_amd: a {what} record has {C.sizeof(struct)} bytes (got {len(raw)})")
    return struct.from_buffer_copy(raw)


# --------------------------------------------------------------------------------------------- scene glue (libbinscene.so)
LUMA_RECORD_BYTES = C.sizeof(L.BinSceneRecord)          # 264: a uint64 SAD, then 64 uint32 bins


def luma_stats(cur_y, prev_y, h, w, out=None):
    """The scene-cut statistics of a luma plane (include/binscene.h): `cur_y`, `prev_y` (or None) are contiguous uint8 device tensors
    of h*w bytes, views into a payload at any byte offset included.  Returns the device uint8 [264] record (`out` when given; it must
    be 8-byte aligned): the sum of |cur - prev| and the 64-bin histogram of cur >> 2.  `read_luma_record` reads a downloaded one."""
    _need_cuda(cur_y, prev_y, out)
    if h < 1 or w < 1:
        raise ValueError(f"bin_amd: luma_stats needs a positive size (got {h}x{w})")
    for name, t in (("cur_y", cur_y), ("prev_y", prev_y)):
        if t is not None and (t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() != h * w):
            raise ValueError(f"bin_amd: {name} of a {w}x{h} frame is a contiguous uint8 tensor of {h * w} bytes "
                             f"(got {t.dtype} {tuple(t.shape)})")
    if prev_y is not None and prev_y.device != cur_y.device:
        raise ValueError("bin_amd: luma_stats takes two planes of one device")
    out = _record_out(out, LUMA_RECORD_BYTES, "luma", "planes", cur_y.device)
    with on_device(cur_y):
        L.check(L.scenelib().binscene_luma_stats(_ptr(cur_y), _ptr(prev_y), h, w, _ptr(out), _stream()), "luma_stats")
    return out


def read_luma_record(record):
    """(sad: int, hist: np.ndarray[64] of int64) of a luma record on the host: a uint8 [264] tensor or array, or its bytes."""
    import numpy as np
    rec = _read_record(record, L.BinSceneRecord, "luma", "read_luma_record")
    return int(rec.sad), np.array(rec.hist, dtype=np.int64)


# --------------------------------------------------------------------------------------------- score glue (libbinscore.so)
PLANE_SCORES_BYTES = C.sizeof(L.BinPlaneScores)         # 64: uint64 sse[3], sad[3] (Y, U, V), then the two SSIMs of the Y plane
_score_ws = {}                                          # (device, stream, h, w, chroma, flags) -> workspace


def payload_scores(a, b, h, w, chroma, ssim=True, out=None):
    """The scores of one Y4M payload against another on the device (include/binscore.h): `a`, `b` are uint8 device payloads of an
    h x w frame of `chroma` (420 | 444), or (y, u, v) triples of plane tensors, views at any byte offset included; `a is b` is
    legal.  Returns the device uint8 [64] record (`out` when given; it must be 8-byte aligned): per plane the exact sums of (a - b)^2
    and |a - b|, and of the Y plane as a one-channel image util.calculate_ssim's SSIM and util.compare_ssim's.  Current stream, no
    host sync; the workspace is cached per stream and shape, so calls on one stream may follow each other freely.  `ssim=False`
    computes only the sums (both SSIMs NaN); an SSIM the plane is too small for is NaN (ssim_g11 below 11 x 11), and below 7 x 7
    an SSIM request raises, as frame_scores does.  `read_plane_scores` reads a downloaded record."""
    global _G11_TAPS
    if chroma not in (420, 444) or h < 1 or w < 1:
        raise ValueError(f"bin_amd: payload_scores needs a positive size and chroma 420 | 444 (got {h}x{w}, {chroma!r})")
    pa, pb = _yuv_planes(a, h, w, chroma), _yuv_planes(b, h, w, chroma)
    first = a[0] if isinstance(a, (tuple, list)) else a
    other = b[0] if isinstance(b, (tuple, list)) else b
    if first.device != other.device:
        raise ValueError("bin_amd: payload_scores takes two payloads of one device")
    _need_cuda(out)
    flags = 0
    if ssim:
        flags = L.PLANE_SSIM_U7 | (L.PLANE_SSIM_G11 if min(h, w) >= 11 else 0)
    if _G11_TAPS is None:
        from .utils.util import _gauss_taps
        _G11_TAPS = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    out = _record_out(out, PLANE_SCORES_BYTES, "score", "payloads", first.device)
    lib = L.scorelib()
    with on_device(first):
        nb = lib.binscore_workspace_bytes(h, w, chroma, flags)
        if nb == 0:
            raise RuntimeError(f"bin_amd: payload_scores: unsupported frame size {h} x {w} (SSIM needs 7 x 7 pixels)")
        stream = _stream()
        key = (_device_key(first.device), stream.value, h, w, chroma, flags)
        ws = _score_ws.get(key)
        if ws is None:
            ws = _score_ws[key] = torch.empty(nb, dtype=torch.uint8, device=first.device)
        L.check(lib.binscore_planes(*pa, *pb, h, w, chroma, flags, _G11_TAPS, _ptr(ws), nb, _ptr(out), stream), "payload_scores")
    return out


def read_plane_scores(record):
    """(sse_y, sse_u, sse_v, sad_y, sad_u, sad_v, ssim_g11, ssim_u7) of a score record on the host, six ints and two floats: a
    uint8 [64] tensor or array, or its bytes."""
    rec = _read_record(record, L.BinPlaneScores, "score", "read_plane_scores")
    return tuple(int(v) for v in rec.sse) + tuple(int(v) for v in rec.sad) + (float(rec.ssim_g11), float(rec.ssim_u7))


def pixel_unshuffle(x, r=2):
    """Exact space-to-depth: out[b, c*r*r + i*r + j, y, x] = in[b, c, y*r+i, x*r+j] (reference RDN.py:107-132)."""
    _need_cuda(x)
    x = x.contiguous().float()
    n, c, h, w = x.shape
    if h % r or w % r or r < 1:
        raise RuntimeError(f"bin_amd: pixel_unshuffle needs H, W divisible by r (got {h}x{w}, r={r})")
    y = torch.empty((n, c * r * r, h // r, w // r), dtype=torch.float32, device=x.device)
    L.check(L.lib().binhip_pixel_unshuffle_f32(_ptr(x), n, c, h, w, r, _ptr(y), _stream()), "pixel_unshuffle")
    return y


# --------------------------------------------------------------------------------------------- evaluation metrics
_G11_TAPS = None


def image_scores(a_u8, b_u8, ssim=True):
    """Scores of image pairs on the device (binhip_image_score; test.py:404-456, utils/util.py:201-251).  `a_u8`, `b_u8`: uint8
    [H,W,3] or [n,H,W,3] device tensors (HWC, either channel order).  Returns a float64 device tensor [n,4] of
    (sse, sad, ssim_g11, ssim_u7) per pair, launched on the current stream without a host sync: sse and sad are exact sums
    (below 2^53, so float64 holds them exactly), ssim_g11 is util.calculate_ssim's SSIM, ssim_u7 the reference test.py's
    (util.compare_ssim).  `ssim=False` computes only the sums; an SSIM the image is too small for is NaN (ssim_g11 below
    11 x 11, as numpy's mean of an empty map), and below 7 x 7 an SSIM request raises.  util.score_row turns a row into
    {psnr, mae, ssim, ssim_sk}."""
    global _G11_TAPS
    _need_cuda(a_u8, b_u8)
    if a_u8.dtype != torch.uint8 or b_u8.dtype != torch.uint8 or a_u8.shape != b_u8.shape:
        raise ValueError("image_scores: two uint8 tensors of one shape")
    a = a_u8.unsqueeze(0) if a_u8.dim() == 3 else a_u8
    b = b_u8.unsqueeze(0) if b_u8.dim() == 3 else b_u8
    if a.dim() != 4 or a.shape[3] != 3:
        raise ValueError(f"image_scores: [H,W,3] or [n,H,W,3] images, got {tuple(a_u8.shape)}")
    a, b = a.contiguous(), b.contiguous()
    n, h, w, _ = a.shape
    flags = 0
    if ssim:
        flags = L.SCORE_SSIM_U7 | (L.SCORE_SSIM_G11 if min(h, w) >= 11 else 0)
    if _G11_TAPS is None:
        from .utils.util import _gauss_taps
        _G11_TAPS = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    lib = L.lib()
    with on_device(a):
        nb = lib.binhip_image_score_workspace_bytes(n, h, w, flags)
        if nb == 0:
            raise RuntimeError(f"bin_amd: image_scores: unsupported shape {tuple(a.shape)} (SSIM needs 7 x 7 pixels)")
        ws = torch.empty(nb, dtype=torch.uint8, device=a.device)
        raw = torch.empty((n, 4), dtype=torch.int64, device=a.device)          # BinImageScore {int64 sse, sad; double g11, u7}
        L.check(lib.binhip_image_score(_ptr(a), _ptr(b), n, h, w, flags, _G11_TAPS, _ptr(ws), nb, _ptr(raw), _stream()),
                "image_score")
        out = torch.empty((n, 4), dtype=torch.float64, device=a.device)
        out[:, :2] = raw[:, :2]
        out[:, 2:] = raw[:, 2:].view(torch.float64)
    return out


def frame_scores(xs, ys, ssim=True):
    """The scores of image_scores straight from fp32 frames (binhip_frame_score; the validation loop of
    models/bin_model.py:564-589).  `xs`, `ys`: equally long sequences of float32 device tensors [3,H,W] or [1,3,H,W] of one
    H x W; pair i is (xs[i], ys[i]) and a tensor may appear in several pairs and on either side.  Every value is quantised
    as util.tensor2img / frame_to_u8 do (clamp to [0, 1], x 255, round half to even; NaN -> 0) inside the kernel, which
    writes no u8 image, and the pair is scored as image_scores scores the two images.  Returns a float64 device tensor
    [n,4] of (sse, sad, ssim_g11, ssim_u7) with image_scores' conventions: current stream, no host sync, NaN for an SSIM
    the frame is too small for, and below 7 x 7 an SSIM request raises.  Lists longer than BINHIP_SCORE_MAX_PAIRS take
    several calls.  A non-contiguous tensor is copied."""
    global _G11_TAPS
    xs, ys = list(xs), list(ys)
    if not xs or len(xs) != len(ys):
        raise ValueError(f"frame_scores: two equally long, non-empty sequences of frames, got {len(xs)} and {len(ys)}")
    _need_cuda(*xs, *ys)
    shape = None
    frames = []
    for t in xs + ys:
        if t.dtype != torch.float32:
            raise ValueError(f"frame_scores: float32 frames, got {t.dtype}")
        if not ((t.dim() == 3 and t.shape[0] == 3) or (t.dim() == 4 and tuple(t.shape[:2]) == (1, 3))):
            raise ValueError(f"frame_scores: [3,H,W] or [1,3,H,W] frames, got {tuple(t.shape)}")
        if shape is None:
            shape = tuple(t.shape[-2:])
        if tuple(t.shape[-2:]) != shape or t.device != xs[0].device:
            raise ValueError(f"frame_scores: frames of one H x W on one device, got {tuple(t.shape)} next to {shape}")
        frames.append(t.detach().contiguous())
    h, w = shape
    n = len(xs)
    flags = 0
    if ssim:
        flags = L.SCORE_SSIM_U7 | (L.SCORE_SSIM_G11 if min(h, w) >= 11 else 0)
    if _G11_TAPS is None:
        from .utils.util import _gauss_taps
        _G11_TAPS = (C.c_double * 11)(*[float(v) for v in _gauss_taps()])
    lib = L.lib()
    dev = xs[0].device
    with on_device(xs[0]):
        raw = torch.empty((n, 4), dtype=torch.int64, device=dev)               # BinImageScore {int64 sse, sad; double g11, u7}
        for i0 in range(0, n, L.SCORE_MAX_PAIRS):
            m = min(L.SCORE_MAX_PAIRS, n - i0)
            nb = lib.binhip_frame_score_workspace_bytes(m, h, w, flags)
            if nb == 0:
                raise RuntimeError(f"bin_amd: frame_scores: unsupported frame size {h} x {w} (SSIM needs 7 x 7 pixels)")
            ws = torch.empty(nb, dtype=torch.uint8, device=dev)
            px = (C.c_void_p * m)(*[frames[i0 + i].data_ptr() for i in range(m)])
            py = (C.c_void_p * m)(*[frames[n + i0 + i].data_ptr() for i in range(m)])
            L.check(lib.binhip_frame_score(px, py, m, h, w, flags, _G11_TAPS, _ptr(ws), nb, _ptr(raw[i0:i0 + m]), _stream()),
                    "frame_score")
        out = torch.empty((n, 4), dtype=torch.float64, device=dev)
        out[:, :2] = raw[:, :2]
        out[:, 2:] = raw[:, 2:].view(torch.float64)
    return out


# --------------------------------------------------------------------------------------------- training data
GATHER_MAX_SLOTS = 32        # n_slots limit of binhip_gather_windows


def gather_windows(frames_u8, table_host, crop):
    """Training crops cut out of a device-resident frame arena in one launch (binhip_gather_windows; the reference loader's
    crop / np.fliplr / BGR -> RGB / read_img's /255 and feed_data's staging, data/BIN_dataset.py, models/bin_model.py).
    `frames_u8`: uint8 [n_frames, H, W, 3] BGR device tensor; `table_host`: int32 [n, n_slots + 3] on the HOST, per sample the
    frame ids in slot order then y0, x0, flip; `crop`: (ch, cw).  The table is checked here (the kernel only clamps), uploaded
    through pinned memory without a host sync and the kernel launched on the current stream.  Returns fp32 [n_slots, n, 3, ch, cw]."""
    import numpy as np
    _need_cuda(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError(f"gather_windows: frames must be a contiguous uint8 [n_frames, H, W, 3] tensor, got "
                         f"{frames_u8.dtype} {tuple(frames_u8.shape)}")
    nf, h, w, _ = frames_u8.shape
    ch, cw = (int(v) for v in crop)
    tab = np.ascontiguousarray(table_host.numpy() if torch.is_tensor(table_host) else table_host, dtype=np.int32)
    if tab.ndim != 2 or tab.shape[0] < 1 or not 1 <= tab.shape[1] - 3 <= GATHER_MAX_SLOTS:
        raise ValueError(f"gather_windows: table must be [n, n_slots + 3] with 1 <= n_slots <= {GATHER_MAX_SLOTS}, "
                         f"got {tab.shape}")
    if not (0 < ch <= h and 0 < cw <= w):
        raise ValueError(f"gather_windows: crop {ch}x{cw} does not fit {h}x{w} frames")
    n, n_slots = tab.shape[0], tab.shape[1] - 3
    ids, y0, x0, flip = tab[:, :n_slots], tab[:, n_slots], tab[:, n_slots + 1], tab[:, n_slots + 2]
    if ids.min() < 0 or ids.max() >= nf:
        raise ValueError(f"gather_windows: frame id outside [0, {nf})")
    if y0.min() < 0 or y0.max() > h - ch or x0.min() < 0 or x0.max() > w - cw:
        raise ValueError(f"gather_windows: crop offset outside the {h}x{w} frame for a {ch}x{cw} crop")
    if ((flip != 0) & (flip != 1)).any():
        raise ValueError("gather_windows: flip must be 0 or 1")
    dev = frames_u8.device
    with on_device(frames_u8):
        table = torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)
        out = torch.empty((n_slots, n, 3, ch, cw), dtype=torch.float32, device=dev)
        L.check(L.lib().binhip_gather_windows(_ptr(frames_u8), nf, h, w, _ptr(table), n, n_slots, ch, cw, _ptr(out), _stream()),
                "gather_windows")
    return out


GATHER_MAX_HALF = 16         # h limit of binhip_gather_windows_blur: exposures of 2h + 1 <= 33 sharp frames


def gather_windows_blur(frames_u8, table_host, crop, n_blur, clip_ranges=None):
    """gather_windows with the first `n_blur` slots synthesised as the reference's blurry frames: the truncated mean of the
    2h + 1 arena frames around the slot's id (binhip_gather_windows_blur; the reference's
    data_scripts/adobe240fps/create_dataset_blur_N_frames_average.py:116-134).  `table_host`: int32 [n, n_slots + 4] on the
    HOST, a gather_windows row followed by the sample's h.  The arena must hold the sharp frames of a clip consecutively in
    file order; `clip_ranges` (int [clips, 2], [start, end) arena ids per clip), when given, is checked against every blurry
    range.  Checked here (the kernel only clamps): everything gather_windows checks, h in [0, 16], id - h .. id + h inside
    the arena and inside one clip.  Returns fp32 [n_slots, n, 3, ch, cw]."""
    import numpy as np
    _need_cuda(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError(f"gather_windows_blur: frames must be a contiguous uint8 [n_frames, H, W, 3] tensor, got "
                         f"{frames_u8.dtype} {tuple(frames_u8.shape)}")
    nf, h, w, _ = frames_u8.shape
    ch, cw = (int(v) for v in crop)
    tab = np.ascontiguousarray(table_host.numpy() if torch.is_tensor(table_host) else table_host, dtype=np.int32)
    if tab.ndim != 2 or tab.shape[0] < 1 or not 1 <= tab.shape[1] - 4 <= GATHER_MAX_SLOTS:
        raise ValueError(f"gather_windows_blur: table must be [n, n_slots + 4] with 1 <= n_slots <= {GATHER_MAX_SLOTS}, "
                         f"got {tab.shape}")
    n, n_slots, n_blur = tab.shape[0], tab.shape[1] - 4, int(n_blur)
    if not 0 <= n_blur <= n_slots:
        raise ValueError(f"gather_windows_blur: n_blur {n_blur} outside [0, {n_slots}]")
    if not (0 < ch <= h and 0 < cw <= w):
        raise ValueError(f"gather_windows_blur: crop {ch}x{cw} does not fit {h}x{w} frames")
    ids, y0, x0, flip, half = (tab[:, :n_slots], tab[:, n_slots], tab[:, n_slots + 1], tab[:, n_slots + 2],
                               tab[:, n_slots + 3])
    if ids.min() < 0 or ids.max() >= nf:
        raise ValueError(f"gather_windows_blur: frame id outside [0, {nf})")
    if y0.min() < 0 or y0.max() > h - ch or x0.min() < 0 or x0.max() > w - cw:
        raise ValueError(f"gather_windows_blur: crop offset outside the {h}x{w} frame for a {ch}x{cw} crop")
    if ((flip != 0) & (flip != 1)).any():
        raise ValueError("gather_windows_blur: flip must be 0 or 1")
    if half.min() < 0 or half.max() > GATHER_MAX_HALF:
        raise ValueError(f"gather_windows_blur: h outside [0, {GATHER_MAX_HALF}]")
    if n_blur:
        lo, hi = ids[:, :n_blur] - half[:, None], ids[:, :n_blur] + half[:, None]
        if lo.min() < 0 or hi.max() >= nf:
            raise ValueError(f"gather_windows_blur: a blurry centre's id - h .. id + h leaves the arena [0, {nf})")
        if clip_ranges is not None:
            cr = np.asarray(clip_ranges, dtype=np.int64).reshape(-1, 2)
            cr = cr[np.argsort(cr[:, 0])]
            clip = np.searchsorted(cr[:, 0], lo, side="right") - 1         # the clip that holds the first frame of the range
            if (clip < 0).any() or (hi >= cr[np.maximum(clip, 0), 1]).any():
                raise ValueError("gather_windows_blur: a blurry centre's id - h .. id + h crosses a clip boundary")
    dev = frames_u8.device
    with on_device(frames_u8):
        table = torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)
        out = torch.empty((n_slots, n, 3, ch, cw), dtype=torch.float32, device=dev)
        L.check(L.lib().binhip_gather_windows_blur(_ptr(frames_u8), nf, h, w, _ptr(table), n, n_slots, n_blur, ch, cw, _ptr(out),
                                                   _stream()), "gather_windows_blur")
    return out


_curve_dev = {}                                          # (the 768 words as bytes, device) -> their device copy


def exposure_curve(gamma, noise=None):
    """The curve of the dataset options `blur_gamma` and `blur_noise` (bin_amd/data/exposure.py): uint32 [3, 256] on the HOST,
    LIN, MID and SIG of include/binexpose.h, built once per (gamma, noise) and accepted by binexpose_check_curve.  `gamma`: a
    number 1.0 .. 2.4 or "srgb"; `noise`: None or (read, shot).  gather_windows_exposed uploads it once per device."""
    from .data import exposure as X
    gamma, noise = X.parse_blur_gamma(gamma), X.parse_blur_noise(noise)
    if gamma is None:
        raise ValueError("exposure_curve: a gamma (a number 1.0 .. 2.4 or \"srgb\") is required")
    return _exposure_curve(gamma, noise)


@functools.lru_cache(maxsize=None)
def _exposure_curve(gamma, noise):
    from .data import exposure as X
    tab = _checked_curve(X.curve_tables(gamma, noise))
    tab.setflags(write=False)
    return tab


def _checked_curve(curve):
    import numpy as np
    tab = np.ascontiguousarray(curve, dtype=np.uint32)
    if tab.shape != (3, L.EXPOSE_TABLE):
        raise ValueError(f"exposure curve: uint32 [3, {L.EXPOSE_TABLE}] tables (LIN, MID, SIG), got {tab.shape}")
    if L.exposelib().binexpose_check_curve(*(tab[i].ctypes.data for i in range(3))) != 0:
        raise ValueError("exposure curve: the tables break a validity rule of include/binexpose.h (binexpose_check_curve)")
    return tab


def gather_windows_exposed(frames_u8, table_host, crop, n_blur, curve, clip_ranges=None):
    """gather_windows_blur with the first `n_blur` slots synthesised as a camera exposure (binexpose_gather, libbinexpose.so): the
    mean of the 2h + 1 arena frames around the slot's id in linear light, sensor noise added there, re-encoded to a code; the
    arithmetic is specified in include/binexpose.h.  `table_host`: int32 [n, n_slots + 6] on the HOST, a gather_windows_blur row
    followed by the sample's key words k0, k1 (their 32 bits); `curve`: exposure_curve's tables.  Checked here (the kernel only
    clamps): everything gather_windows_blur checks, and a curve not seen before by binexpose_check_curve.  Returns fp32
    [n_slots, n, 3, ch, cw]."""
    import numpy as np
    _need_cuda(frames_u8)
    if frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4 or frames_u8.shape[3] != 3 or not frames_u8.is_contiguous():
        raise ValueError(f"gather_windows_exposed: frames must be a contiguous uint8 [n_frames, H, W, 3] tensor, got "
                         f"{frames_u8.dtype} {tuple(frames_u8.shape)}")
    nf, h, w, _ = frames_u8.shape
    ch, cw = (int(v) for v in crop)
    tab = np.ascontiguousarray(table_host.numpy() if torch.is_tensor(table_host) else table_host, dtype=np.int32)
    if tab.ndim != 2 or tab.shape[0] < 1 or not 1 <= tab.shape[1] - 6 <= GATHER_MAX_SLOTS:
        raise ValueError(f"gather_windows_exposed: table must be [n, n_slots + 6] with 1 <= n_slots <= {GATHER_MAX_SLOTS}, "
                         f"got {tab.shape}")
    n, n_slots, n_blur = tab.shape[0], tab.shape[1] - 6, int(n_blur)
    if not 0 <= n_blur <= n_slots:
        raise ValueError(f"gather_windows_exposed: n_blur {n_blur} outside [0, {n_slots}]")
    if not (0 < ch <= h and 0 < cw <= w):
        raise ValueError(f"gather_windows_exposed: crop {ch}x{cw} does not fit {h}x{w} frames")
    ids, y0, x0, flip, half = (tab[:, :n_slots], tab[:, n_slots], tab[:, n_slots + 1], tab[:, n_slots + 2],
                               tab[:, n_slots + 3])
    if ids.min() < 0 or ids.max() >= nf:
        raise ValueError(f"gather_windows_exposed: frame id outside [0, {nf})")
    if y0.min() < 0 or y0.max() > h - ch or x0.min() < 0 or x0.max() > w - cw:
        raise ValueError(f"gather_windows_exposed: crop offset outside the {h}x{w} frame for a {ch}x{cw} crop")
    if ((flip != 0) & (flip != 1)).any():
        raise ValueError("gather_windows_exposed: flip must be 0 or 1")
    if half.min() < 0 or half.max() > GATHER_MAX_HALF:
        raise ValueError(f"gather_windows_exposed: h outside [0, {GATHER_MAX_HALF}]")
    if n_blur:
        lo, hi = ids[:, :n_blur] - half[:, None], ids[:, :n_blur] + half[:, None]
        if lo.min() < 0 or hi.max() >= nf:
            raise ValueError(f"gather_windows_exposed: a blurry centre's id - h .. id + h leaves the arena [0, {nf})")
        if clip_ranges is not None:
            cr = np.asarray(clip_ranges, dtype=np.int64).reshape(-1, 2)
            cr = cr[np.argsort(cr[:, 0])]
            clip = np.searchsorted(cr[:, 0], lo, side="right") - 1         # the clip that holds the first frame of the range
            if (clip < 0).any() or (hi >= cr[np.maximum(clip, 0), 1]).any():
                raise ValueError("gather_windows_exposed: a blurry centre's id - h .. id + h crosses a clip boundary")
    dev = frames_u8.device
    words = np.ascontiguousarray(curve, dtype=np.uint32)
    key = (words.tobytes(), dev)
    with on_device(frames_u8):
        if key not in _curve_dev:
            _curve_dev[key] = torch.from_numpy(_checked_curve(words).reshape(-1).copy()).to(dev)
        table = torch.from_numpy(tab).pin_memory().to(dev, non_blocking=True)
        out = torch.empty((n_slots, n, 3, ch, cw), dtype=torch.float32, device=dev)
        L.check(L.exposelib().binexpose_gather(_ptr(frames_u8), nf, h, w, _ptr(table), n, n_slots, n_blur, ch, cw,
                                               _ptr(_curve_dev[key]), _ptr(out), _stream()), "gather_windows_exposed")
    return out


# --------------------------------------------------------------------------------------------- optimizer
def _check_row_tensors(what, named_tensors):
    """One row of a by-value table (adam_row, ema_row, grad_rows): float32 contiguous device tensors of one size on one device, not
    empty.  `named_tensors`: (name, tensor) pairs; a name of None leaves the ` for <name>` out of the message.  The sizes are compared
    with the tensor named p.  Raises on CPU tensors (there is no CPU fallback)."""
    _need_cuda(*(t for _, t in named_tensors))
    p = dict(named_tensors).get("p", named_tensors[0][1])
    for name, t in named_tensors:
        suffix = "" if name is None else f" for {name}"
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: float32 tensors, got {t.dtype}{suffix}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: contiguous tensors, got strides {tuple(t.stride())} of shape {tuple(t.shape)}{suffix}")
        if t.numel() != p.numel() or t.device != p.device:
            raise ValueError(f"{what}: {name} has {t.numel()} elements on {t.device}, p has {p.numel()} on {p.device}")
    if p.numel() < 1:
        raise ValueError(f"{what}: empty tensor")


def adam_rows(n):
    """A host table of n BinAdamTensor rows for adam_step (bin_amd.optim.Adam keeps one per group and rewrites only what changed)."""
    return (L.BinAdamTensor * max(n, 1))()


def adam_row(table, i, p, g, m, v, step_size, inv_sqrt_bc2):
    """Fill row i of an adam_rows table from four float32 device tensors of one size.  Raises on CPU tensors (there is no CPU
    fallback), on another dtype and on non-contiguous tensors: the kernel walks numel consecutive floats from each pointer."""
    _check_row_tensors("adam_step", (("p", p), ("g", g), ("m", m), ("v", v)))
    r = table[i]
    r.p, r.g, r.m, r.v, r.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel()
    r.step_size, r.inv_sqrt_bc2 = step_size, inv_sqrt_bc2


def adam_launch(table, n, device, beta1, beta2, eps, weight_decay):
    """binopt_adam_step over the first n rows of an adam_rows table, on `device`'s current stream."""
    if n == 0:
        return
    with torch.cuda.device(device):
        L.check(L.optlib().binopt_adam_step(table, n, beta1, beta2, eps, weight_decay, _stream()), "adam_step")


def adam_step(rows, beta1, beta2, eps, weight_decay):
    """One Adam update of every row in place (binopt_adam_step: one elementwise kernel over a by-value table of tensors,
    BINOPT_ADAM_MAX_TENSORS rows per launch, current stream, no host sync).  `rows`: a sequence of
    (p, g, m, v, step_size, inv_sqrt_bc2): float32 contiguous device tensors of one size each (views at any 4-byte offset are
    fine) and the two bias-correction factors lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) of that tensor's step t.  p, m, v
    are written through raw pointers: the caller bumps their version counters (torch.autograd.graph.increment_version).
    Raises on CPU tensors (there is no CPU fallback), on non-float32 and on non-contiguous tensors."""
    rows = list(rows)
    table = adam_rows(len(rows))
    for i, (p, g, m, v, step_size, inv_sqrt_bc2) in enumerate(rows):
        adam_row(table, i, p, g, m, v, step_size, inv_sqrt_bc2)
    if rows:
        if any(r[0].device != rows[0][0].device for r in rows):
            raise ValueError("adam_step: rows of one call live on one device")
        adam_launch(table, len(rows), rows[0][0].device, beta1, beta2, eps, weight_decay)


# --------------------------------------------------------------------------------------------- gradient guard
GRAD_RECORD_WORDS = 8          # BinGradRecord (include/bingrad.h) as int32 words: sumsq (2), norm, coef, flags, status, reserved (2)
GRAD_FLAGS_WORD = 4            # ... the word a data-parallel caller all-reduces with MAX


class GradRows:
    """A host table of BinGradTensor rows over float32 device tensors of one device (grad_rows)."""
    __slots__ = ("table", "n", "device", "workspace_bytes", "numel")

    def __init__(self, table, n, device, workspace_bytes, numel):
        self.table, self.n, self.device, self.workspace_bytes, self.numel = table, n, device, workspace_bytes, numel


def grad_rows(grads):
    """The host row table of grad_norm / grad_scale over `grads`: float32 contiguous device tensors of one device (views at any
    4-byte offset are fine).  The caller keeps it while no pointer changed (bin_amd.optim.GradGuard does).  Raises on CPU tensors
    (there is no CPU fallback), on another dtype and on non-contiguous or empty tensors."""
    grads = list(grads)
    _need_cuda(*grads)
    table = (L.BinGradTensor * max(len(grads), 1))()
    for i, g in enumerate(grads):
        _check_row_tensors("grad_rows", ((None, g),))
        if g.device != grads[0].device:
            raise ValueError("grad_rows: rows of one table live on one device")
        table[i].g, table[i].numel = g.data_ptr(), g.numel()
    nbytes = L.gradlib().bingrad_norm_workspace_bytes(table, len(grads))
    if nbytes < 0:
        L.check(int(nbytes), "grad_norm_workspace_bytes")
    device = grads[0].device if grads else torch.device("cuda", torch.cuda.current_device())
    return GradRows(table, len(grads), device, int(nbytes), sum(g.numel() for g in grads))


def grad_record(device):
    """A device BinGradRecord as 8 int32 words; word GRAD_FLAGS_WORD is `flags`."""
    return torch.zeros(GRAD_RECORD_WORDS, dtype=torch.int32, device=device)


def grad_record_read(words):
    """A BinGradRecord from its 8 int32 words on the HOST (a CPU tensor or a numpy array) -> _lib.BinGradRecord."""
    import numpy as np
    raw = np.ascontiguousarray(words.numpy() if isinstance(words, torch.Tensor) else words, dtype=np.int32)
    assert raw.size == GRAD_RECORD_WORDS
    return L.BinGradRecord.from_buffer_copy(raw.tobytes())


def grad_norm(rows, workspace, record, max_norm=0.0, status=None, status_mask=0):
    """bingrad_norm over a grad_rows table on its device's current stream, no host sync: the global sum of squares in double (one
    deterministic pass, no atomics), its root, the clip coefficient of torch.nn.utils.clip_grad_norm_ for `max_norm` (0 = off) and
    the flags into `record` (grad_record).  `workspace`: the caller's device tensor of at least rows.workspace_bytes bytes;
    `status`: None, or the device status word (status_word), which is read under `status_mask`, never written."""
    _need_cuda(workspace, record, status)
    if workspace.numel() * workspace.element_size() < rows.workspace_bytes or not workspace.is_contiguous():
        raise ValueError(f"grad_norm: workspace of {workspace.numel() * workspace.element_size()} bytes, need {rows.workspace_bytes}")
    if workspace.data_ptr() % 8:
        raise ValueError("grad_norm: the workspace holds doubles: 8-byte aligned")
    if record.dtype != torch.int32 or record.numel() != GRAD_RECORD_WORDS or not record.is_contiguous() or record.data_ptr() % 8:
        raise ValueError("grad_norm: the record is 8 contiguous int32 words, 8-byte aligned (grad_record)")
    if any(t is not None and t.device != rows.device for t in (workspace, record, status)):
        raise ValueError("grad_norm: workspace, record and status word live on the rows' device")
    with torch.cuda.device(rows.device):
        L.check(L.gradlib().bingrad_norm(rows.table, rows.n, float(max_norm), _ptr(status), int(status_mask) & 0xFFFFFFFF, _ptr(workspace),
                                         _ptr(record), _stream()), "grad_norm")


def grad_scale(rows, record):
    """bingrad_scale: g *= record.coef in place in fp32 on the rows' device's current stream; the kernel reads coef on the device and
    writes nothing when it is exactly 1 (not clipped, or a non-finite norm: unlike torch.nn.utils.clip_grad_norm_, which turns a
    gradient set with an inf norm into zeros and NaNs).  The gradients are written through raw pointers."""
    _need_cuda(record)
    if record.dtype != torch.int32 or record.numel() != GRAD_RECORD_WORDS or record.device != rows.device:
        raise ValueError("grad_scale: the record grad_norm wrote (grad_record), on the rows' device")
    if rows.n == 0:
        return
    with torch.cuda.device(rows.device):
        L.check(L.gradlib().bingrad_scale(rows.table, rows.n, _ptr(record), _stream()), "grad_scale")


# --------------------------------------------------------------------------------------------- weight average (EMA)
def ema_rows(n):
    """A host table of n BinEmaTensor rows for ema_launch (bin_amd.optim.WeightEMA keeps one per device while no pointer changed)."""
    return (L.BinEmaTensor * max(n, 1))()


def ema_row(table, i, e, p):
    """Fill row i of an ema_rows table from two float32 device tensors of one size: e, the average, is written; p is only read.
    Raises on CPU tensors (there is no CPU fallback), on another dtype and on non-contiguous tensors: the kernel walks numel
    consecutive floats from each pointer (views at any 4-byte offset are fine)."""
    _check_row_tensors("ema_step", (("e", e), ("p", p)))
    r = table[i]
    r.e, r.p, r.numel = e.data_ptr(), p.data_ptr(), p.numel()


def ema_launch(table, n, device, decay):
    """binema_step over the first n rows of an ema_rows table, on `device`'s current stream, no host sync: e += (1 - decay) * (p - e)
    in fp32, BINEMA_MAX_TENSORS rows per launch.  e is written through raw pointers: the caller bumps its version counters."""
    if n == 0:
        return
    with torch.cuda.device(device):
        L.check(L.emalib().binema_step(table, n, decay, _stream()), "ema_step")


# --------------------------------------------------------------------------------------------- self-ensemble (orient / merge)
def _ens_geometry(what, tensors):
    """(planes, H, W) shared by `tensors`: float32 contiguous device tensors [..., H, W] of one shape on one device.  Raises on CPU
    tensors (there is no CPU fallback), on another dtype and on non-contiguous tensors: the kernels walk planes*H*W consecutive
    floats from each pointer (batch slices and views at any 4-byte offset are fine)."""
    _need_cuda(*tensors)
    first = tensors[0]
    if first.dim() < 2:
        raise ValueError(f"{what}: tensors of at least two dimensions [..., H, W], got shape {tuple(first.shape)}")
    for t in tensors:
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: float32 tensors, got {t.dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: contiguous tensors, got strides {tuple(t.stride())} of shape {tuple(t.shape)}")
        if t.shape != first.shape or t.device != first.device:
            raise ValueError(f"{what}: tensors of one shape on one device, got {tuple(t.shape)} on {t.device} beside "
                             f"{tuple(first.shape)} on {first.device}")
    h, w = first.shape[-2:]
    return first.numel() // max(h * w, 1), h, w


def ens_orient(frames, dsts, flips):
    """binens_orient, one launch, current stream, no host sync: for every frame i (at most BINENS_MAX_SOURCES) and every j,
    dsts[i][j] becomes frames[i] with flips[i][j] (an OR of _lib.ENS_FLIP_W / ENS_FLIP_H) applied per plane.  `dsts` is None, or
    per frame a list whose entries are tensors of the frame's shape (batch slices are fine) or None; what is None is allocated.
    Returns the destinations as a list of lists.  The frames are only read."""
    frames = list(frames)
    flips = [list(f) for f in flips]
    dsts = [[None] * len(f) for f in flips] if dsts is None else [list(d) for d in dsts]
    if len(dsts) != len(frames) or len(flips) != len(frames) or any(len(d) != len(f) for d, f in zip(dsts, flips)):
        raise ValueError("ens_orient: one list of destinations and one list of flips per frame, of equal lengths")
    if not frames:
        return dsts
    _need_cuda(*frames)
    dsts = [[torch.empty_like(x, memory_format=torch.contiguous_format) if d is None else d for d in ds] for x, ds in zip(frames, dsts)]
    planes, h, w = _ens_geometry("ens_orient", frames + [d for ds in dsts for d in ds])
    table = (L.BinEnsOrient * len(frames))()
    for it, x, ds, fs in zip(table, frames, dsts, flips):
        if len(ds) > L.ENS_MAX_ORIENT:
            raise ValueError(f"ens_orient: at most {L.ENS_MAX_ORIENT} destinations per frame, got {len(ds)}")
        it.src, it.n_dst = x.data_ptr(), len(ds)
        for j, (d, f) in enumerate(zip(ds, fs)):
            it.dst[j], it.flip[j] = d.data_ptr(), int(f)
    with on_device(frames[0]):
        L.check(L.enslib().binens_orient(table, len(frames), planes, h, w, _stream()), "ens_orient")
    return dsts


def ens_merge(srcs_per_slot, flip_of, out=None):
    """binens_merge, one launch, current stream, no host sync: for every slot (at most BINENS_MAX_SLOTS) the mean of its M = len(flip_of)
    sources, source o un-flipped by flip_of[o] on the fly, summed as the balanced pairwise tree over o (include/binens.h) and scaled
    by the exact 1/M.  Returns one FRESH tensor per slot (or fills `out`, a list of tensors of the sources' shape): the sources are
    often outputs the network's memo shares with later forwards, and are only read."""
    srcs = [list(s) for s in srcs_per_slot]
    flip_of = [int(f) for f in flip_of]
    m = len(flip_of)
    if any(len(s) != m for s in srcs):
        raise ValueError(f"ens_merge: {m} flips, so {m} sources per slot")
    if not srcs:
        return []
    _need_cuda(*[t for s in srcs for t in s])
    outs = [torch.empty_like(s[0], memory_format=torch.contiguous_format) for s in srcs] if out is None else list(out)
    if len(outs) != len(srcs):
        raise ValueError("ens_merge: one output per slot")
    planes, h, w = _ens_geometry("ens_merge", [t for s in srcs for t in s] + outs)
    if m > L.ENS_MAX_ORIENT:
        raise ValueError(f"ens_merge: at most {L.ENS_MAX_ORIENT} sources per slot, got {m}")
    table = (L.BinEnsMerge * len(srcs))()
    for it, s, o in zip(table, srcs, outs):
        it.dst = o.data_ptr()
        for k, t in enumerate(s):
            it.src[k] = t.data_ptr()
    with on_device(outs[0]):
        L.check(L.enslib().binens_merge(table, len(srcs), m, (C.c_uint8 * max(m, 1))(*flip_of), planes, h, w, _stream()), "ens_merge")
    return outs


# --------------------------------------------------------------------------------------------- chained passes (libbinchain.so)
def reframe(frames, top, left, h, w, pads, out=None):
    """binchain_reframe, one launch, current stream, no host sync: the hand-off between two interpolation passes (include/binchain.h).
    `frames`: a float32 device tensor [N,3,Hs,Ws] (or [3,Hs,Ws]), or a list of at most BINCHAIN_MAX_ITEMS of them, of one shape on one
    device (batch slices and views at any 4-byte offset are fine).  Of each, the crop [top:top+h, left:left+w] goes through
    frame_to_u8's clamp to [0, 1] and is replicate-padded by pads = (left, right, top, bottom).  Returns FRESH tensors
    [..., h+t+b, w+l+r] (one for a tensor, a list for a list), or fills `out` (the same form): the frames are often outputs the
    network's memo shares with later forwards, and are only read."""
    single = isinstance(frames, torch.Tensor)
    srcs = [frames] if single else list(frames)
    if len(pads) != 4 or min(pads) < 0 or h < 1 or w < 1 or top < 0 or left < 0:
        raise ValueError(f"bin_amd: reframe needs a positive crop at a non-negative offset and four non-negative pads "
                         f"(got ({top}, {left}, {h}, {w}), {tuple(pads)})")
    if not srcs:
        return []
    if len(srcs) > L.CHAIN_MAX_ITEMS:
        raise ValueError(f"reframe: at most {L.CHAIN_MAX_ITEMS} frames per call, got {len(srcs)}")
    planes, hs, ws = _ens_geometry("reframe", srcs)
    if top + h > hs or left + w > ws:
        raise ValueError(f"bin_amd: crop ({top}, {left}, {h}, {w}) leaves the {hs}x{ws} frame")
    l, r, t, b = (int(p) for p in pads)
    shape = tuple(srcs[0].shape[:-2]) + (h + t + b, w + l + r)
    if out is None:
        dsts = [torch.empty(shape, dtype=torch.float32, device=srcs[0].device) for _ in srcs]
    else:
        dsts = [out] if isinstance(out, torch.Tensor) else list(out)
        if len(dsts) != len(srcs):
            raise ValueError("reframe: one output per frame")
        _ens_geometry("reframe", dsts)
        if any(tuple(d.shape) != shape or d.device != srcs[0].device for d in dsts):
            raise ValueError(f"reframe: outputs of shape {shape} on the frames' device")
    table = (L.BinChainItem * len(srcs))()
    for it, x, d in zip(table, srcs, dsts):
        it.src, it.dst = x.data_ptr(), d.data_ptr()
    with on_device(srcs[0]):
        L.check(L.chainlib().binchain_reframe(table, len(srcs), planes, hs, ws, int(top), int(left), int(h), int(w), l, r, t, b,
                                              _stream()), "reframe")
    return dsts[0] if single else dsts
