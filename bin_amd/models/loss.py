"""Pixel criteria of bin_model (reference models/bin_model.py:52-60) on the HIP reduction kernels, with backward:
CharbonnierLoss (reference models/loss.py:130-141), and the sum-reduced L1 / L2 losses the option 'pixel_criterion'
can select instead (`nn.L1Loss(reduction='sum')`, `nn.MSELoss(reduction='sum')` in the reference), and CharbonnierSsimLoss
(`cb+ssim`, which the reference names but does not define) on libbinssim.so, and CharbonnierLapLoss (`cb+lap`, the
Laplacian-pyramid criterion of frame interpolation) on libbinlap.so."""
import torch
import torch.nn as nn

from .. import ops
from .. import _lib as L


class _PixelLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, kind, eps):
        ctx.save_for_backward(x, y)
        ctx.kind, ctx.eps = kind, eps
        return ops.pixel_loss(kind, x, y, eps)

    @staticmethod
    def backward(ctx, g):
        x, y = ctx.saved_tensors
        gx = ops.pixel_loss_grad(ctx.kind, x, y, g, ctx.eps)
        return (gx if ctx.needs_input_grad[0] else None,
                -gx if ctx.needs_input_grad[1] else None, None, None)


class _MultiPixelLossFn(torch.autograd.Function):
    """bin_model.get_loss's whole arithmetic as ONE autograd node (round 5): T terms of one criterion and their mean in two
    launches, every gradient in one — instead of a pair of launches and an autograd node per term plus ~100 scalar ATen kernels
    for `sum(loss_list) / len(loss_list)` and its backward, all of which sat between the forward and the backward pass with the
    chip idle.  Same reductions, same rounding order: bit-identical to the per-term path (tests/test_gpu_loss.py)."""

    @staticmethod
    def forward(ctx, kind, eps, index_pairs, *tensors):
        ts = [t.contiguous().float() for t in tensors]
        pairs = [(ts[i], ts[j]) for i, j in index_pairs]
        loss, terms = ops.multi_pixel_loss(kind, pairs, eps)
        ctx.save_for_backward(*ts)
        ctx.kind, ctx.eps, ctx.index_pairs = kind, eps, list(index_pairs)
        ctx.mark_non_differentiable(terms)
        return loss, terms

    @staticmethod
    def backward(ctx, g, _gterms):
        ts = ctx.saved_tensors
        pairs = [(ts[i], ts[j]) for i, j in ctx.index_pairs]
        where = {}
        for term, (i, j) in enumerate(ctx.index_pairs):
            where.setdefault(i, []).append((term, 1.0))
            where.setdefault(j, []).append((term, -1.0))
        need = [k for k in range(len(ts)) if ctx.needs_input_grad[3 + k] and k in where]
        grads = [None] * len(ts)
        # one launch covers every tensor that sits in one or two terms (all of bin_model's); further pairs of terms are added
        chunks = {k: [where[k][i:i + 2] for i in range(0, len(where[k]), 2)] for k in need}
        # (one launch writes at most LOSS_MAX_TERMS gradients: 13-24 pairs with both sides needing one exceed that — advisor r05)
        for i0 in range(0, len(need), L.LOSS_MAX_TERMS):
            part = need[i0:i0 + L.LOSS_MAX_TERMS]
            for k, o in zip(part, ops.multi_pixel_loss_grad(ctx.kind, pairs, g, [(ts[k], chunks[k][0]) for k in part], ctx.eps)):
                grads[k] = o
        for k in need:
            for w in chunks[k][1:]:
                grads[k] = grads[k] + ops.multi_pixel_loss_grad(ctx.kind, pairs, g, [(ts[k], w)], ctx.eps)[0]
        return (None, None, None, *grads)


class _MultiSsimFn(torch.autograd.Function):
    """ssim(x_t, y_t) of T pairs as ONE autograd node: an fp32 [T] from one forward call (two launches), every gradient from one
    backward call (one launch) whichever sides need one.  A tensor that sits in two terms gets the sum of its two buffers."""

    @staticmethod
    def forward(ctx, index_pairs, *tensors):
        ts = [t.contiguous().float() for t in tensors]
        ctx.save_for_backward(*ts)
        ctx.index_pairs = list(index_pairs)
        return ops.ssim_terms([(ts[i], ts[j]) for i, j in index_pairs])

    @staticmethod
    def backward(ctx, gs):
        ts = ctx.saved_tensors
        wants = ctx.needs_input_grad[1:]
        terms = [t for t, (i, j) in enumerate(ctx.index_pairs) if wants[i] or wants[j]]
        grads = [None] * len(ts)
        if terms:
            gs = gs.contiguous().float()
            if len(terms) != len(ctx.index_pairs):
                gs = gs[torch.tensor(terms, device=gs.device)]
            chosen = [ctx.index_pairs[t] for t in terms]
            outs = ops.ssim_terms_grad([(ts[i], ts[j]) for i, j in chosen], gs, [(wants[i], wants[j]) for i, j in chosen])
            for (i, j), (gx, gy) in zip(chosen, outs):
                for k, o in ((i, gx), (j, gy)):
                    if o is not None:
                        grads[k] = o if grads[k] is None else grads[k] + o
        return (None, *grads)


class _MultiLapFn(torch.autograd.Function):
    """lap(x_t, y_t) of T pairs as ONE autograd node: an fp32 [T] from one forward call, every gradient from one backward call
    whichever sides need one.  A tensor that sits in two terms gets the sum of its two buffers."""

    @staticmethod
    def forward(ctx, levels, eps, index_pairs, *tensors):
        ts = [t.contiguous().float() for t in tensors]
        ctx.save_for_backward(*ts)
        ctx.levels, ctx.eps, ctx.index_pairs = levels, eps, list(index_pairs)
        return ops.lap_terms([(ts[i], ts[j]) for i, j in index_pairs], levels, eps)

    @staticmethod
    def backward(ctx, gs):
        ts = ctx.saved_tensors
        wants = ctx.needs_input_grad[3:]
        terms = [t for t, (i, j) in enumerate(ctx.index_pairs) if wants[i] or wants[j]]
        grads = [None] * len(ts)
        if terms:
            gs = gs.contiguous().float()
            if len(terms) != len(ctx.index_pairs):
                gs = gs[torch.tensor(terms, device=gs.device)]
            chosen = [ctx.index_pairs[t] for t in terms]
            outs = ops.lap_terms_grad([(ts[i], ts[j]) for i, j in chosen], gs, [(wants[i], wants[j]) for i, j in chosen],
                                      ctx.levels, ctx.eps)
            for (i, j), (gx, gy) in zip(chosen, outs):
                for k, o in ((i, gx), (j, gy)):
                    if o is not None:
                        grads[k] = o if grads[k] is None else grads[k] + o
        return (None, None, None, *grads)


def _index_pairs(pairs):
    """(the distinct tensors of `pairs`, per pair the two positions in that list)."""
    uniq, index = [], {}
    idx_pairs = []
    for x, y in pairs:
        ij = []
        for t in (x, y):
            if id(t) not in index:
                index[id(t)] = len(uniq)
                uniq.append(t)
            ij.append(index[id(t)])
        idx_pairs.append(tuple(ij))
    return uniq, tuple(idx_pairs)


def _one_shape_on_device(pairs):
    """Whether the fused nodes mean what the per-term path means: every pair of ONE shape on one device (equal numel with different
    shapes, or two devices, raised there and must not be summed silently here — advisor r05)."""
    x0 = pairs[0][0]
    return all(t.is_cuda and t.device == x0.device and t.shape == x0.shape for p in pairs for t in p)


def multi_term_loss(criterion, pairs):
    """(loss, [terms]) of `criterion` over the (x, y) `pairs`, loss = sum(terms) / len(terms): fused when `criterion` is one of this
    module's (they carry `.kind`, `.ssim_weight` for cb+ssim or `.lap_weight` for cb+lap), the plain per-term loop otherwise (an
    injected criterion; tensors of different sizes).  A criterion with `.ssim_weight` or `.lap_weight` leaves the two unweighted
    summands of the loss, detached, in its `last_parts`: (the mean Charbonnier term, the mean of 1 - ssim or of lap)."""
    import os
    kind = getattr(criterion, "kind", None)
    lam = getattr(criterion, "ssim_weight", None)
    mu = getattr(criterion, "lap_weight", None)
    if os.environ.get("BIN_AMD_FUSED_LOSS", "1") == "0":          # diagnostics / A-B only: the per-term path it replaced
        kind = lam = mu = None
    fusable = (kind is not None or lam is not None or mu is not None) and len(pairs) <= L.LOSS_MAX_TERMS and _one_shape_on_device(pairs)
    if not fusable:
        terms, parts = [], []
        for x, y in pairs:
            terms.append(criterion(x, y))
            parts.append(getattr(criterion, "last_parts", None))
        two_parts = getattr(criterion, "ssim_weight", None) is not None or getattr(criterion, "lap_weight", None) is not None
        if two_parts and all(p is not None for p in parts):
            criterion.last_parts = (sum(p[0] for p in parts) / len(parts), sum(p[1] for p in parts) / len(parts))
        return sum(terms) / len(terms), terms
    uniq, idx_pairs = _index_pairs(pairs)
    if mu is not None:
        # cb+lap: the Charbonnier part through the node above, the pyramid part one forward and one backward call for all pairs
        loss_cb, cb_terms = _MultiPixelLossFn.apply(L.LOSS_CHARBONNIER, criterion.eps, idx_pairs, *uniq)
        lap = _MultiLapFn.apply(criterion.levels, criterion.eps, idx_pairs, *uniq)
        lap_mean = lap.sum() / len(pairs)
        criterion.last_parts = (loss_cb.detach(), lap_mean.detach())
        return loss_cb + mu * lap_mean, list((cb_terms + mu * lap).unbind(0))
    if lam is None:
        loss, terms = _MultiPixelLossFn.apply(kind, getattr(criterion, "eps", 0.0), idx_pairs, *uniq)
        return loss, list(terms.unbind(0))
    # cb+ssim: the Charbonnier part through the node above, the SSIM part one forward and one backward call for all pairs
    loss_cb, cb_terms = _MultiPixelLossFn.apply(L.LOSS_CHARBONNIER, criterion.eps, idx_pairs, *uniq)
    d = 1.0 - _MultiSsimFn.apply(idx_pairs, *uniq)
    d_mean = d.sum() / len(pairs)
    criterion.last_parts = (loss_cb.detach(), d_mean.detach())
    return loss_cb + lam * d_mean, list((cb_terms + lam * d).unbind(0))


class CharbonnierLoss(nn.Module):
    """mean(sqrt((x-y)^2 + eps)); eps is NOT squared, as in the reference."""

    kind = L.LOSS_CHARBONNIER
    reduction = "mean"             # over the elements, so over the batch: what train.micro_batch weighs a chunk's loss by

    def __init__(self, eps=1e-6):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        return _PixelLossFn.apply(x, y, L.LOSS_CHARBONNIER, self.eps)


class L1SumLoss(nn.Module):
    """sum |x - y|  (= nn.L1Loss(reduction='sum'), bin_model.py:55)."""
    kind, eps = L.LOSS_L1_SUM, 0.0
    reduction = "sum"

    def forward(self, x, y):
        return _PixelLossFn.apply(x, y, L.LOSS_L1_SUM, 0.0)


class L2SumLoss(nn.Module):
    """sum (x - y)^2  (= nn.MSELoss(reduction='sum'), bin_model.py:57)."""
    kind, eps = L.LOSS_L2_SUM, 0.0
    reduction = "sum"

    def forward(self, x, y):
        return _PixelLossFn.apply(x, y, L.LOSS_L2_SUM, 0.0)


class CharbonnierSsimLoss(nn.Module):
    """cb(x, y) + ssim_weight * (1 - ssim(x, y)) (`pixel_criterion: cb+ssim`; the reference names a CharbonnierLossPlusSSIM that its
    models/loss.py does not define): cb the Charbonnier mean above, ssim the mean over all planes and all valid 11 x 11 Gaussian
    windows of the unquantised fp32 frames with data range 1 (include/binssim.h) — the SSIM the validation log prints.  x, y: at
    least 3-D, the last two dimensions H, W.  `last_parts`: the last call's (cb, 1 - ssim), detached."""

    reduction = "mean"             # both summands are means over the batch's elements / windows

    def __init__(self, ssim_weight, eps=1e-6):
        super().__init__()
        if isinstance(ssim_weight, bool) or not isinstance(ssim_weight, (int, float)) or not 0.0 < float(ssim_weight) < float("inf"):
            raise ValueError(f"CharbonnierSsimLoss: ssim_weight {ssim_weight!r} is not a finite number > 0")
        self.ssim_weight = float(ssim_weight)
        self.eps = eps
        self.last_parts = None

    def forward(self, x, y):
        cb = _PixelLossFn.apply(x, y, L.LOSS_CHARBONNIER, self.eps)
        uniq, idx_pairs = _index_pairs([(x, y)])
        d = 1.0 - _MultiSsimFn.apply(idx_pairs, *uniq)[0]
        self.last_parts = (cb.detach(), d.detach())
        return cb + self.ssim_weight * d


class CharbonnierLapLoss(nn.Module):
    """cb(x, y) + lap_weight * lap(x, y) (`pixel_criterion: cb+lap`): cb the Charbonnier mean above, lap the Laplacian-pyramid loss
    of include/binlap.h over `levels` octave bands of x - y, each band's Charbonnier mean with the same eps, on the unquantised fp32
    frames (the reference's models/loss.py carries a multi_scale_loss that nothing calls).  x, y: at least 3-D, the last two
    dimensions H, W of at least 2^(levels - 1) pixels.  `last_parts`: the last call's (cb, lap), detached."""

    reduction = "mean"             # both summands are means over the batch's elements

    def __init__(self, lap_weight, levels=5, eps=1e-6):
        super().__init__()
        if isinstance(lap_weight, bool) or not isinstance(lap_weight, (int, float)) or not 0.0 < float(lap_weight) < float("inf"):
            raise ValueError(f"CharbonnierLapLoss: lap_weight {lap_weight!r} is not a finite number > 0")
        if isinstance(levels, bool) or not isinstance(levels, int) or not 1 <= levels <= L.LAP_MAX_LEVELS:
            raise ValueError(f"CharbonnierLapLoss: levels {levels!r} is not an integer 1 .. {L.LAP_MAX_LEVELS}")
        self.lap_weight = float(lap_weight)
        self.levels = levels
        self.eps = eps
        self.last_parts = None

    def forward(self, x, y):
        cb = _PixelLossFn.apply(x, y, L.LOSS_CHARBONNIER, self.eps)
        uniq, idx_pairs = _index_pairs([(x, y)])
        lap = _MultiLapFn.apply(self.levels, self.eps, idx_pairs, *uniq)[0]
        self.last_parts = (cb.detach(), lap.detach())
        return cb + self.lap_weight * lap
