"""Adam as one HIP multi-tensor kernel (`train.optimizer: hip`): torch.optim.Adam's update (its non-capturable
single-tensor arithmetic, torch/optim/adam.py) over a whole parameter group through binopt_adam_step — one elementwise kernel
that walks a table of tensors passed by value, instead of the seven multi-tensor passes, 540 temporaries and 540 host-side
step-counter adds of torch's default `foreach` path on bin_stage4's 540 parameters.

The optimizer STATE is torch's, key for key and dtype for dtype (`step`: float32 scalar on the CPU; `exp_avg`, `exp_avg_sq`:
like the parameter, created at the parameter's first gradient), and `param_groups` carry every key torch.optim.Adam keeps, so a
`state_dict()` of either class loads into the other and `.state` checkpoint files interchange.  There is no CPU fallback:
`step()` on CPU parameters raises.

`GradGuard` (`train.grad_clip`, `train.skip_bad_steps`) sits between the backward and either Adam class: the global gradient norm in
one deterministic HIP pass with double accumulation (bingrad_norm), torch.nn.utils.clip_grad_norm_'s clip in place (bingrad_scale),
and the decision to skip a step whose gradients are not finite or that saturated an fp16 plane, before Adam writes anything.

`WeightEMA` (`train.ema_decay`) runs after the optimizer step: an exponential moving average of the weights in one flat fp32 buffer,
updated by binema_step (the work split of the Adam kernel over a by-value table of {e, p, numel} rows), and a context that puts the
averaged weights in place of the training ones for validation and saving without copying either."""
import contextlib
from collections import namedtuple

import numpy as np
import torch

from . import ops

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")
# BinAdamTensor (include/binopt.h) as a numpy record, to write a column of the host row table at once
_ROW_DTYPE = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("numel", "i8"), ("step_size", "f4"), ("inv_sqrt_bc2", "f4")])


def _by_device(tensors):
    """{device: the indices of `tensors` on it}: a library call takes the rows of one device."""
    by_dev = {}
    for i, t in enumerate(tensors):
        by_dev.setdefault(t.device, []).append(i)
    return by_dev


def _reuse(cached, key, build):
    """The (key, host row table) pair the three classes keep: `cached` while no pointer in `key` changed, else a table built anew."""
    return cached if cached is not None and cached[0] == key else (key, build())


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False,
                 capturable=False, differentiable=False):
        for name, flag in zip(_UNSUPPORTED, (amsgrad, maximize, capturable, differentiable)):
            if flag:
                raise NotImplementedError(f"bin_amd.optim.Adam: {name}=True is not implemented (use torch.optim.Adam)")
        if isinstance(lr, torch.Tensor) or any(isinstance(b, torch.Tensor) for b in betas):
            raise NotImplementedError("bin_amd.optim.Adam: tensor lr / betas are not implemented (use torch.optim.Adam)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # every key torch.optim.Adam keeps in a group, with the values of the one configuration implemented here
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False)
        super().__init__(params, defaults)
        self._tables = {}            # (group index, device) -> (pointers, table): the host row table, reused while no pointer changed

    def __setstate__(self, state):
        super().__setstate__(state)
        self._tables = {}

    def _init_state(self, p):
        state = self.state[p]
        if len(state) == 0:
            state["step"] = torch.tensor(0.0, dtype=torch.float32)           # torch's: a float32 scalar on the CPU
            state["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return state

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            for name in _UNSUPPORTED + ("decoupled_weight_decay",):
                if group.get(name):
                    raise NotImplementedError(f"bin_amd.optim.Adam: a param group with {name}=True (loaded from another "
                                              "optimizer's state?) is not implemented")
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                if not p.is_cuda:
                    raise RuntimeError("bin_amd.optim.Adam: parameters must live on a HIP device (there is no CPU fallback; "
                                       "use torch.optim.Adam, `train.optimizer: torch`)")
                if p.grad.is_sparse:
                    raise RuntimeError("Adam does not support sparse gradients, please consider SparseAdam instead")
            states = [self._init_state(p) for p in params]
            steps = [s["step"] for s in states]
            torch._foreach_add_(steps, 1)
            ts = torch.stack(steps).tolist()
            beta1, beta2 = group["betas"]
            lr = float(group["lr"])
            for dev, idx in _by_device(params).items():
                self._launch(gi, dev, idx, params, states, ts, lr, beta1, beta2, float(group["eps"]),
                             float(group["weight_decay"]))
            # the kernel wrote through raw pointers: the relayout cache key, the streaming memo and autograd's saved-tensor
            # checks all rest on the version counters
            torch.autograd.graph.increment_version(params)
        return loss

    def _launch(self, gi, dev, idx, params, states, ts, lr, beta1, beta2, eps, weight_decay):
        n = len(idx)
        rows = [(params[i], params[i].grad, states[i]["exp_avg"], states[i]["exp_avg_sq"]) for i in idx]

        def build():
            table = ops.adam_rows(n)
            for r, row in enumerate(rows):
                ops.adam_row(table, r, *row, 0.0, 0.0)
            return table
        self._tables[(gi, dev)] = _reuse(self._tables.get((gi, dev)), tuple(t.data_ptr() for row in rows for t in row), build)
        table = self._tables[(gi, dev)][1]
        # the bias corrections in double, rounded once by the float fields of the rows; t may differ between parameters
        t = np.asarray([ts[i] for i in idx], dtype=np.float64)
        view = np.frombuffer(table, dtype=_ROW_DTYPE, count=n)
        view["step_size"] = lr / (1.0 - beta1 ** t)
        view["inv_sqrt_bc2"] = 1.0 / np.sqrt(1.0 - beta2 ** t)
        ops.adam_launch(table, n, dev, beta1, beta2, eps, weight_decay)


GradState = namedtuple("GradState", "norm coef flags skipped consecutive")


class GradGuard:
    """The guard between `backward()` (and the data-parallel reduce) and `optimizer.step()`.  It acts on `.grad` in place, as torch's
    clipping does, so it works with torch.optim.Adam and with `Adam` above; parameters without a gradient are left out.

    max_norm        0 = no clipping; > 0: the gradients are multiplied by min(1, max_norm / (norm + 1e-6)), the formula of
                    torch.nn.utils.clip_grad_norm_, with the norm accumulated in double.  Unlike torch, a gradient set whose norm is
                    not finite is left as it is (coef = 1).
    skip_bad_steps  0 = `apply()` never synchronises the host and always returns True.  N > 0: `apply()` waits for the 32-byte record
                    and returns False (skip the optimizer step) when the norm is not finite or the device status word reports fp16
                    saturation; after more than N consecutive skipped steps it raises.  Under torch.distributed the flags are
                    all-reduced (MAX) first: the status word is per rank, and the ranks must agree.
    There is no CPU fallback: `apply()` on CPU gradients raises."""

    def __init__(self, params, max_norm=0.0, skip_bad_steps=0, process_group=None):
        max_norm = float(max_norm)
        if not 0.0 <= max_norm < float("inf"):
            raise ValueError(f"Invalid max_norm: {max_norm}")
        if isinstance(skip_bad_steps, bool) or int(skip_bad_steps) != skip_bad_steps or skip_bad_steps < 0:
            raise ValueError(f"Invalid skip_bad_steps: {skip_bad_steps!r}")
        self.params = [p for p in params]
        self.max_norm, self.skip_bad_steps, self.process_group = max_norm, int(skip_bad_steps), process_group
        self.consecutive = 0          # skipped steps in a row
        self.skipped_total = 0        # skipped steps since construction
        self._rows = None             # (pointers, ops.GradRows): the host row table, reused while no pointer changed
        self._workspace = self._record = self._host = self._event = None
        self._pending = False         # the record of the last apply() has not been read from `_host` yet
        self._last = GradState(0.0, 1.0, 0, False, 0)

    # -------------------------------------------------------------------------------------------- the decision (host only)
    @staticmethod
    def cause(flags):
        names = [n for bit, n in ((ops.L.GRAD_FLAG_NONFINITE, "non-finite gradient norm"), (ops.L.GRAD_FLAG_STATUS, "fp16 saturation"))
                 if flags & bit]
        return " and ".join(names)

    def _judge(self, flags):
        """Count a step with these (agreed) flags: True = take it, False = skip it; raises beyond `skip_bad_steps` in a row."""
        if not flags:
            self.consecutive = 0
            return True
        self.consecutive += 1
        self.skipped_total += 1
        if self.consecutive > self.skip_bad_steps:
            raise RuntimeError(f"bin_amd: {self.cause(flags)} on {self.consecutive} consecutive training steps "
                               f"(train.skip_bad_steps tolerates {self.skip_bad_steps}); the optimizer has not been stepped")
        return False

    def _agree(self, flags):
        """All-reduce (MAX) the one-element int32 `flags` tensor over the process group when there is more than one rank."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(self.process_group) == 1:
            return flags
        if flags.is_cuda and dist.get_backend(self.process_group) == "gloo":          # as utils/dist_util.py stages device tensors
            stream = torch.cuda.current_stream(flags.device)
            host = torch.empty(flags.shape, dtype=flags.dtype, pin_memory=True)
            host.copy_(flags, non_blocking=True)
            stream.synchronize()
            dist.all_reduce(host, op=dist.ReduceOp.MAX, group=self.process_group)
            flags.copy_(host, non_blocking=True)
            stream.synchronize()
        else:
            dist.all_reduce(flags, op=dist.ReduceOp.MAX, group=self.process_group)
        return flags

    # -------------------------------------------------------------------------------------------- the step
    @torch.no_grad()
    def apply(self):
        """Norm (and clip) of every present `.grad` on the current stream.  True: step the optimizer; False: skip this step."""
        grads = [p.grad for p in self.params if p.grad is not None]
        if not grads:
            self._pending, self._last = False, GradState(0.0, 1.0, 0, False, self.consecutive)
            return True
        if not all(g.is_cuda for g in grads):
            raise RuntimeError("bin_amd.optim.GradGuard: gradients must live on a HIP device (there is no CPU fallback; "
                               "use torch.nn.utils.clip_grad_norm_)")
        key = tuple(g.data_ptr() for g in grads) + tuple(g.numel() for g in grads)
        self._rows = _reuse(self._rows, key, lambda: ops.grad_rows(grads))
        rows = self._rows[1]
        dev = rows.device
        if self._record is None or self._record.device != dev:
            self._record = ops.grad_record(dev)
            self._host = torch.zeros(ops.GRAD_RECORD_WORDS, dtype=torch.int32).pin_memory()
            self._event = torch.cuda.Event()
            self._workspace = None
        if self._workspace is None or self._workspace.numel() * 8 < rows.workspace_bytes:
            self._workspace = torch.empty((rows.workspace_bytes + 7) // 8, dtype=torch.float64, device=dev)
        skipping = self.skip_bad_steps > 0
        word = ops.status_word(dev) if skipping else None
        ops.grad_norm(rows, self._workspace, self._record, self.max_norm, word, ops.L.STATUS_SATURATED if skipping else 0)
        stream = torch.cuda.current_stream(dev)
        if skipping:
            self._agree(self._record[ops.GRAD_FLAGS_WORD:ops.GRAD_FLAGS_WORD + 1])
        with torch.cuda.device(dev):
            self._host.copy_(self._record, non_blocking=True)
            self._event.record(stream)
        self._pending = True
        if self.max_norm > 0:
            ops.grad_scale(rows, self._record)               # queued before the host waits below
            torch.autograd.graph.increment_version(grads)    # written through raw pointers
        if not skipping:
            return True
        rec = self._read()
        if rec.flags & ops.L.GRAD_FLAG_STATUS:
            word.bitwise_and_(~ops.L.STATUS_SATURATED)       # this step is dealt with here: check_status need not raise for it
        try:
            return self._judge(rec.flags)
        finally:                                             # also when _judge raises: `last` names the step that was refused
            self._last = self._last._replace(skipped=bool(rec.flags), consecutive=self.consecutive)

    def _read(self):
        self._event.synchronize()                            # this stream's copy of the record, not the whole device
        rec = ops.grad_record_read(self._host)
        self._pending = False
        self._last = GradState(float(rec.norm), float(rec.coef), int(rec.flags), False, self.consecutive)
        return rec

    @property
    def last(self):
        """(norm, coef, flags, skipped, consecutive) of the last `apply()`.  With skip_bad_steps == 0 this is where the record is
        read (an event wait): ask where the host synchronises anyway."""
        if self._pending:
            self._read()
        return self._last


class WeightEMA:
    """An exponential moving average of `params` (`train.ema_decay`): after every optimizer step `update()` moves each shadow
    towards its parameter, e += (1 - decay) * (p - e) in fp32, with one binema_step call per device on the current stream: no
    allocation and no host synchronisation.  The shadows are views into ONE flat fp32 buffer on the parameters' device, each
    starting on a 16-byte boundary (so every row takes the kernel's 16-byte path when its parameter does), initialised to the
    parameters' current values; `shadow` lists them in parameter order.

    `applied()` is the context in which the parameters hold the averaged values (validation, saving).  There is no CPU fallback:
    `update()` on CPU parameters raises; building, `state_dict()` and `load_state_dict()` work anywhere."""

    def __init__(self, params, decay):
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:   # NaN fails both
            raise ValueError(f"Invalid decay: {decay!r} (0 <= decay < 1)")
        self.decay = float(decay)
        self.params = [p for p in params]
        for p in self.params:
            if p.dtype != torch.float32:
                raise ValueError(f"bin_amd.optim.WeightEMA: float32 parameters, got {p.dtype}")
        self._alloc()
        self._tables = {}             # device -> (pointers, table): the host row table, reused while no pointer changed
        self._held = None             # inside applied(): the training values' tensors, in parameter order

    def _alloc(self):
        """One flat buffer per device; a tensor's slice starts on a multiple of 4 floats from the (allocator-aligned) base."""
        self._flat, self.shadow = {}, [None] * len(self.params)
        with torch.no_grad():
            for dev, idx in _by_device(self.params).items():
                offsets, total = [], 0
                for i in idx:
                    offsets.append(total)
                    total += (self.params[i].numel() + 3) // 4 * 4
                flat = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
                assert flat.data_ptr() % 16 == 0
                for i, o in zip(idx, offsets):
                    p = self.params[i]
                    view = flat[o:o + p.numel()].view(p.shape)
                    view.copy_(p.detach().contiguous())
                    self.shadow[i] = view
                self._flat[dev] = flat

    @torch.no_grad()
    def update(self):
        """One averaging step of every shadow towards its parameter, on the current stream of each device."""
        if self._held is not None:
            raise RuntimeError("bin_amd.optim.WeightEMA: update() inside applied(): the parameters hold the averaged values")
        if not all(p.is_cuda for p in self.params):
            raise RuntimeError("bin_amd.optim.WeightEMA: parameters must live on a HIP device (there is no CPU fallback; "
                               "leave `train.ema_decay` out)")
        for dev, idx in _by_device(self.params).items():
            def build():
                table = ops.ema_rows(len(idx))
                for r, i in enumerate(idx):
                    ops.ema_row(table, r, self.shadow[i], self.params[i].detach())
                return table
            key = tuple(self.params[i].data_ptr() for i in idx) + tuple(self.shadow[i].data_ptr() for i in idx)
            self._tables[dev] = _reuse(self._tables.get(dev), key, build)
            ops.ema_launch(self._tables[dev][1], len(idx), dev, self.decay)
        # the kernel wrote through raw pointers: whatever keys on the shadows' version counters must see a new weight set
        torch.autograd.graph.increment_version(self.shadow)

    @contextlib.contextmanager
    def applied(self, invalidate=()):
        """Inside, the parameters hold the averaged values; on exit the training values again, bit for bit, at the same storage
        addresses and with the same `_version` as before entry.  Each parameter's `.data` is exchanged with its shadow's, so nothing
        is copied: inside, a parameter IS its shadow's memory (torch keeps the parameter's own version counter across the exchange),
        and Adam's cached row table, FlatGradAllReduce's views and autograd's saved-tensor checks see nothing afterwards.
        `invalidate`: the modules (or one module) whose `invalidate_kernel_weights()`, where they have it, is called on entry and
        on exit, since the parameters' version counters do not tell the two weight sets apart.  Not re-entrant; entering it with a
        forward outstanding is the caller's error."""
        if self._held is not None:
            raise RuntimeError("bin_amd.optim.WeightEMA: applied() is not re-entrant")
        mods = list(invalidate.modules()) if isinstance(invalidate, torch.nn.Module) else \
            [m for top in invalidate for m in top.modules()]
        mods = [m for m in mods if hasattr(m, "invalidate_kernel_weights")]
        for p, e in zip(self.params, self.shadow):
            if p.shape != e.shape or p.device != e.device:
                raise RuntimeError("bin_amd.optim.WeightEMA: a parameter changed shape or device since the shadows were made")
        self._held = [p.data for p in self.params]
        try:
            for p, e in zip(self.params, self.shadow):
                p.data = e
            for m in mods:
                m.invalidate_kernel_weights()
            yield self
        finally:
            for p, d in zip(self.params, self._held):
                p.data = d
            self._held = None
            for m in mods:
                m.invalidate_kernel_weights()

    def state_dict(self):
        return {"decay": self.decay, "shadow": [e.detach().cpu().clone() for e in self.shadow]}

    @torch.no_grad()
    def load_shadow(self, tensors):
        """Copy `tensors` (parameter order, any device) into the shadows.  A count or shape mismatch raises, naming the first."""
        tensors = list(tensors)
        if len(tensors) != len(self.shadow):
            raise ValueError(f"bin_amd.optim.WeightEMA: {len(tensors)} shadow tensors for {len(self.shadow)} parameters")
        for i, (e, t) in enumerate(zip(self.shadow, tensors)):
            if tuple(t.shape) != tuple(e.shape):
                raise ValueError(f"bin_amd.optim.WeightEMA: shadow {i} has shape {tuple(t.shape)}, parameter {i} has "
                                 f"{tuple(e.shape)}")
        for e, t in zip(self.shadow, tensors):
            e.copy_(t)                                       # copy_ bumps the shadow's version counter

    def load_state_dict(self, state):
        self.load_shadow(state["shadow"])
        decay = state["decay"]
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"Invalid decay: {decay!r} (0 <= decay < 1)")
        self.decay = float(decay)
