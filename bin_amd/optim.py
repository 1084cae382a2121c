"""Adam as one HIP multi-tensor kernel (`train.optimizer: hip`): torch.optim.Adam's update (its non-capturable
single-tensor arithmetic, torch/optim/adam.py) over a whole parameter group through binopt_adam_step — one elementwise kernel
that walks a table of tensors passed by value, instead of the seven multi-tensor passes, 540 temporaries and 540 host-side
step-counter adds of torch's default `foreach` path on bin_stage4's 540 parameters.

The optimizer STATE is torch's, key for key and dtype for dtype (`step`: float32 scalar on the CPU; `exp_avg`, `exp_avg_sq`:
like the parameter, created at the parameter's first gradient), and `param_groups` carry every key torch.optim.Adam keeps, so a
`state_dict()` of either class loads into the other and `.state` checkpoint files interchange.  There is no CPU fallback:
`step()` on CPU parameters raises."""
import numpy as np
import torch

from . import ops

_UNSUPPORTED = ("amsgrad", "maximize", "capturable", "differentiable")
# BinAdamTensor (include/binopt.h) as a numpy record, to write a column of the host row table at once
_ROW_DTYPE = np.dtype([("p", "u8"), ("g", "u8"), ("m", "u8"), ("v", "u8"), ("numel", "i8"), ("step_size", "f4"), ("inv_sqrt_bc2", "f4")])


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
            by_dev = {}
            for i, p in enumerate(params):
                by_dev.setdefault(p.device, []).append(i)
            for dev, idx in by_dev.items():
                self._launch(gi, dev, idx, params, states, ts, lr, beta1, beta2, float(group["eps"]),
                             float(group["weight_decay"]))
            # the kernel wrote through raw pointers: the relayout cache key, the streaming memo and autograd's saved-tensor
            # checks all rest on the version counters
            torch.autograd.graph.increment_version(params)
        return loss

    def _launch(self, gi, dev, idx, params, states, ts, lr, beta1, beta2, eps, weight_decay):
        n = len(idx)
        ptrs = []
        for i in idx:
            p, s = params[i], states[i]
            ptrs += [p.data_ptr(), p.grad.data_ptr(), s["exp_avg"].data_ptr(), s["exp_avg_sq"].data_ptr()]
        key = tuple(ptrs)
        cached = self._tables.get((gi, dev))
        if cached is not None and cached[0] == key:
            table = cached[1]
        else:
            table = ops.adam_rows(n)
            for r, i in enumerate(idx):
                s = states[i]
                ops.adam_row(table, r, params[i], params[i].grad, s["exp_avg"], s["exp_avg_sq"], 0.0, 0.0)
            self._tables[(gi, dev)] = (key, table)
        # the bias corrections in double, rounded once by the float fields of the rows; t may differ between parameters
        t = np.asarray([ts[i] for i in idx], dtype=np.float64)
        view = np.frombuffer(table, dtype=_ROW_DTYPE, count=n)
        view["step_size"] = lr / (1.0 - beta1 ** t)
        view["inv_sqrt_bc2"] = 1.0 / np.sqrt(1.0 - beta2 ** t)
        ops.adam_launch(table, n, dev, beta1, beta2, eps, weight_decay)
