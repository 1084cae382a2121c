"""Host-side base class of the model wrapper: same public surface as the reference's `BaseModel`
(models/base_model.py:8-125 — device pick, LR warm-up, network / training-state checkpoints), written
for the one-process-per-GPU design.

Checkpoint formats are the reference's, so files interchange both ways:
  `{iter}_G.pth`   CPU state_dict of the unwrapped generator (1332 aliased keys for bin_stage4)
  `{iter}.state`   {"epoch", "iter", "schedulers": [...], "optimizers": [...]}
"""
import logging
import os
from collections import OrderedDict

import torch
import torch.nn as nn

_PREFIXES = ("module.", "InterpNet.")


def unwrap(network):
    """The bare generator behind a DataParallel / DDP / SingleProcessParallel style wrapper."""
    inner = getattr(network, "module", None)
    return inner if isinstance(inner, nn.Module) else network


class _NoCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _direct_param_grads(network):
    """The generator's own `direct_param_grads()` context (bin_amd/models/archs/RDN.py) when it has one — an injected
    CPU test generator does not — else a no-op."""
    net = unwrap(network)
    ctx = getattr(net, "direct_param_grads", None)
    return ctx() if callable(ctx) else _NoCtx()


def clean_state_dict_keys(loaded, strict):
    """Key clean-up of the reference's load_network (base_model.py:93-102): a leading 'module.' or
    'InterpNet.' is stripped.  The reference also keeps a 'module.'-prefixed key under its original name
    (its `else` belongs to the second `if`); that duplicate makes a strict load of a DataParallel-saved
    file impossible, so under strict=True it is dropped when the stripped twin exists."""
    out = OrderedDict()
    for key, value in loaded.items():
        stripped = next((key[len(p):] for p in _PREFIXES if key.startswith(p)), None)
        if stripped is not None:
            out[stripped] = value
        if not key.startswith("InterpNet."):
            out[key] = value
    if strict:
        for key in [k for k in out if k.startswith("module.") and k[len("module."):] in out]:
            del out[key]
    return out


class BaseModel:
    def __init__(self, opt):
        self.opt = opt
        self.is_train = opt["is_train"]
        # reference rule (base_model.py:11): any gpu_ids => 'cuda' (the process's current HIP device), else cpu
        self.device = torch.device("cpu" if opt["gpu_ids"] is None else "cuda")
        # The reference's non-distributed default wraps the generator in nn.DataParallel over `gpu_ids` (bin_model.py:41-42; the
        # shipped yml has gpu_ids: [2, 3] with dist: false).  Here a process drives ONE GPU: several ids without `dist` would
        # silently train on one device at the full batch, so that is an error with the way out spelled out.
        ids = opt["gpu_ids"]
        if ids is not None and len(ids) > 1 and not opt["dist"]:
            raise RuntimeError(
                f"bin_amd: gpu_ids = {list(ids)} with dist = false asks for nn.DataParallel over {len(ids)} GPUs (reference "
                "bin_model.py:41-42); this build runs one process per GPU over RCCL instead.  Launch\n"
                f"  python -m torch.distributed.run --nnodes=1 --nproc-per-node={len(ids)} --master-addr 127.0.0.1 "
                "-m bin_amd.train -opt <yml> --launcher pytorch\n"
                "(each rank takes gpu_ids = [LOCAL_RANK], batch_size is per process), or list a single id.")
        self.optimizers = []
        self.schedulers = []
        self.weight_ema = None       # train.ema_decay: the wrapper builds a bin_amd.optim.WeightEMA after load()
        self.micro_batch = None      # train.micro_batch: samples per forward / backward of a training step; None = the whole batch

    # ---- interface stubs the concrete wrapper overrides (kept for API parity) ----------------------
    def feed_data(self, data):
        pass

    def optimize_parameters(self):
        pass

    def get_current_visuals(self):
        pass

    def get_current_losses(self):
        pass

    def print_network(self):
        pass

    def save(self, label):
        pass

    def load(self):
        pass

    # ---- train.micro_batch (bin_amd extension): one optimizer step as several forward / backward passes -------------------
    def _micro_batch_chunks(self, batch):
        """The (start, n) chunks this step cuts its `batch` fed samples into: one, unless `train.micro_batch` is below the batch."""
        from ..options.options import micro_batches
        return micro_batches(batch, getattr(self, "micro_batch", None))

    def _for_each_micro_batch(self, names, chunks, body):
        """Run `body(weight)` once per chunk with the batch tensors `names` (attributes of self) narrowed to the chunk along N —
        views, nothing is copied — and the data-parallel reducer held for every chunk but the last; `weight` is what the chunk's
        loss is multiplied by so that the accumulated gradient is the whole batch's.  The whole-batch tensors are put back on
        every exit."""
        from ..options.options import micro_batch_weights
        weights = micro_batch_weights(chunks, getattr(self.cri_pix, "reduction", None))
        whole = {nm: getattr(self, nm) for nm in names}
        sync = getattr(self, "grad_sync", None)
        try:
            for k, ((start, n), weight) in enumerate(zip(chunks, weights)):
                if sync is not None:
                    sync.hold(k + 1 < len(chunks))
                for nm, t in whole.items():
                    setattr(self, nm, t.narrow(0, start, n))
                body(weight)
        finally:
            for nm, t in whole.items():
                setattr(self, nm, t)
            if sync is not None:
                sync.hold(False)

    # ---- learning rate -----------------------------------------------------------------------------
    def _set_lr(self, lr_groups_l):
        """lr_groups_l[i][j]: learning rate of param group j of optimizer i."""
        for opt_, group_lrs in zip(self.optimizers, lr_groups_l):
            for group, lr in zip(opt_.param_groups, group_lrs):
                group["lr"] = lr

    def _get_init_lr(self):
        """The schedulers record each group's starting rate as 'initial_lr'."""
        return [[g["initial_lr"] for g in opt_.param_groups] for opt_ in self.optimizers]

    def update_learning_rate(self, cur_iter, warmup_iter=-1):
        """Step every scheduler, then override with the linear warm-up ramp while cur_iter < warmup_iter
        (reference base_model.py:51-63)."""
        for sched in self.schedulers:
            sched.step()
        if cur_iter < warmup_iter:
            # same arithmetic order as the reference: initial_lr / warmup_iter * cur_iter
            self._set_lr([[lr0 / warmup_iter * cur_iter for lr0 in grp] for grp in self._get_init_lr()])

    def get_current_learning_rate(self):
        return [g["lr"] for g in self.optimizers[0].param_groups]

    # ---- description / checkpoints -------------------------------------------------------------------
    def get_network_description(self, network):
        net = unwrap(network)
        return str(net), sum(p.numel() for p in net.parameters())

    def save_network(self, network, network_label, iter_label):
        target = os.path.join(self.opt["path"]["models"], f"{iter_label}_{network_label}.pth")
        torch.save(OrderedDict((k, v.cpu()) for k, v in unwrap(network).state_dict().items()), target)

    def load_network(self, load_path, network, strict=True):
        loaded = torch.load(load_path, map_location="cpu")
        net = unwrap(network)
        net.load_state_dict(clean_state_dict_keys(loaded, strict), strict=strict)
        for mod in net.modules():                    # load_state_dict copies in place (versions bump), but be explicit:
            if hasattr(mod, "invalidate_kernel_weights"):        # the relayouted kernel weights must be rebuilt
                mod.invalidate_kernel_weights()

    # ---- train.ema_decay (bin_amd extension): the averaged weights ---------------------------------------
    def ema_scope(self):
        """Context in which the generator holds the averaged weights (validation, saving); a no-op with `train.ema_decay` off."""
        ema = getattr(self, "weight_ema", None)
        return ema.applied(self.netG) if ema is not None else _NoCtx()

    def save_ema(self, iter_label):
        """`{iter}_G_ema.pth`: the averaged weights as an ordinary generator checkpoint (save_network under ema_scope), so
        bin_amd.test, `pretrain_model_G` and the reference load it unchanged.  Nothing is written with the option off."""
        if getattr(self, "weight_ema", None) is not None:
            with self.ema_scope():
                self.save_network(self.netG, "G_ema", iter_label)

    def load_ema(self, load_path):
        """The shadows from a `{iter}_G_ema.pth` file, by parameter name."""
        loaded = clean_state_dict_keys(torch.load(load_path, map_location="cpu"), True)
        names = [name for name, _ in unwrap(self.netG).named_parameters()]
        missing = [name for name in names if name not in loaded]
        if missing:
            raise KeyError(f"{load_path}: no key {missing[0]!r} ({len(missing)} of {len(names)} parameters are missing)")
        self.weight_ema.load_shadow([loaded[name] for name in names])

    def save_training_state(self, epoch, iter_step):
        """`{iter}.state` with everything needed to resume (reference base_model.py:105-114)."""
        state = {"epoch": epoch, "iter": iter_step,
                 "schedulers": [s.state_dict() for s in self.schedulers],
                 "optimizers": [o.state_dict() for o in self.optimizers]}
        torch.save(state, os.path.join(self.opt["path"]["training_state"], f"{iter_step}.state"))

    def resume_training(self, resume_state):
        saved_opt, saved_sched = resume_state["optimizers"], resume_state["schedulers"]
        assert len(saved_opt) == len(self.optimizers), "Wrong lengths of optimizers"
        assert len(saved_sched) == len(self.schedulers), "Wrong lengths of schedulers"
        for target, state in zip(self.optimizers, saved_opt):
            target.load_state_dict(state)
        for target, state in zip(self.schedulers, saved_sched):
            target.load_state_dict(state)
        if getattr(self, "weight_ema", None) is not None:
            # `.state` files do not carry the average: it is the `{iter}_G_ema.pth` beside the `{iter}_G.pth` check_resume named
            path = self.opt["path"].get("pretrain_model_G_ema")
            if path is not None and os.path.exists(path):
                self.load_ema(path)
            else:
                logging.getLogger("base").warning(
                    "train.ema_decay: no averaged weights [%s] to resume from; the average starts from the loaded weights.", path)
