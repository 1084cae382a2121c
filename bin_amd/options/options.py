"""YAML option files (reference options/options.py:9-128): `parse` fills in the derived entries the wrappers read
(`is_train`, per-dataset `phase`/`data_type`/`scale`, the experiment / results directory tree under
`path.save_path`), `dict_to_nonedict` makes absent keys read as None, `check_resume` points the pretrain path at
the checkpoint that belongs to a resume state."""
import logging
import os
import os.path as osp
from collections import OrderedDict

import yaml


def _ordered_loader():
    class Loader(yaml.SafeLoader):
        pass

    Loader.add_constructor(yaml.resolver.BaseResolver.DEFAULT_MAPPING_TAG,
                           lambda loader, node: OrderedDict(loader.construct_pairs(node)))
    return Loader


VAL_METRICS = ("host", "device")


def val_metrics(opt):
    """`train.val_metrics` (bin_amd extension): where train.validate scores the 14 outputs.  Absent or `host`: numpy on
    frames copied to the host, as the reference does; `device`: ops.frame_scores on the fp32 outputs where they are.
    Anything else raises."""
    train = opt.get("train") if isinstance(opt, dict) else None
    value = train.get("val_metrics") if isinstance(train, dict) else None
    if value is None:
        return "host"
    if value not in VAL_METRICS:
        raise ValueError(f"train.val_metrics: {value!r} is not one of {', '.join(VAL_METRICS)}")
    return value


OPTIMIZERS = ("torch", "hip")


def optimizer(opt):
    """`train.optimizer` (bin_amd extension): which Adam the wrappers build.  Absent or `torch`: torch.optim.Adam, as the
    reference does; `hip`: bin_amd.optim.Adam, the same update as one HIP multi-tensor kernel with torch's state format.
    Anything else raises."""
    train = opt.get("train") if isinstance(opt, dict) else None
    value = train.get("optimizer") if isinstance(train, dict) else None
    if value is None:
        return "torch"
    if value not in OPTIMIZERS:
        raise ValueError(f"train.optimizer: {value!r} is not one of {', '.join(OPTIMIZERS)}")
    return value


def adam_class(opt):
    """The Adam class `train.optimizer` names."""
    if optimizer(opt) == "hip":
        from ..optim import Adam
        return Adam
    import torch
    return torch.optim.Adam


def _train_value(opt, key):
    train = opt.get("train") if isinstance(opt, dict) else None
    return train.get(key) if isinstance(train, dict) else None


def grad_clip(opt):
    """`train.grad_clip` (bin_amd extension): the max global L2 norm the gradients are clipped to before the optimizer step
    (bin_amd.optim.GradGuard: the formula of torch.nn.utils.clip_grad_norm_ with the norm accumulated in double by a HIP kernel).
    Absent, null or 0: off -> 0.0; a positive finite number: the max norm.  Anything else raises."""
    value = _train_value(opt, "grad_clip")
    if value is None:
        return 0.0
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"train.grad_clip: {value!r} is not a number (in YAML write 1.0e+3 or !!float 1e3, not 1e3)")
    if not 0.0 <= float(value) < float("inf"):                # NaN fails both comparisons
        raise ValueError(f"train.grad_clip: {value!r} is not a finite number >= 0")
    return float(value)


def skip_bad_steps(opt):
    """`train.skip_bad_steps` (bin_amd extension): how many consecutive training steps may be skipped (optimizer not stepped, weights
    untouched) because the gradient norm was not finite or an fp16 plane saturated, before the run stops.  Absent, null or 0: off -> 0
    (the status word is checked after the step, as before); a positive int.  Anything else raises."""
    value = _train_value(opt, "skip_bad_steps")
    if value is None:
        return 0
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"train.skip_bad_steps: {value!r} is not an integer")
    if value < 0:
        raise ValueError(f"train.skip_bad_steps: {value!r} is negative")
    return value


def grad_guard(opt, params, process_group=None):
    """The bin_amd.optim.GradGuard `train.grad_clip` / `train.skip_bad_steps` ask for over `params`, or None when both are off (then
    nothing of it is imported, built or loaded)."""
    clip, skip = grad_clip(opt), skip_bad_steps(opt)
    if not clip and not skip:
        return None
    from ..optim import GradGuard
    return GradGuard(params, max_norm=clip, skip_bad_steps=skip, process_group=process_group)


def ema_decay(opt):
    """`train.ema_decay` (bin_amd extension): the decay of the exponential moving average of the generator weights that is
    validated and saved beside the training weights (bin_amd.optim.WeightEMA: e += (1 - decay) * (p - e) after every optimizer step,
    one HIP pass).  Absent, null or 0: off -> 0.0; a number in (0, 1): the decay.  Anything else raises."""
    value = _train_value(opt, "ema_decay")
    if value is None:
        return 0.0
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"train.ema_decay: {value!r} is not a number")
    if not 0.0 <= float(value) < 1.0:                         # NaN fails both comparisons
        raise ValueError(f"train.ema_decay: {value!r} is not a number >= 0 and < 1")
    return float(value)


def weight_ema(opt, params):
    """The bin_amd.optim.WeightEMA `train.ema_decay` asks for over `params`, or None when it is off (then nothing of it is
    imported, built or loaded)."""
    decay = ema_decay(opt)
    if not decay:
        return None
    from ..optim import WeightEMA
    return WeightEMA(params, decay)


def micro_batch(opt):
    """`train.micro_batch` (bin_amd extension): how many samples of the fed batch run through one forward / backward inside an
    optimizer step; the step accumulates the gradients of ceil(B / m) such passes and updates the weights once, so the activations
    that are alive at a time are those of m samples, not of B.  Absent or null: off -> None (the whole batch in one pass); a positive
    int.  Anything else raises."""
    value = _train_value(opt, "micro_batch")
    if value is None:
        return None
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"train.micro_batch: {value!r} is not an integer")
    if value < 1:
        raise ValueError(f"train.micro_batch: {value!r} is not a positive integer")
    return value


def ssim_weight(opt):
    """`train.ssim_weight` (bin_amd extension): the weight of the structural term of `pixel_criterion: cb+ssim`, whose loss is
    cb(x, y) + ssim_weight * (1 - ssim(x, y)) (bin_amd.models.loss.CharbonnierSsimLoss).  Required, a finite number > 0, with that
    criterion; refused beside any other criterion, where it would silently do nothing.  Returns the weight, or None without the
    criterion."""
    value = _train_value(opt, "ssim_weight")
    criterion = _train_value(opt, "pixel_criterion")
    if criterion != "cb+ssim":
        if value is not None:
            raise ValueError(f"train.ssim_weight: {value!r} is set, but train.pixel_criterion is {criterion!r}: the weight belongs to "
                             "pixel_criterion: cb+ssim")
        return None
    if value is None:
        raise ValueError("train.ssim_weight: pixel_criterion: cb+ssim needs it (a finite number > 0)")
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"train.ssim_weight: {value!r} is not a number (in YAML write 1.0e-1 or !!float 1e-1, not 1e-1)")
    if not 0.0 < float(value) < float("inf"):                 # NaN fails both comparisons
        raise ValueError(f"train.ssim_weight: {value!r} is not a finite number > 0")
    return float(value)


def lap_weight(opt):
    """`train.lap_weight` (bin_amd extension): the weight of the multi-scale term of `pixel_criterion: cb+lap`, whose loss is
    cb(x, y) + lap_weight * lap(x, y) (bin_amd.models.loss.CharbonnierLapLoss).  Required, a finite number > 0, with that criterion;
    refused beside any other criterion, where it would silently do nothing.  Returns the weight, or None without the criterion."""
    value = _train_value(opt, "lap_weight")
    criterion = _train_value(opt, "pixel_criterion")
    if criterion != "cb+lap":
        if value is not None:
            raise ValueError(f"train.lap_weight: {value!r} is set, but train.pixel_criterion is {criterion!r}: the weight belongs to "
                             "pixel_criterion: cb+lap")
        return None
    if value is None:
        raise ValueError("train.lap_weight: pixel_criterion: cb+lap needs it (a finite number > 0)")
    if isinstance(value, bool) or not isinstance(value, (int, float)):
        raise ValueError(f"train.lap_weight: {value!r} is not a number (in YAML write 1.0e-1 or !!float 1e-1, not 1e-1)")
    if not 0.0 < float(value) < float("inf"):                  # NaN fails both comparisons
        raise ValueError(f"train.lap_weight: {value!r} is not a finite number > 0")
    return float(value)


LAP_LEVELS_DEFAULT, LAP_LEVELS_MAX = 5, 8


def lap_levels(opt):
    """`train.lap_levels` (bin_amd extension): the number of pyramid levels of `pixel_criterion: cb+lap`, an integer 1 .. 8; the
    training crop must be at least 2^(levels - 1) pixels high and wide.  Absent or null: 5.  Refused beside any other criterion.
    Returns the count, or None without the criterion."""
    value = _train_value(opt, "lap_levels")
    criterion = _train_value(opt, "pixel_criterion")
    if criterion != "cb+lap":
        if value is not None:
            raise ValueError(f"train.lap_levels: {value!r} is set, but train.pixel_criterion is {criterion!r}: the level count belongs "
                             "to pixel_criterion: cb+lap")
        return None
    if value is None:
        return LAP_LEVELS_DEFAULT
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"train.lap_levels: {value!r} is not an integer")
    if not 1 <= value <= LAP_LEVELS_MAX:
        raise ValueError(f"train.lap_levels: {value!r} is not an integer 1 .. {LAP_LEVELS_MAX}")
    return value


CACHE_FORMATS = ("bgr", "yuv")


def device_cache_format(dataset_opt, phase=None):
    """`datasets.<phase>.device_cache_format` (bin_amd extension): what the device frame cache of a `BIN_video` dataset holds.  Absent,
    null or `bgr`: uint8 BGR frames, converted once while the arena fills; `yuv`: the Y4M payloads as they are (half the bytes at
    4:2:0, clips of different sizes allowed), each batch's crops decoded by one HIP launch (bin_amd/data/video_dataset.py).  Anything
    else raises, and so does `yuv` on a dataset of another mode, where it would silently do nothing."""
    key = f"datasets.{phase or dataset_opt.get('phase') or '<phase>'}.device_cache_format"
    value = dataset_opt.get("device_cache_format")
    if value is None:
        return "bgr"
    if value not in CACHE_FORMATS:
        raise ValueError(f"{key}: {value!r} is not one of {', '.join(CACHE_FORMATS)}")
    if value == "yuv" and dataset_opt.get("mode") != "BIN_video":
        raise ValueError(f"{key}: yuv keeps the payloads of Y4M clips, so it needs mode BIN_video, not mode {dataset_opt.get('mode')!r}")
    return value


def micro_batches(batch, m):
    """The consecutive (start, n) chunks along N that a batch of `batch` samples is cut into with `train.micro_batch: m`:
    ceil(batch / m) chunks of m, the last one smaller when m does not divide the batch; one chunk when m is None or >= batch."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"micro_batches: a batch of {batch} samples")
    if m is None or m >= batch:
        return [(0, batch)]
    if m < 1:
        raise ValueError(f"micro_batches: micro_batch {m!r} is not a positive integer")
    return [(start, min(m, batch - start)) for start in range(0, batch, m)]


REDUCTIONS = ("mean", "sum")


def micro_batch_weights(chunks, reduction):
    """What each chunk's loss is multiplied by so that the accumulated loss and gradient are the whole batch's: n_k / B under a
    criterion that takes the mean over its elements, 1 under one that sums them."""
    if reduction not in REDUCTIONS:
        raise ValueError(f"train.micro_batch: the criterion's reduction is {reduction!r}, not one of {', '.join(REDUCTIONS)}: "
                         "how a chunk's loss adds up to the whole batch's is not known")
    total = sum(n for _, n in chunks)
    return [n / total if reduction == "mean" else 1.0 for _, n in chunks]


def val_self_ensemble(opt):
    """`train.val_self_ensemble` (bin_amd extension): the self-ensemble group validation runs the generator under
    (bin_amd/ensemble.py: letters of `hvt`, `flipx4`, `x8`).  Absent, null, "" or `none`: off -> ""; otherwise the group's canonical
    spelling.  Anything else raises."""
    from ..ensemble import parse_group
    try:
        return parse_group(_train_value(opt, "val_self_ensemble"))
    except ValueError as e:
        raise ValueError(f"train.val_self_ensemble: {e}") from None


def parse(opt_path, is_train=True):
    with open(opt_path) as f:
        opt = yaml.load(f, Loader=_ordered_loader())
    if is_train:
        val_metrics(opt)                     # a misspelt value stops the run here, not at the first validation pass
        optimizer(opt)
        grad_clip(opt)
        skip_bad_steps(opt)
        ema_decay(opt)
        micro_batch(opt)
        ssim_weight(opt)
        lap_weight(opt)
        lap_levels(opt)
        val_self_ensemble(opt)
    if is_train and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        # the reference exports CUDA_VISIBLE_DEVICES from gpu_ids (torch on ROCm honours the same variable); under
        # a one-process-per-GPU launcher the launcher owns device visibility, so it is left alone there
        os.environ["CUDA_VISIBLE_DEVICES"] = ",".join(str(g) for g in opt["gpu_ids"])
    opt["is_train"] = is_train
    sr = opt["distortion"] == "sr"
    scale = opt["scale"] if sr else 1

    for phase, ds in opt["datasets"].items():
        ds["phase"] = phase
        device_cache_format(ds, phase)       # a misspelt value, or yuv on a mode without payloads, stops the run here
        if sr:
            ds["scale"] = scale
        lmdb = False
        for key in ("dataroot_GT", "dataroot_LQ"):
            if ds.get(key) is not None:
                ds[key] = osp.expanduser(ds[key])
                lmdb = lmdb or ds[key].endswith("lmdb")
        ds["data_type"] = "lmdb" if lmdb else "img"
        if ds["mode"].endswith("mc"):
            ds["data_type"] = "mc"
            ds["mode"] = ds["mode"].replace("_mc", "")

    paths = opt["path"]
    for key, value in paths.items():
        if value and key != "strict_load":
            paths[key] = osp.expanduser(value)
    paths["root"] = paths["save_path"]
    if is_train:
        exp = osp.join(paths["root"], "experiments", opt["name"])
        paths.update(experiments_root=exp, models=osp.join(exp, "models"),
                     training_state=osp.join(exp, "training_state"), log=exp,
                     val_images=osp.join(exp, "val_images"), train_images=osp.join(exp, "train_images"))
        if "debug" in opt["name"]:
            opt["train"]["val_freq"] = 1
            opt["logger"]["print_freq"] = 1
            opt["logger"]["save_checkpoint_freq"] = 1
    else:
        results = osp.join(paths["root"], "results", opt["name"])
        paths.update(results_root=results, log=results)
    if sr:
        opt["network_G"]["scale"] = scale
    return opt


def dict2str(opt, indent_l=1):
    """Indented dump of a (nested) option dict for the log."""
    pad = " " * (indent_l * 2)
    out = []
    for k, v in opt.items():
        if isinstance(v, dict):
            out.append(f"{pad}{k}:[\n{dict2str(v, indent_l + 1)}{pad}]\n")
        else:
            out.append(f"{pad}{k}: {v}\n")
    return "".join(out)


class NoneDict(dict):
    def __missing__(self, key):
        return None


def dict_to_nonedict(opt):
    if isinstance(opt, dict):
        return NoneDict(**{k: dict_to_nonedict(v) for k, v in opt.items()})
    if isinstance(opt, list):
        return [dict_to_nonedict(v) for v in opt]
    return opt


def check_resume(opt, resume_iter):
    """When resuming, the generator weights come from `<models>/<iter>_G.pth`, whatever pretrain path was set."""
    log = logging.getLogger("base")
    if not opt["path"]["resume_state"]:
        return
    if opt["path"].get("pretrain_model_G") is not None or opt["path"].get("pretrain_model_D") is not None:
        log.warning("pretrain_model path will be ignored when resuming training.")
    opt["path"]["pretrain_model_G"] = osp.join(opt["path"]["models"], f"{resume_iter}_G.pth")
    log.info("Set [pretrain_model_G] to " + opt["path"]["pretrain_model_G"])
    # train.ema_decay: the averaged weights saved beside them; read after resume_training, only when the option is on
    opt["path"]["pretrain_model_G_ema"] = osp.join(opt["path"]["models"], f"{resume_iter}_G_ema.pth")
    if "gan" in opt["model"]:
        opt["path"]["pretrain_model_D"] = osp.join(opt["path"]["models"], f"{resume_iter}_D.pth")
        log.info("Set [pretrain_model_D] to " + opt["path"]["pretrain_model_D"])
