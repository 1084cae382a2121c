"""Dataset / dataloader factories under the reference's names (data/__init__.py:7-46).

Loader policy, as there: the training loader never shuffles itself (order comes from the sampler or from the dataset's
own shuffled window list), drops the ragged last batch, and — under torch.distributed — gives every rank
batch_size // world_size samples with n_workers workers; single-process runs scale the workers by the number of GPUs
listed in the options.  Every other phase is an in-order loader of single samples (from the device frame cache too, when
the phase's `device_cache` asks for it)."""
import logging

import torch
import torch.utils.data as tud


def _train_loader_shape(dataset_opt, opt):
    """(per-process batch, workers) of the training loader."""
    batch, workers = dataset_opt["batch_size"], dataset_opt["n_workers"]
    if opt["dist"]:
        world = torch.distributed.get_world_size()
        if batch % world:
            raise AssertionError(f"batch_size {batch} is not divisible by the {world} ranks")
        return batch // world, workers
    return batch, workers * max(1, len(opt["gpu_ids"] or [0]))


def create_dataloader(dataset, dataset_opt, opt=None, sampler=None, vscode_debug=False):
    common = dict(shuffle=False, pin_memory=torch.cuda.is_available())
    train = dataset_opt["phase"] == "train"
    batch, workers = _train_loader_shape(dataset_opt, opt) if train else (1, 1)
    if hasattr(dataset, "make_device_cache"):
        # bin_amd extension, mode BIN_video: windows of sharp Y4M clips (data/video_dataset.py), served from the device frame cache in
        # every phase
        from .device_cache import create_device_loader
        from .video_dataset import NO_HOST_LOADER
        if not dataset_opt.get("device_cache"):
            raise ValueError(NO_HOST_LOADER)
        return create_device_loader(dataset, dataset_opt, batch, sampler if train else None)
    if dataset_opt.get("device_cache"):
        # bin_amd extension: batches cut out of a device-resident frame cache (data/device_cache.py); BIN windows only.  Any
        # other phase: single windows in order, nothing dropped; the loader (and with it the cache) is built once and
        # iterated by every validation pass
        from .BIN_dataset import BINDataset
        if isinstance(dataset, BINDataset):
            from .device_cache import create_device_loader
            return create_device_loader(dataset, dataset_opt, batch, sampler if train else None)
        logging.getLogger("base").warning("device_cache applies to mode BIN datasets only; [%s] uses the host loader",
                                          type(dataset).__name__)
    if not train:
        return tud.DataLoader(dataset, batch_size=1, num_workers=0 if vscode_debug else 1, **common)
    return tud.DataLoader(dataset, batch_size=batch, sampler=sampler, drop_last=True,
                          num_workers=0 if vscode_debug else workers, **common)


def create_dataset(dataset_opt):
    # "synthetic_texture" is a bin_amd extension: clips rendered on the fly with the structure of the reference's windows
    # and "BIN_video": windows of sharp high-frame-rate Y4M clips, their blurry inputs synthesised (data/video_dataset.py)
    kinds = {"BIN": ("BIN_dataset", "BINDataset"), "synthetic_texture": ("synthetic", "SyntheticTextureDataset"),
             "BIN_video": ("video_dataset", "VideoClipDataset")}
    mode = dataset_opt["mode"]
    if mode not in kinds:
        raise NotImplementedError("Dataset [{:s}] is not recognized.".format(mode))
    module, cls = kinds[mode]
    dataset = getattr(__import__(f"{__name__}.{module}", fromlist=[cls]), cls)(dataset_opt)
    logging.getLogger("base").info("Dataset [%s - %s] is created.", cls, dataset_opt["name"])
    return dataset


__all__ = ("create_dataloader", "create_dataset")
