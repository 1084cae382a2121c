#!/usr/bin/env python3
"""Golden fixture g14_flipx4.npz: the REFERENCE's four-flip self-ensemble helper `flipx4_forward` (utils/test_util.py:110-132: the
forward of the input, of its W flip, its H flip and both, each flipped back, summed in that order, divided by 4) on
tests/ensemble_cases.py::StubNet (an exact 3x3 convolution) and a seeded [1,3,6,10] input on the 1/8 grid.  Every value is exact in
fp32 whatever the order of the sum, so bin_amd.ensemble's tree over `hv` must reproduce the output bit for bit.
cv2 is stubbed as in make_golden_stitch.py.  Build container only (imports /root/reference); run:
python tests/golden/make_golden_flipx4.py"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, "/root/reference")
for name in ("cv2", "torchvision", "torchvision.utils", "torchvision.models"):
    if name not in sys.modules:
        m = types.ModuleType(name)
        m.make_grid = lambda *a, **k: None
        sys.modules[name] = m
sys.modules["torchvision"].utils = sys.modules["torchvision.utils"]
sys.modules["torchvision"].models = sys.modules["torchvision.models"]

from utils.test_util import flipx4_forward                         # noqa: E402
import ensemble_cases as EC                                        # noqa: E402

SEED, SHAPE = 1404, (1, 3, 6, 10)
torch.set_num_threads(1)
x = EC.grid_frame(SEED, SHAPE)
y = flipx4_forward(EC.StubNet().eval(), x)
assert tuple(y.shape) == SHAPE and y.dtype == torch.float32
assert torch.equal(y * 32, (y * 32).round()), "on the 1/32 grid: the four exact forwards, summed and divided by 4"
out = {"x": x.numpy(), "y": y.numpy(), "seed": np.int64(SEED)}
np.savez_compressed(os.path.join(HERE, "g14_flipx4.npz"), **out)
print("wrote g14_flipx4.npz", {k: getattr(v, "shape", v) for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "g14_flipx4.npz")), "B")
