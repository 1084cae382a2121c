"""Case table and references of the self-ensemble (bin_amd/ensemble.py, include/binens.h), shared by test_cpu_ensemble.py and
test_gpu_ensemble.py.

References: `orient_ref` and `merge_ref32` restate the two kernels in numpy float32 — the merge with the SAME balanced pairwise tree,
so the kernels are held to it bit for bit (the arithmetic is adds and a power-of-two scale); `merge_ref64` is the plain float64 mean.
Values lie in [-1, 2] (a frame's range with some headroom) plus one case with inf and NaN planted.  Denormal RESULTS are not
covered: 1/M is exact only while the scaled sum stays normal, and no value here comes near 1e-38.

Arenas: every tensor of a case sits in one float32 array per tensor at an offset of 0, 1, 2 or 3 floats (0, 4, 8, 12 bytes) from a
16-byte boundary, with GUARD floats before and after, as test_gpu_ema.py builds them; the guards must come back untouched.

StubNet is a fixed, exact 3x3 convolution: small integer weights that are symmetric under neither flip, inputs on a 1/8 grid, so
every fp32 sum is exact in any order and the reference helper's sequential sum and our tree agree bit for bit.  FakeNetG is a
recording six-frame stand-in built from it for the scheduler tests; TorchKernels states ops.ens_orient / ops.ens_merge in torch."""
import collections

import numpy as np
import torch

from bin_amd import ensemble as E

GUARD = np.float32(-777.25)
PAD = 8                                            # guard floats on either side (and room for the offset)
SHAPES = ((1, 1, 1), (3, 1, 2), (3, 2, 2), (3, 2, 6), (3, 3, 5), (6, 7, 9), (3, 6, 10), (6, 32, 48), (3, 4, 260), (3, 66, 130))
FULL_SIZE = (3, 768, 1344)
MS = (1, 2, 4, 8)
OFFSETS = (0, 1, 2, 3)                             # floats past a 16-byte boundary

Case = collections.namedtuple("Case", "tag shape M offs special seed")
# offs: per buffer (src 0..M-1 then dst for a merge; src then dst 0..M-1 for an orient) the offset in floats, cycled


def _cases():
    out = []
    k = 0
    for shape in SHAPES:
        for M in MS:
            # every shape x M at: everything aligned; and one misaligned pattern that walks through the offsets
            out.append(Case(f"{'x'.join(map(str, shape))}_M{M}_aligned", shape, M, (0,), False, 100 + k))
            out.append(Case(f"{'x'.join(map(str, shape))}_M{M}_off{OFFSETS[1 + k % 3]}", shape, M, (OFFSETS[1 + k % 3],), False, 200 + k))
            k += 1
    # each offset on its own for a 16 B-capable shape, and mixed offsets (one buffer off is enough to leave the 16 B path)
    for off in OFFSETS:
        out.append(Case(f"3x6x8_M4_off{off}", (3, 6, 8), 4, (off,), False, 300 + off))
    out.append(Case("6x32x48_M8_mixed", (6, 32, 48), 8, (0, 1, 2, 3), False, 310))
    out.append(Case("3x4x260_M4_dst_off", (3, 4, 260), 4, (0, 0, 0, 0, 3), False, 311))
    out.append(Case("6x7x9_M8_inf_nan", (6, 7, 9), 8, (0,), True, 312))
    out.append(Case("6x32x48_M4_inf_nan", (6, 32, 48), 4, (0,), True, 313))
    return tuple(out)


CASES = _cases()
TAGS = tuple(c.tag for c in CASES)
CASE_BY_TAG = {c.tag: c for c in CASES}
FULL_CASE = Case("full_3x768x1344_M8", FULL_SIZE, 8, (0,), False, 400)


def flips_of(M):
    """The flip of each orientation of a case: the spatial group {0, W, H, W|H}, repeated for M = 8 (the time-reversed half)."""
    return [o & 3 for o in range(M)]


def values(case, count):
    """`count` float32 arrays of the case's shape, seeded, in [-1, 2]; a `special` case has inf, -inf and NaN planted in distinct
    sources at distinct positions."""
    rng = np.random.Generator(np.random.PCG64(case.seed))
    xs = [rng.uniform(-1.0, 2.0, size=case.shape).astype(np.float32) for _ in range(count)]
    if case.special:
        flat = [x.reshape(-1) for x in xs]
        n = flat[0].size
        flat[0][1 % n] = np.inf
        flat[min(1, count - 1)][(n // 2) % n] = -np.inf
        flat[count - 1][n - 1] = np.nan
        flat[count // 2][(n // 3) % n] = np.inf          # inf + (-inf) somewhere is possible too: NaN, as IEEE says
    return xs


def flip_np(a, flip):
    if flip & E.FLIP_W:
        a = a[..., ::-1]
    if flip & E.FLIP_H:
        a = a[..., ::-1, :]
    return np.ascontiguousarray(a)


def orient_ref(src, flips):
    return [flip_np(src, f) for f in flips]


def merge_ref32(srcs, flip_of):
    """float32, the kernel's tree and its scale."""
    leaves = [flip_np(s, f).astype(np.float32) for s, f in zip(srcs, flip_of)]
    with np.errstate(invalid="ignore"):
        return (E.tree_sum(leaves) * np.float32(1.0 / len(leaves))).astype(np.float32)


def merge_ref64(srcs, flip_of):
    with np.errstate(invalid="ignore"):
        return np.mean([flip_np(s, f).astype(np.float64) for s, f in zip(srcs, flip_of)], axis=0)


def arena(x, off):
    """x in a guarded float32 array: [GUARD * (PAD + off)] x [GUARD * PAD]; returns (array, start)."""
    a = np.full(x.size + 2 * PAD + off, GUARD, dtype=np.float32)
    a[PAD + off:PAD + off + x.size] = x.reshape(-1)
    return a, PAD + off


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ exact stand-ins for the network
class StubNet(torch.nn.Module):
    """3 -> 3 channels, 3x3, zero padding, no bias; integer weights in [-3, 3], symmetric under neither flip."""

    def __init__(self):
        super().__init__()
        w = torch.tensor([[1, -2, 0], [3, 1, -1], [0, 2, -3]], dtype=torch.float32)
        k = torch.stack([torch.stack([torch.roll(w, shifts=(i, j), dims=(0, 1)) * (1 if (i + j) % 2 == 0 else -1) for j in range(3)])
                         for i in range(3)])                     # [3 out, 3 in, 3, 3]
        assert not torch.equal(k, k.flip(-1)) and not torch.equal(k, k.flip(-2))
        self.register_buffer("weight", k)

    def forward(self, x):
        return torch.nn.functional.conv2d(x, self.weight.to(x.dtype), padding=1)


def grid_frame(seed, shape):
    """A seeded tensor on the 1/8 grid in [-1, 2]: every product with a small integer and every sum of a few dozen is exact."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 17, shape, generator=g).to(torch.float32) / 8


class FakeNetG(torch.nn.Module):
    """Six frames -> 14 outputs, exact and deterministic: out[k] = stub(B[k % 6]) + (k + 1) * B[(k + 2) % 6].  Records, per call, the
    input objects, the batch size and the cache dict it was handed.  `small` answers the model's own fill rule."""

    reuse_schedule = True

    def __init__(self, small=False):
        super().__init__()
        self.stub = StubNet()
        self.small = small
        self.calls = []

    def _use_four_calls_infer(self, frame):
        return self.small

    def forward(self, *B, stage1_cache=None):
        assert len(B) == 6
        self.calls.append({"inputs": B, "batch": B[0].shape[0], "cache": stage1_cache})
        return tuple(self.stub(B[k % 6]) + (k + 1) * B[(k + 2) % 6] for k in range(14))


def torch_flip(x, flip):
    dims = [d for d, bit in ((-1, E.FLIP_W), (-2, E.FLIP_H)) if flip & bit]
    return torch.flip(x, dims) if dims else x.clone()


class TorchKernels:
    """ops.ens_orient / ops.ens_merge in torch (CPU or GPU): the same contract, the same tree."""

    def __init__(self):
        self.orient_launches = self.merge_launches = 0

    def ens_orient(self, frames, dsts, flips):
        self.orient_launches += 1
        out = []
        for i, (x, fs) in enumerate(zip(frames, flips)):
            row = []
            for j, f in enumerate(fs):
                y = torch_flip(x, f)
                if dsts is not None and dsts[i][j] is not None:
                    dsts[i][j].copy_(y)
                    y = dsts[i][j]
                row.append(y)
            out.append(row)
        return out

    def ens_merge(self, srcs_per_slot, flip_of, out=None):
        self.merge_launches += 1
        return [E.tree_sum([torch_flip(s, f) for s, f in zip(srcs, flip_of)]) * (1.0 / len(flip_of)) for srcs in srcs_per_slot]


def by_hand(netG, frames, group, flip=torch_flip):
    """The ensemble composed from the generator, torch.flip, SLOT_REVERSED and the tree: one generator call per orientation."""
    orient = E.orientations(group)
    runs = []
    for f, rev in orient:
        ins = [flip(x, f).contiguous() for x in (frames[::-1] if rev else frames)]
        runs.append(netG(*ins))
    out = []
    for k in range(14):
        leaves = [flip(runs[o][E.SLOT_REVERSED[k] if rev else k], f) for o, (f, rev) in enumerate(orient)]
        out.append(E.tree_sum(leaves) * (1.0 / len(orient)))
    return out
