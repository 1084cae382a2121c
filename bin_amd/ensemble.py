"""Test-time self-ensemble of the 6-frame generator over the symmetries its training loader draws: a horizontal flip, a vertical
flip and a reversal of time (data/BIN_dataset.py::draw_window_aug).  The network runs once per orientation of the input and the
estimates of one frame are averaged after each is brought back to the input's orientation.

A group is a subset of three letters: `h` (flip W), `v` (flip H), `t` (reverse time); k letters give M = 2^k orientations.  The
orientation index o carries one bit per letter PRESENT, compacted in the order h, v, t.  The spatial letters flip the padded frames
at the generator's boundary and flip its outputs back; `t` feeds the frames as (B11, B9, B7, B5, B3, B1), after which output slot
SLOT_REVERSED[k] holds the estimate of the frame (at the pyramid level) that slot k holds in a forward run.

For slot k:   E_k = (1/M) * sum over o of unflip_o( net(orient_o(frames))[ SLOT_REVERSED[k] if o reverses time else k ] )
with the sum taken as the balanced pairwise tree over o, ((x0+x1)+(x2+x3))+((x4+x5)+(x6+x7)).  The group acts on o by XOR, the tree
is invariant under XOR (fp32 addition commutes) and 1/M is a power of two, so the ensemble of an oriented input is the oriented
ensemble bit for bit — which a sequential sum would not give.

The flips and the merge are two HIP kernels (include/binens.h, ops.ens_orient / ops.ens_merge); SelfEnsemble is the host scheduler
that keeps the network's own schedules effective under it."""
import torch

FLIP_W, FLIP_H = 1, 2                  # = BINENS_FLIP_W / BINENS_FLIP_H (include/binens.h)
LETTERS = "hvt"
ALIASES = {"flipx4": "hv", "x8": "hvt"}

# which frame, at which pyramid level, each of the 14 outputs estimates (archs/RDN.py::_forward_streams `outs`, bin_model.get_info)
SLOT_FRAME = (2, 4, 6, 8, 3, 5, 7, 4, 6, 5, 10, 9, 8, 7)
SLOT_LEVEL = (1, 1, 1, 1, 2, 2, 2, 3, 3, 4, 1, 2, 3, 4)
# the reversed run's slot p[k] estimates original frame 12 - SLOT_FRAME[p[k]] at the same level: the unique p with
# SLOT_FRAME[p[k]] == 12 - SLOT_FRAME[k] and SLOT_LEVEL[p[k]] == SLOT_LEVEL[k]; an involution
SLOT_REVERSED = (10, 3, 2, 1, 11, 6, 5, 12, 8, 13, 0, 4, 7, 9)
N_SLOTS = 14


def parse_group(s):
    """The canonical spelling of a group: its letters in the order h, v, t, or "" for off.  Accepts any combination of the letters in
    any order without repeats, the aliases `flipx4` (= hv, the four flips) and `x8` (= hvt), and None, "" or `none` for off.
    Anything else raises ValueError."""
    if s is None:
        return ""
    if not isinstance(s, str):
        raise ValueError(f"self-ensemble group: {s!r} is not a string of the letters h, v, t")
    name = s.strip().lower()
    if name in ("", "none"):
        return ""
    name = ALIASES.get(name, name)
    if any(c not in LETTERS for c in name) or len(set(name)) != len(name):
        raise ValueError(f"self-ensemble group: {s!r} is not a combination of the letters h, v, t without repeats, "
                         f"nor one of {sorted(ALIASES)} or 'none'")
    return "".join(c for c in LETTERS if c in name)


def orientations(group):
    """[(spatial flip bits, time reversed)] of the M = 2^k orientations of `group`, by orientation index."""
    group = parse_group(group)
    out = []
    for o in range(1 << len(group)):
        on = {c for i, c in enumerate(group) if (o >> i) & 1}
        out.append(((FLIP_W if "h" in on else 0) | (FLIP_H if "v" in on else 0), "t" in on))
    return out


def tree_sum(xs):
    """The balanced pairwise tree over the index (numpy arrays, torch tensors or numbers); len(xs) is a power of two."""
    xs = list(xs)
    while len(xs) > 1:
        xs = [xs[i] + xs[i + 1] for i in range(0, len(xs), 2)]
    return xs[0]


class SelfEnsemble:
    """`SelfEnsemble(netG, group)(frames)` -> the 14 ensemble estimates of a window (fresh tensors; the network's own outputs, which
    its memo shares across forwards, are never written).

    Two strategies over the same two kernels:
      batched : one orient launch writes six [M*N,3,H,W] inputs (orientation o in batch rows [o*N, (o+1)*N); for a reversed
                orientation the flips of frame j go to input 5-j), ONE generator call at batch M*N, one merge launch over batch
                slices.  Chosen when one orientation does not fill the chip by the model's own rule (`_use_four_calls_infer`).
      streamed: one generator call per orientation at the input's own N, each with its OWN memo dict (the generator evicts the keys
                a forward did not touch, so a shared dict would thrash), then one merge launch.  `orient(frame)` is one launch per
                NEW frame; a caller that streams windows keeps the oriented frames per frame id beside the padded frame (or lets
                `window()` do it), so that input identities stay long-lived and the memo hits in every orientation.  The reversed
                orientations re-use whatever recurs by identity.
    `strategy`: None (the rule above), "batched" or "streamed".  `kernels`: the provider of ens_orient / ens_merge (bin_amd.ops)."""

    def __init__(self, netG, group, strategy=None, kernels=None):
        self.group = parse_group(group)
        if not self.group:
            raise ValueError("SelfEnsemble: an empty group is no ensemble (call the generator itself)")
        if strategy not in (None, "batched", "streamed"):
            raise ValueError("SelfEnsemble: strategy is None, 'batched' or 'streamed'")
        self.netG = netG
        self.strategy = strategy
        self.orient_of = orientations(self.group)
        self.M = len(self.orient_of)
        self.flip_of = [f for f, _ in self.orient_of]
        self.reversed_of = [r for _, r in self.orient_of]
        # the distinct spatial flips, in orientation order: index 0 is the identity (the frame itself, never copied)
        self.spatial = sorted(set(self.flip_of), key=self.flip_of.index)
        if kernels is None:
            from . import ops as kernels
        self.kernels = kernels
        self._oriented, self._caches = {}, None        # window(): oriented frames per frame id, one memo dict per orientation

    # ------------------------------------------------------------------------------------------------ pieces
    def _inner(self):
        return self.netG.module if hasattr(self.netG, "module") else self.netG

    def strategy_for(self, frame):
        if self.strategy is not None:
            return self.strategy
        rule = getattr(self._inner(), "_use_four_calls_infer", None)
        return "batched" if rule is not None and rule(frame) else "streamed"

    def orient(self, frame):
        """The spatial orientations of one frame, by index into `self.spatial`: the frame itself, then its flipped copies (one
        launch)."""
        if len(self.spatial) == 1:
            return (frame,)
        frame = frame.contiguous().float()
        return (frame,) + tuple(self.kernels.ens_orient([frame], None, [self.spatial[1:]])[0])

    def slot_source(self, k, o):
        """The output slot of orientation o's run that estimates what slot k estimates."""
        return SLOT_REVERSED[k] if self.reversed_of[o] else k

    def _merge(self, slots, source):
        """`source(o, slot)` -> tensor; one merge launch over the requested slots."""
        slots = list(slots)
        merged = self.kernels.ens_merge([[source(o, self.slot_source(k, o)) for o in range(self.M)] for k in slots], self.flip_of)
        out = [None] * N_SLOTS
        for k, t in zip(slots, merged):
            out[k] = t
        return out

    # ------------------------------------------------------------------------------------------------ the two strategies
    def _batched(self, frames, slots):
        n = frames[0].shape[0]
        shape = (self.M * n,) + tuple(frames[0].shape[1:])
        inputs = [torch.empty(shape, dtype=torch.float32, device=frames[0].device) for _ in range(6)]
        dsts = [[inputs[5 - j if rev else j][o * n:(o + 1) * n] for o, rev in enumerate(self.reversed_of)] for j in range(6)]
        self.kernels.ens_orient([f.contiguous().float() for f in frames], dsts, [self.flip_of] * 6)
        outs = self.netG(*inputs)
        return self._merge(slots, lambda o, k: outs[k][o * n:(o + 1) * n])

    def _streamed(self, frames, slots, oriented, caches):
        if oriented is None:
            oriented = [self.orient(f) for f in frames]
        if caches is not None and len(caches) != self.M:
            raise ValueError(f"SelfEnsemble: one cache dict per orientation ({self.M}), got {len(caches)}")
        outs = []
        for o, (flip, rev) in enumerate(self.orient_of):
            s = self.spatial.index(flip)
            ins = [oriented[5 - j if rev else j][s] for j in range(6)]
            outs.append(self.netG(*ins) if caches is None else self.netG(*ins, stage1_cache=caches[o]))
        return self._merge(slots, lambda o, k: outs[o][k])

    @torch.no_grad()
    def __call__(self, frames, slots=range(N_SLOTS), oriented=None, caches=None):
        """frames: the six [N,3,H,W] inputs (B1 .. B11).  Returns a 14-list: the estimates of `slots`, None elsewhere.
        oriented: optionally, per frame, what `orient(frame)` returned for it (streamed strategy; a caller's per-frame cache).
        caches  : optionally M dicts, the generator's `stage1_cache` of each orientation (streamed strategy)."""
        frames = list(frames)
        if len(frames) != 6:
            raise ValueError("SelfEnsemble: six frames")
        if self.strategy_for(frames[0]) == "batched":
            return self._batched(frames, slots)
        return self._streamed(frames, slots, oriented, caches)

    # ------------------------------------------------------------------------------------------------ streaming callers
    def reset(self):
        """Forget the oriented frames and the per-orientation memo dicts (a clip change)."""
        self._oriented.clear()
        self._caches = None

    def window(self, ids, frames, slots=range(N_SLOTS), reuse=True):
        """One window of a streamed clip: `ids` are the clip's frame ids of the six `frames` (the caller's cached, padded tensors).
        Keeps the oriented copies per frame id while a window still names the id, and one memo dict per orientation when `reuse`
        (and the streamed strategy) holds; `reset()` at a clip change."""
        if self.strategy_for(frames[0]) == "batched":
            return self._batched(list(frames), slots)
        for i in [i for i in self._oriented if i < min(ids)]:
            del self._oriented[i]
        for i, f in zip(ids, frames):
            hit = self._oriented.get(i)
            if hit is None or hit[0] is not f:
                self._oriented[i] = (f, self.orient(f))
        caches = None
        if reuse and getattr(self._inner(), "reuse_schedule", False):
            if self._caches is None:
                self._caches = [{} for _ in range(self.M)]
            caches = self._caches
        return self(frames, slots, oriented=[self._oriented[i][1] for i in ids], caches=caches)
