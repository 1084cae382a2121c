"""Frame-rate factors above 2: interpolation passes chained on their own fp32 outputs (`--factor 4 | 8`, harness.interpolate_video's
`factor=`).  Host side only, pure Python: nothing here touches a device; the frames are whatever the caller's callables exchange
(device tensors in the runners, stubs in the CPU tests).

The network produces the midpoint of a frame pair, so a factor F = 2^k is k passes.  For one scene of n input frames:

    level 1   S1 = (D_0, I_0, D_1, ..., I_(n-2), D_(n-1)), 2(n-1)+1 frames: the generator's padded fp32 outputs on the input frames
              (`level1_plan`: window i gives D_i from slot 8 when it opens the scene, I_i from slot 13, D_(i+1) from slot 12);
    level p   from S = S(p-1) of length L:  Sp[2j] = S[j], the same object, and Sp[2j+1] = slot 13 of the generator on
              reframe(S[i]) for i in window_ids(j, L), j = 0 .. L-2; 2L-1 frames, so F(n-1)+1 at level k.

`reframe` is the hand-off (ops.reframe, include/binchain.h): crop, clamp to [0, 1], replicate-pad: what makes a network output a
network input.  Every frame is reframed once, by the first pass that consumes it; the result travels with the frame to the later
passes and stays one long-lived object until no later window names it, which is what the generator's memo keys on.

`Chain` is the scheduler of the passes 2 .. k.  It is incremental, because the length of a piped stream is unknown: level-1 frames
are pushed as they appear, `end` says that the scene is complete.  Pass p runs its window j as soon as S(p-1)[j+3] exists or the
end of that sequence is known, hands S[j] and the new frame on to pass p+1 in order, and drops what no later window names, so
the number of live frames per pass does not depend on the length of the stream.  The last level is emitted in display order at
positions F*start + index; the scene's last frame D_(n-1) is followed by F-1 holds when a cut follows it (the positions up to the
next scene's F*e) and is not emitted at all when the stream ends there: a stream of T frames gives F(T-1) outputs, and every second
one of them is the output at F/2.

`run_stream` is the window loop of every video run (bin_amd.test's on a pipe, harness.interpolate_video's in memory): level 1 over a
feed of frames into a Chain.  Factor 2 is the same loop: levels(2) == 1, the Chain is its emitter alone."""

HOLD = None                                # emit()'s frame of a held position: the payload emitted just before, once more
FACTORS = (2, 4, 8)
SLOTS = (13, 8, 12)                        # what a level-1 forward is asked for: interpolated, first deblurred, second deblurred


def levels(factor):
    """k of F = 2^k; ValueError for anything but 2, 4, 8 (bools and floats that merely compare equal included)."""
    if type(factor) is not int or factor not in FACTORS:
        raise ValueError(f"factor must be one of {FACTORS} (got {factor!r})")
    return factor.bit_length() - 1


def sequence_length(n_frames, level):
    """Frames of level `level` of a scene of n_frames input frames: 2^level (n_frames - 1) + 1."""
    return (1 << level) * (n_frames - 1) + 1


def window_ids(index, length):
    """The six sequence ids of the window centred on `index` (the reference's test.py:257-261): index + [-2 .. 3], clamped."""
    return [min(max(index + d, 0), length - 1) for d in (-2, -1, 0, 1, 2, 3)]


def level1_plan(i, s, e):
    """Window i of the scene [s, e) of input frames, s <= i < e: (ids, slots, last).  ids: the six input frame ids of the forward
    (clamped to the scene: the reference's end-of-clip rule, applied at scene ends), or None when none is run; slots: the Ft_p slots that are the next level-1 frames, in
    order; last: whether the scene ends with this window (a cut follows frame i).  The window of a scene's last frame exists only
    when a cut follows; at the end of the stream the scene ends with window e-2."""
    if not s <= i < e:
        raise ValueError(f"level1_plan: window {i} of scene [{s}, {e})")
    if i + 1 < e:
        return [min(max(i + d, s), e - 1) for d in (-2, -1, 0, 1, 2, 3)], ((8,) if i == s else ()) + (13, 12), False
    if i == s:
        return [s] * 6, (8,), True                  # a one-frame scene: D_s from six copies of itself
    return None, (), True                           # D_i came from window i-1's slot 12


class _Pass:
    """Pass `level` >= 2: consumes S(level-1) in order, hands S(level) to `sink` in order."""

    def __init__(self, chain, level, sink):
        self.chain, self.level, self.sink = chain, level, sink
        self.frames = {}                            # sequence id -> [frame (until handed on), reframed frame]
        self.n, self.length, self.next_window, self.group = 0, None, 0, []

    def held(self):
        return [t for pair in self.frames.values() for t in pair if t is not None]

    def push(self, pairs):
        """pairs: [(frame, its reframed copy or None)], the next frames of the sequence."""
        new = [f for f, r in pairs if r is None]
        made = iter(self.chain.reframe(new) if new else ())
        for f, r in pairs:
            self.frames[self.n] = [f, next(made) if r is None else r]
            self.n += 1
            self.chain._note()
            self._advance()

    def end(self):
        self.length = self.n
        self._advance()
        self._flush()
        if self.n:
            last = self.frames.pop(self.n - 1)
            self.sink.push([(last[0], last[1])])
        self.frames.clear()
        self.sink.end()

    def _advance(self):
        while True:
            j = self.next_window
            if self.length is None:
                if j + 3 >= self.n:
                    return
                known = j + 4                       # clamping at the far end only bites once the end is known
            elif j > self.length - 2:
                return
            else:
                known = self.length
            ids = window_ids(j, known)
            self.group.append((j, ids, [self.frames[i][1] for i in ids]))
            self.next_window += 1
            if len(self.group) >= self.chain.batch:
                self._flush()

    def _flush(self):
        if not self.group:
            return
        outs = self.chain.forward(self.level, [(ids, frames) for _, ids, frames in self.group])
        self.chain.windows[self.level - 2] += len(self.group)
        down = []
        for (j, _, _), out in zip(self.group, outs):
            down += [(self.frames[j][0], self.frames[j][1]), (out, None)]
            self.frames[j][0] = None
        self.group.clear()
        for i in [i for i in self.frames if i < self.next_window - 2]:      # no later window names them
            del self.frames[i]
        self.sink.push(down)


class _Emitter:
    """The last level in display order.  One frame is held back: whether the scene's last frame is emitted is known at its end."""

    def __init__(self, chain):
        self.chain, self.last = chain, None

    def held(self):
        return [] if self.last is None else [self.last]

    def push(self, pairs):
        for f, _ in pairs:
            if self.last is not None:
                self.chain._emit(self.last)
            self.last = f
            self.chain._note()

    def end(self):
        if self.last is not None and not self.chain.final:
            self.chain._emit(self.last)
            for _ in range(self.chain.factor - 1):
                self.chain._emit(HOLD)
        self.last = None


class Chain:
    """The passes 2 .. k of a factor-2^k run over the scenes of one stream.

        forward(level, [(ids, frames), ...]) -> [frame, ...]   slot 13 of the generator per window of pass `level`: `frames` are
                                                               the six reframed inputs, `ids` their sequence ids; at most `batch`
                                                               windows per call, consecutive ones of one scene;
        reframe([frame, ...]) -> [frame, ...]                  the hand-off, fresh objects;
        emit(position, frame | HOLD)                           the output stream, in display order;
        new_scene()                                            optional: a scene begins, nothing memoised belongs to it.

    Per scene: begin(start), push(frames) with the next level-1 frames (any number at a time), end(final).  `final`: the stream
    ends with this scene.  `windows[p-2]` counts the forwards of pass p, `frames_resident_peak` is the largest number of distinct
    frames (hand-off frames and their reframed copies) the passes held at any time."""

    def __init__(self, factor, forward, reframe, emit, batch=1, new_scene=None):
        self.factor, self.k = factor, levels(factor)
        self.forward, self.reframe, self.emit, self.new_scene = forward, reframe, emit, new_scene
        self.batch = max(1, int(batch))
        self.windows = [0] * (self.k - 1)
        self.frames_resident_peak = 0
        self.position, self.final, self.head, self.stages = None, False, None, []

    def begin(self, start):
        if self.head is not None:
            raise RuntimeError("Chain.begin: the scene before has not ended")
        if self.new_scene is not None:
            self.new_scene()
        self.position, self.final = self.factor * start, False
        sink = _Emitter(self)
        self.stages = [sink]
        for level in range(self.k, 1, -1):
            sink = _Pass(self, level, sink)
            self.stages.append(sink)
        self.head = sink

    def push(self, frames):
        self.head.push([(f, None) for f in frames])

    def end(self, final):
        self.final = bool(final)
        self.head.end()
        self.head, self.stages = None, []

    def _emit(self, frame):
        self.emit(self.position, frame)
        self.position += 1

    def _note(self):
        live = len({id(t) for stage in self.stages for t in stage.held()})
        self.frames_resident_peak = max(self.frames_resident_peak, live)


def run_stream(feed, net, emit, factor, batch=1, around=lambda flush: flush()):
    """The window loop of every video run, factor 2 included: level 1 over the frames of `feed`, scene by scene, into a Chain.

        feed    read_to(i) makes the frames up to i exist in `frames_dev` (id -> frame) or learns the stream's length `n_frames`
                (None until then); with `scene_on`, resolve_cuts() decides every frame read so far into the sorted list `cuts`;
        net     run(level, [(ids, six frames)], slots) -> one {slot: frame} per window, forward, reframe, new_scene (Chain's);
        emit    Chain's;
        around  around(flush) is called where a level-1 forward is due; flush() runs it with everything that follows from
                it (the passes above, the emits) and returns how many windows it took care of.  For timing and for handing over.

    The length of a piped stream is not known ahead: window i runs once frame i + 3 or the end of the stream has been read, and
    needs the cuts up to the pair (i + 2, i + 3) only.  Consecutive forward-running windows share a forward in groups of `batch`,
    whether or not a scene ends inside the group (windows are independent; a window that only holds a frame runs no forward and does
    not count); what a group's windows mean to the Chain (a scene begins, frames to push, a scene ends) is replayed in order around
    the forward, which is queued when the replay reaches the group's first window: with batch 1 the end of the scene before and the
    `begin` come ahead of it, so new_scene() follows the last forward of every pass of that scene and precedes the scene's first.  Frames no later window names are dropped from
    `frames_dev`.  Returns {windows, windows_per_pass, frames_resident_peak}: the windows considered (T - 1), the forwards per pass."""
    passes = Chain(factor, net.forward, net.reframe, emit, batch=batch, new_scene=net.new_scene)
    group, jobs, level1 = [], [], [0]              # (scene start to begin or None, slots, ends its scene) per window; [(ids, frames)]
    index, start, is_open = 0, 0, False

    def flush(final=False):
        outs = None
        for begin, slots, last in group:
            if begin is not None:
                passes.begin(begin)
            if slots:
                if outs is None:
                    outs = iter(net.run(1, jobs, SLOTS))
                out = next(outs)
                passes.push([out[slot] for slot in slots])
            if last:
                passes.end(final=False)
        if final and is_open:
            passes.end(final=True)
        n = len(group)
        level1[0] += len(jobs)
        group.clear()
        jobs.clear()
        return n

    while True:
        feed.read_to(index + 3)
        n_frames = feed.n_frames
        if n_frames is not None and index > n_frames - 2:
            break
        end = n_frames if n_frames is not None else index + 4      # clamping only bites once the end is known
        if feed.scene_on:
            feed.resolve_cuts()                     # every pair up to (index + 2, index + 3), or up to the stream's end
            if index in feed.cuts:
                start = index
            # the scene's end: the next cut when it is in sight; beyond index + 3 any end gives the same window
            end = next((c for c in feed.cuts if c > index), end)
        ids, slots, last = level1_plan(index, start, end)
        group.append((None if is_open else start, slots, last))
        is_open = not last
        if ids is not None:
            jobs.append((ids, [feed.frames_dev[f] for f in ids]))   # (the windows in `jobs` hold their own references)
            for f in [f for f in feed.frames_dev if f < min(ids)]:
                del feed.frames_dev[f]
        if len(jobs) >= passes.batch:
            around(flush)
        index += 1
    around(lambda: flush(final=True))
    return {"windows": index, "windows_per_pass": level1 + passes.windows, "frames_resident_peak": passes.frames_resident_peak}
