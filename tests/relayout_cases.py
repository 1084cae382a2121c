"""The weight relayout stated in numpy from the text of include/binhip.h, not from the kernel: what
binhip_weights_relayout, _dgrad, _rdb_gather and _batch must write, byte for byte, and the case table the CPU and GPU tests share.

A plane is fp16 [rows_pad / cb][cin_chunks][k * k][cb][2][8]: row block, 16-channel input chunk, tap dy * k + dx, row in the block,
16-byte half slot, eight channels.  Half slot s of row `row` holds channel half s ^ ((row >> 3) & 1) of the chunk (the XOR swizzle
of the fragment reads).  hi = fp16(v), lo = fp16(v - fp32(hi)).  The planes are those of the zero-padded forward-shaped operator
Wp[rows_pad][16 * cin_chunks][k][k] of the item, so that every kind is `conv2d(x, Wp)`:
  FWD         Wp[r, ci] = W[src(r), ci], bias_out[r] = bias[src(r)]; src(r) = (r % (cout/4)) * 4 + r // (cout/4) with `shuffle`
              (PixelShuffle's channel order as a row order), else r; zero where src(r) >= cout or ci >= cin
  DGRAD       Wp[r, j, dy, dx] = W[co(j), r, k-1-dy, k-1-dx], co(j) the same permutation under `shuffle`; zero where r >= cin or
              j >= cout; bias_out = 0
  RDB_GATHER  group g of a dense block (G0, C, G): Wp[r, G (c - g) + co, dy, dx] = W_c[co, base_g + r, 2-dy, 2-dx] for c = g .. C-1,
              base_0 = 0, base_g = G0 + G (g - 1); rows = G0 (g = 0) or G; bias_out = 0
"""
import collections

import numpy as np

FWD, DGRAD, GATHER = 0, 1, 2

Case = collections.namedtuple("Case", "kind cout cin k rows_pad chunks cb sg shape")
# kind, cout, cin, k, rows_pad, cin_chunks, cout_block, shuffle (FWD / DGRAD) or group (GATHER), (G0, C, G) of a GATHER block.
# Ragged cin and cout, both cout blocks, both permutations, k = 1 / 3 / 5, a row block above 0, every group, and a block other than
# bin_stage4's (which only the batch entry can express).
CASES = (
    Case(FWD, 40, 24, 3, 64, 2, 32, 0, None),
    Case(FWD, 64, 16, 1, 64, 1, 64, 1, None),
    Case(FWD, 12, 24, 5, 32, 2, 32, 0, None),
    Case(DGRAD, 3, 64, 3, 64, 1, 64, 0, None),
    Case(DGRAD, 64, 40, 3, 64, 4, 32, 1, None),
) + tuple(Case(GATHER, 32, 96 + 32 * g, 3, 96 if g == 0 else 32, 2 * (4 - g), 96 if g == 0 else 32, g, (96, 4, 32)) for g in range(4)) \
  + tuple(Case(GATHER, 64, 64 + 64 * g, 3, 64, 4 * (3 - g), 64 if g == 0 else 32, g, (64, 3, 64)) for g in range(3))


def case_id(c):
    name = ("fwd", "dgrad", "gather")[c.kind]
    if c.kind == GATHER:
        return "%s-%d.%d.%d-g%d" % ((name,) + c.shape + (c.sg,))
    return "%s-%dx%dx%d-%s" % (name, c.cout, c.cin, c.k, "shuffle" if c.sg else "plain")


def permuted(i, n):
    """The channel that position i of PixelShuffle(2)'s order holds: positions are [sub][n / 4], channels [n / 4][sub]."""
    q = n // 4
    return (i % q) * 4 + i // q


def fwd_operator(w, bias, rows_pad, chunks, shuffle):
    cout, cin, k, _ = w.shape
    wp = np.zeros((rows_pad, 16 * chunks, k, k), dtype=w.dtype)
    bp = np.zeros(rows_pad, dtype=w.dtype)
    for r in range(rows_pad):
        src = permuted(r, cout) if shuffle else r
        if src < cout:
            wp[r, :cin] = w[src]
            if bias is not None:
                bp[r] = bias[src]
    return wp, bp


def dgrad_operator(w, rows_pad, chunks, shuffle):
    cout, cin, k, _ = w.shape
    wp = np.zeros((rows_pad, 16 * chunks, k, k), dtype=w.dtype)
    for j in range(cout):
        co = permuted(j, cout) if shuffle else j
        wp[:cin, j] = w[co, :, ::-1, ::-1]
    return wp, np.zeros(rows_pad, dtype=w.dtype)


def gather_operator(ws, group, shape):
    G0, C, G = shape
    assert len(ws) == C and all(tuple(ws[c].shape) == (G, G0 + G * c, 3, 3) for c in range(C))
    rows = G0 if group == 0 else G
    base = 0 if group == 0 else G0 + G * (group - 1)
    wp = np.zeros((rows, G * (C - group), 3, 3), dtype=ws[0].dtype)
    for c in range(group, C):
        wp[:, G * (c - group):G * (c - group + 1)] = ws[c][:, base:base + rows, ::-1, ::-1].transpose(1, 0, 2, 3)
    return wp, np.zeros(rows, dtype=ws[0].dtype)


def case_sources(c, seed=0):
    """fp32 OIHW sources of a case (a list: one tensor, or the C convs of a dense block) and its bias (FWD) or None.  Magnitudes
    from 1e-3 to 10, so that hi spans fp16's normal range downwards and most lo values are fp16 subnormals."""
    g = np.random.Generator(np.random.PCG64([seed, CASES.index(c)]))

    def tensor(*shape):
        return (g.standard_normal(shape) * 10.0 ** g.uniform(-3.0, 1.0, shape)).astype(np.float32)

    if c.kind == GATHER:
        G0, C, G = c.shape
        return [tensor(G, G0 + G * i, 3, 3) for i in range(C)], None
    return [tensor(c.cout, c.cin, c.k, c.k)], (tensor(c.cout) if c.kind == FWD else None)


def case_operator(c, srcs, bias):
    if c.kind == FWD:
        return fwd_operator(srcs[0], bias, c.rows_pad, c.chunks, c.sg)
    if c.kind == DGRAD:
        return dgrad_operator(srcs[0], c.rows_pad, c.chunks, c.sg)
    return gather_operator(srcs, c.sg, c.shape)


def planes(wp, cb):
    """(hi, lo): the two fp16 planes of the fp32 operator wp [rows_pad][16 * chunks][k][k] at cout block cb, flat."""
    rows_pad, K, k, _ = wp.shape
    assert wp.dtype == np.float32 and rows_pad % cb == 0 and K % 16 == 0
    a = wp.reshape(rows_pad // cb, cb, K // 16, 2, 8, k * k).transpose(0, 2, 5, 1, 3, 4)   # [zb][chunk][tap][row][half][8]
    odd = ((np.arange(cb) >> 3) & 1).astype(bool)
    a = np.where(odd[:, None, None], a[..., ::-1, :], a)                                   # slot s <- half s ^ ((row >> 3) & 1)
    hi = a.astype(np.float16)
    lo = (a - hi.astype(np.float32)).astype(np.float16)
    return np.ascontiguousarray(hi).reshape(-1), np.ascontiguousarray(lo).reshape(-1)


def case_expected(c, srcs, bias):
    """(hi, lo, bias_out) of a case: fp16, fp16, fp32, flat."""
    wp, bp = case_operator(c, srcs, bias)
    return planes(wp, c.cb) + (bp,)
