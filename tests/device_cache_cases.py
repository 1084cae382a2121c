"""Shared by tests/test_cpu_device_cache.py and tests/test_gpu_device_cache.py: the numpy restatement of binhip_gather_windows
and the frames of an Adobe tree as the device cache holds them."""
import numpy as np


def gather_reference(frames, table, crop):
    """out[s][b][c][y][x] = float32(frames[id][y0 + y][flip ? x0 + cw - 1 - x : x0 + x][2 - c]) / float32(255), id = table[b][s]
    (include/binhip.h, binhip_gather_windows).  frames: uint8 [n_frames, H, W, 3] BGR; table: int [n, n_slots + 3]."""
    ch, cw = crop
    table = np.asarray(table)
    n, n_slots = table.shape[0], table.shape[1] - 3
    out = np.empty((n_slots, n, 3, ch, cw), np.float32)
    for b in range(n):
        y0, x0, flip = (int(v) for v in table[b, n_slots:])
        xs = x0 + cw - 1 - np.arange(cw) if flip else x0 + np.arange(cw)
        for s in range(n_slots):
            win = frames[int(table[b, s])][y0:y0 + ch][:, xs]                      # ch, cw, 3 (BGR)
            out[s, b] = win[:, :, ::-1].transpose(2, 0, 1).astype(np.float32) / np.float32(255)
    return out


def arena_of(windows):
    """(uint8 [n_frames, H, W, 3] BGR, path -> id) for the unique frames of `windows`, in DeviceFrameCache's order."""
    from bin_amd.data.device_cache import window_slots
    from bin_amd.data.util import imread_u8
    index, paths = {}, []
    for w in windows:
        for p in window_slots(w, False):
            if p not in index:
                index[p] = len(paths)
                paths.append(p)
    return np.stack([imread_u8(p)[:, :, :3] for p in paths]), index


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
