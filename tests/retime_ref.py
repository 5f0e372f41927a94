"""An independent restatement of the frame-rate conversion in `fractions.Fraction` and Python ints /
numpy int64, written from the definition and not from retime.py or csrc/retime.hip.h.

Source rate Fi, target rate Fo > Fi; output frame j sits at input time t = j * Fi / Fo.  Interval i = floor(t), phase
t - i.  The grid has G = 2**depth rows per interval; the row below the frame is floor(phase * G), and the weight of the
row above is the rest, phase * G - floor(phase * G), a fraction with denominator q (the denominator of Fi / Fo reduced).
"""
from fractions import Fraction
from math import floor

import numpy as np


def ratio(src_fps, fps):
    return Fraction(src_fps) / Fraction(fps)


def n_out(n_frames, src_fps, fps):
    """Frames j >= 0 with j * Fi / Fo <= n_frames - 1."""
    step = ratio(src_fps, fps)
    return floor(Fraction(n_frames - 1) / step) + 1


def place(j, src_fps, fps, depth):
    """-> (i, on_input, lo, w): interval, whether the frame sits exactly on input frame i, grid row below (within the
    interval), and the weight of the row above as a Fraction."""
    t = j * ratio(src_fps, fps)
    i = floor(t)
    g = (t - i) * (1 << depth)
    lo = floor(g)
    return i, t == i, lo, g - lo


def _read(a, bits):
    a = np.asarray(a)
    if bits == 10:
        a = a.view(np.uint16) if a.dtype == np.int16 else a
        return np.minimum(a.astype(np.int64), 1023)
    return a.astype(np.int64)


def frame(grid, j, src_fps, fps, depth, bits, mode="blend", flags=None, first_interval=0):
    """Output frame j from `grid` [(n_intervals << depth) + 1, ...], which covers clip intervals from first_interval."""
    G = 1 << depth
    q = ratio(src_fps, fps).denominator
    i, on_input, lo, w = place(j, src_fps, fps, depth)
    k = i - first_interval
    if flags is not None and not on_input and flags[k]:
        return grid[k * G].copy()
    a = grid[k * G + lo]
    if w == 0:
        return a.copy()
    b = grid[k * G + lo + 1]
    if mode == "nearest":
        return (b if w > Fraction(1, 2) else a).copy()
    wn = w * q
    assert wn.denominator == 1
    wn = int(wn)
    val = (_read(a, bits) * (q - wn) + _read(b, bits) * wn + q // 2) // q
    return val.astype(grid.dtype)


def resample(grid, n_frames, src_fps, fps, depth, bits, mode="blend", flags=None):
    """The whole clip: `grid` is the factor-2**depth result of a clip of n_frames frames."""
    return np.stack([frame(grid, j, src_fps, fps, depth, bits, mode, flags)
                     for j in range(n_out(n_frames, src_fps, fps))])
