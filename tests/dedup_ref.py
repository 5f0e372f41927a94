"""An independent restatement of the re-timing of repeated frames in `fractions.Fraction`, Python ints
and numpy int64, written from the definition and not from retime.py or the kernels.

  peak[i]  the largest sum of |F[i+1] - F[i]| over the aligned 64-sample segments of a frame as stored (the last one may
           be short; 10-bit words above 1023 read as 1023); interval i is dead iff peak[i] <= floor(dedup * 64)
  span     a maximal run of m >= 1 dead intervals a .. a+m-1 and the live interval i = a+m after it, where i is not a
           flagged cut and L = m + 1 <= max_gap
  time     output frame j at t = j * step (step = source rate / target rate): inside a span the time runs evenly over
           the live interval, u = (t - a) / L in [0, 1); the frame is the grid of interval i at u
"""
from fractions import Fraction
from math import floor

import numpy as np


def _read(a, bits):
    a = np.asarray(a)
    if bits == 10:
        a = a.view(np.uint16) if a.dtype == np.int16 else a
        return np.minimum(a.astype(np.int64), 1023)
    return a.astype(np.int64)


def pair_peak(stacks, bits=8):
    """int64 [N-1]; `stacks`: one [N, ...] array or several holding planes of the same frames."""
    if isinstance(stacks, np.ndarray):
        stacks = [stacks]
    n = stacks[0].shape[0]
    peaks = np.zeros(max(n - 1, 0), np.int64)
    for s in stacks:
        v = _read(s, bits).reshape(n, -1)
        d = np.abs(v[1:] - v[:-1])
        for lo in range(0, d.shape[1], 64):
            peaks = np.maximum(peaks, d[:, lo:lo + 64].sum(axis=1))
    return peaks


def dead_of(peaks, dedup):
    return [int(p) <= floor(Fraction(dedup) * 64) for p in peaks]


def span_of(f, dead, cuts, max_gap):
    """(a, i, L) of the span that holds interval f, or (f, f, 1)."""
    n = len(dead)
    if f >= n:
        return f, f, 1
    # the live interval at or after f that ends f's run
    i = f
    while i < n and dead[i]:
        i += 1
    if i == n:                                    # the run reaches the end of the clip
        return f, f, 1
    a = i
    while a > 0 and dead[a - 1]:
        a -= 1
    if a == i or (cuts is not None and cuts[i]) or i - a + 1 > max_gap:
        return f, f, 1
    return a, i, i - a + 1


def place(j, step, G, dead, cuts, max_gap):
    """-> (interval whose grid is read, row in it, weight of the row after as a Fraction, or None: the cut rule)."""
    t = j * Fraction(step)
    f = floor(t)
    if cuts is not None and f < len(cuts) and cuts[f] and t != f:
        return f, 0, None
    a, i, L = span_of(f, dead, cuts, max_gap)
    g = (t - a) / L * G
    lo = floor(g)
    return i, lo, g - lo


def frame(grid, j, step, G, bits, mode, dead, cuts, max_gap):
    i, lo, w = place(j, step, G, dead, cuts, max_gap)
    a = grid[i * G + lo]
    if w is None or w == 0:
        return a.copy()
    b = grid[i * G + lo + 1]
    if mode == "nearest":
        return (b if w > Fraction(1, 2) else a).copy()
    num, den = w.numerator, w.denominator
    val = (_read(a, bits) * (den - num) + _read(b, bits) * num) * 2 + den    # floor(x + 1/2) = floor((2 N + den) / 2 den)
    return (val // (2 * den)).astype(grid.dtype)


def n_out(n_frames, step):
    return floor(Fraction(n_frames - 1) / Fraction(step)) + 1


def resample(grid, n_frames, step, G, bits, mode, dead, cuts, max_gap):
    """The whole clip from `grid`, the factor-G result of its n_frames frames."""
    return np.stack([frame(grid, j, step, G, bits, mode, dead, cuts, max_gap) for j in range(n_out(n_frames, step))])
