"""Conversion to any lower frame rate with a synthesized shutter: the definition in numpy and `Fraction`s,
written from the definition's text alone - it shares no code with retime.py, and it gets to the weights another way (the
antiderivative of a row's hat function, taken over the unflagged pieces of the window, where retime.py walks the grid cells).

  rates     Fi / Fo reduced is p / q; a clip of N frames gives J = (N - 1) q // p + 1 frames
  time      grid time u = t G, grid row k at u = k; between rows the clip is the straight line between row floor(u) and
            the next one; in an interval i flagged as a cut it is row i G throughout
  window    frame j opens at u0 = j p G / q and closes at u1 = u0 + s p G / q, cut short at (N - 1) G and at the end of
            the first flagged interval it touches
  weights   W_k = (the integral of row k's hat function over the unflagged part of the window, and for k = i G the length
            of the window inside flagged interval i) / (u1 - u0); quantised to D = 2**20 by largest remainder, ties to
            the lower row; rows of weight 0 dropped
  frame     (sum_k w_k x_k + D / 2) >> 20 in int64, 10-bit words above 1023 read as 1023; one tap: a copy of the row
  s == 0    point sampling: retime.py's blend / nearest rule, which tests/retime_ref.py states for p < q, for any p, q
"""
import math
from fractions import Fraction

import numpy as np

D = 1 << 20


def n_out(n_frames, p, q):
    return (n_frames - 1) * q // p + 1


def window(p, q, G, s, j, n_frames, cuts=None):
    """(u0, u1) of output frame j of a clip of n_frames frames; cuts: one truth value per interval, or None."""
    u0 = Fraction(j * p * G, q)
    u1 = min(u0 + Fraction(s) * p * G / q, Fraction((n_frames - 1) * G))
    assert u0 <= u1
    if cuts is not None:
        for i in range(math.floor(u0 / G), len(cuts)):
            if i > math.floor(u0 / G) and i * G >= u1:
                break
            if cuts[i]:
                u1 = min(u1, Fraction((i + 1) * G))
                break
    return u0, u1


def _hat_integral(k, x):
    """The integral of row k's hat function max(0, 1 - |u - k|) from minus infinity to x."""
    d = Fraction(x) - k
    if d <= -1:
        return Fraction(0)
    if d <= 0:
        return (d + 1) ** 2 / 2
    if d <= 1:
        return Fraction(1, 2) + d - d * d / 2
    return Fraction(1)


def exact_weights(u0, u1, G, cuts=None):
    """{row: W_k} as exact Fractions that sum to 1."""
    def flagged(i):
        return cuts is not None and 0 <= i < len(cuts) and bool(cuts[i])
    W = {}
    if u0 == u1:
        i, k = math.floor(u0 / G), math.floor(u0)
        if flagged(i):
            return {i * G: Fraction(1)}
        W = {k: 1 - (u0 - k), k + 1: u0 - k}
        return {k: v for k, v in W.items() if v}
    # the window in pieces, one per interval it touches: flagged ones hold their first row, the others are hats
    i = math.floor(u0 / G)
    while i * G < u1:
        a, b = max(u0, Fraction(i * G)), min(u1, Fraction((i + 1) * G))
        if b > a:
            if flagged(i):
                W[i * G] = W.get(i * G, 0) + (b - a)
            else:
                for k in range(math.floor(a), math.ceil(b) + 1):
                    v = _hat_integral(k, b) - _hat_integral(k, a)
                    if v:
                        W[k] = W.get(k, 0) + v
        i += 1
    total = u1 - u0
    assert sum(W.values()) == total, (u0, u1, W)
    return {k: v / total for k, v in W.items()}


def quantise(W):
    """Largest remainder to D = 2**20: floors, then the left-over units to the largest fractional parts, ties to the lower
    row; rows of weight 0 are dropped."""
    rows = sorted(W)
    w = {k: math.floor(W[k] * D) for k in rows}
    left = D - sum(w.values())
    assert 0 <= left < max(len(rows), 1) + 1
    order = sorted(rows, key=lambda k: (-(W[k] * D - w[k]), k))
    for k in order[:left]:
        w[k] += 1
    assert sum(w.values()) == D
    return {k: v for k, v in w.items() if v}


def weights(p, q, G, s, j, n_frames, cuts=None):
    """{grid row of the clip: 20-bit weight} of output frame j."""
    u0, u1 = window(p, q, G, s, j, n_frames, cuts)
    return quantise(exact_weights(u0, u1, G, cuts))


def read(x, bits):
    x = np.asarray(x)
    if bits == 10:
        return np.minimum(x.view(np.uint16) if x.dtype == np.int16 else x, 1023).astype(np.int64)
    return x.astype(np.int64)


def mix(grid, w, bits):
    """One output frame from grid [rows, ...] and {row: weight}: int64 accumulation; a single tap is a copy."""
    grid = np.asarray(grid)
    if len(w) == 1:
        (k, v), = w.items()
        assert v == D
        return grid[k].copy()
    acc = np.zeros(grid.shape[1:], np.int64)
    for k, v in w.items():
        acc += read(grid[k], bits) * v
    return ((acc + D // 2) >> 20).astype(grid.dtype)


def apply_entries(grid, entries, bits):
    """What fiunet_shutter_* computes for (first_row, [w ...]) entries: one live tap (a weight of 2**20) is a copy."""
    return np.stack([mix(grid, {r + t: v for t, v in enumerate(w) if v}, bits) for r, w in entries])


def point(grid, p, q, G, j, bits, mode="blend", cuts=None):
    """Point sampling (s == 0), retime.py's rule for any p / q."""
    i, r = divmod(j * p, q)
    if r != 0 and cuts is not None and i < len(cuts) and cuts[i]:
        return grid[i * G].copy()
    lo, wn = divmod(r * G, q)
    a = i * G + lo
    if mode == "nearest":
        return grid[a + (1 if 2 * wn > q else 0)].copy()
    if wn == 0:
        return grid[a].copy()
    g = math.gcd(wn, q)
    wn, den = wn // g, q // g
    x = read(grid[a], bits) * (den - wn) + read(grid[a + 1], bits) * wn + den // 2
    return (x // den).astype(grid.dtype)


def convert(grid, n_frames, src_fps, fps, G, s, bits, cuts=None, mode="blend"):
    """Every output frame of the conversion from the frames of the factor = G run, grid [(n_frames - 1) G + 1, ...]."""
    ratio = Fraction(src_fps) / Fraction(fps)
    p, q = ratio.numerator, ratio.denominator
    assert grid.shape[0] == (n_frames - 1) * G + 1
    J = n_out(n_frames, p, q)
    if Fraction(s) == 0:
        return np.stack([point(grid, p, q, G, j, bits, mode, cuts) for j in range(J)])
    return np.stack([mix(grid, weights(p, q, G, s, j, n_frames, cuts), bits) for j in range(J)])
