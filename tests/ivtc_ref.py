"""Inverse telecine's definition in numpy (include/fiunet.h): the home of the definition.  The kernels of
csrc/ivtc.hip.h equal `comb_scores` and `weave` bit for bit (tests/test_gpu_ivtc.py); tests/test_ivtc_host.py holds the
whole of it to hand-computed values and to what inverse telecine is for.  It is the project's own, in the spirit of
ffmpeg's fieldmatch + decimate, and NOT pinned against ffmpeg.  Written from the definition, not from ivtc.py.

A clip is an integer array [N, H, W] of one plane, or frame rows [N, samples] with the planes of a layout.

  candidates  frame F[t] keeps the rows of parity k (0 for "tff", 1 for "bff"); the others come from F[t-1] (p), F[t] (c)
              or F[t+1] (n), clamped to the window
  comb score  H >= 3, int32: sample (y, x), 1 <= y <= H-2, is combed iff (W[y-1][x] - W[y][x]) * (W[y+1][x] - W[y][x])
              > T*T (10-bit words above 1023 read as 1023); the score is the largest count over the blocks of 16 rows x
              64 columns aligned to the plane's origin
  choice      c if sc <= min(sp, sn), else p if sp <= sn, else n; combed iff the chosen score > `combed`
  fallback    "deinterlace": a combed frame is tests/deinterlace_ref.py's frame-rate adaptive output for F[t];
              "keep": the chosen weave
  decimation  in every complete cycle (t // cycle) the output frame with the smallest peak (tests/dedup_ref.py's
              pair_peak on the whole frame row) against the output frame before it is dropped; frame 0 counts as
              infinite, ties drop the earliest, a trailing incomplete cycle is kept whole"""
import os
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref  # noqa: E402
import deinterlace_ref  # noqa: E402

ORDERS = ("tff", "bff")
CANDIDATES = ("p", "c", "n")
BLOCK_ROWS, BLOCK_COLS = 16, 64
INF = float("inf")


def default_threshold(bits):
    return 48 if bits == 10 else 12


def _read(a, bits):
    a = np.asarray(a)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    a = a.astype(np.int64)
    return np.minimum(a, 1023) if bits == 10 else a


def telecine(film, order="tff", phase=0):
    """Film frames [F, H, W] (or rows with `planes` handled by the caller) -> hard-telecined frames: film frame f gives 2
    fields (f even) or 3 (f odd), the fields alternate in parity beginning with the first field's, the first 2 * phase
    fields are dropped and the rest paired into frames (an odd field left over is dropped).  Also returns, per frame, the
    film indices (first field's, second field's)."""
    film = np.asarray(film)
    assert order in ORDERS
    k = 1 if order == "bff" else 0
    src = [f for f in range(film.shape[0]) for _ in range(2 if f % 2 == 0 else 3)][2 * phase:]
    pairs = [(src[2 * t], src[2 * t + 1]) for t in range(len(src) // 2)]
    out = np.empty((len(pairs),) + film.shape[1:], film.dtype)
    for t, (a, b) in enumerate(pairs):
        out[t, k::2] = film[a, k::2]
        out[t, 1 - k::2] = film[b, 1 - k::2]
    return out, pairs


def candidate(frames, t, which, order="tff"):
    """Candidate `which` ("p", "c", "n") of frame t of the window `frames` [N, H, W]."""
    frames = np.asarray(frames)
    k = 1 if order == "bff" else 0
    n = frames.shape[0]
    s = {"p": max(t - 1, 0), "c": t, "n": min(t + 1, n - 1)}[which]
    out = frames[t].copy()
    out[1 - k::2] = frames[s, 1 - k::2]
    return out


def comb_score(plane, threshold, bits=8):
    """The comb score of one woven plane [H, W]."""
    w = _read(plane, bits)
    h, width = w.shape
    assert h >= 3
    u, m, d = w[:-2], w[1:-1], w[2:]
    combed = (u - m) * (d - m) > threshold * threshold          # row i of this is plane row i + 1
    best = 0
    for y0 in range(0, h, BLOCK_ROWS):
        lo, hi = max(y0, 1), min(y0 + BLOCK_ROWS, h - 1)         # plane rows of the block that have both neighbours
        if lo >= hi:
            continue
        for x0 in range(0, width, BLOCK_COLS):
            best = max(best, int(combed[lo - 1:hi - 1, x0:x0 + BLOCK_COLS].sum()))
    return best


def comb_scores(frames, order="tff", threshold=None, bits=8, first=0, count=None):
    """[count, 3] int64: the scores (p, c, n) of frames first .. first + count - 1 of the window [N, H, W]."""
    frames = np.asarray(frames)
    n = frames.shape[0]
    count = n - first if count is None else count
    threshold = default_threshold(bits) if threshold is None else threshold
    out = np.zeros((count, 3), np.int64)
    for i in range(count):
        for c, which in enumerate(CANDIDATES):
            out[i, c] = comb_score(candidate(frames, first + i, which, order), threshold, bits)
    return out


def choose(scores, combed=48):
    """-> (matches: a list of "p" / "c" / "n", flags: a list of bools)."""
    matches, flags = [], []
    for sp, sc, sn in np.asarray(scores).tolist():
        if sc <= min(sp, sn):
            m, s = "c", sc
        elif sp <= sn:
            m, s = "p", sp
        else:
            m, s = "n", sn
        matches.append(m)
        flags.append(s > combed)
    return matches, flags


def plane_index(plane):
    off, h, w, pitch, step = tuple(plane)[-5:]
    return off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :] * step


def weave(rows, planes, entries, order="tff"):
    """Frame rows [N, samples] -> [len(entries), samples]: output j takes the rows of the kept parity of every plane from
    frame keep_j and the others from other_j; samples outside every plane come out 0."""
    rows = np.asarray(rows)
    k = 1 if order == "bff" else 0
    out = np.zeros((len(entries), rows.shape[1]), rows.dtype)
    for pl in planes:
        idx = plane_index(pl)
        for j, (keep, other) in enumerate(entries):
            out[j, idx[k::2]] = rows[keep][idx[k::2]]
            out[j, idx[1 - k::2]] = rows[other][idx[1 - k::2]]
    return out


def decimate_plan(peaks, cycle=5, start=0):
    """peaks[i]: the peak of clip frame start + i against the frame before it (INF for the clip's first) -> the clip
    indices kept.  Only a cycle that lies in start .. start + len(peaks) - 1 whole is complete."""
    n = len(peaks)
    kept = []
    for t in range(start, start + n):
        c0 = t // cycle * cycle
        if c0 >= start and c0 + cycle <= start + n:
            vals = [peaks[i - start] for i in range(c0, c0 + cycle)]
            if t - c0 == vals.index(min(vals)):
                continue
        kept.append(t)
    return kept


def out_rate(rate, cycle=5, decimate=True):
    f = Fraction(int(rate[0]), int(rate[1]))
    if decimate:
        f = f * (cycle - 1) / cycle
    return f.numerator, f.denominator


def ivtc(rows, planes, bits=8, order="tff", threshold=None, combed=48, fallback="deinterlace", decimate=True, cycle=5):
    """The whole pipeline on frame rows [N, samples] with planes [(name,) offset, h, w, pitch, step]; the first plane is the
    metric plane.  -> (output rows, report dict)."""
    rows = np.asarray(rows)
    n = rows.shape[0]
    metric = rows[:, plane_index(planes[0])]
    scores = comb_scores(metric, order, threshold, bits)
    matches, flags = choose(scores, combed)
    entries = [(t, {"p": max(t - 1, 0), "c": t, "n": min(t + 1, n - 1)}[m]) for t, m in enumerate(matches)]
    out = weave(rows, planes, entries, order)
    if fallback == "deinterlace":
        for t in range(n):
            if flags[t]:
                out[t] = deinterlace_ref.deinterlace_planes(rows, planes, order=order, rate="frame", method="adaptive",
                                                            first=t, count=1)[0]
    else:
        assert fallback == "keep"
    peaks = [INF] + [int(v) for v in dedup_ref.pair_peak(out, bits)] if n else []
    kept = decimate_plan(peaks, cycle) if decimate else list(range(n))
    report = {"frames_in": n, "frames_out": len(kept), "matches": {c: matches.count(c) for c in CANDIDATES},
              "combed": [t for t in range(n) if flags[t]], "dropped": sorted(set(range(n)) - set(kept))}
    return out[kept], report
