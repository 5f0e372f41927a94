"""The deinterlacer's definition in numpy (include/fiunet.h): the home of the definition.  The kernels of
csrc/deinterlace.hip.h equal it bit for bit (tests/test_gpu_deinterlace.py); tests/test_deinterlace_host.py holds it to
hand-computed samples and to what a deinterlacer is for.  It is the project's own, in the spirit of yadif, and NOT pinned
against ffmpeg.

A clip is an integer array [N, H, W] of one plane, H >= 2.  Everything is int32 arithmetic on the samples as they are (no
masking: a result lies between the smallest and the largest input), and every `>>` acts on a non-negative value."""
import numpy as np

ORDERS = ("tff", "bff")
RATES = ("field", "frame")
METHODS = ("adaptive", "bob")


def interlace(progressive, order="tff"):
    """A field-rate progressive clip [2N, H, W] -> N interlaced frames: frame t takes the rows of the first field's
    parity from progressive frame 2t and the others from 2t + 1."""
    prog = np.asarray(progressive)
    assert prog.ndim == 3 and prog.shape[0] % 2 == 0 and order in ORDERS
    p = 1 if order == "bff" else 0
    out = np.empty((prog.shape[0] // 2,) + prog.shape[1:], prog.dtype)
    out[:, p::2] = prog[0::2, p::2]
    out[:, 1 - p::2] = prog[1::2, 1 - p::2]
    return out


def _shift(a, j):
    """a[:, x + j] where that column exists, 0 elsewhere (the direction search reads inside the plane only)."""
    out = np.zeros_like(a)
    w = a.shape[1]
    lo, hi = max(0, -j), min(w, w - j)
    if lo < hi:
        out[:, lo:hi] = a[:, lo + j:hi + j]
    return out


def missing_rows(prev, cur, nxt, i, rows, method="adaptive", spatial_check=True):
    """The samples of rows `rows` (an int array) of field `i` of `cur` [H, W] between `prev` and `nxt`, as [len(rows), W]
    int32: section 1 of the definition, sample for sample."""
    prev, cur, nxt = (np.asarray(a).astype(np.int32) for a in (prev, cur, nxt))
    h, w = cur.shape
    y = np.asarray(rows, dtype=np.int64)
    ym = np.where(y == 0, y + 1, y - 1)
    yp = np.where(y == h - 1, y - 1, y + 1)
    c, e = cur[ym], cur[yp]
    pred = (c + e) >> 1
    if method == "bob":
        return pred
    assert method == "adaptive"
    prev2, next2 = (prev, cur) if i == 0 else (cur, nxt)
    d = (prev2[y] + next2[y]) >> 1
    t0 = np.abs(prev2[y] - next2[y])
    t1 = (np.abs(prev[ym] - c) + np.abs(prev[yp] - e)) >> 1
    t2 = (np.abs(nxt[ym] - c) + np.abs(nxt[yp] - e)) >> 1
    diff = np.maximum(t0 >> 1, np.maximum(t1, t2))

    def S(j):
        return sum(np.abs(_shift(c, k + j) - _shift(e, k - j)) for k in (-1, 0, 1))

    x = np.arange(w)[None, :]
    inside = (x >= 3) & (x < w - 3)
    score = S(0) - 1
    for sign in (-1, 1):
        s1 = S(sign)
        take1 = inside & (s1 < score)
        score = np.where(take1, s1, score)
        pred = np.where(take1, (_shift(c, sign) + _shift(e, -sign)) >> 1, pred)
        s2 = S(2 * sign)
        take2 = take1 & (s2 < score)
        score = np.where(take2, s2, score)
        pred = np.where(take2, (_shift(c, 2 * sign) + _shift(e, -2 * sign)) >> 1, pred)
    if spatial_check:
        ok = (y - 2 >= 0) & (y + 2 < h)
        y0, y1 = np.where(ok, y - 2, y), np.where(ok, y + 2, y)
        b = (prev2[y0] + next2[y0]) >> 1
        f = (prev2[y1] + next2[y1]) >> 1
        mx = np.maximum(np.maximum(d - e, d - c), np.minimum(b - c, f - e))
        mn = np.minimum(np.minimum(d - e, d - c), np.maximum(b - c, f - e))
        diff = np.where(ok[:, None], np.maximum(diff, np.maximum(mn, -mx)), diff)
    return np.minimum(np.maximum(pred, d - diff), d + diff)


def deinterlace(frames, order="tff", rate="field", method="adaptive", spatial_check=True, first=0, count=None):
    """frames [N, H, W] (a window) -> the deinterlaced frames first .. first + count - 1 (default: to the end), in the
    dtype of `frames`: 2 * count frames at rate "field" (frame 2k + i from field i of frame first + k), count at rate
    "frame" (field 0).  Neighbours outside the window clamp to its ends."""
    frames = np.asarray(frames)
    assert frames.ndim == 3 and frames.shape[1] >= 2, frames.shape
    assert order in ORDERS and rate in RATES and method in METHODS
    n, h, _ = frames.shape
    count = n - first if count is None else count
    assert 0 <= first and 0 <= count and first + count <= n
    fields = (0, 1) if rate == "field" else (0,)
    out = np.empty((count * len(fields),) + frames.shape[1:], frames.dtype)
    for k in range(count):
        t = first + k
        prev, cur, nxt = frames[max(t - 1, 0)], frames[t], frames[min(t + 1, n - 1)]
        for i in fields:
            p = (1 if order == "bff" else 0) ^ i
            o = out[k * len(fields) + i]
            o[p::2] = cur[p::2]
            rows = np.arange(1 - p, h, 2)
            o[1 - p::2] = missing_rows(prev, cur, nxt, i, rows, method, spatial_check).astype(frames.dtype)
    return out


def deinterlace_planes(rows, planes, **kw):
    """`deinterlace` on frame rows [N, samples] plane by plane: planes are (name, offset, h, w, pitch, step) or
    (offset, h, w, pitch, step) in samples of a row, as `layout.frame_layout` gives them.  Samples outside every plane
    come out 0."""
    rows = np.asarray(rows)
    n = rows.shape[0]
    out = None
    for pl in planes:
        off, h, w, pitch, step = tuple(pl)[-5:]
        idx = off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :] * step
        res = deinterlace(rows[:, idx], **kw)
        if out is None:
            out = np.zeros((res.shape[0], rows.shape[1]), rows.dtype)
        out[:, idx] = res
    return out
