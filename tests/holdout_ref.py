"""TEST INFRASTRUCTURE ONLY: a numpy restatement of hold-out scoring - the two plane metrics with the
peak as a parameter (skimage's definitions, as oracle/metrics_oracle.py restates them at peak 255), the three methods'
predictions and the triplet sets.  At peak 1023 a 16-bit word above 1023 reads as 1023, as on the device."""
from fractions import Fraction

import numpy as np
from scipy import ndimage

WIN = 7


def peak_of(bits: int) -> int:
    return {8: 255, 10: 1023}[bits]


def samples(a: np.ndarray, peak: int) -> np.ndarray:
    """The plane as the integers the metrics see."""
    a = np.asarray(a)
    if a.dtype == np.int16:
        a = a.view(np.uint16)
    return np.minimum(a.astype(np.int64), peak)


def sse(pred, target, peak: int) -> int:
    d = samples(pred, peak) - samples(target, peak)
    return int((d * d).sum(dtype=np.int64))


def psnr_of_sse(s: int, pixels: int, peak: int) -> float:
    if s == 0:
        return float("inf")
    return float(10.0 * np.log10((float(peak) * float(peak)) / (float(s) / float(pixels))))


def psnr(pred, target, peak: int) -> float:
    return psnr_of_sse(sse(pred, target, peak), int(np.asarray(pred).size), peak)


def _constants(peak: int):
    return (0.01 * float(peak)) ** 2, (0.03 * float(peak)) ** 2


def ssim(pred, target, peak: int) -> float:
    """structural_similarity(target, pred, data_range=peak) with skimage's defaults, by uniform_filter."""
    x, y = samples(target, peak).astype(np.float64), samples(pred, peak).astype(np.float64)
    if min(x.shape) < WIN:
        raise ValueError("win_size exceeds image extent")
    n = WIN * WIN
    norm = n / (n - 1.0)
    f = lambda im: ndimage.uniform_filter(im, size=WIN)   # noqa: E731
    ux, uy = f(x), f(y)
    vx, vy, vxy = norm * (f(x * x) - ux * ux), norm * (f(y * y) - uy * uy), norm * (f(x * y) - ux * uy)
    c1, c2 = _constants(peak)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    p = WIN // 2
    return float(s[p:s.shape[0] - p, p:s.shape[1] - p].mean(dtype=np.float64))


def ssim_bruteforce(pred, target, peak: int) -> float:
    """The definition window by window in exact rationals (the constants are the doubles the other form uses); small
    images only."""
    x, y = samples(target, peak), samples(pred, peak)
    h, w = x.shape
    c1, c2 = (Fraction(c) for c in _constants(peak))
    n = WIN * WIN
    total = Fraction(0)
    for i in range(h - WIN + 1):
        for j in range(w - WIN + 1):
            a = [int(v) for v in x[i:i + WIN, j:j + WIN].ravel()]
            b = [int(v) for v in y[i:i + WIN, j:j + WIN].ravel()]
            sa, sb = sum(a), sum(b)
            ma, mb = Fraction(sa, n), Fraction(sb, n)
            va = Fraction(n * sum(v * v for v in a) - sa * sa, n * (n - 1))
            vb = Fraction(n * sum(v * v for v in b) - sb * sb, n * (n - 1))
            vab = Fraction(n * sum(p * q for p, q in zip(a, b)) - sa * sb, n * (n - 1))
            total += ((2 * ma * mb + c1) * (2 * vab + c2)) / ((ma * ma + mb * mb + c1) * (va + vb + c2))
    return float(total / ((h - WIN + 1) * (w - WIN + 1)))


# ---- triplets and methods -----------------------------------------------------------------------------------------
def targets(n_frames: int, triplets: str):
    """The held-out source frame indices, in order."""
    if triplets == "disjoint":
        return list(range(1, n_frames - 1, 2))
    if triplets == "sliding":
        return list(range(1, n_frames - 1))
    raise ValueError(triplets)


def predict(method: str, before: np.ndarray, after: np.ndarray, bits: int) -> np.ndarray:
    """"linear": the rounded integer average of every sample (10 bits: of the samples read as at most 1023);
    "repeat": the earlier neighbour as it is."""
    if method == "repeat":
        return before.copy()
    if method == "linear":
        peak = peak_of(bits)
        a, b = (samples(v, peak) if bits == 10 else v.astype(np.int64) for v in (before, after))
        return ((a + b + 1) >> 1).astype(before.dtype)
    raise ValueError(method)


def planes_of_i420(row: np.ndarray, h: int, w: int):
    """One packed 4:2:0 row -> {"y", "u", "v"} planes."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    ny, nc = h * w, hc * wc
    return {"y": row[:ny].reshape(h, w), "u": row[ny:ny + nc].reshape(hc, wc), "v": row[ny + nc:ny + 2 * nc].reshape(hc, wc)}
