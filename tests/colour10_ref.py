"""numpy restatement of the 10-bit YUV 4:2:0 <-> RGB conversion (csrc/colour.hip.h on uint16 samples)
and of pre10 / post10 (csrc/pointwise.hip.h).

A plain helper module for the 10-bit tests (not a conftest): the device kernels must agree with it bit for bit, and
it is checked against the float64 textbook BT.601 / BT.709 / BT.2020 formulas.  Frames are packed 4:2:0 rows [B, F] of
10-bit codes; inputs above 1023 are read as 1023."""
import math

import numpy as np

from colour_ref import upsample16   # the chroma up-sampling is the same integer rule at every depth

S = 1 << 14
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
MAX, CENTRE = 1023, 512


def _rnd(x: float) -> int:
    return int(math.floor(x * 16384.0 + 0.5))


def coef(matrix: str = "bt709", colour_range: str = "limited") -> dict:
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    full = colour_range == "full"
    ys = 1.0 if full else 876.0 / 1023.0
    cs = 1.0 if full else 896.0 / 1023.0
    k = dict(yr=_rnd(kr * ys), yb=_rnd(kb * ys), yoff=0 if full else 64)
    k["yg"] = _rnd(ys) - k["yr"] - k["yb"]
    k["cbr"], k["cbb"] = _rnd(-kr / (2.0 * (1.0 - kb)) * cs), _rnd(0.5 * cs)
    k["cbg"] = -k["cbr"] - k["cbb"]
    k["crr"], k["crb"] = _rnd(0.5 * cs), _rnd(-kb / (2.0 * (1.0 - kr)) * cs)
    k["crg"] = -k["crr"] - k["crb"]
    k["dy"] = _rnd(1.0 / ys)
    k["dcr"] = _rnd(2.0 * (1.0 - kr) / cs)
    k["dcb"] = _rnd(2.0 * (1.0 - kb) / cs)
    k["dgb"] = _rnd(-2.0 * kb * (1.0 - kb) / kg / cs)
    k["dgr"] = _rnd(-2.0 * kr * (1.0 - kr) / kg / cs)
    return k


def frame_samples(h: int, w: int) -> int:
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def _p10(v):
    return np.clip(v, 0, MAX).astype(np.uint16)


def read(x):
    """How the kernels take an input sample: int64, above 1023 read as 1023."""
    return np.minimum(np.asarray(x).astype(np.int64), MAX)


# ---- per-sample pieces (int64 numpy arrays in, uint16 out) ------------------------------------------------------
def encode_y(r, g, b, k):
    return _p10((k["yr"] * r + k["yg"] * g + k["yb"] * b + k["yoff"] * S + S // 2) >> 14)


def encode_c(sr, sg, sb, n, k):
    """Cb, Cr from channel sums over n samples (n = 4: jpeg, 8: mpeg2)."""
    sh = 14 + n.bit_length() - 1
    bias = (CENTRE << sh) + (1 << (sh - 1))
    return (_p10((k["cbr"] * sr + k["cbg"] * sg + k["cbb"] * sb + bias) >> sh),
            _p10((k["crr"] * sr + k["crg"] * sg + k["crb"] * sb + bias) >> sh))


def decode_terms(y, u16, v16, k):
    """The int32 intermediates of the decode (before the shift): R, G, B."""
    yy = 16 * k["dy"] * (y - k["yoff"]) + (1 << 17)
    u, v = u16 - 16 * CENTRE, v16 - 16 * CENTRE
    return yy + k["dcr"] * v, yy + k["dgb"] * u + k["dgr"] * v, yy + k["dcb"] * u


def decode(y, u16, v16, k):
    """RGB from Y and chroma x16 (up-sampled, not rounded)."""
    return tuple(_p10(t >> 18) for t in decode_terms(y, u16, v16, k))


# ---- whole frames ------------------------------------------------------------------------------------------------
def rgb_to_yuv420p10(rgb: np.ndarray, siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited"):
    """uint16 [B, 3, H, W] -> uint16 [B, F] packed 4:2:0."""
    k = coef(matrix, colour_range)
    b, _, h, w = rgb.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    x = read(rgb)
    y = encode_y(x[:, 0], x[:, 1], x[:, 2], k)
    rows = np.minimum(np.arange(2 * hc), h - 1)
    xr = x[:, :, rows]
    vsum = xr[:, :, 0::2] + xr[:, :, 1::2]
    j = np.arange(wc)
    col = lambda c: np.clip(c, 0, w - 1)  # noqa: E731
    if siting == "jpeg":
        s, n = vsum[..., col(2 * j)] + vsum[..., col(2 * j + 1)], 4
    else:
        s, n = vsum[..., col(2 * j - 1)] + 2 * vsum[..., col(2 * j)] + vsum[..., col(2 * j + 1)], 8
    cb, cr = encode_c(s[:, 0], s[:, 1], s[:, 2], n, k)
    return np.concatenate([y.reshape(b, -1), cb.reshape(b, -1), cr.reshape(b, -1)], axis=1)


def yuv420p10_to_rgb(frames: np.ndarray, h: int, w: int, siting: str = "jpeg", matrix: str = "bt709",
                     colour_range: str = "limited"):
    """uint16 [B, F] packed 4:2:0 -> uint16 [B, 3, H, W]."""
    k = coef(matrix, colour_range)
    b = frames.shape[0]
    hc, wc = (h + 1) // 2, (w + 1) // 2
    f = read(frames)
    y = f[:, :h * w].reshape(b, h, w)
    u = f[:, h * w:h * w + hc * wc].reshape(b, hc, wc)
    v = f[:, h * w + hc * wc:h * w + 2 * hc * wc].reshape(b, hc, wc)
    r, g, bl = decode(y, upsample16(u, h, w, siting), upsample16(v, h, w, siting), k)
    return np.stack([r, g, bl], axis=1)


# ---- pre10 / post10 (fp32 numpy: IEEE division, the ops in the kernels' order) ------------------------------------
def pre10(x) -> np.ndarray:
    q = read(x).astype(np.float32) / np.float32(1023.0)
    return (np.float32(2.0) * q - np.float32(1.0)).astype(np.float32)


def post10(t) -> np.ndarray:
    t = np.asarray(t, np.float32)
    v = np.clip((t + np.float32(1.0)) / np.float32(2.0), np.float32(0.0), np.float32(1.0))
    v = np.where(np.isnan(v), np.float32(0.0), v)   # fminf(fmaxf(NaN, 0), 1) = 0
    return (v * np.float32(1023.0)).astype(np.uint16)


# ---- float64 textbook formulas (E' in [0, 1] from RGB codes / 1023) ------------------------------------------------
def textbook_encode(r, g, b, matrix="bt709", colour_range="limited"):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    r, g, b = (np.asarray(t, np.float64) / 1023.0 for t in (r, g, b))
    ey = kr * r + kg * g + kb * b
    pb, pr = (b - ey) / (2 * (1 - kb)), (r - ey) / (2 * (1 - kr))
    if colour_range == "full":
        return 1023.0 * ey, 512.0 + 1023.0 * pb, 512.0 + 1023.0 * pr
    return 64.0 + 876.0 * ey, 512.0 + 896.0 * pb, 512.0 + 896.0 * pr


def textbook_decode(y, cb, cr, matrix="bt709", colour_range="limited"):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y, cb, cr = (np.asarray(t, np.float64) for t in (y, cb, cr))
    if colour_range == "full":
        ey, pb, pr = y / 1023.0, (cb - 512.0) / 1023.0, (cr - 512.0) / 1023.0
    else:
        ey, pb, pr = (y - 64.0) / 876.0, (cb - 512.0) / 896.0, (cr - 512.0) / 896.0
    r = ey + 2 * (1 - kr) * pr
    b = ey + 2 * (1 - kb) * pb
    g = (ey - kr * r - kb * b) / kg
    return 1023.0 * r, 1023.0 * g, 1023.0 * b
