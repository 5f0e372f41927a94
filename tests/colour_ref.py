"""numpy restatement of the integer YUV 4:2:0 <-> RGB conversion of csrc/colour.hip.h (DESIGN.md "Colour video").

A plain helper module for the colour tests (not a conftest): the device kernels must agree with it bit for bit, and
it is checked against the float64 textbook BT.601 / BT.709 formulas.  Frames are packed I420 rows [B, F]."""
import math

import numpy as np

S = 1 << 14
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def _rnd(x: float) -> int:
    return int(math.floor(x * 16384.0 + 0.5))


def coef(matrix: str = "bt709", colour_range: str = "limited") -> dict:
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    full = colour_range == "full"
    ys = 1.0 if full else 219.0 / 255.0
    cs = 1.0 if full else 224.0 / 255.0
    k = dict(yr=_rnd(kr * ys), yb=_rnd(kb * ys), yoff=0 if full else 16)
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


def frame_bytes(h: int, w: int) -> int:
    return h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)


def _u8(v):
    return np.clip(v, 0, 255).astype(np.uint8)


# ---- per-sample pieces (int64 numpy arrays in, uint8 out) -------------------------------------------------------
def encode_y(r, g, b, k):
    return _u8((k["yr"] * r + k["yg"] * g + k["yb"] * b + k["yoff"] * S + S // 2) >> 14)


def encode_c(sr, sg, sb, n, k):
    """Cb, Cr from channel sums over n samples (n = 4: jpeg, 8: mpeg2)."""
    sh = 14 + n.bit_length() - 1
    bias = (128 << sh) + (1 << (sh - 1))
    return (_u8((k["cbr"] * sr + k["cbg"] * sg + k["cbb"] * sb + bias) >> sh),
            _u8((k["crr"] * sr + k["crg"] * sg + k["crb"] * sb + bias) >> sh))


def decode(y, u16, v16, k):
    """RGB from Y and chroma x16 (up-sampled, not rounded)."""
    yy = 16 * k["dy"] * (y - k["yoff"]) + (1 << 17)
    u, v = u16 - 2048, v16 - 2048
    return (_u8((yy + k["dcr"] * v) >> 18), _u8((yy + k["dgb"] * u + k["dgr"] * v) >> 18),
            _u8((yy + k["dcb"] * u) >> 18))


# ---- whole frames ------------------------------------------------------------------------------------------------
def rgb_to_yuv420(rgb: np.ndarray, siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited"):
    """uint8 [B, 3, H, W] -> uint8 [B, F] packed I420."""
    k = coef(matrix, colour_range)
    b, _, h, w = rgb.shape
    hc, wc = (h + 1) // 2, (w + 1) // 2
    x = rgb.astype(np.int64)
    y = encode_y(x[:, 0], x[:, 1], x[:, 2], k)
    rows = np.minimum(np.arange(2 * hc), h - 1)
    xr = x[:, :, rows]
    vsum = xr[:, :, 0::2] + xr[:, :, 1::2]                         # [B, 3, Hc, W]: rows 2i, 2i+1 (replicated)
    j = np.arange(wc)
    col = lambda c: np.clip(c, 0, w - 1)  # noqa: E731
    if siting == "jpeg":
        s, n = vsum[..., col(2 * j)] + vsum[..., col(2 * j + 1)], 4
    else:
        s, n = vsum[..., col(2 * j - 1)] + 2 * vsum[..., col(2 * j)] + vsum[..., col(2 * j + 1)], 8
    cb, cr = encode_c(s[:, 0], s[:, 1], s[:, 2], n, k)
    return np.concatenate([y.reshape(b, -1), cb.reshape(b, -1), cr.reshape(b, -1)], axis=1)


def upsample16(c: np.ndarray, h: int, w: int, siting: str) -> np.ndarray:
    """int64 [B, Hc, Wc] chroma -> [B, H, W] chroma x16."""
    hc, wc = c.shape[-2:]
    yy = np.arange(h)
    i0 = yy >> 1
    i1 = np.clip(np.where(yy & 1, i0 + 1, i0 - 1), 0, hc - 1)
    v = 3 * c[:, i0] + c[:, i1]                                    # x4, [B, H, Wc]
    xx = np.arange(w)
    j0 = xx >> 1
    if siting == "jpeg":
        j1 = np.clip(np.where(xx & 1, j0 + 1, j0 - 1), 0, wc - 1)
        return 3 * v[..., j0] + v[..., j1]
    jn = np.clip(j0 + 1, 0, wc - 1)
    return np.where(xx & 1, 2 * (v[..., j0] + v[..., jn]), 4 * v[..., j0])


def yuv420_to_rgb(frames: np.ndarray, h: int, w: int, siting: str = "jpeg", matrix: str = "bt709",
                  colour_range: str = "limited"):
    """uint8 [B, F] packed I420 -> uint8 [B, 3, H, W]."""
    k = coef(matrix, colour_range)
    b = frames.shape[0]
    hc, wc = (h + 1) // 2, (w + 1) // 2
    f = frames.astype(np.int64)
    y = f[:, :h * w].reshape(b, h, w)
    u = f[:, h * w:h * w + hc * wc].reshape(b, hc, wc)
    v = f[:, h * w + hc * wc:h * w + 2 * hc * wc].reshape(b, hc, wc)
    r, g, bl = decode(y, upsample16(u, h, w, siting), upsample16(v, h, w, siting), k)
    return np.stack([r, g, bl], axis=1)


# ---- float64 textbook formulas (E' in [0, 1] from RGB codes / 255) -------------------------------------------------
def textbook_encode(r, g, b, matrix="bt709", colour_range="limited"):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    r, g, b = (np.asarray(t, np.float64) / 255.0 for t in (r, g, b))
    ey = kr * r + kg * g + kb * b
    pb, pr = (b - ey) / (2 * (1 - kb)), (r - ey) / (2 * (1 - kr))
    if colour_range == "full":
        return 255.0 * ey, 128.0 + 255.0 * pb, 128.0 + 255.0 * pr
    return 16.0 + 219.0 * ey, 128.0 + 224.0 * pb, 128.0 + 224.0 * pr


def textbook_decode(y, cb, cr, matrix="bt709", colour_range="limited"):
    kr, kb = KR_KB[matrix]
    kg = 1.0 - kr - kb
    y, cb, cr = (np.asarray(t, np.float64) for t in (y, cb, cr))
    if colour_range == "full":
        ey, pb, pr = y / 255.0, (cb - 128.0) / 255.0, (cr - 128.0) / 255.0
    else:
        ey, pb, pr = (y - 16.0) / 219.0, (cb - 128.0) / 224.0, (cr - 128.0) / 224.0
    r = ey + 2 * (1 - kr) * pr
    b = ey + 2 * (1 - kb) * pb
    g = (ey - kr * r - kb * b) / kg
    return 255.0 * r, 255.0 * g, 255.0 * b
