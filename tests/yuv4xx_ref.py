"""numpy restatement of the 4:2:2 / 4:4:4 YUV <-> RGB conversion (csrc/yuv4xx.hip.h).

A plain helper module for the yuv4xx tests (not a conftest): the device kernels must agree with it bit for bit.  The
coefficients, the Y row and the RGB stage are `colour_ref`'s (8 bits) and `colour10_ref`'s (10 bits), taken by import;
what is restated here is the sub-sampling pattern: 4:4:4 (per pixel, n = 1) and 4:2:2 (the horizontal half of the 4:2:0
rule; chroma row y belongs to luma row y).  Planar frames are tight rows [B, F]; the two one-plane formats have pack /
unpack helpers to and from planar 4:2:2, tight or pitched."""
import numpy as np

import colour10_ref
import colour_ref

FORMATS = {"yuv422p": (8, "422"), "yuv444p": (8, "444"), "yuv422p10le": (10, "422"), "yuv444p10le": (10, "444"),
           "uyvy422": (8, "packed"), "yuyv422": (8, "packed")}


def ref_of(bits: int):
    return colour10_ref if bits == 10 else colour_ref


def _read(x, bits):
    return colour10_ref.read(x) if bits == 10 else np.asarray(x).astype(np.int64)


def _store(v, bits):
    return np.clip(v, 0, 1023).astype(np.uint16) if bits == 10 else np.clip(v, 0, 255).astype(np.uint8)


def frame_samples(fmt: str, h: int, w: int) -> int:
    kind = FORMATS[fmt][1]
    if kind == "444":
        return 3 * h * w
    if kind == "packed":
        assert w % 2 == 0
        return 2 * h * w
    return h * w + 2 * h * ((w + 1) // 2)


# ---- chroma patterns (int64 in) ----------------------------------------------------------------------------------
def chroma_sums_422(x: np.ndarray, siting: str):
    """int64 [B, 3, H, W] RGB -> ([B, 3, H, Wc] channel sums, n): jpeg columns 2j, 2j+1 (n = 2); mpeg2 [1,2,1] over
    2j-1, 2j, 2j+1 (n = 4); columns clamped into the image."""
    w = x.shape[-1]
    j = np.arange((w + 1) // 2)
    col = lambda c: np.clip(c, 0, w - 1)  # noqa: E731
    if siting == "jpeg":
        return x[..., col(2 * j)] + x[..., col(2 * j + 1)], 2
    return x[..., col(2 * j - 1)] + 2 * x[..., col(2 * j)] + x[..., col(2 * j + 1)], 4


def upsample16_422(c: np.ndarray, w: int, siting: str) -> np.ndarray:
    """int64 [B, H, Wc] chroma -> [B, H, W] chroma x16: the 4:2:0 horizontal taps times 4."""
    wc = c.shape[-1]
    xx = np.arange(w)
    j0 = xx >> 1
    if siting == "jpeg":
        j1 = np.clip(np.where(xx & 1, j0 + 1, j0 - 1), 0, wc - 1)
        return 4 * (3 * c[..., j0] + c[..., j1])
    jn = np.clip(j0 + 1, 0, wc - 1)
    return np.where(xx & 1, 8 * (c[..., j0] + c[..., jn]), 16 * c[..., j0])


def encode_c(sr, sg, sb, n: int, k: dict, bits: int):
    """Cb, Cr from channel sums over n samples (n = 1, 2 or 4), bias centre n S + n S / 2."""
    sh = 14 + n.bit_length() - 1
    centre = 512 if bits == 10 else 128
    bias = (centre << sh) + (1 << (sh - 1))
    return (_store((k["cbr"] * sr + k["cbg"] * sg + k["cbb"] * sb + bias) >> sh, bits),
            _store((k["crr"] * sr + k["crg"] * sg + k["crb"] * sb + bias) >> sh, bits))


# ---- whole frames, planar ----------------------------------------------------------------------------------------
def rgb_to_planes(rgb: np.ndarray, kind: str, bits: int, siting="mpeg2", matrix="bt709", colour_range="limited"):
    """[B, 3, H, W] RGB codes -> (Y [B,H,W], U, V [B,H,Wc]) in the sample dtype; kind "422" or "444"."""
    ref = ref_of(bits)
    k = ref.coef(matrix, colour_range)
    x = _read(rgb, bits)
    y = ref.encode_y(x[:, 0], x[:, 1], x[:, 2], k)
    if kind == "444":
        s, n = x, 1
    else:
        s, n = chroma_sums_422(x, siting)
    u, v = encode_c(s[:, 0], s[:, 1], s[:, 2], n, k, bits)
    return y, u, v


def planes_to_rgb(y, u, v, kind: str, bits: int, siting="mpeg2", matrix="bt709", colour_range="limited"):
    ref = ref_of(bits)
    k = ref.coef(matrix, colour_range)
    y, u, v = (_read(t, bits) for t in (y, u, v))
    w = y.shape[-1]
    if kind == "444":
        u16, v16 = 16 * u, 16 * v
    else:
        u16, v16 = upsample16_422(u, w, siting), upsample16_422(v, w, siting)
    r, g, b = ref.decode(y, u16, v16, k)
    return np.stack([r, g, b], axis=1)


def split_planar(frames: np.ndarray, kind: str, h: int, w: int):
    """tight planar rows [B, F] -> (Y [B,H,W], U, V [B,H,Wc]) views."""
    b = frames.shape[0]
    wc = w if kind == "444" else (w + 1) // 2
    y = frames[:, :h * w].reshape(b, h, w)
    u = frames[:, h * w:h * w + h * wc].reshape(b, h, wc)
    v = frames[:, h * w + h * wc:h * w + 2 * h * wc].reshape(b, h, wc)
    return y, u, v


def join_planar(y, u, v) -> np.ndarray:
    b = y.shape[0]
    return np.concatenate([t.reshape(b, -1) for t in (y, u, v)], axis=1)


# ---- the two one-plane formats -----------------------------------------------------------------------------------
_ORDER = {"uyvy422": (1, 3, 0, 2), "yuyv422": (0, 2, 1, 3)}   # byte of Y0, Y1, U, V in a 4-byte group


def pack422(y, u, v, fmt: str, row_pitch: int = 0, frame_stride: int = 0, fill: int = 0) -> np.ndarray:
    """planar 4:2:2 planes (uint8, W even) -> [B, frame_stride] rows of `fmt`; bytes no pixel covers hold `fill`."""
    b, h, w = y.shape
    assert w % 2 == 0
    rp = row_pitch or 2 * w
    fs = frame_stride or h * rp
    out = np.full((b, fs), fill, np.uint8)
    g = np.empty((b, h, w // 2, 4), np.uint8)
    y0, y1, iu, iv = _ORDER[fmt]
    g[..., y0], g[..., y1], g[..., iu], g[..., iv] = y[..., 0::2], y[..., 1::2], u, v
    rows = g.reshape(b, h, 2 * w)
    for r in range(h):
        out[:, r * rp:r * rp + 2 * w] = rows[:, r]
    return out


def unpack422(frames: np.ndarray, fmt: str, h: int, w: int, row_pitch: int = 0):
    """[B, frame_stride] rows of `fmt` -> planar 4:2:2 planes (Y, U, V)."""
    b = frames.shape[0]
    rp = row_pitch or 2 * w
    rows = np.stack([frames[:, r * rp:r * rp + 2 * w] for r in range(h)], axis=1)
    g = rows.reshape(b, h, w // 2, 4)
    y0, y1, iu, iv = _ORDER[fmt]
    y = np.empty((b, h, w), np.uint8)
    y[..., 0::2], y[..., 1::2] = g[..., y0], g[..., y1]
    return y, g[..., iu].copy(), g[..., iv].copy()


# ---- by format name ----------------------------------------------------------------------------------------------
def rgb_to_yuv(rgb: np.ndarray, fmt: str, siting="mpeg2", matrix="bt709", colour_range="limited", row_pitch=0,
               frame_stride=0, fill=0) -> np.ndarray:
    bits, kind = FORMATS[fmt]
    if kind == "packed":
        y, u, v = rgb_to_planes(rgb, "422", 8, siting, matrix, colour_range)
        return pack422(y, u, v, fmt, row_pitch, frame_stride, fill)
    return join_planar(*rgb_to_planes(rgb, kind, bits, siting, matrix, colour_range))


def yuv_to_rgb(frames: np.ndarray, h: int, w: int, fmt: str, siting="mpeg2", matrix="bt709", colour_range="limited",
               row_pitch=0) -> np.ndarray:
    bits, kind = FORMATS[fmt]
    if kind == "packed":
        return planes_to_rgb(*unpack422(frames, fmt, h, w, row_pitch), "422", 8, siting, matrix, colour_range)
    return planes_to_rgb(*split_planar(frames, kind, h, w), kind, bits, siting, matrix, colour_range)
