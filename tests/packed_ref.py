"""Plain numpy restatement of the packed RGB conversions, for the packed tests.

Index shuffles between packed frames (a pixel = 3 or 4 consecutive bytes, rows a pitch apart) and planar RGB
[B, 3, H, W], and the one piece of arithmetic there is: the rounded average of two alpha bytes.  Nothing here touches the
library.  Layouts are (row_pitch, frame_stride) in bytes, both set (`tight(fmt, h, w)` gives the tight one)."""
import numpy as np

BPP = {"rgb24": 3, "bgr24": 3, "rgba": 4, "bgra": 4}
# byte position of R, G, B inside a pixel
ORDER = {"rgb24": (0, 1, 2), "bgr24": (2, 1, 0), "rgba": (0, 1, 2), "bgra": (2, 1, 0)}


def tight(fmt, h, w):
    return (w * BPP[fmt], h * w * BPP[fmt])


def pixels(frames, fmt, h, w, layout=None):
    """[B, frame_stride] uint8 frames -> their pixels [B, H, W, bpp]."""
    bpp = BPP[fmt]
    rp, fs = layout or tight(fmt, h, w)
    b = frames.shape[0]
    assert frames.dtype == np.uint8 and frames.shape == (b, fs)
    rows = np.stack([frames[:, y * rp:y * rp + w * bpp] for y in range(h)], axis=1)
    return rows.reshape(b, h, w, bpp)


def unpack(frames, fmt, h, w, layout=None):
    """-> (planar RGB [B, 3, H, W], the alpha plane [B, H, W] or None)"""
    px = pixels(frames, fmt, h, w, layout)
    rgb = np.stack([px[..., k] for k in ORDER[fmt]], axis=1)
    return np.ascontiguousarray(rgb), (np.ascontiguousarray(px[..., 3]) if BPP[fmt] == 4 else None)


def alpha_average(a1, a2):
    return ((a1.astype(np.uint16) + a2.astype(np.uint16) + 1) >> 1).astype(np.uint8)


def pack(rgb, fmt, layout=None, alpha=None, fill=0):
    """Planar RGB [B, 3, H, W] -> [B, frame_stride] frames; alpha: the plane [B, H, W] a 4-byte format carries (None:
    255); every byte no pixel covers is `fill`."""
    b, _, h, w = rgb.shape
    bpp = BPP[fmt]
    rp, fs = layout or tight(fmt, h, w)
    px = np.empty((b, h, w, bpp), np.uint8)
    for ch, k in enumerate(ORDER[fmt]):
        px[..., k] = rgb[:, ch]
    if bpp == 4:
        px[..., 3] = 255 if alpha is None else alpha
    out = np.full((b, fs), fill, np.uint8)
    for y in range(h):
        out[:, y * rp:y * rp + w * bpp] = px[:, y].reshape(b, w * bpp)
    return out


def used_mask(fmt, h, w, layout):
    rp, fs = layout
    m = np.zeros(fs, bool)
    for y in range(h):
        m[y * rp:y * rp + w * BPP[fmt]] = True
    return m
