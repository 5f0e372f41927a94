"""The layout table: where the samples of one tight frame lie, stated once for every frame format the video routes,
hold-out scoring and the resize take (host only: nothing here touches the device).

`frame_layout(kind, h, w)` gives, everything in samples (bytes at 8 bits, 16-bit words at 10):

  planes   [(name, offset, h, w, row pitch, sample step)]: every sample of the frame belongs to exactly one plane
  groups   [(S, offset, h, w, row pitch, {plane name: component})]: the interleaved groups (U V of nv12, the bytes of
           packed RGB, the byte positions of uyvy422 / yuyv422), w in samples per component and row; exactly the stepped
           planes of a raw format go through a group
  bits     the sample depth, 8 or 10
  samples  the samples per frame

kind: a name of RAW_FORMATS (headerless raw video); ("y4m", tag) for a Y4M stream of colourspace `tag` ("mono",
"420jpeg", "420p10", ...: Y, then U and V of the chroma size the header parser derives); "npy" for a [H,W] frame,
("npy", C) for [H,W,C] (interleaved channels, no group).  The public size functions (`colour.yuv_frame_samples`,
`packed.frame_bytes`, `colour.i420_frame_bytes`, the Y4M header's `frame_samples`) state the frame sizes a second time
for the kernels' wrappers; tests/test_layout_host.py pins the table against them."""
from __future__ import annotations

from typing import NamedTuple

from . import colour, imageio_lite, packed

RAW_FORMATS = ("nv12",) + tuple(packed.FORMATS) + tuple(colour.YUV_FORMATS)
_PACKED_BYTES = {"rgb24": "rgb", "bgr24": "bgr", "rgba": "rgba", "bgra": "bgra"}


class Layout(NamedTuple):
    planes: list
    groups: list
    bits: int
    samples: int


def frame_samples(planes) -> int:
    """Samples of the tight frame that `planes` describe (the end of its last sample)."""
    return max(off + (h - 1) * pitch + (w - 1) * step + 1 for _, off, h, w, pitch, step in planes)


def _raw(raw: str, h: int, w: int):
    hc, wc = (h + 1) // 2, (w + 1) // 2
    if raw == "nv12":
        return ([("y", 0, h, w, w, 1), ("u", h * w, hc, wc, 2 * wc, 2), ("v", h * w + 1, hc, wc, 2 * wc, 2)],
                [(2, h * w, hc, wc, 2 * wc, {"u": 0, "v": 1})], 8)
    if raw in _PACKED_BYTES:
        order = _PACKED_BYTES[raw]
        s = len(order)
        names = "rgb" + ("a" if s == 4 else "")
        return ([(c, order.index(c), h, w, s * w, s) for c in names],
                [(s, 0, h, w, s * w, {c: order.index(c) for c in names})], 8)
    _, bits, kind = colour.YUV_FORMATS[raw]
    if kind == "packed":
        colour.yuv_frame_samples(raw, h, w)   # (refuses an odd width)
        y, u, v = (1, 0, 2) if raw == "uyvy422" else (0, 1, 3)
        return ([("y", y, h, w, 2 * w, 2), ("u", u, h, w // 2, 2 * w, 4), ("v", v, h, w // 2, 2 * w, 4)],
                [(2, 0, h, w, 2 * w, {"y": y}), (4, 0, h, w // 2, 2 * w, {"u": u, "v": v})], bits)
    cw = w if kind == "444" else wc
    return [("y", 0, h, w, w, 1), ("u", h * w, h, cw, cw, 1), ("v", h * w + h * cw, h, cw, cw, 1)], [], bits


def frame_layout(kind, h: int, w: int) -> Layout:
    """The `Layout` of one tight h x w frame of `kind` (the module's head).  ValueError for a non-positive size, an
    unknown kind, and an odd width of uyvy422 / yuyv422."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"a frame's height and width must be positive, got {h} x {w}")
    groups, bits = [], 8
    if kind == "npy":
        planes = [("gray", 0, h, w, w, 1)]
    elif isinstance(kind, tuple) and len(kind) == 2 and kind[0] == "npy":
        c = int(kind[1])
        if c < 1:
            raise ValueError(f"an [H,W,C] frame has at least one channel, got {kind[1]!r}")
        planes = [(f"c{i}", i, h, w, c * w, c) for i in range(c)]
    elif isinstance(kind, tuple) and len(kind) == 2 and kind[0] == "y4m":
        tag = str(kind[1])
        bits = 10 if tag in imageio_lite.Y4M_P10_TAGS else 8
        hdr = imageio_lite._y4m_stream_header(imageio_lite._y4m_header_line(w, h, (30, 1), tag, None, bits), bits)
        hc, wc = hdr["chroma"]
        planes = [("y", 0, h, w, w, 1)]
        if hc * wc:
            planes += [("u", h * w, hc, wc, wc, 1), ("v", h * w + hc * wc, hc, wc, wc, 1)]
    elif isinstance(kind, str):
        if kind not in RAW_FORMATS:
            raise ValueError(f"raw must be one of {list(RAW_FORMATS)}, got {kind!r}")
        planes, groups, bits = _raw(kind, h, w)
    else:
        raise ValueError(f"unknown frame kind {kind!r}")
    return Layout(planes, groups, bits, frame_samples(planes))


__all__ = ["RAW_FORMATS", "Layout", "frame_layout", "frame_samples"]
