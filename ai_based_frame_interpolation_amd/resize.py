"""Resize frames on the device (csrc/resize.hip.h): the bilinear filter of `cv2.resize(...,
INTER_LINEAR)` that every entry point of the reference puts in front of the network, as one HIP kernel over plane
descriptors, and an area filter for alias-free down-scaling as a second kernel over the same descriptors.

  definition  8 bits: `imageio_lite.resize_linear_u8` to the last bit (half-pixel centres, the coordinate in fp64 rounded
              to fp32, 11-bit coefficients, OpenCV's two-stage vertical rounding).  That function is the project's
              statement of OpenCV's uchar path; OpenCV is not installed where this is tested, so neither it nor the
              kernel is pinned against OpenCV itself.  10 bits: the same taps in integers, out = min((b0 * S0 + b1 * S1
              + 2^21) >> 22, 1023) with samples above 1023 read as 1023 (OpenCV's ushort path is float arithmetic, whose
              bits hang on summation order).  A destination of the source's size is a copy, sample for sample.
              tests/resize_ref.py restates all of it in numpy.
  planes      a plane is (name, offset, h, w, row pitch, sample step) in samples of one tight frame, what the layout
              table (layout.py) gives for every frame kind: raw video, Y4M and .npy; `frame_planes` forwards to it.  Every
              plane of the source format is resampled on its own grid into the same plane of the destination format;
              chroma planes get the size the format gives at the destination size.
  aliasing    the linear filter reads two samples per axis whatever the scale: a large down-scale aliases, as it does in
              the reference.
  area        `filter="area"`: every destination sample is the mean of the source area it covers.  Per axis, in units of
              1 / n_dst of a source sample, destination d covers [d * n_src, (d + 1) * n_src) and source j covers
              [j * n_dst, (j + 1) * n_dst); the weight is the overlap length.  Per plane N = sum wy * wx * v, D = sw * sh,
              out = (N + D // 2) // D: integers only, exact, the same at 8 and 10 bits (samples above 1023 read as 1023).
              `imageio_lite.resize_area` states it in numpy, tests/resize_area_ref.py by brute force.  It only
              down-scales (a plane pair that grows on either axis is a ValueError: use "linear") and covers ratios up
              to 64 on either axis.  Not pinned against OpenCV's INTER_AREA, whose fractional path is float.

Out of scope: cubic / Lanczos filters, an automatic choice of filter, area on up-scales, siting-aware chroma resampling,
resizing the result back, pitched decoder surfaces in `resize_frames` (tight frames only; `resize_planes` takes
pitches)."""
from __future__ import annotations

import numbers
import re

import torch

from . import _native, imageio_lite
from .layout import frame_layout, frame_samples

MAX_PLANES = 4   # csrc/resize.hip.h kResizeMaxPlanes: plane pairs per launch
FILTERS = {"linear": _native.RESIZE_LINEAR, "area": _native.RESIZE_AREA}


def check_filter(filter) -> str:
    """"linear" or "area" -> the same name.  Everything else is a ValueError."""
    if not isinstance(filter, str) or filter not in FILTERS:
        raise ValueError(f"resize filter must be one of {sorted(FILTERS)}, got {filter!r}")
    return filter


def check_resize_filter(resize, resize_filter) -> str:
    """The `resize_filter` of a route beside its `resize`: a name `check_filter` accepts, and "linear" (the default)
    where nothing is resized."""
    name = check_filter(resize_filter)
    if resize is None and name != "linear":
        raise ValueError(f"resize_filter={name!r} needs resize: without it nothing is resized")
    return name


def check_filter_planes(filter: str, src_planes, dst_planes) -> None:
    """The area filter's refusals for every plane pair ((..., h, w, pitch, step) tuples), before any device work."""
    if check_filter(filter) == "area":
        for s, d in zip(src_planes, dst_planes):
            imageio_lite.check_area(s[-4], s[-3], d[-4], d[-3], imageio_lite.AREA_MAX_RATIO)


def check_size(size):
    """(width, height) as positive ints, or a "WxH" string -> (width, height).  Everything else is a ValueError."""
    if isinstance(size, str):
        m = re.fullmatch(r"\s*([0-9]+)\s*[xX]\s*([0-9]+)\s*", size)
        if not m:
            raise ValueError(f"size must be (width, height) or 'WxH', got {size!r}")
        size = (int(m.group(1)), int(m.group(2)))
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f"size must be (width, height) or 'WxH', got {size!r}") from None
    for v in (w, h):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"size must be (width, height) as positive ints or 'WxH', got {size!r}")
    return int(w), int(h)


def _bits_of(t: torch.Tensor) -> int:
    if t.dtype == torch.uint8:
        return 8
    if t.dtype in (torch.uint16, torch.int16):
        return 10
    raise ValueError(f"expected uint8 samples or 16-bit words of 10-bit codes, got {t.dtype}")


def y4m_header_at(hdr: dict, size) -> dict:
    """The header fields of a Y4M stream `hdr` (imageio_lite.Y4MReader.header) at another (width, height): the same tag,
    rate and range; chroma size and frame size as the tag gives them at the new size."""
    w, h = check_size(size)
    line = imageio_lite._y4m_header_line(w, h, hdr["fps"], hdr["colourspace"], hdr["colour_range"], hdr["bits"])
    return imageio_lite._y4m_stream_header(line, hdr["bits"])


def frame_planes(kind, h: int, w: int):
    """The planes [(name, offset, h, w, row pitch, sample step)] of one tight h x w frame of `kind`, in samples: the
    layout table's (`layout.frame_layout`, which names the kinds)."""
    return [tuple(p) for p in frame_layout(kind, h, w).planes]


def _launch(src, src_planes, dst, dst_planes, n: int, bits: int, stream=None, filter: str = "linear") -> None:
    for i in range(0, len(src_planes), MAX_PLANES):
        _native.resize_planes(src, src_planes[i:i + MAX_PLANES], dst, dst_planes[i:i + MAX_PLANES], n, bits, stream,
                              filter=FILTERS[filter])


def resize_frames(rows: torch.Tensor, src_planes, dst_planes, bits: int, out: torch.Tensor | None = None,
                  stream=None, filter: str = "linear") -> torch.Tensor:
    """Device rows [k, row_src] of tight frames -> [k, row_dst]: plane i of `src_planes` of every frame is resampled on
    its own grid into plane i of `dst_planes` (both as `frame_planes` gives them, for the same format at the two sizes),
    the alpha plane of rgba / bgra like any other.  Chroma planes are resampled as planes of their own size: where the
    chroma samples sit against the luma grid (the siting) is not modelled.  bits: 8 (uint8 rows) or 10 (16-bit words).
    filter: "linear" or "area" (the module's head; area refuses a plane pair that grows, and ratios above 64).
    out: a contiguous [k, row_dst] tensor of the rows' dtype to write into (else a new one).  On the rows' current
    stream (or the raw handle `stream`), without allocation when `out` is given and without synchronisation."""
    if rows.dim() != 2 or not rows.is_contiguous():
        raise ValueError("rows must be a contiguous [k, row] tensor of tight frames")
    if _bits_of(rows) != bits:
        raise ValueError(f"bits={bits!r} does not match rows of {rows.dtype}")
    if len(src_planes) != len(dst_planes) or not src_planes:
        raise ValueError(f"{len(src_planes)} source planes for {len(dst_planes)} destination planes")
    check_filter_planes(filter, [tuple(p[-5:]) for p in src_planes], [tuple(p[-5:]) for p in dst_planes])
    k, row_src = rows.shape
    if frame_samples(src_planes) > row_src:
        raise ValueError(f"the source planes describe a frame of {frame_samples(src_planes)} samples, the rows have {row_src}")
    row_dst = frame_samples(dst_planes)
    if out is None:
        out = torch.empty((k, row_dst), dtype=rows.dtype, device=rows.device)
    elif out.shape != (k, row_dst) or out.dtype != rows.dtype or not out.is_contiguous() or out.device != rows.device:
        raise ValueError(f"out must be a contiguous [{k}, {row_dst}] {rows.dtype} tensor on the rows' device")
    if k:
        _launch(rows, [tuple(p[-5:]) + (row_src,) for p in src_planes], out,
                [tuple(p[-5:]) + (row_dst,) for p in dst_planes], k, bits, stream, filter)
    return out


def resize_planes(t: torch.Tensor, size, stream=None, filter: str = "linear") -> torch.Tensor:
    """A device uint8 (8-bit) or uint16 / int16 (10-bit codes) tensor [N, C, H, W] or [N, H, W], contiguous or with a row
    pitch (stride 1 along W; any non-overlapping strides elsewhere) -> a new contiguous [N, C, H', W'] (or [N, H', W'])
    for size = (width, height), as `inference.preprocess_image` and cv2 take it.  filter: "linear" or "area"."""
    tw, th = check_size(size)
    check_filter(filter)
    bits = _bits_of(t)
    if t.dim() not in (3, 4):
        raise ValueError(f"expected [N, C, H, W] or [N, H, W], got {tuple(t.shape)}")
    v = t if t.dim() == 4 else t.unsqueeze(1)
    n, c, h, w = v.shape
    if h < 1 or w < 1:
        raise ValueError(f"expected planes of at least one sample, got {tuple(t.shape)}")
    if filter == "area":
        imageio_lite.check_area(h, w, th, tw, imageio_lite.AREA_MAX_RATIO)
    out = torch.empty((n, c, th, tw), dtype=t.dtype, device=t.device)
    if n and c:
        sn, sc, sh, sw = v.stride()
        body = (h - 1) * sh + w
        # one plane per channel, frames sn apart: needs rows inside the pitch, planes inside the frame stride
        if sw != 1 or sh < w or (c > 1 and sc < body) or (n > 1 and sn < (c - 1) * sc + body):
            v = v.contiguous()
            sn, sc, sh, sw = v.stride()
            body = (h - 1) * sh + w
        fs = max(sn, (c - 1) * sc + body)   # (n == 1: any stride will do)
        flat = v.as_strided(((n - 1) * fs + (c - 1) * sc + body,), (1,), v.storage_offset())
        _launch(flat, [(i * sc, h, w, sh, 1, fs) for i in range(c)], out.view(-1),
                [(i * th * tw, th, tw, tw, 1, c * th * tw) for i in range(c)], n, bits, stream, filter)
    return out if t.dim() == 4 else out[:, 0]


class FrameResize:
    """What a video route needs to resize its chunks: the source planes and row (what the reader and the input ring
    hold) and the destination planes and row (what everything after it sees), and the filter ("linear" or "area":
    the area filter's refusals for these planes are raised here)."""

    def __init__(self, src_planes, dst_planes, bits: int, size, source_size, filter: str = "linear"):
        self.src_planes, self.dst_planes, self.bits = list(src_planes), list(dst_planes), bits
        check_filter_planes(filter, self.src_planes, self.dst_planes)
        self.filter = filter
        self.row, self.out_row = frame_samples(self.src_planes), frame_samples(self.dst_planes)
        self.size, self.source_size = tuple(size), tuple(source_size)

    def __call__(self, rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        return resize_frames(rows, self.src_planes, self.dst_planes, self.bits, out=out, filter=self.filter)


__all__ = ["check_size", "check_filter", "frame_planes", "frame_samples", "resize_frames", "resize_planes", "y4m_header_at", "FrameResize"]
