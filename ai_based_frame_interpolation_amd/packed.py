"""Packed RGB frames through the RGB (6->3) network, on the device.

Content that is RGB at its source - screen and game capture, renders, image sequences, whatever `cv2.imread` returns -
arrives with its pixels interleaved: `ffmpeg -f rawvideo -pix_fmt rgb24 | bgr24 | rgba | bgra` pipes it losslessly, and an
image library holds it as HWC bytes whose rows may lie a line size apart.  The network takes planar RGB; `packed_to_rgb` /
`rgb_to_packed` and `FrameInterpolationUNet.forward_rgb_packed` move the bytes between the two in HIP kernels
(`fiunet_packed_to_rgb_u8`, `fiunet_rgb_to_packed_u8`), where and how the frames lie in device memory: nothing is
subsampled, no colour matrix is applied, nothing is repacked on the host or by torch.

Formats (`FORMATS`): "rgb24" (R G B), "bgr24" (B G R), "rgba" (R G B A), "bgra" (B G R A): a pixel is 3 or 4 consecutive
bytes.  Alpha does not go through the network: a 4-byte frame is written with alpha 255, with a copy of another packed
frame's alpha, or with the rounded average (a1 + a2 + 1) >> 1 of two (what an inserted frame gets from its neighbours).
"""
from __future__ import annotations

import numbers
from typing import NamedTuple

import torch

from . import _native

# name -> (fiunet_packed_format code, bytes per pixel)
FORMATS = {"rgb24": (0, 3), "bgr24": (1, 3), "rgba": (2, 4), "bgra": (3, 4)}


class PackedLayout(NamedTuple):
    """Where the pixels of a packed frame lie, both fields in bytes; 0 = the tight value.  A frame is H rows `row_pitch`
    apart, each W*bpp bytes of pixels; frames `frame_stride` apart.  Tight: row_pitch W*bpp, frame_stride H*row_pitch."""
    row_pitch: int = 0
    frame_stride: int = 0


def _format(format) -> tuple[int, int]:
    try:
        return FORMATS[format]
    except (KeyError, TypeError):
        raise ValueError(f"format must be one of {list(FORMATS)}, got {format!r}") from None


def bytes_per_pixel(format: str) -> int:
    return _format(format)[1]


def frame_bytes(format: str, height: int, width: int) -> int:
    """Bytes of one tight packed frame of height x width."""
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"bad frame size {height!r}x{width!r}")
    return h * w * _format(format)[1]


def resolve_layout(layout: PackedLayout | None, format: str, height: int, width: int) -> PackedLayout:
    """-> `layout` with every 0 replaced by its tight value (None: the tight layout); ValueError where it cannot hold
    a height x width frame of `format` (the rules of include/fiunet.h, fiunet_packed_layout)."""
    bpp = _format(format)[1]
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"bad frame size {height!r}x{width!r}")
    vals = tuple(layout) if layout is not None else (0, 0)
    if len(vals) != 2 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0 or v > 1 << 40 for v in vals):
        raise ValueError(f"layout must be a PackedLayout of two ints in [0, 2^40] (bytes), got {layout!r}")
    row = w * bpp
    rp = int(vals[0]) or row
    fs = int(vals[1]) or h * rp
    if rp < row:
        raise ValueError(f"layout: row_pitch {rp} < {row}, the {w} {format} pixels of a row")
    if fs < (h - 1) * rp + row:
        raise ValueError(f"layout: frame_stride {fs} does not cover the last row (it ends at {(h - 1) * rp + row} bytes)")
    return PackedLayout(rp, fs)


def _check_frames(frames: torch.Tensor, height: int, width: int, what: str, format: str, layout: PackedLayout) -> None:
    """layout: resolved.  uint8 [B, layout.frame_stride] on the GPU, every frame contiguous."""
    fb = layout.frame_stride
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 2 or frames.shape[1] != fb:
        got = f"{frames.dtype} {tuple(frames.shape)}" if isinstance(frames, torch.Tensor) else repr(type(frames))
        raise ValueError(f"{what} must be uint8 [B, {fb}] packed {format} frames of {height}x{width}, got {got}")
    if not frames.is_cuda:
        raise RuntimeError(f"{what} must be on the GPU: there is no CPU path in this package")
    if frames.stride(1) != 1 or (frames.shape[0] > 1 and frames.stride(0) < fb):
        raise ValueError(f"{what}: every frame must be contiguous (strides {tuple(frames.stride())})")


@torch.no_grad()
def packed_to_rgb(frames: torch.Tensor, height: int, width: int, format: str, *, layout: PackedLayout | None = None,
                  out: torch.Tensor | None = None, return_alpha: bool = False):
    """uint8 [B, frame_stride] packed frames on the GPU ([B, H*W*bpp] when tight: layout None) -> uint8 planar RGB
    [B, 3, H, W] (`fiunet_packed_to_rgb_u8`).  `frames` may be a view whose frames lie further apart than frame_stride.
    return_alpha (rgba / bgra): -> (rgb, alpha), alpha the uint8 [B, H, W] plane of fourth bytes."""
    code, bpp = _format(format)
    h, w = int(height), int(width)
    lay = resolve_layout(layout, format, h, w)
    if return_alpha and bpp != 4:
        raise ValueError(f"return_alpha: {format} has no alpha byte")
    _check_frames(frames, h, w, "frames", format, lay)
    shape = (frames.shape[0], 3, h, w)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 {shape} tensor on {frames.device}")
    alpha = torch.empty((frames.shape[0], h, w), dtype=torch.uint8, device=frames.device) if return_alpha else None
    with torch.cuda.device(frames.device):
        _native.packed_to_rgb(frames, lay, out, alpha, h, w, code)
    return (out, alpha) if return_alpha else out


@torch.no_grad()
def rgb_to_packed(rgb: torch.Tensor, format: str, *, layout: PackedLayout | None = None,
                  out: torch.Tensor | None = None, alpha_from=None,
                  alpha_layout: PackedLayout | None = None) -> torch.Tensor:
    """uint8 planar RGB [B, 3, H, W] on the GPU -> uint8 [B, frame_stride] packed frames (`fiunet_rgb_to_packed_u8`).
    Bytes outside the used columns and between frames are left untouched (zero in a tensor made here).  `out` may be a
    view whose frames lie further apart than frame_stride.  alpha_from (rgba / bgra): None - alpha 255; a packed tensor
    of the same format and frame size - a copy of its alpha; a pair of them - the rounded average (a1 + a2 + 1) >> 1.
    alpha_layout: their layout (None: tight)."""
    code, bpp = _format(format)
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[1] != 3:
        got = f"{rgb.dtype} {tuple(rgb.shape)}" if isinstance(rgb, torch.Tensor) else repr(type(rgb))
        raise ValueError(f"rgb must be uint8 [B, 3, H, W], got {got}")
    if not rgb.is_cuda:
        raise RuntimeError("rgb must be on the GPU: there is no CPU path in this package")
    b, _, h, w = rgb.shape
    lay = resolve_layout(layout, format, h, w)
    if not rgb.is_contiguous():
        raise ValueError("rgb must be contiguous")
    alphas = () if alpha_from is None else (alpha_from,) if isinstance(alpha_from, torch.Tensor) else tuple(alpha_from)
    alay = resolve_layout(alpha_layout, format, h, w)
    if alphas:
        if bpp != 4:
            raise ValueError(f"alpha_from: {format} has no alpha byte")
        if len(alphas) > 2:
            raise ValueError(f"alpha_from is one packed tensor or a pair of them, got {len(alphas)}")
        for i, a in enumerate(alphas):
            _check_frames(a, h, w, f"alpha_from[{i}]", format, alay)
            if a.device != rgb.device or a.shape[0] != b:
                raise ValueError(f"alpha_from[{i}] must hold {b} frames on {rgb.device}")
        if len(alphas) == 2 and b > 1 and alphas[0].stride(0) != alphas[1].stride(0):
            raise ValueError("alpha_from: both tensors must have their frames the same distance apart")
    elif alpha_layout is not None:
        raise ValueError("alpha_layout describes alpha_from")
    if out is None:
        # (a pitched frame has bytes no pixel covers: they are never written, so a new one starts as zeros)
        out = (torch.empty if lay == resolve_layout(None, format, h, w) else torch.zeros)(
            (b, lay.frame_stride), dtype=torch.uint8, device=rgb.device)
    elif not isinstance(out, torch.Tensor) or out.device != rgb.device or out.shape[0] != b:
        raise ValueError(f"out must hold {b} frames on {rgb.device}")
    _check_frames(out, h, w, "out", format, lay)
    with torch.cuda.device(rgb.device):
        _native.rgb_to_packed(rgb, out, lay, alphas, alay, code)
    return out


__all__ = ["FORMATS", "PackedLayout", "bytes_per_pixel", "frame_bytes", "resolve_layout", "packed_to_rgb",
           "rgb_to_packed"]
