"""YUV 4:2:0 colour video for the RGB (6->3) network: option parsing and the two device conversions.

A frame is packed I420 - the Y plane H x W, then U, then V, each ceil(H/2) x ceil(W/2) bytes - exactly a Y4M frame
payload, so a decoded video (`ffmpeg -i in.mp4 -pix_fmt yuv420p in.y4m`) reaches the network without a host-side
conversion.  The conversion is defined in integer arithmetic (csrc/colour.hip.h, DESIGN.md "Colour video") and runs
in HIP kernels (`fiunet_yuv420_to_rgb_u8`, `fiunet_rgb_to_yuv420_u8`); the network's forward between them is
`FrameInterpolationUNet.forward_yuv420`.

10-bit video (`C420p10` Y4M: every sample a 10-bit code in a little-endian 16-bit word) has the same layout in uint16
samples: `yuv420p10_to_rgb` / `rgb_to_yuv420p10` and `FrameInterpolationUNet.forward_yuv420p10`.

Decoder surfaces: a hardware decoder leaves semi-planar frames in device memory - NV12 at 8 bits (the
Y plane, then one plane of interleaved U,V pairs), P010 at 10 (the same in 16-bit words, the code in the upper ten bits),
rows a pitch apart.  `nv12_to_rgb` / `rgb_to_nv12`, `p010_to_rgb` / `rgb_to_p010` and
`FrameInterpolationUNet.forward_nv12` / `forward_p010` are the conversions above on that layout (`SurfaceLayout`), with
the same arithmetic bit for bit.

4:2:2 and 4:4:4 video: `YUV_FORMATS` names, by ffmpeg's -pix_fmt names, what mezzanine codecs decode to
("yuv422p10le"), what capture cards deliver ("uyvy422", "yuyv422") and what YUV screen and grading sources hold
("yuv444p", "yuv444p10le"), plus "yuv422p".  `yuv_to_rgb` / `rgb_to_yuv` and `FrameInterpolationUNet.forward_yuv` take them
by name; the arithmetic is the 4:2:0 one with the sub-sampling pattern changed (4:2:2 is its horizontal half, 4:4:4 has
none), siting defaults to "mpeg2" for 4:2:2 and means nothing for 4:4:4.

Options (the keywords of every colour entry point):
  siting        "jpeg" (Y4M C420jpeg, C420 or no tag: chroma centred in its 2x2 luma block) or "mpeg2" (C420mpeg2:
                co-sited with the even luma column, centred vertically)
  matrix        "bt709" (the default: the inputs are HD video; Y4M does not carry the matrix) or "bt601"; for 10-bit
                video also "bt2020" (non-constant luminance, the matrix of HDR10 / HLG content)
  colour_range  "limited" (Y 16-235, C 16-240; the default, and what a Y4M header without XCOLORRANGE means) or "full"
"""
from __future__ import annotations

import numbers
from typing import NamedTuple

import torch

from . import _native

SITINGS = {"jpeg": 0, "mpeg2": _native.YUV_MPEG2}
MATRICES = {"bt601": 0, "bt709": _native.YUV_BT709}
MATRICES_P10 = dict(MATRICES, bt2020=_native.YUV_BT2020)   # BT.2020 defines 10- and 12-bit coding only
RANGES = {"limited": 0, "full": _native.YUV_FULL_RANGE}

#: Y4M colourspace tags the RGB network reads, and the chroma siting each one means
Y4M_SITING = {"420jpeg": "jpeg", "420": "jpeg", "420mpeg2": "mpeg2"}


def colour_flags(siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited", bits: int = 8) -> int:
    """-> the `colour` flags word of the C ABI (include/fiunet.h, enum fiunet_colour).  bits: 8 or 10, the sample depth
    of the entry point the flags go to; matrix "bt2020" is valid with 10 only."""
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    matrices = MATRICES_P10 if bits == 10 else MATRICES
    for name, value, table in (("siting", siting, SITINGS), ("matrix", matrix, matrices),
                               ("colour_range", colour_range, RANGES)):
        if value not in table:
            raise ValueError(f"{name} must be one of {sorted(table)} for {bits}-bit video, got {value!r}")
    return SITINGS[siting] | matrices[matrix] | RANGES[colour_range]


def i420_frame_bytes(height: int, width: int) -> int:
    """Bytes of one packed I420 frame: H*W + 2 * ceil(H/2) * ceil(W/2)."""
    return height * width + 2 * ((height + 1) // 2) * ((width + 1) // 2)


def yuv420p10_frame_samples(height: int, width: int) -> int:
    """Samples (uint16 words) of one packed 4:2:0 10-bit frame: H*W + 2 * ceil(H/2) * ceil(W/2)."""
    return i420_frame_bytes(height, width)


class SurfaceLayout(NamedTuple):
    """Where the samples of an NV12 / P010 frame lie, every field in samples (bytes at 8 bits, 16-bit words at 10); 0 =
    the tight value.  A frame is H luma rows `luma_pitch` apart, then, `chroma_offset` samples after the frame's base,
    ceil(H/2) chroma rows `chroma_pitch` apart, each ceil(W/2) pairs U0 V0 U1 V1 ...; frames `frame_stride` apart.
    Tight: luma_pitch W, chroma_offset H*W, chroma_pitch 2*ceil(W/2), frame_stride `i420_frame_bytes(H, W)`."""
    luma_pitch: int = 0
    chroma_offset: int = 0
    chroma_pitch: int = 0
    frame_stride: int = 0


def resolve_layout(layout: SurfaceLayout | None, height: int, width: int) -> SurfaceLayout:
    """-> `layout` with every 0 replaced by its tight value (None: the tight layout); ValueError where it cannot hold
    a height x width frame (the rules of include/fiunet.h, fiunet_surface_layout)."""
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"bad frame size {height!r}x{width!r}")
    hc, wc = (h + 1) // 2, (w + 1) // 2
    vals = tuple(layout) if layout is not None else (0, 0, 0, 0)
    if len(vals) != 4 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0 or v > 1 << 40 for v in vals):
        raise ValueError(f"layout must be a SurfaceLayout of four ints in [0, 2^40] (samples), got {layout!r}")
    lp, co, cp, fs = (int(v) or t for v, t in zip(vals, (w, h * w, 2 * wc, i420_frame_bytes(h, w))))
    if lp < w:
        raise ValueError(f"layout: luma_pitch {lp} < width {w}")
    if cp < 2 * wc:
        raise ValueError(f"layout: chroma_pitch {cp} < {2 * wc}, the {wc} U,V pairs of a row")
    if co < (h - 1) * lp + w:
        raise ValueError(f"layout: chroma_offset {co} lies inside the luma plane ({(h - 1) * lp + w} samples)")
    if fs < co + (hc - 1) * cp + 2 * wc:
        raise ValueError(f"layout: frame_stride {fs} does not cover the chroma plane (it ends at "
                         f"{co + (hc - 1) * cp + 2 * wc} samples)")
    return SurfaceLayout(lp, co, cp, fs)


#: name (ffmpeg's -pix_fmt) -> (fiunet_yuv_format code, bits, kind): "422" / "444" planar, "packed" one-plane 4:2:2
YUV_FORMATS = {"yuv422p": (0, 8, "422"), "yuv444p": (1, 8, "444"), "yuv422p10le": (0, 10, "422"),
               "yuv444p10le": (1, 10, "444"), "uyvy422": (2, 8, "packed"), "yuyv422": (3, 8, "packed")}


def _yuv_format(format) -> tuple[int, int, str]:
    try:
        return YUV_FORMATS[format]
    except (KeyError, TypeError):
        raise ValueError(f"format must be one of {list(YUV_FORMATS)}, got {format!r}") from None


def yuv_frame_samples(format: str, height: int, width: int) -> int:
    """Samples of one tight frame of `format` (bytes at 8 bits, 16-bit words at 10): H*W + 2*H*ceil(W/2) for planar
    4:2:2, 3*H*W for 4:4:4, 2*H*W for uyvy422 / yuyv422, which need an even width."""
    _, _, kind = _yuv_format(format)
    h, w = int(height), int(width)
    if h < 1 or w < 1:
        raise ValueError(f"bad frame size {height!r}x{width!r}")
    if kind == "packed":
        if w % 2:
            raise ValueError(f"{format} frames have an even width (two pixels share a chroma pair), got {w}")
        return 2 * h * w
    return 3 * h * w if kind == "444" else h * w + 2 * h * ((w + 1) // 2)


def resolve_yuv_layout(layout, format: str, height: int, width: int):
    """-> a `packed.PackedLayout` (row_pitch, frame_stride) in samples with every 0 of `layout` replaced by its tight
    value (None: the tight layout); ValueError where it cannot hold a height x width frame of `format` (the rules of
    include/fiunet.h, fiunet_yuv_to_rgb_u8).  Planar frames are tight inside: their row_pitch stays 0 and must be 0."""
    from .packed import PackedLayout
    _, _, kind = _yuv_format(format)
    tight = yuv_frame_samples(format, height, width)
    h, w = int(height), int(width)
    vals = tuple(layout) if layout is not None else (0, 0)
    if len(vals) != 2 or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0 or v > 1 << 40 for v in vals):
        raise ValueError(f"layout must be a PackedLayout of two ints in [0, 2^40] (samples), got {layout!r}")
    if kind != "packed":
        if vals[0]:
            raise ValueError(f"layout: {format} frames are tight inside (row_pitch must be 0, got {vals[0]})")
        fs = int(vals[1]) or tight
        if fs < tight:
            raise ValueError(f"layout: frame_stride {fs} is smaller than one frame ({tight} samples)")
        return PackedLayout(0, fs)
    rp = int(vals[0]) or 2 * w
    fs = int(vals[1]) or h * rp
    if rp < 2 * w:
        raise ValueError(f"layout: row_pitch {rp} < {2 * w}, the {w} {format} pixels of a row")
    if fs < (h - 1) * rp + 2 * w:
        raise ValueError(f"layout: frame_stride {fs} does not cover the last row (it ends at {(h - 1) * rp + 2 * w} bytes)")
    return PackedLayout(rp, fs)


def yuv_flags(format: str, siting, matrix: str, colour_range: str) -> int:
    """`colour_flags` at the depth of `format`; siting None means "mpeg2" (what decoders and ffmpeg assume for 4:2:2;
    4:4:4 has no siting: any valid value is accepted and ignored)."""
    return colour_flags("mpeg2" if siting is None else siting, matrix, colour_range, bits=_yuv_format(format)[1])


def _check_yuv_frames(frames, height, width, what, format, layout) -> None:
    """layout: resolved.  [B, layout.frame_stride] in the dtype of `format` on the GPU, every frame contiguous."""
    dtype = torch.uint16 if _yuv_format(format)[1] == 10 else torch.uint8
    fb = layout.frame_stride
    if not isinstance(frames, torch.Tensor) or frames.dtype != dtype or frames.dim() != 2 or frames.shape[1] != fb:
        got = f"{frames.dtype} {tuple(frames.shape)}" if isinstance(frames, torch.Tensor) else repr(type(frames))
        raise ValueError(f"{what} must be {str(dtype).split('.')[-1]} [B, {fb}] {format} frames of {height}x{width}, "
                         f"got {got}")
    if not frames.is_cuda:
        raise RuntimeError(f"{what} must be on the GPU: there is no CPU path in this package")
    if frames.stride(1) != 1 or (frames.shape[0] > 1 and frames.stride(0) < fb):
        raise ValueError(f"{what}: every frame must be contiguous (strides {tuple(frames.stride())})")


@torch.no_grad()
def yuv_to_rgb(frames: torch.Tensor, height: int, width: int, format: str, *, siting: str | None = None,
               matrix: str = "bt709", colour_range: str = "limited", layout=None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """[B, frame_stride] frames of `format` (a `YUV_FORMATS` name; uint8 at 8 bits, uint16 words of 10-bit codes at
    10, above 1023 read as 1023) on the GPU -> planar RGB [B, 3, H, W] of the same dtype (`fiunet_yuv_to_rgb_u8` /
    `fiunet_yuv_to_rgb_p10`).  layout: a `packed.PackedLayout` in samples or None for tight frames - uyvy422 / yuyv422
    take a row pitch and a frame stride, the planar formats a frame stride only; `frames` may be a view whose frames
    lie further apart.  siting None is "mpeg2"; matrix also takes "bt2020" at 10 bits."""
    code, bits, _ = _yuv_format(format)
    h, w = int(height), int(width)
    lay = resolve_yuv_layout(layout, format, h, w)
    flags = yuv_flags(format, siting, matrix, colour_range)
    _check_yuv_frames(frames, h, w, "frames", format, lay)
    dtype = frames.dtype
    shape = (frames.shape[0], 3, h, w)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=frames.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {str(dtype).split('.')[-1]} {shape} tensor on {frames.device}")
    with torch.cuda.device(frames.device):
        _native.yuv_to_rgb(frames, code, lay, out, h, w, flags, bits)
    return out


@torch.no_grad()
def rgb_to_yuv(rgb: torch.Tensor, format: str, *, siting: str | None = None, matrix: str = "bt709",
               colour_range: str = "limited", layout=None, out: torch.Tensor | None = None) -> torch.Tensor:
    """Planar RGB [B, 3, H, W] on the GPU (uint8, or uint16 of 10-bit codes for a 10-bit format) -> [B, frame_stride]
    frames of `format` (`fiunet_rgb_to_yuv_u8` / `fiunet_rgb_p10_to_yuv`).  Samples outside the used columns of a
    pitched row and between frames are left untouched (zero in a tensor made here).  `out` may be a view whose frames
    lie further apart than frame_stride.  layout, siting, matrix: as for `yuv_to_rgb`."""
    code, bits, _ = _yuv_format(format)
    dtype = torch.uint16 if bits == 10 else torch.uint8
    if not isinstance(rgb, torch.Tensor) or rgb.dtype != dtype or rgb.dim() != 4 or rgb.shape[1] != 3:
        got = f"{rgb.dtype} {tuple(rgb.shape)}" if isinstance(rgb, torch.Tensor) else repr(type(rgb))
        raise ValueError(f"rgb must be {str(dtype).split('.')[-1]} [B, 3, H, W] for {format}, got {got}")
    b, _, h, w = rgb.shape
    lay = resolve_yuv_layout(layout, format, h, w)
    flags = yuv_flags(format, siting, matrix, colour_range)
    if not rgb.is_cuda:
        raise RuntimeError("rgb must be on the GPU: there is no CPU path in this package")
    if not rgb.is_contiguous():
        raise ValueError("rgb must be contiguous")
    if out is None:
        # (a pitched frame has bytes no pixel covers: they are never written, so a new one starts as zeros)
        out = (torch.empty if lay == resolve_yuv_layout(None, format, h, w) else torch.zeros)(
            (b, lay.frame_stride), dtype=dtype, device=rgb.device)
    elif not isinstance(out, torch.Tensor) or out.device != rgb.device or out.shape[0] != b:
        raise ValueError(f"out must hold {b} frames on {rgb.device}")
    _check_yuv_frames(out, h, w, "out", format, lay)
    with torch.cuda.device(rgb.device):
        _native.rgb_to_yuv(rgb, out, code, lay, flags, bits)
    return out


def siting_of_y4m(colourspace: str) -> str:
    """Chroma siting of a Y4M `C` tag; ValueError naming the tag for the layouts the RGB network does not read."""
    try:
        return Y4M_SITING[colourspace]
    except KeyError:
        raise ValueError(f"Y4M colourspace C{colourspace} is not supported by the RGB network: it reads 4:2:0 "
                         f"video tagged {', '.join('C' + t for t in Y4M_SITING)} or untagged") from None


def _check_frames(frames: torch.Tensor, height: int, width: int, what: str, dtype=torch.uint8,
                  layout: SurfaceLayout | None = None) -> None:
    """layout: a resolved SurfaceLayout: the frames are NV12 / P010 surfaces of layout.frame_stride samples."""
    fb = i420_frame_bytes(height, width) if layout is None else layout.frame_stride
    if frames.dtype != dtype or frames.dim() != 2 or frames.shape[1] != fb:
        kind = "I420" if dtype == torch.uint8 else "4:2:0 10-bit"
        if layout is not None:
            kind = "NV12" if dtype == torch.uint8 else "P010"
        raise ValueError(f"{what} must be {str(dtype).split('.')[-1]} [B, {fb}] packed {kind} frames of "
                         f"{height}x{width}, got {frames.dtype} {tuple(frames.shape)}")
    if not frames.is_cuda:
        raise RuntimeError(f"{what} must be on the GPU: there is no CPU path in this package")
    if frames.shape[0] > 1 and (frames.stride(1) != 1 or frames.stride(0) < fb):
        raise ValueError(f"{what}: every frame must be contiguous (strides {tuple(frames.stride())})")


@torch.no_grad()
def yuv420_to_rgb(frames: torch.Tensor, height: int, width: int, *, siting: str = "jpeg", matrix: str = "bt709",
                  colour_range: str = "limited", out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [B, F] packed I420 frames on the GPU -> uint8 planar RGB [B, 3, H, W] (`fiunet_yuv420_to_rgb_u8`)."""
    flags = colour_flags(siting, matrix, colour_range)
    _check_frames(frames, height, width, "frames")
    shape = (frames.shape[0], 3, height, width)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=frames.device)
    elif out.dtype != torch.uint8 or tuple(out.shape) != shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 {shape} tensor on {frames.device}")
    with torch.cuda.device(frames.device):
        _native.yuv420_to_rgb(frames, out, height, width, flags, 8)
    return out


@torch.no_grad()
def rgb_to_yuv420(rgb: torch.Tensor, *, siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited",
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 planar RGB [B, 3, H, W] on the GPU -> uint8 [B, F] packed I420 frames (`fiunet_rgb_to_yuv420_u8`).
    `out` may be a view whose frames lie further apart than F bytes; the bytes between them are left untouched."""
    flags = colour_flags(siting, matrix, colour_range)
    if rgb.dtype != torch.uint8 or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"rgb must be uint8 [B, 3, H, W], got {rgb.dtype} {tuple(rgb.shape)}")
    if not rgb.is_cuda:
        raise RuntimeError("rgb must be on the GPU: there is no CPU path in this package")
    b, _, h, w = rgb.shape
    rgb = rgb.contiguous()
    if out is None:
        out = torch.empty((b, i420_frame_bytes(h, w)), dtype=torch.uint8, device=rgb.device)
    elif out.device != rgb.device or out.shape[0] != b:
        raise ValueError(f"out must hold {b} frames on {rgb.device}")
    _check_frames(out, h, w, "out")
    with torch.cuda.device(rgb.device):
        _native.rgb_to_yuv420(rgb, out, flags, 8)
    return out


@torch.no_grad()
def yuv420p10_to_rgb(frames: torch.Tensor, height: int, width: int, *, siting: str = "jpeg", matrix: str = "bt709",
                     colour_range: str = "limited", out: torch.Tensor | None = None) -> torch.Tensor:
    """uint16 [B, F] packed 4:2:0 10-bit frames on the GPU -> uint16 planar RGB [B, 3, H, W] of 10-bit codes
    (`fiunet_yuv420p10_to_rgb_p10`).  Samples above 1023 are read as 1023."""
    flags = colour_flags(siting, matrix, colour_range, bits=10)
    _check_frames(frames, height, width, "frames", torch.uint16)
    shape = (frames.shape[0], 3, height, width)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint16, device=frames.device)
    elif out.dtype != torch.uint16 or tuple(out.shape) != shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint16 {shape} tensor on {frames.device}")
    with torch.cuda.device(frames.device):
        _native.yuv420_to_rgb(frames, out, height, width, flags, 10)
    return out


@torch.no_grad()
def rgb_to_yuv420p10(rgb: torch.Tensor, *, siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited",
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """uint16 planar RGB [B, 3, H, W] of 10-bit codes on the GPU -> uint16 [B, F] packed 4:2:0 10-bit frames
    (`fiunet_rgb_p10_to_yuv420p10`).  `out` may be a view whose frames lie further apart than F samples; the samples
    between them are left untouched."""
    flags = colour_flags(siting, matrix, colour_range, bits=10)
    if rgb.dtype != torch.uint16 or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"rgb must be uint16 [B, 3, H, W], got {rgb.dtype} {tuple(rgb.shape)}")
    if not rgb.is_cuda:
        raise RuntimeError("rgb must be on the GPU: there is no CPU path in this package")
    b, _, h, w = rgb.shape
    if not rgb.is_contiguous():
        raise ValueError("rgb must be contiguous")
    if out is None:
        out = torch.empty((b, yuv420p10_frame_samples(h, w)), dtype=torch.uint16, device=rgb.device)
    elif out.device != rgb.device or out.shape[0] != b:
        raise ValueError(f"out must hold {b} frames on {rgb.device}")
    _check_frames(out, h, w, "out", torch.uint16)
    with torch.cuda.device(rgb.device):
        _native.rgb_to_yuv420(rgb, out, flags, 10)
    return out


def _surface_to_rgb(frames, height, width, siting, matrix, colour_range, out, layout, bits):
    dtype = torch.uint16 if bits == 10 else torch.uint8
    flags = colour_flags(siting, matrix, colour_range, bits=bits)
    lay = resolve_layout(layout, height, width)
    _check_frames(frames, height, width, "frames", dtype, lay)
    shape = (frames.shape[0], 3, height, width)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=frames.device)
    elif out.dtype != dtype or tuple(out.shape) != shape or out.device != frames.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {str(dtype).split('.')[-1]} {shape} tensor on {frames.device}")
    with torch.cuda.device(frames.device):
        _native.surface_to_rgb(frames, lay, out, height, width, flags, bits)
    return out


def _rgb_to_surface(rgb, siting, matrix, colour_range, out, layout, bits):
    dtype = torch.uint16 if bits == 10 else torch.uint8
    flags = colour_flags(siting, matrix, colour_range, bits=bits)
    if rgb.dtype != dtype or rgb.dim() != 4 or rgb.shape[1] != 3:
        raise ValueError(f"rgb must be {str(dtype).split('.')[-1]} [B, 3, H, W], got {rgb.dtype} {tuple(rgb.shape)}")
    if not rgb.is_cuda:
        raise RuntimeError("rgb must be on the GPU: there is no CPU path in this package")
    b, _, h, w = rgb.shape
    lay = resolve_layout(layout, h, w)
    if not rgb.is_contiguous():
        raise ValueError("rgb must be contiguous")
    if out is None:
        # (a pitched surface has samples no frame covers: they are never written, so a new one starts as zeros)
        out = (torch.empty if lay == resolve_layout(None, h, w) else torch.zeros)(
            (b, lay.frame_stride), dtype=dtype, device=rgb.device)
    elif out.device != rgb.device or out.shape[0] != b:
        raise ValueError(f"out must hold {b} frames on {rgb.device}")
    _check_frames(out, h, w, "out", dtype, lay)
    with torch.cuda.device(rgb.device):
        _native.rgb_to_surface(rgb, out, lay, flags, bits)
    return out


@torch.no_grad()
def nv12_to_rgb(frames: torch.Tensor, height: int, width: int, *, siting: str = "mpeg2", matrix: str = "bt709",
                colour_range: str = "limited", out: torch.Tensor | None = None,
                layout: SurfaceLayout | None = None) -> torch.Tensor:
    """uint8 [B, frame_stride] NV12 surfaces on the GPU ([B, F] when tight: layout None) -> uint8 planar RGB
    [B, 3, H, W] (`fiunet_nv12_to_rgb_u8`): `yuv420_to_rgb` on the semi-planar layout, bit for bit.  siting defaults
    to "mpeg2", what decoders produce."""
    return _surface_to_rgb(frames, int(height), int(width), siting, matrix, colour_range, out, layout, 8)


@torch.no_grad()
def rgb_to_nv12(rgb: torch.Tensor, *, siting: str = "mpeg2", matrix: str = "bt709", colour_range: str = "limited",
                out: torch.Tensor | None = None, layout: SurfaceLayout | None = None) -> torch.Tensor:
    """uint8 planar RGB [B, 3, H, W] on the GPU -> uint8 [B, frame_stride] NV12 surfaces (`fiunet_rgb_to_nv12_u8`).
    Samples outside the used columns and between the planes and frames are left untouched (zero in a surface made
    here).  `out` may be a view whose frames lie further apart than frame_stride."""
    return _rgb_to_surface(rgb, siting, matrix, colour_range, out, layout, 8)


@torch.no_grad()
def p010_to_rgb(frames: torch.Tensor, height: int, width: int, *, siting: str = "mpeg2", matrix: str = "bt709",
                colour_range: str = "limited", out: torch.Tensor | None = None,
                layout: SurfaceLayout | None = None) -> torch.Tensor:
    """uint16 [B, frame_stride] P010 surfaces on the GPU (a word is code << 6; the low six bits are ignored) -> uint16
    planar RGB [B, 3, H, W] of 10-bit codes (`fiunet_p010_to_rgb_p10`).  matrix also takes "bt2020"."""
    return _surface_to_rgb(frames, int(height), int(width), siting, matrix, colour_range, out, layout, 10)


@torch.no_grad()
def rgb_to_p010(rgb: torch.Tensor, *, siting: str = "mpeg2", matrix: str = "bt709", colour_range: str = "limited",
                out: torch.Tensor | None = None, layout: SurfaceLayout | None = None) -> torch.Tensor:
    """uint16 planar RGB [B, 3, H, W] of 10-bit codes on the GPU -> uint16 [B, frame_stride] P010 surfaces, every word
    code << 6 with the low six bits zero (`fiunet_rgb_p10_to_p010`).  `out` / `layout`: as for `rgb_to_nv12`."""
    return _rgb_to_surface(rgb, siting, matrix, colour_range, out, layout, 10)
