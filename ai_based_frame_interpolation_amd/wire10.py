"""10-bit 4:2:2 frames as capture cards and broadcast files carry them: v210, y210le and p210le.

Uncompressed 10-bit SDI / HDMI capture and every uncompressed broadcast `.mov` is v210; y210le and p210le are what GPU
decoders and the Windows / VA-API surfaces call Y210 and P210.  All three carry exactly the samples of `yuv422p10le`,
the 10-bit 4:2:2 format the package already runs (colour.py); only where the bits lie differs.  So the
package keeps one working format - tight `yuv422p10le` frames, uint16 words holding the code, Y H x W, then U, then V,
each H x ceil(W/2) - and `unpack` / `pack` move the bits between a packing and it, in two HIP kernels
(`fiunet_unpack_422p10`, `fiunet_pack_422p10`, csrc/wire10.hip.h).  Nothing is computed: a round trip is exact.

Packings (`PACKINGS`), every wire word little-endian:

  v210    one plane, even width.  Group g holds pixels 6g .. 6g+5 in four 32-bit words with a low, a middle and a high
          10-bit field each: w0 = U0 Y0 V0, w1 = Y1 U1 Y2, w2 = V1 Y3 U2, w3 = Y4 V2 Y5 (Uk, Vk: chroma sample 3g + k).
          A tight row is 128 * ceil(W / 48) bytes.  layout: a `packed.PackedLayout` in bytes.
  y210le  one plane, even width.  16-bit words Y0 U0 Y1 V0 per two pixels, each code << 6; a tight row is 4 W bytes.
          layout: a `packed.PackedLayout` in bytes.
  p210le  two planes, any width: Y of H x W words, then H rows of interleaved U V pairs, each word code << 6 (P010 with
          chroma of full height).  layout: a `colour.SurfaceLayout` in samples, its chroma plane H rows high.

Reading ignores bits 30-31 of a v210 word and the low six bits of a y210le / p210le word; writing leaves them zero, and
zeroes the v210 fields behind the last pixel and the padding up to the tight row size, so a tight frame is fully
determined.  Bytes between the tight row and a larger pitch, and between frames, are neither read nor written.  A working
word above 1023 packs as 1023.  The layout is a restatement of the formats' published definitions, unpinned against
ffmpeg (which is not part of the test environment).
"""
from __future__ import annotations

import numbers

import torch

from . import _native
from .colour import SurfaceLayout
from .packed import PackedLayout

# name -> fiunet_packing10 code
PACKINGS = {"v210": 0, "y210le": 1, "p210le": 2}
WORKING_FORMAT = "yuv422p10le"
_WORDS = (torch.int16, torch.uint16)


def _packing(packing) -> int:
    try:
        return PACKINGS[packing]
    except (KeyError, TypeError):
        raise ValueError(f"packing must be one of {list(PACKINGS)}, got {packing!r}") from None


def _size(packing: str, height, width) -> tuple[int, int]:
    _packing(packing)
    for name, v in (("height", height), ("width", width)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be a positive int, got {v!r}")
    if packing != "p210le" and width % 2:
        raise ValueError(f"{packing} frames have an even width (two pixels share a chroma pair), got {width}")
    return int(height), int(width)


def row_bytes(packing: str, width: int) -> int:
    """Bytes of one tight row of a one-plane packing (v210: whole 48-pixel blocks of 128 bytes)."""
    _size(packing, 1, width)
    if packing == "p210le":
        raise ValueError("p210le has two planes: its rows are 2 * width and 4 * ceil(width / 2) bytes")
    return 128 * ((width + 47) // 48) if packing == "v210" else 4 * width


def planar_samples(height: int, width: int) -> int:
    """16-bit words of one tight frame of the working format (yuv422p10le)."""
    return height * width + 2 * height * ((width + 1) // 2)


def frame_bytes(packing: str, height: int, width: int) -> int:
    """Bytes of one tight wire frame of height x width; always even."""
    h, w = _size(packing, height, width)
    return 2 * planar_samples(h, w) if packing == "p210le" else h * row_bytes(packing, w)


def resolve_layout(layout, packing: str, height: int, width: int):
    """-> `layout` with every 0 replaced by its tight value (None: the tight layout): a `packed.PackedLayout` in bytes
    for v210 / y210le, a `colour.SurfaceLayout` in samples for p210le; ValueError where it cannot hold a height x width
    frame (the rules of include/fiunet.h, fiunet_unpack_422p10)."""
    h, w = _size(packing, height, width)
    n = 4 if packing == "p210le" else 2
    vals = tuple(layout) if layout is not None else (0,) * n
    if len(vals) != n or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 0 or v > 1 << 40 for v in vals):
        kind = "SurfaceLayout of four ints (samples)" if n == 4 else "PackedLayout of two ints (bytes)"
        raise ValueError(f"layout of {packing} frames must be a {kind} in [0, 2^40], got {layout!r}")
    if packing == "p210le":
        wc = (w + 1) // 2
        lp, co, cp, fs = (int(v) or t for v, t in zip(vals, (w, h * w, 2 * wc, planar_samples(h, w))))
        if lp < w:
            raise ValueError(f"layout: luma_pitch {lp} < width {w}")
        if cp < 2 * wc:
            raise ValueError(f"layout: chroma_pitch {cp} < {2 * wc}, the {wc} U,V pairs of a row")
        if co < (h - 1) * lp + w:
            raise ValueError(f"layout: chroma_offset {co} lies inside the luma plane ({(h - 1) * lp + w} samples)")
        if fs < co + (h - 1) * cp + 2 * wc:
            raise ValueError(f"layout: frame_stride {fs} does not cover the chroma plane (it ends at "
                             f"{co + (h - 1) * cp + 2 * wc} samples)")
        return SurfaceLayout(lp, co, cp, fs)
    row = row_bytes(packing, w)
    rp = int(vals[0]) or row
    fs = int(vals[1]) or h * rp
    if rp < row:
        raise ValueError(f"layout: row_pitch {rp} < {row}, the tight {packing} row of {w} pixels")
    if fs < (h - 1) * rp + row:
        raise ValueError(f"layout: frame_stride {fs} does not cover the last row (it ends at {(h - 1) * rp + row} bytes)")
    if rp % 2 or fs % 2:
        raise ValueError(f"layout: row_pitch {rp} and frame_stride {fs} must be even (the wire words are 16-bit aligned)")
    return PackedLayout(rp, fs)


def _stride_bytes(packing: str, lay) -> int:
    return 2 * lay.frame_stride if packing == "p210le" else lay.frame_stride


def _check_wire(t, what: str, packing: str, h: int, w: int, lay) -> None:
    """lay: resolved.  uint8 or 16-bit [B, one frame stride] on the GPU, every frame contiguous."""
    fb = _stride_bytes(packing, lay)
    ok = isinstance(t, torch.Tensor) and t.dtype in (torch.uint8,) + _WORDS and t.dim() == 2
    if not ok or t.shape[1] * t.element_size() != fb:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else repr(type(t))
        raise ValueError(f"{what} must be uint8 [B, {fb}] (or 16-bit [B, {fb // 2}]) {packing} frames of {h}x{w}, got {got}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be on the GPU: there is no CPU path in this package")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        raise ValueError(f"{what}: every frame must be contiguous (strides {tuple(t.stride())})")


def _check_planar(t, what: str, h: int, w: int) -> None:
    n = planar_samples(h, w)
    if not isinstance(t, torch.Tensor) or t.dtype not in _WORDS or t.dim() != 2 or t.shape[1] != n:
        got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else repr(type(t))
        raise ValueError(f"{what} must be 16-bit [B, {n}] {WORKING_FORMAT} frames of {h}x{w}, got {got}")
    if not t.is_cuda:
        raise RuntimeError(f"{what} must be on the GPU: there is no CPU path in this package")
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < n):
        raise ValueError(f"{what}: every frame must be contiguous (strides {tuple(t.stride())})")


@torch.no_grad()
def unpack(frames: torch.Tensor, height: int, width: int, packing: str, layout=None, out: torch.Tensor | None = None,
           *, stream=None) -> torch.Tensor:
    """Wire frames on the GPU - uint8 [B, frame bytes] or 16-bit [B, frame bytes / 2], tight (`frame_bytes`) or in
    `layout` - -> uint16 [B, `planar_samples`] tight yuv422p10le frames (`fiunet_unpack_422p10`).  `frames` may be a view
    whose frames lie further apart.  out: write there (uint16 or int16 [B, planar_samples], rows contiguous)."""
    code = _packing(packing)
    h, w = _size(packing, height, width)
    lay = resolve_layout(layout, packing, h, w)
    _check_wire(frames, "frames", packing, h, w, lay)
    if out is None:
        out = torch.empty((frames.shape[0], planar_samples(h, w)), dtype=torch.uint16, device=frames.device)
    else:
        _check_planar(out, "out", h, w)
        if out.device != frames.device or out.shape[0] != frames.shape[0]:
            raise ValueError(f"out must hold {frames.shape[0]} frames on {frames.device}")
    if frames.shape[0]:
        with torch.cuda.device(frames.device):
            _native.unpack_422p10(frames, code, lay, out, h, w, stream)
    return out


@torch.no_grad()
def pack(planar: torch.Tensor, height: int, width: int, packing: str, layout=None, out: torch.Tensor | None = None,
         *, stream=None) -> torch.Tensor:
    """uint16 (or int16) [B, `planar_samples`] yuv422p10le frames on the GPU -> wire frames of `packing`, uint8 [B, frame
    bytes], tight or in `layout` (`fiunet_pack_422p10`).  Bytes behind the tight rows and between frames are left
    untouched (zero in a tensor made here).  out: write there (uint8 or 16-bit, one frame stride per row; it may be a view
    whose frames lie further apart)."""
    code = _packing(packing)
    h, w = _size(packing, height, width)
    lay = resolve_layout(layout, packing, h, w)
    _check_planar(planar, "planar", h, w)
    b = planar.shape[0]
    if out is None:
        tight = lay == resolve_layout(None, packing, h, w)
        out = (torch.empty if tight else torch.zeros)((b, _stride_bytes(packing, lay)), dtype=torch.uint8,
                                                      device=planar.device)
    elif not isinstance(out, torch.Tensor) or out.device != planar.device or out.shape[0] != b:
        raise ValueError(f"out must hold {b} frames on {planar.device}")
    _check_wire(out, "out", packing, h, w, lay)
    if b:
        with torch.cuda.device(planar.device):
            _native.pack_422p10(planar, out, code, lay, h, w, stream)
    return out


@torch.no_grad()
def forward(model, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, packing: str, layout=None,
            out_layout=None, **colour_opts) -> torch.Tensor:
    """The RGB network on wire frames of `packing`: bit for bit `unpack` (both inputs) ->
    `model.forward_yuv(..., format="yuv422p10le", **colour_opts)` -> `pack` into `out_layout` (None: tight).
    colour_opts: siting, matrix, colour_range as `forward_yuv` takes them."""
    a = unpack(frame1, height, width, packing, layout)
    b = unpack(frame2, height, width, packing, layout)
    mid = model.forward_yuv(a, b, int(height), int(width), format=WORKING_FORMAT, **colour_opts)
    return pack(mid, height, width, packing, out_layout)


__all__ = ["PACKINGS", "WORKING_FORMAT", "row_bytes", "planar_samples", "frame_bytes", "resolve_layout", "unpack",
           "pack", "forward"]
