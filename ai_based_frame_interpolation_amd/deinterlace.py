"""Deinterlace interlaced video on the device (csrc/deinterlace.hip.h): the two fields of every frame of
1080i / 576i / 480i material become whole frames, so that the network, the blend, the flow and the scores behind it see
one instant per frame.

  definition  motion-adaptive, in integers, the project's own in the spirit of yadif: the kept rows of a field are copied,
              a missing sample is an edge-directed average of the rows above and below, held within a band around the
              temporal average whose width is the local temporal change (include/fiunet.h states it sample for sample,
              tests/deinterlace_ref.py in numpy; the kernels equal that to the last bit).  NOT pinned against ffmpeg's
              yadif, which is not installed where this is tested.  method "bob" is the vertical average alone.
  fields      order "tff": the even rows of a frame come first in time; "bff": the odd rows.  rate "field": two output
              frames per frame (the frame rate doubles); "frame": one, from the first field.
  planes      every plane of a frame is filtered on its own, where it lies: the chroma of 4:2:0 (whose rows alternate
              between the fields too), the interleaved U and V of NV12, the bytes of uyvy422 / yuyv422 and packed RGB.
              A plane needs two rows or more.
  window      a frame needs the frame before and behind it; outside the clip the nearest frame stands in.
              `deinterlace(first=, count=)` filters part of a window, so a stream runs in chunks with one context frame
              either side (`deinterlace_video`): byte-identical for every chunk size.

`deinterlace_video` is file to file or pipe to pipe and needs no model; it sits in front of the `video` command:

    ffmpeg -i 1080i.mxf -f yuv4mpegpipe - | python -m ai_based_frame_interpolation_amd.cli deinterlace --input - \\
        --output - | python -m ai_based_frame_interpolation_amd.cli video --input - --output - --model best_model.pth

Out of scope: bwdif / w3fdif taps, .npy input, a deinterlacer inside the `video` / `evaluate` engine (they warn where a
Y4M header says interlaced, and pipe).  Hard-telecined film goes through `ivtc.py` instead, which matches its fields."""
from __future__ import annotations

import os
import warnings
from fractions import Fraction

import numpy as np
import torch

from . import _native, imageio_lite
from .layout import RAW_FORMATS, Layout, frame_layout

ORDERS = {"tff": _native.DEINT_TFF, "bff": _native.DEINT_BFF}
RATES = {"field": _native.DEINT_FIELD_RATE, "frame": _native.DEINT_FRAME_RATE}
METHODS = {"adaptive": _native.DEINT_ADAPTIVE, "bob": _native.DEINT_BOB}
MAX_PLANES = 4   # planes per call of the library


def _choice(name: str, value, table) -> str:
    if not isinstance(value, str) or value not in table:
        raise ValueError(f"{name} must be one of {list(table)}, got {value!r}")
    return value


def check_options(order, rate, method, auto: bool = False):
    """The names of a call, checked -> (order, rate, method); auto: order may be "auto" (deinterlace_video)."""
    if not (auto and order == "auto"):
        _choice("order", order, ["auto"] + list(ORDERS) if auto else ORDERS)
    return order, _choice("rate", rate, RATES), _choice("method", method, METHODS)


def interlaced_warning(interlace, what: str) -> None:
    """One UserWarning where a Y4M header says `It`, `Ib` or `Im` and the frames go on untreated (`interlace`: what
    `imageio_lite.y4m_interlace` gives)."""
    if interlace in ("t", "b", "m"):
        warnings.warn(f"{what}: the Y4M header says I{interlace} (interlaced): every frame holds two fields taken at "
                      "different times, and they are processed as one picture.  Deinterlace first: pipe the clip through "
                      "`python -m ai_based_frame_interpolation_amd.cli deinterlace`", UserWarning, stacklevel=3)


def _planes_of(layout_or_planes):
    planes = layout_or_planes.planes if isinstance(layout_or_planes, Layout) else list(layout_or_planes)
    if not planes:
        raise ValueError("no planes to deinterlace")
    planes = [tuple(int(v) for v in tuple(p)[-5:]) for p in planes]
    for off, h, w, pitch, step in planes:
        if h < 2:
            raise ValueError(f"a plane of {h} x {w} cannot be deinterlaced: a field needs a row of its own (h >= 2)")
    return planes


def _bits_of(t: torch.Tensor) -> int:
    if t.dtype == torch.uint8:
        return 8
    if t.dtype in (torch.uint16, torch.int16):
        return 10
    raise ValueError(f"expected uint8 samples or 16-bit words of 10-bit codes, got {t.dtype}")


def deinterlace(frames: torch.Tensor, layout_or_planes, bits: int, order: str = "tff", rate: str = "field",
                method: str = "adaptive", spatial_check: bool = True, first: int = 0, count: int | None = None,
                out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Device rows [n, samples] of interlaced frames (a window; uint8 at 8 bits, int16 / uint16 words at 10) -> the
    deinterlaced frames first .. first + count - 1 (default: to the end) as rows [count, samples], or [2 * count, samples]
    at rate "field" (row 2k + i from field i of frame first + k).  layout_or_planes: a `layout.Layout` or its planes
    [(name, offset, h, w, pitch, step)] (the name may be left out) in samples of a row.  The neighbours of a frame come
    from the window and clamp to its ends.  Samples of a row that belong to no plane are not written.  out: a contiguous
    tensor of the result's shape and the rows' dtype to write into.  On the rows' current stream (or the raw handle
    `stream`), without allocation when `out` is given and without synchronisation."""
    order, rate, method = check_options(order, rate, method)
    if frames.dim() != 2 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous [n, samples] tensor of tight frames")
    if _bits_of(frames) != bits:
        raise ValueError(f"bits={bits!r} does not match frames of {frames.dtype}")
    planes = _planes_of(layout_or_planes)
    n, row = frames.shape
    need = max(off + (h - 1) * pitch + (w - 1) * step + 1 for off, h, w, pitch, step in planes)
    if need > row:
        raise ValueError(f"the planes describe a frame of {need} samples, the rows have {row}")
    first = int(first)
    count = n - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > n:
        raise ValueError(f"first={first} and count={count} do not name frames of a window of {n}")
    n_out = count * (2 if rate == "field" else 1)
    if out is None:
        out = torch.empty((n_out, row), dtype=frames.dtype, device=frames.device)
    elif out.shape != (n_out, row) or out.dtype != frames.dtype or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"out must be a contiguous [{n_out}, {row}] {frames.dtype} tensor on the frames' device")
    if count:
        flags = METHODS[method] | (0 if spatial_check else _native.DEINT_NO_SPATIAL_CHECK)
        full = [p + (row,) for p in planes]
        for k in range(0, len(full), MAX_PLANES):
            _native.deinterlace(frames, n, full[k:k + MAX_PLANES], out, full[k:k + MAX_PLANES], first, count, ORDERS[order],
                                RATES[rate], flags, bits, stream)
    return out


def interlace(progressive: torch.Tensor, layout, order: str = "tff") -> torch.Tensor:
    """The inverse, in torch, for tests and scoring: a field-rate progressive clip of 2N rows [2N, samples] -> N interlaced
    frames; frame t takes the rows of the first field's parity of every plane from row 2t and the others from 2t + 1."""
    _choice("order", order, ORDERS)
    if progressive.dim() != 2 or progressive.shape[0] % 2:
        raise ValueError("progressive must be [2N, samples]: two progressive frames per interlaced frame")
    p = 1 if order == "bff" else 0
    a, b = progressive[0::2], progressive[1::2]
    out = a.clone()
    for off, h, w, pitch, step in _planes_of(layout):
        rows = torch.arange(1 - p, h, 2, device=progressive.device)
        idx = (off + rows[:, None] * pitch + torch.arange(w, device=progressive.device)[None, :] * step).reshape(-1)
        out[:, idx] = b[:, idx]
    return out


# ---- file to file -----------------------------------------------------------------------------------------------------
def _is_path(x) -> bool:
    return isinstance(x, (str, bytes, os.PathLike))


def order_of(order: str, interlace_tag, raw) -> str:
    """The field order of a run: `order` itself, or under "auto" what the Y4M header's `I` token says."""
    if order != "auto":
        return order
    if raw is not None:
        raise ValueError('order="auto" reads the field order off a Y4M header, and raw video has none: pass order="tff" '
                         'or order="bff"')
    if interlace_tag == "t":
        return "tff"
    if interlace_tag == "b":
        return "bff"
    if interlace_tag == "m":
        raise ValueError('the Y4M header says Im (mixed field orders), which order="auto" cannot follow: pass order="tff" '
                         'or order="bff" for the whole clip')
    said = "no field order" if interlace_tag is None else f"I{interlace_tag}" + (" (progressive)" if interlace_tag == "p" else "")
    raise ValueError(f'the Y4M header says {said}: if the frames are interlaced all the same, pass order="tff" (or "bff")')


def _fps_pair(fps) -> tuple[int, int]:
    """A rate as (num, den) ints, a Fraction (what `retime.parse_fps` gives) or a whole number -> (num, den)."""
    f = Fraction(int(fps[0]), int(fps[1])) if isinstance(fps, (tuple, list)) else Fraction(fps)
    if f <= 0:
        raise ValueError(f"src_fps must be positive, got {fps!r}")
    return f.numerator, f.denominator


def double_rate(fps) -> tuple[int, int]:
    """Twice the rate (num, den), as an exact fraction in lowest terms."""
    f = Fraction(2 * int(fps[0]), int(fps[1]))
    return f.numerator, f.denominator


def deinterlace_video(src, dst, order: str = "auto", rate: str = "field", method: str = "adaptive",
                      spatial_check: bool = True, chunk_frames: int = 32, raw=None, width=None, height=None, src_fps=None,
                      packing=None, device=None) -> int:
    """Deinterlace a clip of any length in memory bounded by the chunk -> the number of frames written.

    src / dst: a path or a binary file object (a pipe, `sys.stdin.buffer`).  Y4M (8 and 10 bits, every tag the readers
    take), or with raw= a name of `layout.RAW_FORMATS` headerless tight frames of width x height; packing= "v210" /
    "y210le" / "p210le" with raw="yuv422p10le": the frames are unpacked, deinterlaced and packed on the device.  The
    output has the input's format.  A Y4M result carries `Ip` and, at rate "field", twice the source rate as an exact
    fraction (src_fps overrides the header's).  order: "tff", "bff", or "auto" (the Y4M header's `It` / `Ib`; refused
    for `Ip`, `Im`, no token, and raw video).

    Each step uploads a window of chunk_frames + 2 source frames - one context frame either side - and carries two of
    them over to the next, so device and host memory depend on the chunk, not on the clip, and the bytes written are the
    same for every chunk_frames."""
    from . import stream as _stream
    order, rate, method = check_options(order, rate, method, auto=True)
    chunk = _stream.check_chunk_frames(chunk_frames)
    if raw is None and (width is not None or height is not None or packing is not None):
        raise ValueError("width, height and packing describe raw= video: a Y4M stream carries its own header")
    close_src = close_dst = None
    writer = wire = None
    try:
        if raw is None:
            reader = imageio_lite.Y4MReader(src)
            close_src = reader.close
            hdr = reader.header
            order = order_of(order, reader.interlace, None)
            lay = frame_layout(("y4m", hdr["colourspace"]), hdr["height"], hdr["width"])
            in_row = out_row = lay.samples
        else:
            if raw not in RAW_FORMATS:
                raise ValueError(f"raw must be one of {list(RAW_FORMATS)}, got {raw!r}")
            order = order_of(order, None, raw)
            if width is None or height is None:
                raise ValueError("raw video has no header: pass width and height")
            lay = frame_layout(raw, int(height), int(width))
            wire = _stream.check_packing(packing, raw, int(height), int(width))
            in_row = out_row = lay.samples if wire is None else wire.in_row
            hdr = None
        _planes_of(lay)   # (a plane of one row is refused before anything is opened for writing)
        ndtype = np.uint8 if lay.bits == 8 else np.dtype("<u2")
        row_bytes = in_row * np.dtype(ndtype).itemsize
        if raw is not None:
            if _is_path(src):
                if not os.path.exists(src):
                    raise FileNotFoundError(f"Video file not found: {src}")
                fin = open(src, "rb")
                close_src = fin.close
            else:
                fin = src
            reader = _stream._RawReader(fin, row_bytes)
        dev = torch.device("cuda" if device is None else device)
        if hdr is not None:
            fps = hdr["fps"] if src_fps is None else _fps_pair(src_fps)
            writer = imageio_lite.Y4MWriter(dst, hdr["width"], hdr["height"], double_rate(fps) if rate == "field" else fps,
                                            hdr["colourspace"], hdr["colour_range"], lay.bits)
            close_dst, write = writer.close, writer.write
        else:
            fout = open(dst, "wb") if _is_path(dst) else dst
            close_dst = fout.close if _is_path(dst) else fout.flush

            def write(rows):
                fout.write(memoryview(np.ascontiguousarray(rows)).cast("B"))

        buf = np.empty((chunk + 2, in_row), dtype=ndtype)
        have = reader.read_into(buf, chunk + 1)
        eof = have < chunk + 1
        lead, written = 0, 0
        while True:
            count = have - lead - (0 if eof else 1)   # the last frame of a window that goes on is context only
            if count > 0:
                d = torch.from_numpy(buf[:have].view(np.int16) if lay.bits == 10 else buf[:have]).to(dev)
                if wire is not None:
                    d = wire.unpack(d)
                res = deinterlace(d, lay, lay.bits, order, rate, method, spatial_check, first=lead, count=count)
                if wire is not None:
                    res = wire.pack(res)
                host = res.cpu().numpy()
                write(host.view(ndtype) if lay.bits == 10 else host)
                written += host.shape[0]
            if eof:
                break
            buf[0:2] = buf[have - 2:have].copy()   # the last frame done and the one behind it
            lead = 1
            got = reader.read_into(buf[2:], chunk)
            have, eof = 2 + got, got < chunk
        return written
    finally:
        for close in (close_src, close_dst):
            if close is not None:
                close()


# the helpers other modules build on (ivtc.py), under public names
choice, planes_of, bits_of, is_path, fps_pair = _choice, _planes_of, _bits_of, _is_path, _fps_pair

__all__ = ["ORDERS", "RATES", "METHODS", "MAX_PLANES", "deinterlace", "interlace", "deinterlace_video", "interlaced_warning",
           "order_of", "double_rate", "check_options", "choice", "planes_of", "bits_of", "is_path", "fps_pair"]
