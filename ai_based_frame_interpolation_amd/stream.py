"""The video routes: interpolate a clip of any length, from a file or a pipe, whole or in memory bounded by the chunk.

There is one implementation of each route (`_y4m_route`, `_npy_route`, `_raw_route`: what it computes, refuses and
writes; `row` and `bits` from the layout table, layout.py); `FrameInterpolator.interpolate_video` dispatches into the
three `interpolate_*_stream` functions here.  A source is opened in one place (`_open_y4m`, `_open_npy`, `_open_raw` ->
`_Opened`: every host-side check of the source, the route at the destination size, the reader, the resize, the packing,
`ingest` and `upload`), which hold-out scoring (holdout.py) uses too; `_job` turns a route's keyword arguments into the
`_Job` that the engines take as `_run(model, route, reader, write, job)` / `_run_whole(...)`.
"Resident" (chunk_frames=None) means one chunk: `_run_whole` holds the whole clip in host memory and on the device.
`_run` takes the same route chunk by chunk:

  chunk      `chunk_frames` input pairs plus the overlap frame it shares with the next chunk.  On the device each
             chunk runs the route's levels (`interpolate_sequence*`, `_interleave_average_*`, `_padded_chunk` inside
             them, `_hold`), one level per factor bit.  Every middle depends only on its two neighbours and
             `_padded_chunk` makes a pair's result independent of the pairs that share its call, so the output is byte
             for byte the whole-clip one for every chunk_frames >= 1.  The overlap frame is written once.
  scene cuts the two-sided score of interval i needs mafd[i-1] and mafd[i+1]: with `scene_cut` on, a chunk carries
             one lookahead frame and the previous chunk's last interval sum; `scene.score_window` scores the window
             (carried interval, the chunk's intervals, lookahead interval) and the chunk keeps its own flags, which
             equal `scene.detect_cuts` on the whole clip bit for bit.
  pipeline   a reader thread fills a ring of pinned input slots; H2D copies go on one copy stream, the chunk computes
             on the caller's stream, D2H copies of the result go into pinned output slots on a second copy stream, and
             a writer thread writes each slot once its event has completed.  Events order the streams (no device-wide
             synchronise per chunk); the host waits only for a slot it is about to reuse.

  fps        with `fps=` (retime.py) a chunk of c intervals starting at s builds its c x G + 1-frame
             grid as the factor = G run does (G = 2**time_depth), holds it, and `retime.resample` writes the frames of
             `plan.span(s, c, last)` from it: a time belongs to exactly one chunk, so the overlap frame is written
             once.  A clip that ends on a chunk's edge sends one more chunk of no intervals for its last frame.

  dedup      with `dedup=` (retime.py) a run always has a plan (without fps: p / q = 1 / factor).  A chunk
             reads max_gap - 1 lookahead frames (max_gap with scene_cut), computes `scene.pair_peak` on its rows, reads
             the dead (and cut) flags back - the one host read per chunk - and `retime.classify_chunk` finds its spans
             from them and a carried count of dead intervals.  A span across the chunk's end makes the grid longer by
             the lookahead intervals it needs; `retime.table_entries` turns the frames of `plan.span` into (row, wn,
             den) entries and `retime.resample_table` writes them.  In the sizes below C + 2 becomes C + 1 + max_gap
             and the output slots hold the frames of C + max_gap - 1 intervals (the last chunk; `_run`).

  shutter    with `shutter=` (retime.py) fps may be any rate, a lower one included.  A chunk reads
             ceil(shutter x p / q) lookahead frames (one more with scene_cut), and its grid goes on over the lookahead
             intervals that the windows of its own frames reach (`retime.shutter_reach`); a frame belongs to the chunk
             that holds its opening time, and a chunk without one (p > q) writes nothing.  `retime.shutter_entries` /
             `resample_shutter` write the frames; shutter 0 point-samples through `table_entries` / `resample_table`.
             With scene_cut the cut flags are read back once per chunk: the windows end at a cut.

Memory is bounded by the chunk, never by the clip (C = chunk_frames, F = factor, one frame of the input layout):
  host pinned    3 x (C + 2) input frames + 2 x (C x F + 1) output frames
  device         2 x (C + 2) input frames + one chunk's levels + the previous chunk's result (C x F + 1 frames of
                 the output layout; at factor 2 the levels are one result, at factor F about 2 x (C x F + 1) frames)
Raw video (`interpolate_raw_stream`): headerless tight NV12 frames, what `ffmpeg -f rawvideo -pix_fmt
nv12` writes and reads, through the same engine with `interpolate_sequence_nv12` as the level: factor, fps, scene_cut
and chunk_frames work as they do for Y4M (the retime and hold kernels see packed rows of samples, whatever their order).
The packed RGB formats rgb24 / bgr24 / rgba / bgra take the same route with
`interpolate_sequence_rgb_packed` as the level and no colour conversion.  The 4:2:2 / 4:4:4 formats yuv422p, yuv444p,
yuv422p10le, yuv444p10le, uyvy422 and yuyv422 take it with `interpolate_sequence_yuv` as the level; the
10-bit ones are two bytes per sample on the wire (little-endian words) and int16 words in the rings.

With `fps=` (source / target rate = p / q, G = 2**time_depth) F is G in the levels, a chunk's result is its
R = ceil(C x q / p) + 1 resampled frames, and the device holds them beside the grid:
  host pinned    3 x (C + 2) input frames + 2 x R output frames
  device         2 x (C + 2) input frames + one chunk's levels (about 2 x (C x G + 1) frames) + 2 x R output frames

With `resize=` (resize.py) the reader, the pinned input slots and their device twins hold frames of the
SOURCE size; a chunk is resized once, right after its upload, into a tensor of its own, and scene cuts, dedup, the route
and everything after them see frames of the DESTINATION size only:
  host pinned    3 x (C + 2) source frames + 2 x (C x F + 1) destination frames
  device         2 x (C + 2) source frames + (C + 2) destination frames (the resized chunk, until its levels have run)
                 + one chunk's levels + the previous chunk's result, all at the destination size
A resident run (`_run_whole`) uploads and resizes 64 frames at a time: the device holds the whole clip at the destination
size and 64 frames at the source size.

With `packing=` (wire10.py; raw "yuv422p10le" only) the reader, the pinned slots and their device twins
hold v210 / y210le / p210le frames (`_Wire`): a chunk is unpacked once, right after its upload and before the resize,
into yuv422p10le rows in a tensor of its own, and the rows about to be downloaded are packed into a device twin of
their pinned output slot.  Everything between is the yuv422p10le route, so the output is that route's output packed:
  host pinned    3 x (C + 2) wire frames in + 2 x (C x F + 1) wire frames out
  device         2 x (C + 2) wire frames + (C + 2) working frames (the unpacked chunk, until its levels have run) + one
                 chunk's levels + the previous chunk's result + 2 x (C x F + 1) wire frames out

With retime="motion" (retime.py) every resampled frame between two grid rows is warped along the flow
between them, after the blend pass and into the same output rows: the planes come from the source's layout (the
destination size, the working format), flows are computed `batch` pairs at a time, and the device holds beside the grid
  device         2 x batch lead planes + batch flow fields (8 bytes a lead sample each) + the flow workspace of batch
                 pairs (21 fp32 planes a pair, `fiunet_flow_workspace_bytes`), kept per frame size

With chroma="motion" (chroma.py; Y4M through the grayscale network) a level holds beside its luma result
  device         the level's chroma stack (2 chroma planes a frame) + batch flow fields + batch pick maps (a byte per 8x8
                 luma block) + the flow workspace of batch pairs
"""
from __future__ import annotations

import dataclasses
import numbers
import os
import queue
import stat
import threading

import numpy as np
import torch

from . import chroma as _chroma
from . import deinterlace as _deinterlace
from . import colour, imageio_lite, packed, scene, wire10
from . import resize as _resize
from . import retime as _retime
from .layout import RAW_FORMATS, frame_layout
from . import optical_flow as _flow
from .inference import (_hold, _interleave_average_p10, _interleave_average_u8, _pair_batches, interpolate_sequence,
                        interpolate_sequence_nv12, interpolate_sequence_p10, interpolate_sequence_rgb_packed,
                        interpolate_sequence_yuv, interpolate_sequence_yuv420, interpolate_sequence_yuv420p10)

R_IN, R_OUT = 3, 2   # pinned input / output slots in the rings


# ---- argument checks (host only: nothing here touches the device) ---------------------------------------------------
def check_chunk_frames(chunk_frames) -> int:
    if isinstance(chunk_frames, bool) or not isinstance(chunk_frames, numbers.Integral) or chunk_frames < 1:
        raise ValueError(f"chunk_frames must be a positive int, got {chunk_frames!r}")
    return int(chunk_frames)


def _check_common(factor, batch, chunk_frames, scene_cut):
    """chunk_frames None (the whole clip as one chunk, `_run_whole`) passes as None."""
    thr = scene.check_threshold(scene_cut)
    if isinstance(factor, bool) or not isinstance(factor, numbers.Integral) or factor < 2 or factor & (factor - 1):
        raise ValueError("factor must be a power of two (the network has no time input)")
    if isinstance(batch, bool) or not isinstance(batch, numbers.Integral) or batch < 1:
        raise ValueError(f"batch must be a positive int, got {batch!r}")
    return thr, None if chunk_frames is None else check_chunk_frames(chunk_frames)


def check_retime(fps, src_fps, time_depth, retime, factor):
    """The checks of the frame-rate keywords that need no source: -> (fps Fraction or None, src_fps Fraction or None,
    time_depth, retime).  With `fps`, `factor` must be left at 2."""
    depth, mode = _retime.check_time_depth(time_depth), _retime.check_mode(retime)
    if fps is None:
        return None, None, depth, mode
    if factor != 2:
        raise ValueError(f"fps and factor are two ways to say how many frames to make: with fps={fps!r} leave factor "
                         f"at 2 (got factor={factor!r}); time_depth sets the bisection depth")
    return _retime.parse_fps(fps), None if src_fps is None else _retime.parse_fps(src_fps), depth, mode


def _is_path(x) -> bool:
    return isinstance(x, (str, os.PathLike))


def _levels(factor: int) -> int:
    return factor.bit_length() - 1


# ---- routes: one chunk [k, row] of input frames -> [(k-1) x factor + 1, out_row] output rows on the device -----------
class _Route:
    """bits: sample depth (8: uint8 rows; 10: int16 words of 10-bit codes on the device, uint16 on the host); row /
    out_row: samples per input / output frame; run(d, factor): the levels of one chunk (the whole clip is one chunk)."""

    def __init__(self, bits, row, out_row, run):
        self.bits, self.row, self.out_row, self.run = bits, row, out_row, run
        self.tdtype = torch.uint8 if bits == 8 else torch.int16
        self.ndtype = np.uint8 if bits == 8 else np.uint16


def _y4m_route(model, hdr, npy_out: bool, batch: int, matrix, siting, chroma: str = "average") -> _Route:
    """The route of Y4M video for this stream header and model, with its refusals and messages: the RGB network on
    4:2:0 frames (8-bit: siting from the tag; `C420p10`: siting None is "mpeg2"; range from `XCOLORRANGE`), or the
    grayscale network on the luma plane with the chroma of an inserted frame the rounded average of its neighbours'
    (chroma "average") or carried along the motion where the network's luma confirms it (chroma "motion": chroma.py,
    DESIGN.md 3.3u; the route's `chroma_stats` then counts the blocks that were warped)."""
    h, w, (hc, wc) = hdr["height"], hdr["width"], hdr["chroma"]
    if model.frame_channels == 3:
        _chroma.refuse_motion(chroma, "the RGB network (its colour goes through the network itself)")
    else:
        _chroma.check_mode(chroma)
    _, _, bits, row = frame_layout(("y4m", hdr["colourspace"]), h, w)
    ny, nc = h * w, hc * wc
    if model.frame_channels == 3:
        rng = "full" if hdr["colour_range"] == "FULL" else "limited"
        if bits == 10:
            if hdr["colourspace"] != "420p10":
                raise ValueError(f"Y4M colourspace C{hdr['colourspace']} is not supported by the RGB network: it "
                                 "reads 10-bit 4:2:0 video tagged C420p10")
            if npy_out:
                raise ValueError("colour Y4M video through the RGB network is written as .y4m (no .npy output)")
            opts = dict(siting="mpeg2" if siting is None else siting, matrix=matrix, colour_range=rng)
            colour.colour_flags(**opts, bits=10)

            def run(d, factor):
                t = d.view(torch.uint16)
                for _ in range(_levels(factor)):
                    t = interpolate_sequence_yuv420p10(model, t, h, w, batch, **opts)
                return t.view(torch.int16)
            return _Route(10, row, row, run)
        if npy_out:
            raise ValueError("colour Y4M video through the RGB network is written as .y4m (no .npy output)")
        tag_siting = colour.siting_of_y4m(hdr["colourspace"])
        opts = dict(siting=tag_siting if siting is None else siting, matrix=matrix, colour_range=rng)
        colour.colour_flags(**opts)

        def run(d, factor):
            for _ in range(_levels(factor)):
                d = interpolate_sequence_yuv420(model, d, h, w, batch, **opts)
            return d
        return _Route(8, row, row, run)
    if model.frame_channels != 1:
        raise ValueError("Y4M video goes through the grayscale (2->1) network")
    out_row = ny if npy_out else row

    def run(d, factor):
        k = d.shape[0]
        y = d[:, :ny].reshape(k, h, w).contiguous()
        cu = cv = None
        if nc:
            cu, cv = (d[:, ny + i * nc:ny + (i + 1) * nc].reshape(k, hc, wc) for i in (0, 1))
            if bits == 10:   # 10-bit chroma is averaged in int32: the 16-bit words as unsigned samples
                cu, cv = ((c.to(torch.int32) & 0xFFFF) for c in (cu, cv))
            else:
                cu, cv = cu.contiguous(), cv.contiguous()
        if bits == 10:
            y = y.view(torch.uint16)
        for _ in range(_levels(factor)):
            if bits == 10:
                y = interpolate_sequence_p10(model, y, batch)
                if cu is not None:
                    cu, cv = (_interleave_average_p10(c) for c in (cu, cv))
            else:
                y = interpolate_sequence(model, y, batch)
                if cu is not None:
                    cu, cv = (_interleave_average_u8(c) for c in (cu, cv))
        n = y.shape[0]
        y = (y.view(torch.int16) if bits == 10 else y).reshape(n, ny)
        if npy_out or cu is None:
            return y
        return torch.cat([y] + [c.to(y.dtype).reshape(n, nc) for c in (cu, cv)], dim=1)
    if chroma != "motion" or not nc or npy_out:   # (a mono stream has no chroma, a luma .npy output writes none)
        return _Route(bits, row, out_row, run)
    sub = _chroma.subsampling((h, w), (hc, wc))
    stats = {"warped": None, "blocks": 0}

    def run_motion(d, factor):
        # luma: the frames of `run`.  Chroma: U and V of a frame side by side, [k, 2, hc, wc], as they are stored; at
        # each level the flows of the stored pairs, `batch` at a time (a pair's flow does not depend on its batch),
        # the pick from (y[k], y[k + 1], y'[2k + 1]) where the level's result holds them, and the fill of u and v
        y = d[:, :ny].reshape(d.shape[0], h, w).contiguous()
        c = d[:, ny:ny + 2 * nc].reshape(d.shape[0], 2, hc, wc).contiguous()
        if bits == 10:
            y = y.view(torch.uint16)
        for _ in range(_levels(factor)):
            k = y.shape[0]
            y2 = interpolate_sequence_p10(model, y, batch) if bits == 10 else interpolate_sequence(model, y, batch)
            c2 = torch.empty((2 * k - 1, 2, hc, wc), dtype=c.dtype, device=c.device)
            c2[0::2] = c
            for s, cnt in _pair_batches(k - 1, batch):
                ya, yb, ym = (y2[2 * s + o:2 * (s + cnt) + o:2] for o in (0, 2, 1))
                field = _flow.farneback_flow(ya, yb, "hip", bits=bits)
                pk = _chroma.pick(ya, yb, ym, field, bits)
                _chroma.fill(c[s:s + cnt], c[s + 1:s + cnt + 1], field, pk, c2[2 * s + 1:2 * (s + cnt):2], bits, sub=sub)
                warped = pk.sum(dtype=torch.int64)
                stats["warped"] = warped if stats["warped"] is None else stats["warped"] + warped
                stats["blocks"] += pk.numel()
            y, c = y2, c2
        n = y.shape[0]
        y = (y.view(torch.int16) if bits == 10 else y).reshape(n, ny)
        return torch.cat([y, c.reshape(n, 2 * nc)], dim=1)
    route = _Route(bits, row, out_row, run_motion)
    route.chroma_stats = stats
    return route


def _raw_route(model, raw, height, width, npy_out: bool, batch: int, matrix, siting) -> _Route:
    """The route of headerless raw video (`raw`: one of RAW_FORMATS, tight frames), with its refusals.  Nothing in the
    stream says how it was made: for "nv12" siting None is "mpeg2" (what decoders produce) and the range is limited.
    The packed RGB formats (packed.FORMATS) have no colour conversion: matrix and siting are not used.
    The 4:2:2 / 4:4:4 formats (colour.YUV_FORMATS) take matrix and siting as "nv12" does; the 10-bit ones
    give a 10-bit route, whose `row` counts 16-bit samples."""
    if raw not in RAW_FORMATS:
        raise ValueError(f"raw must be one of {list(RAW_FORMATS)} (or None: Y4M / .npy), got {raw!r}")
    for name, v in (("height", height), ("width", width)):
        if v is None:
            raise ValueError(f"raw {raw} video has no header: pass width and height (missing: {name})")
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
            raise ValueError(f"{name} must be a positive int, got {v!r}")
    if model.frame_channels != 3:
        raise ValueError(f"raw {raw} video goes through the RGB (6->3) network; this model is grayscale")
    if npy_out:
        raise ValueError(f"raw {raw} video through the RGB network is written as raw {raw} (no .npy output)")
    h, w = int(height), int(width)
    _, _, bits, row = frame_layout(raw, h, w)   # (refuses an odd width of uyvy422 / yuyv422)
    if raw in packed.FORMATS:
        def run_packed(d, factor):
            for _ in range(_levels(factor)):
                d = interpolate_sequence_rgb_packed(model, d, h, w, raw, batch)
            return d
        return _Route(8, row, row, run_packed)
    if raw in colour.YUV_FORMATS:
        opts = dict(siting=siting, matrix=matrix, colour_range="limited")
        colour.yuv_flags(raw, **opts)

        def run_yuv(d, factor):
            t = d.view(torch.uint16) if bits == 10 else d
            for _ in range(_levels(factor)):
                t = interpolate_sequence_yuv(model, t, h, w, raw, batch, **opts)
            return t.view(torch.int16) if bits == 10 else t
        return _Route(bits, row, row, run_yuv)
    opts = dict(siting="mpeg2" if siting is None else siting, matrix=matrix, colour_range="limited")
    colour.colour_flags(**opts)

    def run(d, factor):
        for _ in range(_levels(factor)):
            d = interpolate_sequence_nv12(model, d, h, w, batch, **opts)
        return d
    return _Route(8, row, row, run)


class _RawReader:
    """`read_into` over headerless frames of `row` bytes from a binary file object (Y4MReader's interface).  A stream
    that ends inside a frame is an error at that point.  row: BYTES per frame on the wire (a 10-bit route's
    samples x 2: little-endian words, what the rings' uint16 rows hold on a little-endian host)."""

    def __init__(self, f, row: int):
        self.f, self.row, self.frames = f, row, 0

    def read_into(self, buf: np.ndarray, max_frames: int) -> int:
        flat = memoryview(buf).cast("B")
        k = 0
        while k < max_frames:
            got, frame = 0, flat[k * self.row:(k + 1) * self.row]
            while got < self.row:   # a pipe hands over what it has
                n = self.f.readinto(frame[got:])
                if not n:
                    break
                got += n
            if got == 0:
                break
            if got < self.row:
                raise ValueError(f"the raw stream ends inside a frame ({got} of {self.row} bytes of frame "
                                 f"{self.frames + k})")
            k += 1
        self.frames += k
        return k


class _Wire:
    """A 10-bit 4:2:2 wire packing around the yuv422p10le raw route (wire10.py): the reader, the pinned
    slots and their device twins hold `packing` frames - in_row int16 words a source frame, out_row an output frame (the
    size after `resize=`) - and `unpack` / `pack` move a chunk between them and the rows of the working format, which
    is all that resize, scene cuts, dedup, the route and the retime kernels see."""

    def __init__(self, packing: str, height: int, width: int, out_height: int, out_width: int):
        self.packing, self.src, self.dst = packing, (int(height), int(width)), (int(out_height), int(out_width))
        self.in_row = wire10.frame_bytes(packing, *self.src) // 2    # (refuses an odd width of v210 / y210le)
        self.out_row = wire10.frame_bytes(packing, *self.dst) // 2

    def unpack(self, d: torch.Tensor) -> torch.Tensor:
        """int16 [k, in_row] wire frames -> int16 [k, samples] working rows in a tensor of their own."""
        out = torch.empty((d.shape[0], wire10.planar_samples(*self.src)), dtype=torch.int16, device=d.device)
        return wire10.unpack(d, *self.src, self.packing, out=out)

    def pack(self, rows: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """int16 [k, samples] working rows of the output size -> int16 [k, out_row] wire frames (`out`, or a new tensor)."""
        if out is None:
            out = torch.empty((rows.shape[0], self.out_row), dtype=torch.int16, device=rows.device)
        return wire10.pack(rows, *self.dst, self.packing, out=out)


def check_packing(packing, raw, height=None, width=None, size=None):
    """The host checks of `packing` (None passes as None) -> a `_Wire` for `raw` video of height x width written at `size`
    = (width, height) or None: packing describes yuv422p10le samples only, is one of wire10.PACKINGS, and v210 / y210le
    need an even width at both sizes."""
    if packing is None:
        return None
    if raw != wire10.WORKING_FORMAT:
        raise ValueError(f"packing={packing!r} says how {wire10.WORKING_FORMAT} samples are packed on the wire: pass "
                         f"raw=\"{wire10.WORKING_FORMAT}\" with it (got raw={raw!r}; Y4M and .npy video take no packing)")
    if packing not in wire10.PACKINGS:
        raise ValueError(f"packing must be one of {list(wire10.PACKINGS)} (or None), got {packing!r}")
    oh, ow = (height, width) if size is None else (size[1], size[0])
    return _Wire(packing, height, width, oh, ow)


def _npy_route(model, shape, batch: int) -> _Route:
    """The .npy route for uint8 frames of `shape` ([H,W] or [H,W,C])."""
    row = int(np.prod(shape))
    if len(shape) == 2:
        h, w = shape

        def run(d, factor):
            t = d.reshape(d.shape[0], h, w)
            for _ in range(_levels(factor)):
                t = interpolate_sequence(model, t, batch)
            return t.reshape(t.shape[0], row)
        return _Route(8, row, row, run)
    h, w, c = shape

    def run(d, factor):
        k = d.shape[0]
        t = d.reshape(k, h, w, c).permute(0, 3, 1, 2).contiguous()
        if model.frame_channels == 1:   # per-channel application of the 2->1 network
            t = t.permute(1, 0, 2, 3).reshape(c * k, h, w)
            outs = []
            for ci in range(c):
                seq = t[ci * k:(ci + 1) * k]
                for _ in range(_levels(factor)):
                    seq = interpolate_sequence(model, seq, batch)
                outs.append(seq)
            res = torch.stack(outs, dim=-1)
        else:
            for _ in range(_levels(factor)):
                t = interpolate_sequence(model, t, batch)
            res = t.permute(0, 2, 3, 1).contiguous()
        return res.reshape(res.shape[0], row)
    return _Route(8, row, row, run)


# ---- sources and sinks over .npy files --------------------------------------------------------------------------
class _NpyRows:
    """`read_into` over the rows of a memory-mapped .npy stack (Y4MReader's interface)."""

    def __init__(self, mm: np.ndarray):
        self.mm, self.pos = mm, 0

    def read_into(self, buf: np.ndarray, max_frames: int) -> int:
        k = min(int(max_frames), self.mm.shape[0] - self.pos)
        if k > 0:
            buf[:k] = self.mm[self.pos:self.pos + k].reshape(k, -1)
            self.pos += k
        return max(k, 0)


class _NpyWriter:
    """`write` of output rows into a .npy file made by `np.lib.format.open_memmap` (the header np.save writes), at
    `<path>.part` until `close(ok)` renames it (or removes it)."""

    def __init__(self, path, dtype, shape):
        self.path, self.part = path, path + ".part"
        self.mm = np.lib.format.open_memmap(self.part, mode="w+", dtype=dtype, shape=tuple(shape))
        self.pos = 0

    def write(self, rows: np.ndarray) -> None:
        k = rows.shape[0]
        self.mm[self.pos:self.pos + k] = rows.reshape((k,) + self.mm.shape[1:])
        self.pos += k

    def close(self, ok: bool) -> None:
        self.mm.flush()
        del self.mm
        if ok:
            os.replace(self.part, self.path)
        else:
            os.remove(self.part)


# ---- opened sources: every host-side check of a source, no GPU work ----------------------------------------------------
class _Opened:
    """An opened video source, what the video routes and hold-out scoring (holdout.py) run on.  route: the route at the
    destination size; reader: `read_into` over frames as they are on the wire; rs: None or the `resize.FrameResize` from
    the source size; wire: None or the `_Wire` of the packing; layout: the `layout.Layout` of a route frame (the
    destination size, the working format); row / out_row: samples per frame as read / as written; count: the frame
    count where it is known up front (a regular file), else None; header: the Y4M header at the destination size (else
    None) and fps its rate; shape: the destination shape of a .npy frame (else None); close(): releases the source."""

    def __init__(self, route, reader, layout, rs=None, wire=None, count=None, header=None, shape=None, close=None):
        self.route, self.reader, self.layout, self.rs, self.wire = route, reader, layout, rs, wire
        self.count, self.header, self.shape = count, header, shape
        self.fps = None if header is None else header["fps"]
        self.close = close or (lambda: None)
        self.row = wire.in_row if wire is not None else route.row if rs is None else rs.row
        self.out_row = route.out_row if wire is None else wire.out_row

    def ingest(self, d: torch.Tensor) -> torch.Tensor:
        """Device frames as read [k, row] -> the route's rows [k, route.row]: unpacked, then resized, each into a tensor
        of its own (neither: `d` itself)."""
        if self.wire is not None:
            d = self.wire.unpack(d)
        return d if self.rs is None else self.rs(d)

    def upload(self, a: np.ndarray, device) -> torch.Tensor:
        """Host frames as read -> the route's rows on `device` (10 bits: the uint16 words as int16)."""
        return self.ingest(torch.from_numpy(a.view(np.int16) if self.route.bits == 10 else a).to(device))


def _is_file(src) -> bool:
    return _is_path(src) and stat.S_ISREG(os.stat(src).st_mode)


def _resized(kind, height, width, size, rfilter):
    """-> (None or the `resize.FrameResize` of tight `kind` frames of height x width to `size` = (width, height), the
    layout at the size that results)."""
    lay = frame_layout(kind, height, width)
    if size is None:
        return None, lay
    dst = frame_layout(kind, size[1], size[0])
    return _resize.FrameResize(lay.planes, dst.planes, lay.bits, size, (int(width), int(height)), rfilter), dst


def _open_y4m(model, src, npy_out: bool, batch, matrix, siting, size, rfilter, count: bool,
              chroma: str = "average") -> _Opened:
    """Y4M from a path or a readable binary file.  count: whether the frames of a regular file are counted (one pass
    over its FRAME lines)."""
    if npy_out and not _is_file(src):
        raise ValueError("a .npy output needs the frame count up front, and a Y4M stream from a pipe cannot be "
                         "counted before it is read: write Y4M, or read the stream from a regular file")
    reader = imageio_lite.Y4MReader(src)
    try:
        _deinterlace.interlaced_warning(reader.interlace, "video")   # (the frames go on as they are)
        hdr = reader.header
        rs, lay = _resized(("y4m", hdr["colourspace"]), hdr["height"], hdr["width"], size, rfilter)
        if size is not None:   # everything from here on is a clip of the new size; the reader keeps the source's
            hdr = _resize.y4m_header_at(hdr, size)
        route = _y4m_route(model, hdr, npy_out, batch, matrix, siting, chroma)
        n = imageio_lite.y4m_frame_count(src) if count and _is_file(src) else None
    except BaseException:
        reader.close()
        raise
    return _Opened(route, reader, lay, rs, count=n, header=hdr, close=reader.close)


def _open_npy(model, src, batch, size, rfilter) -> _Opened:
    """A uint8 .npy stack [N,H,W] or [N,H,W,C], memory-mapped."""
    mm = np.load(src, mmap_mode="r")
    if mm.dtype != np.uint8 or mm.ndim not in (3, 4):
        raise ValueError("expected a uint8 .npy stack [N,H,W] or [N,H,W,3]")
    shape = tuple(mm.shape[1:])
    rs, lay = _resized("npy" if len(shape) == 2 else ("npy", shape[2]), shape[0], shape[1], size, rfilter)
    if size is not None:
        shape = (size[1], size[0]) + shape[2:]
    return _Opened(_npy_route(model, shape, batch), _NpyRows(mm), lay, rs, count=mm.shape[0], shape=shape)


def _open_raw(model, src, raw, width, height, npy_out: bool, batch, matrix, siting, size, rfilter, packing) -> _Opened:
    """Headerless tight `raw` frames (or, with `packing`, wire frames) of height x width from a path or a readable binary
    file; a regular file must hold a whole number of them."""
    route = _raw_route(model, raw, height, width, npy_out, batch, matrix, siting)
    wire = check_packing(packing, raw, height, width, size)
    wire_row = route.row * np.dtype(route.ndtype).itemsize   # bytes per frame on the wire: the source's
    if wire is not None:
        wire_row = 2 * wire.in_row
    rs, lay = _resized(raw, height, width, size, rfilter)
    if size is not None:
        route = _raw_route(model, raw, size[1], size[0], npy_out, batch, matrix, siting)
    count = None
    if _is_path(src):
        if not os.path.exists(src):
            raise FileNotFoundError(f"Video file not found: {src}")
        st = os.stat(src)
        if stat.S_ISREG(st.st_mode):
            if st.st_size % wire_row:
                raise ValueError(f"{os.fspath(src)}: {st.st_size} bytes is not a whole number of {width}x{height} "
                                 f"{raw if wire is None else packing} frames of {wire_row} bytes")
            count = st.st_size // wire_row
    fin = open(src, "rb") if _is_path(src) else src
    return _Opened(route, _RawReader(fin, wire_row), lay, rs, wire, count, close=fin.close if _is_path(src) else None)


# ---- the engine ---------------------------------------------------------------------------------------------------
class _Failure:
    def __init__(self):
        self.exc = None
        self.stop = threading.Event()

    def set(self, exc):
        if self.exc is None:
            self.exc = exc
        self.stop.set()

    def get(self, q: queue.Queue):
        """q.get() that gives up once another thread has failed."""
        while True:
            try:
                return q.get(timeout=0.05)
            except queue.Empty:
                if self.stop.is_set():
                    raise _Stopped()


class _Stopped(Exception):
    pass


def check_dedup(dedup, max_gap, fps, factor):
    """The checks of `dedup` / `max_gap` that need no source -> (the tolerance or None, max_gap)."""
    tol, gap = _retime.check_dedup(dedup, max_gap)
    if tol is not None and fps is None:
        _retime.dedup_plan(None, factor, gap)   # (refuses factor > 16)
    return tol, gap


def _dedup_of(tol, gap, plan, factor):
    """-> (the plan of the run, None or (dead limit, max_gap)): with dedup a run always has a plan."""
    if tol is None:
        return plan, None
    return _retime.dedup_plan(plan, factor, gap), (_retime.dead_limit(tol), gap)


def _dead_and_cuts(d, bits, limit, cut_flags):
    """One device-to-host read: -> (peaks on the device, dead flags, cut flags or None as host bool arrays) of the
    intervals of the device frames `d`; cut_flags: their uint8 device flags or None."""
    peaks = scene.pair_peak([d], bits)
    dead = (peaks <= limit).to(torch.uint8)
    if cut_flags is None:
        return peaks, dead.cpu().numpy().astype(bool), None
    host = torch.stack([dead, cut_flags]).cpu().numpy().astype(bool)
    return peaks, host[0], host[1]


@dataclasses.dataclass
class _Job:
    """What a run is asked to do, beside (model, route, reader, write): the engines' fifth argument.  source: the
    `_Opened` source (`ingest`, `row`, `out_row`, `count`, `wire`); factor: the frames per interval of the levels (with
    fps: the plan's G); chunk_frames: None for a resident run; thr: the scene-cut threshold or None; plan: None or a
    `retime.Plan`: each chunk's grid is resampled to the plan's frames; mode: the retime mode; dd: None or (dead limit,
    max_gap), with a plan: repeated frames are re-timed (retime.py); rate: the output's frame rate (n, d)
    where the source's header carries one; scene_log / dedup_log: None or the lists that receive each chunk's arrays."""
    source: _Opened
    factor: int
    chunk_frames: int | None = None
    thr: float | None = None
    plan: object = None
    mode: str = "blend"
    dd: tuple | None = None
    rate: tuple | None = None
    scene_log: list | None = None
    dedup_log: list | None = None
    batch: int = 8
    shutter: object = None   # None, or the checked shutter (a Fraction in [0, 1]): any rate, retime.py / DESIGN.md 3.3y


def check_shutter(shutter, fps, retime, dedup):
    """The checks of `shutter` that need no source -> None or the shutter as a Fraction.  With a shutter, fps is
    required and may be any positive rate; dedup is refused; a shutter above 0 needs retime "blend"."""
    s = _retime.check_shutter(shutter)
    if s is None:
        return None
    if fps is None:
        raise ValueError(f"shutter={shutter!r} says how a frame of the new rate is exposed: pass fps with shutter")
    if dedup is not None:
        raise ValueError(f"shutter={shutter!r} and dedup={dedup!r} do not go together: re-time the repeated frames "
                         "first, then convert the result with shutter")
    if s > 0 and retime != "blend":
        raise ValueError(f'a shutter above 0 averages the frames of retime="blend": got retime={retime!r} with '
                         f'shutter={shutter!r} (shutter=0, point sampling, takes every retime)')
    return s


def _shutter_frames(job: "_Job", grid, first: int, n_own: int, ext: int, j0: int, nj: int, cuts, clip_last, out=None):
    """The frames j0 .. j0 + nj - 1 of a run with a shutter from `grid`, which covers intervals first .. first + n_own +
    ext: the synthesized exposure, or for shutter 0 the point samples of `retime.table_entries` (cuts: host truth values
    of the grid's intervals or None; clip_last: the clip's last frame number where the chunk is the last)."""
    plan, bits = job.plan, job.source.route.bits
    if job.shutter > 0:
        entries = _retime.shutter_entries(plan, job.shutter, first, j0, nj, n_own + ext, cuts, clip_last)
        return _retime.resample_shutter(grid, entries, bits, out=out)
    entries = _retime.table_entries(plan, [], first, j0, nj, n_own, "blend" if job.mode == "motion" else job.mode, cuts)
    return _retime.resample_table(grid, entries, bits, out=out, mode=job.mode, **_retime_opts(job))


def _retime_opts(job: "_Job") -> dict:
    """The keywords `retime.resample` / `resample_table` take beside the mode: nothing, or for "motion" the layout of an
    output row (the source's; a luma-only .npy output of Y4M: its luma plane alone) and the pairs per flow call."""
    if job.mode != "motion":
        return {}
    lay, row = job.source.layout, job.source.route.out_row
    if lay.samples != row:
        planes = [p for p in lay.planes if p[1] + (p[2] - 1) * p[4] + (p[3] - 1) * p[5] + 1 <= row]
        lay = type(lay)(planes, [], lay.bits, row)
    return dict(layout=lay, batch=job.batch)


def check_motion_layout(lay, what) -> None:
    """ValueError where samples of a tight frame belong to no plane of its layout, or to two: retime "motion" warps
    plane by plane, and would leave such samples blended."""
    seen = np.zeros(lay.samples, dtype=np.uint8)
    for _, off, h, w, pitch, step in lay.planes:
        idx = off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :] * step
        np.add.at(seen, idx.ravel(), 1)
    if not (seen == 1).all():
        raise ValueError(f'retime="motion" is not available for {what}: {int((seen != 1).sum())} samples of a frame '
                         "belong to no plane of its layout, or to more than one")


@torch.no_grad()
def _run(model, route: _Route, reader, write, job: _Job) -> int:
    """Stream `reader` through `route` into `write(rows)` as `job` says; returns the number of output frames.  The
    reader, the pinned input slots and their device twins hold frames as read (source.row samples: the source size, the
    packing); each chunk goes through `source.ingest` once, right after its upload, into rows of route.row samples, which
    is all that scene cuts, dedup and the route see.  With a packing the rows about to be downloaded are packed into the
    device twin of their output slot.

    Sizes.  A chunk is read with `look` lookahead frames behind its C + 1 own: 0, 1 with scene_cut; with dd max_gap - 1,
    and max_gap with scene_cut too; with a shutter ceil(shutter x p / q) more.
    A read that comes up short of C + 1 + look frames is the clip's last chunk, and
    holds whatever is left: up to C + look - 1 intervals (C when look is 0 or 1).  `tail` is that bound, and the
    pinned output slots and their device twins are sized for it; the pinned input slots and the device input twins
    hold C + 1 + look frames, and the reader carries 1 + look of them over.  (C = 1, max_gap 4: 5 frames per read, 4
    carried; a clip of 4 frames is one last chunk of 3 intervals, one of 5 a chunk of 1 interval and a last of 3.)"""
    dev = next(model.parameters()).device
    source, factor, thr, plan, mode, dd = job.source, job.factor, job.thr, job.plan, job.mode, job.dd
    scene_log, dedup_log, wire = job.scene_log, job.dedup_log, source.wire
    motion, table_mode = _retime_opts(job), "blend" if mode == "motion" else mode
    C, look = job.chunk_frames, 1 if thr is not None else 0
    if dd is not None:
        look = dd[1] if thr is not None else dd[1] - 1
    sh = job.shutter
    if sh is not None:   # the frames its windows can reach, and with scene_cut one more: the last flag read is not used
        look += _retime.shutter_lookahead(plan, sh)
    tail = C + max(look - 1, 0)
    in_rows, out_rows = C + 1 + look, tail * factor + 1
    if plan is not None:
        out_rows = -(-tail * plan.q // plan.p) + 1
    src_row, dst_row = source.row, source.out_row
    in_slots = [torch.empty((in_rows, src_row), dtype=route.tdtype).pin_memory() for _ in range(R_IN)]
    out_slots = [torch.empty((out_rows, dst_row), dtype=route.tdtype).pin_memory() for _ in range(R_OUT)]
    in_np = [s.numpy().view(route.ndtype) for s in in_slots]
    out_np = [s.numpy().view(route.ndtype) for s in out_slots]
    free_in, filled, free_out, done = queue.Queue(), queue.Queue(), queue.Queue(), queue.Queue()
    for i in range(R_IN):
        free_in.put(i)
    for i in range(R_OUT):
        free_out.put(i)
    fail = _Failure()

    def reader_main():
        try:
            s, carry, prev, prev_m = 0, 0, None, 0
            while True:
                i = fail.get(free_in)
                buf = in_np[i]
                if carry:   # the overlap frame (and the lookahead frame) of the previous chunk
                    buf[:carry] = in_np[prev][prev_m - carry:prev_m]
                m = carry + reader.read_into(buf[carry:], in_rows - carry)
                if m == in_rows:
                    filled.put((i, s, m, C, False))
                    s, carry, prev, prev_m = s + C, 1 + look, i, m
                    continue
                if m == 0:
                    raise ValueError("no frames to interpolate")
                # the last chunk (a one-frame clip is one chunk without pairs; with a plan, so is the last frame of a
                # clip that ended on the previous chunk's edge)
                if m > 1 or s == 0 or plan is not None:
                    filled.put((i, s, m, m - 1, True))
                filled.put(None)
                return
        except _Stopped:
            pass
        except BaseException as e:  # noqa: BLE001 - re-raised by the main thread
            fail.set(e)

    def writer_main():
        try:
            while True:
                item = fail.get(done)
                if item is None:
                    return
                o, n, ev = item
                ev.synchronize()
                write(out_np[o][:n])
                free_out.put(o)
        except _Stopped:
            pass
        except BaseException as e:  # noqa: BLE001
            fail.set(e)

    threads = [threading.Thread(target=reader_main, daemon=True), threading.Thread(target=writer_main, daemon=True)]
    for t in threads:
        t.start()
    compute = torch.cuda.current_stream(dev)
    h2d, d2h = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    d_in = [torch.empty((in_rows, src_row), dtype=route.tdtype, device=dev) for _ in range(2)]
    d_free = [None, None]   # event: the compute stream's last read of d_in[j]
    # with a plan, the resampled frames of a chunk go into the device twin of its pinned output slot: every chunk's
    # result has the same allocation, whatever its frame count, and the grid is released before the next chunk runs
    d_out = None if plan is None else [torch.empty((out_rows, route.out_row), dtype=route.tdtype, device=dev)
                                       for _ in range(R_OUT)]
    # the packed rows of a chunk go into a device twin of their own in the same way
    d_wire = None if wire is None else [torch.empty(tuple(slot.shape), dtype=route.tdtype, device=dev) for slot in out_slots]
    count = route.row       # samples per frame, as scene.detect_cuts counts them
    carried = None          # int64 [1]: the previous chunk's last interval sum
    dead_before = 0         # dd: dead intervals directly before this chunk, saturated at max_gap
    total, j = 0, 0
    try:
        while True:
            item = fail.get(filled)
            if item is None:
                break
            i, s, m, c, last = item
            # the output slot of chunk i - R_OUT: written out, and (R_OUT = 2) that chunk's result is back in the
            # allocator before this chunk allocates: the device holds this chunk's levels and the previous result
            o = fail.get(free_out)
            with torch.cuda.stream(h2d):
                if d_free[j] is not None:
                    h2d.wait_event(d_free[j])
                d_in[j][:m].copy_(in_slots[i][:m], non_blocking=True)
                up = torch.cuda.Event()
                up.record(h2d)
            compute.wait_event(up)
            d = source.ingest(d_in[j][:m])   # unpacked, resized: tensors of their own, used on this stream alone
            flags = seen = None
            if thr is not None and c > 0:
                sums = scene.pair_sad([d], route.bits)   # c own intervals, then the lookahead intervals that were read
                window = sums if carried is None else torch.cat([carried, sums])
                scores, fl = scene.score_window(window, count, route.bits, thr)
                off = 0 if carried is None else 1
                flags = fl[off:off + c]
                seen = fl[off:off + m - 1]   # every interval read (the last one's score lacks a neighbour: not used)
                carried = sums[c - 1:c]
                if scene_log is not None:
                    scene_log.append((scores[off:off + c].cpu().numpy(), flags.cpu().numpy()))
            spans, ext, cuts = [], 0, None
            if dd is not None and c > 0:
                # the plan of this chunk depends on its data: one small read of the dead (and cut) flags, which waits
                # for the compute stream, the previous chunk's forwards included: the price of `dedup`
                peaks, dead, cuts = _dead_and_cuts(d, route.bits, dd[0], seen)
                spans, ext, dead_before = _retime.classify_chunk(dead, cuts, dead_before, s, c, dd[1])
                if dedup_log is not None:
                    dedup_log.append((peaks[:c].cpu().numpy(), dead[:c].copy()))
                if ext and seen is not None:
                    flags = seen[:c + ext]
            if sh is not None:
                # a frame belongs to the chunk that holds its opening time; the grid goes on over the lookahead
                # intervals that this chunk's windows reach.  With scene_cut the windows depend on the flags: one small
                # read, which waits for the compute stream as dedup's does
                j0, nj = plan.span(s, c, last)
                clip_last = s + c if last else None
                cuts = None if seen is None else seen.cpu().numpy().astype(bool)
                if sh > 0:
                    ext = _retime.shutter_reach(plan, sh, s, c, j0, nj, cuts, clip_last)
                    if ext and seen is not None:
                        flags = seen[:c + ext]
                if cuts is not None:
                    cuts = cuts[:c + ext]
            # with a span across the chunk's end, the grid goes on over the ext <= max_gap - 1 lookahead intervals that
            # the span needs (ext <= look, and the last chunk has ext == 0: no span reaches past the clip)
            out = route.run(d[:c + 1 + ext], factor)   # (a one-frame clip: the frame itself)
            _hold(flags, factor, out)
            d_free[j] = torch.cuda.Event()
            d_free[j].record(compute)
            if plan is None:
                rows = out if s == 0 else out[1:]   # a later chunk's first frame is the previous chunk's last
            else:
                # (pinned slot o is free, so the D2H copy that last read d_out[o] has completed)
                j0, nj = plan.span(s, c, last)
                if sh is not None:   # (a chunk without a frame of its own, p > q, writes nothing)
                    rows = _shutter_frames(job, out, s, c, ext, j0, nj, cuts, clip_last, out=d_out[o][:nj])
                elif dd is None:
                    rows = _retime.resample(out, plan, s, j0, nj, bits=route.bits, flags=flags, mode=mode,
                                            out=d_out[o][:nj], **motion)
                else:   # (every row an entry names is checked against `out` here, and again behind the C ABI)
                    entries = _retime.table_entries(plan, spans, s, j0, nj, c + ext, table_mode,
                                                    None if cuts is None else cuts[:c + ext])
                    rows = _retime.resample_table(out, entries, route.bits, out=d_out[o][:nj], mode=mode, **motion)
                out = None   # the grid is used on the compute stream alone: it may go back to the allocator now
            if wire is not None:   # (pinned slot o is free: the copy that last read d_wire[o] has completed)
                rows = wire.pack(rows, d_wire[o][:rows.shape[0]])
                out = None
            with torch.cuda.stream(d2h):
                d2h.wait_stream(compute)
                out_slots[o][:rows.shape[0]].copy_(rows, non_blocking=True)
                if plan is None and wire is None:   # `rows` is a view of this chunk's `out`, which is dropped while the copy may run;
                    rows.record_stream(d2h)   # d_out[o] lives for the whole run and is guarded by the free_out queue
                ev = torch.cuda.Event()
                ev.record(d2h)
            done.put((o, rows.shape[0], ev))
            total += rows.shape[0]
            up.synchronize()   # the input slot's H2D copy has completed: the reader may refill it
            free_in.put(i)
            j ^= 1
        done.put(None)
        threads[1].join()
    except _Stopped:
        pass
    except BaseException as e:  # noqa: BLE001
        fail.set(e)
    if fail.exc is not None:
        fail.stop.set()
        for t in threads:
            t.join(timeout=5.0)
        compute.synchronize()
        raise fail.exc
    threads[0].join()
    d2h.synchronize()
    compute.synchronize()
    for t in d_in:   # read by the h2d stream: back to the allocator only after it
        t.record_stream(h2d)
    return total


@torch.no_grad()
def _run_whole(model, route: _Route, reader, write, job: _Job) -> int:
    """The resident form of `_run` (every uploaded piece goes through `source.upload` as it arrives, so the device holds
    the frames of one piece only as they were read): the whole clip on the device as one chunk (flags once over every
    sample of the packed rows, one run of the route, one hold at the full factor; with a plan: one grid, one resample;
    with dd: one read of the dead and cut flags, one table).  Where source.count, the clip's frame count, is known up
    front (a regular file) the clip is read into one array; a stream of unknown length is uploaded 64 frames at a time,
    so that the host never holds it twice."""
    dev = next(model.parameters()).device
    source, factor, thr, plan, mode, dd = job.source, job.factor, job.thr, job.plan, job.mode, job.dd
    scene_log, dedup_log, wire, n_frames, src_row = job.scene_log, job.dedup_log, source.wire, source.count, source.row
    motion, table_mode = _retime_opts(job), "blend" if mode == "motion" else mode

    def upload(a):
        return source.upload(a, dev)
    whole = source.rs is None and wire is None
    if n_frames is not None:
        frames = np.empty((n_frames, src_row), dtype=route.ndtype)
        if reader.read_into(frames, n_frames) != n_frames:
            raise ValueError("the clip has fewer frames than were counted")
        d = upload(frames) if whole else torch.cat([upload(frames[i:i + 64]) for i in range(0, max(n_frames, 1), 64)])
        del frames
    else:
        parts = []
        while True:
            buf = np.empty((64, src_row), dtype=route.ndtype)
            k = reader.read_into(buf, 64)
            if k:
                parts.append(upload(buf[:k]))
            if k < 64:
                break
        if not parts:
            raise ValueError("no frames to interpolate")
        d = parts[0] if len(parts) == 1 else torch.cat(parts)
        del parts
    flags = None
    if thr is not None and d.shape[0] > 1:
        scores, flags = scene.detect_cuts([d], thr, route.bits)
        if scene_log is not None:
            scene_log.append((scores.cpu().numpy(), flags.cpu().numpy()))
    grid = route.run(d, factor)
    _hold(flags, factor, grid)
    if plan is None:   # (the raw route without fps: the factor run's frames as they are)
        write((grid if wire is None else wire.pack(grid)).cpu().numpy().view(route.ndtype))
        return grid.shape[0]
    n = plan.n_out(d.shape[0])
    if job.shutter is not None:
        cuts = None if flags is None else flags.cpu().numpy().astype(bool)
        rows = _shutter_frames(job, grid, 0, d.shape[0] - 1, 0, 0, n, cuts, d.shape[0] - 1)
    elif dd is None:
        rows = _retime.resample(grid, plan, 0, 0, n, bits=route.bits, flags=flags, mode=mode, **motion)
    else:
        spans, cuts = [], None
        if d.shape[0] > 1:
            peaks, dead, cuts = _dead_and_cuts(d, route.bits, dd[0], flags)
            spans = _retime.dedup_spans(dead, cuts, dd[1])
            if dedup_log is not None:
                dedup_log.append((peaks.cpu().numpy(), dead.copy()))
        entries = _retime.table_entries(plan, spans, 0, 0, n, d.shape[0] - 1, table_mode, cuts)
        rows = _retime.resample_table(grid, entries, route.bits, mode=mode, **motion)
    write((rows if wire is None else wire.pack(rows)).cpu().numpy().view(route.ndtype))
    return n


def _plan_of(fps, src_fps, header_fps, depth, any_rate: bool = False):
    """The plan of a checked `fps` (None: no plan) against `src_fps`, or the stream header's rate when that is None.
    any_rate: with a shutter, a rate at or below the source's is a plan too."""
    if fps is None:
        return None
    if src_fps is None:
        if header_fps is None:
            raise ValueError("a .npy stack carries no frame rate: pass src_fps with fps")
        try:
            src_fps = _retime.parse_fps(tuple(int(v) for v in header_fps))
        except ValueError:
            raise ValueError(f"the Y4M header's frame rate F{header_fps[0]}:{header_fps[1]} is not a rate: pass "
                             "src_fps") from None
    return _retime.plan(src_fps, fps, depth, any_rate)


def _job(open_source, *, factor, batch, chunk_frames, scene_cut, scene_log, fps, src_fps, time_depth, retime, dedup,
         max_gap, dedup_log, resize, resize_filter, headerless: bool = False, shutter=None) -> _Job:
    """The job of a route's keyword arguments: every check that needs no source, in the routes' order; then
    `open_source(size, filter)` -> the `_Opened` source, with its own checks; then the plan, which may need the source's
    rate.  headerless: the stream carries no rate, so src_fps is required.  Nothing here touches the device; a
    refusal after the source was opened closes it."""
    thr, C = _check_common(factor, batch, chunk_frames, scene_cut)
    if headerless:
        if src_fps is None:
            raise ValueError("raw video carries no frame rate: pass src_fps")
        _retime.parse_fps(src_fps)
    fps, src_fps, depth, mode = check_retime(fps, src_fps, time_depth, retime, factor)
    tol, gap = check_dedup(dedup, max_gap, fps, factor)
    sh = check_shutter(shutter, fps, mode, tol)
    size = None if resize is None else _resize.check_size(resize)
    source = open_source(size, _resize.check_resize_filter(resize, resize_filter))
    try:
        plan, rate = _plan_of(fps, src_fps, source.fps, depth, sh is not None), None
        if sh:
            _retime.check_shutter_plan(plan, sh)
        if plan is not None:
            factor, rate = plan.G, (plan.fps.numerator, plan.fps.denominator)
        elif source.fps is not None:
            rate = (source.fps[0] * factor, source.fps[1])
        plan, dd = _dedup_of(tol, gap, plan, factor)   # (without fps: p / q = 1 / factor; the rate as above)
        if mode == "motion" and plan is not None:   # (without a plan `retime` has no effect, as for "nearest")
            check_motion_layout(source.layout, "this source's frame format")
    except BaseException:
        source.close()
        raise
    return _Job(source, factor, C, thr, plan, mode, dd, rate, scene_log, dedup_log, int(batch), sh)


def _drive(model, job: _Job, make_write, finish) -> int:
    """Run `job` into the sink: make_write() -> write(rows), made once the sink is open; finish(ok) closes the sink.
    `_run` and `_run_whole` are looked up when the job runs (tests replace them)."""
    ok = False
    try:
        engine = _run_whole if job.chunk_frames is None else _run
        total = engine(model, job.source.route, job.source.reader, make_write(), job)
        ok = True
    finally:
        finish(ok)
    return total


def _open_sink(dst):
    """-> (file object, finish(ok)).  A path is written to `<dst>.part` and renamed on success, removed on error; a
    file object (a pipe) keeps what was written before an error."""
    if not _is_path(dst):
        return dst, lambda ok: dst.flush()
    part = os.fspath(dst) + ".part"
    f = open(part, "wb")

    def finish(ok):
        f.close()
        if ok:
            os.replace(part, dst)
        else:
            os.remove(part)
    return f, finish


def interpolate_y4m_stream(model, src, dst, factor: int = 2, *, batch: int = 8, chunk_frames: int = 32,
                           matrix: str = "bt709", siting: str | None = None, scene_cut: float | None = None,
                           scene_log: list | None = None, fps=None, src_fps=None, time_depth: int = 2,
                           retime: str = "blend", dedup=None, max_gap: int = 4, dedup_log: list | None = None,
                           resize=None, resize_filter: str = "linear", chroma: str = "average",
                           chroma_log: list | None = None, shutter=None) -> int:
    """Y4M in (a path or a readable binary file: a pipe, `sys.stdin.buffer`) -> Y4M out (a path or a writable binary
    file), or a `.npy` path of the luma frames (grayscale network; the input must then be a regular file, whose frame
    count a first pass reads).  This is what `FrameInterpolator.interpolate_video` runs; the result is the same, byte
    for byte, for any `chunk_frames` >= 1 and for None (the whole clip as one chunk, resident on the device).  The
    output header has the input's `C` tag, rate x factor, and the input's `XCOLORRANGE` except on the 8-bit grayscale
    route, which writes none.  Returns the output frame count.  Every argument
    is checked before anything is pinned, before any GPU work and before the output exists.  scene_log: a list that
    receives (scores float64, flags uint8) host arrays of each chunk's intervals (a resident run: of the clip's, once;
    costs a synchronise).
    fps / src_fps / time_depth / retime: frame-rate conversion (retime.py): the output has `fps` frames per second,
    resampled from a 2**time_depth bisection; src_fps overrides the header's rate; factor stays 2.
    dedup / max_gap: re-time repeated frames (retime.py): dedup is None (off) or a tolerance >= 0 in
    code values, max_gap (2..8) the longest run of equal frames that is re-timed; with `factor` (at most 16) or with
    `fps`.  dedup_log: a list that receives (peaks, dead) host arrays of each chunk's intervals (scene_log's twin).
    resize: None, or (width, height) / "WxH": every frame is resized on the device right after its upload (resize.py,
    DESIGN.md 3.3q; each plane on its own grid, the chroma size as the tag gives it at the new size), and the route, its
    refusals, scene cuts, dedup and the output header are those of a clip of that size.  resize_filter: "linear" (the
    filter of cv2.resize's INTER_LINEAR) or "area" (alias-free down-scaling, DESIGN.md 3.3r: refused where a plane would
    grow on either axis, or shrink more than 64 times); anything but "linear" is an error without `resize`.
    chroma: "average", or "motion" (grayscale network; chroma.py): the chroma of every inserted frame is
    warped along the luma flow of its two neighbours, 8x8 luma block by block, where the network's luma for the frame
    is closer to the warped luma than to the averaged one, and is the average elsewhere; the luma of every frame and
    the source frames are those of "average", for every chunk_frames.  One Farneback flow per inserted frame.  Refused for
    the RGB network; no effect on a mono stream or a luma .npy output.  chroma_log: a list that receives one (warped
    blocks, blocks) pair of ints after a "motion" run that had chroma to make (one device-to-host read, at the end).
    shutter: None, or an exact rational in [0, 1] (an int, a Fraction, an (n, d) pair or "n/d"; retime.py):
    with it `fps` is required and may be ANY positive rate, a lower one included (60 -> 24, 59.94 -> 50); every output
    frame is the clip averaged over that fraction of the output frame period from its own time on (1/2: a 180 degree
    shutter), never across a scene cut or past the clip's end.  0 is point sampling and takes every `retime`; above 0
    `retime` must be "blend".  Refused with dedup."""
    npy_out = _is_path(dst) and os.fspath(dst).lower().endswith(".npy")
    _chroma.check_mode(chroma)
    job = _job(lambda size, rfilter: _open_y4m(model, src, npy_out, batch, matrix, siting, size, rfilter,
                                               chunk_frames is None or npy_out, chroma),
               factor=factor, batch=batch, chunk_frames=chunk_frames, scene_cut=scene_cut, scene_log=scene_log, fps=fps,
               src_fps=src_fps, time_depth=time_depth, retime=retime, dedup=dedup, max_gap=max_gap, dedup_log=dedup_log,
               resize=resize, resize_filter=resize_filter, shutter=shutter)
    source, hdr, bits = job.source, job.source.header, job.source.route.bits
    try:
        if npy_out:
            n_out = (source.count - 1) * job.factor + 1 if job.plan is None else job.plan.n_out(source.count)
            sink = _NpyWriter(os.fspath(dst), source.route.ndtype, (n_out, hdr["height"], hdr["width"]))
            return _drive(model, job, lambda: sink.write, sink.close)
        f, finish = _open_sink(dst)
        total = _drive(model, job, lambda: imageio_lite.Y4MWriter(
            f, hdr["width"], hdr["height"], job.rate, hdr["colourspace"],
            hdr["colour_range"] if (bits == 10 or model.frame_channels == 3) else None, bits=bits).write, finish)
        stats = getattr(source.route, "chroma_stats", None)
        if chroma_log is not None and stats is not None:
            chroma_log.append((0 if stats["warped"] is None else int(stats["warped"]), stats["blocks"]))
        return total
    finally:
        source.close()


def interpolate_npy_stream(model, src, dst, factor: int = 2, *, batch: int = 8, chunk_frames: int = 32,
                           scene_cut: float | None = None, scene_log: list | None = None, fps=None, src_fps=None,
                           time_depth: int = 2, retime: str = "blend", dedup=None, max_gap: int = 4,
                           dedup_log: list | None = None, resize=None, resize_filter: str = "linear",
                           shutter=None) -> int:
    """`.npy` stack in (uint8 [N,H,W] or [N,H,W,C], read through `np.load(mmap_mode="r")`) -> `.npy` out (written
    through `np.lib.format.open_memmap`, the file `np.save` would write; a name without `.npy` gets it).  An
    [N,H,W,C] stack goes through the RGB network, or channel by channel through the grayscale one.  Returns the output
    frame count.  fps / src_fps / time_depth / retime and chunk_frames None: as for `interpolate_y4m_stream`; a .npy
    stack carries no rate, so `fps` needs `src_fps`.  resize / resize_filter: as for `interpolate_y4m_stream`; the output
    stack has the new height and width.  shutter: as for `interpolate_y4m_stream`."""
    def open_source(size, rfilter):
        if not _is_path(dst):
            raise ValueError("a .npy output is a path")
        return _open_npy(model, src, batch, size, rfilter)
    job = _job(open_source, factor=factor, batch=batch, chunk_frames=chunk_frames, scene_cut=scene_cut,
               scene_log=scene_log, fps=fps, src_fps=src_fps, time_depth=time_depth, retime=retime, dedup=dedup,
               max_gap=max_gap, dedup_log=dedup_log, resize=resize, resize_filter=resize_filter, shutter=shutter)
    n = job.source.count
    if n < 1:
        raise ValueError("no frames to interpolate")
    dst = os.fspath(dst)
    if not dst.endswith(".npy"):   # what np.save does with the name
        dst += ".npy"
    n_out = (n - 1) * job.factor + 1 if job.plan is None else job.plan.n_out(n)
    sink = _NpyWriter(dst, np.uint8, (n_out,) + job.source.shape)
    return _drive(model, job, lambda: sink.write, sink.close)


def interpolate_raw_stream(model, src, dst, factor: int = 2, *, raw: str = "nv12", width=None, height=None,
                           batch: int = 8, chunk_frames: int | None = 32, matrix: str = "bt709",
                           siting: str | None = None, scene_cut: float | None = None, scene_log: list | None = None,
                           fps=None, src_fps=None, time_depth: int = 2, retime: str = "blend", dedup=None,
                           max_gap: int = 4, dedup_log: list | None = None, resize=None,
                           resize_filter: str = "linear", packing: str | None = None, shutter=None) -> int:
    """Headerless raw video in (a path or a readable binary file: a pipe) -> the same format out (a path or a writable
    binary file): tight NV12 frames of height x width (`ffmpeg ... -f rawvideo -pix_fmt nv12 -`) through the RGB
    network, `interpolate_sequence_nv12` per level; or, with raw "rgb24" / "bgr24" / "rgba" / "bgra", tight packed RGB
    frames (`-pix_fmt rgb24`), `interpolate_sequence_rgb_packed` per level, where matrix and siting are not used; or, with
    raw "yuv422p" / "yuv444p" / "yuv422p10le" / "yuv444p10le" / "uyvy422" / "yuyv422", tight 4:2:2 / 4:4:4 frames
    (`-pix_fmt yuv422p10le`; 10 bits: little-endian 16-bit words), `interpolate_sequence_yuv` per level.  factor, scene_cut, chunk_frames (None: the whole clip resident)
    and fps / time_depth / retime as for `interpolate_y4m_stream`; the stream carries no rate, so src_fps is required
    (with fps it sets the resampling; the output has fps, or src_fps x factor, frames per second - pass that rate to
    whatever reads the result).  siting None is "mpeg2", the range limited.  Every argument - the model's network, the
    output name, the size of a regular input file (a whole number of frames) - is checked before any GPU work and
    before the output exists; a pipe that ends inside a frame is an error at that point.  Returns the output frame
    count.  resize / resize_filter: as for `interpolate_y4m_stream`: width and height stay the size of the source, the
    output is raw video of the new size, and the format's refusals (an odd width of uyvy422 / yuyv422) apply to both sizes.
    packing: None, or with raw "yuv422p10le" one of wire10.PACKINGS ("v210", "y210le", "p210le"; wire10.py, DESIGN.md
    3.3s): input and output are tight frames of that 10-bit 4:2:2 packing (`ffmpeg -c:v v210 -f rawvideo`), unpacked to
    yuv422p10le rows on the device right after each chunk's upload and packed again before its download; everything
    between is the yuv422p10le route, and the output is, byte for byte, that route's output packed.  The file size of a
    regular input counts wire frames (`wire10.frame_bytes`); v210 / y210le need an even width at both sizes.
    shutter: as for `interpolate_y4m_stream`."""
    npy_out = _is_path(dst) and os.fspath(dst).lower().endswith(".npy")
    job = _job(lambda size, rfilter: _open_raw(model, src, raw, width, height, npy_out, batch, matrix, siting, size,
                                               rfilter, packing),
               factor=factor, batch=batch, chunk_frames=chunk_frames, scene_cut=scene_cut, scene_log=scene_log, fps=fps,
               src_fps=src_fps, time_depth=time_depth, retime=retime, dedup=dedup, max_gap=max_gap, dedup_log=dedup_log,
               resize=resize, resize_filter=resize_filter, headerless=True, shutter=shutter)
    try:
        if job.source.count == 0:
            raise ValueError("no frames to interpolate")
        f, finish = _open_sink(dst)

        def write(rows):
            f.write(np.ascontiguousarray(rows).data)
        return _drive(model, job, lambda: write, finish)
    finally:
        job.source.close()


__all__ = ["check_chunk_frames", "check_retime", "check_dedup", "check_shutter", "interpolate_y4m_stream", "interpolate_npy_stream",
           "interpolate_raw_stream"]
