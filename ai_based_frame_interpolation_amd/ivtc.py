"""Inverse telecine on the device (csrc/ivtc.hip.h): hard-telecined film - 24 fps carried as 29.97 fps
interlaced video by 2:3 pulldown - becomes its film frames again, byte for byte, at 23.976 fps.

  definition  the project's own, in integers, in the spirit of ffmpeg's fieldmatch + decimate and NOT pinned against
              ffmpeg, which is not installed where this is tested (include/fiunet.h states it, tests/ivtc_ref.py in numpy;
              the kernels equal that to the last bit).
  match       a frame keeps the rows of its first field ("tff": the even rows) and takes the others from the frame before
              (p), from itself (c) or from the frame behind (n): the candidate with the smallest comb score - the largest
              count of combed samples in a block of 16 x 64 of the layout's first plane - wins, ties c, then p.
  combed      a frame whose best score exceeds `combed` is an orphan field at an edit, or true interlaced video: under
              fallback "deinterlace" it is replaced by `deinterlace` of that frame (rate "frame", method "adaptive"),
              under "keep" the chosen weave is written.
  decimate    of every complete cycle of `cycle` frames (aligned to the clip's frame index) the output frame with the
              smallest `scene.pair_peak` against the output frame before it is dropped; the rate becomes
              rate * (cycle - 1) / cycle.
  planes      every plane of a frame is woven where it lies, with the one choice of the frame.

`ivtc_video` is file to file or pipe to pipe and needs no model; it sits in front of the `video` command:

    ffmpeg -i telecined.vob -f yuv4mpegpipe - | python -m ai_based_frame_interpolation_amd.cli ivtc --input - \\
        --output - | python -m ai_based_frame_interpolation_amd.cli video --input - --output - --model best_model.pth \\
        --fps 60000/1001 | ffmpeg -f yuv4mpegpipe -i - out.mkv

Out of scope: cadences other than a fixed cycle (2:2 PAL speed-up, mixed 3:2 and video), soft telecine flags, per-block
matching, matching on the second field, IVTC inside the `video` / `evaluate` engine (they pipe), .npy input."""
from __future__ import annotations

import os
from fractions import Fraction

import numpy as np
import torch

from . import _native, imageio_lite
from .deinterlace import MAX_PLANES, ORDERS, bits_of, choice, deinterlace, fps_pair, is_path, order_of, planes_of
from .layout import RAW_FORMATS, Layout, frame_layout

CANDIDATES = ("p", "c", "n")
FALLBACKS = ("deinterlace", "keep")
COMBED = 48           # the largest block count a matched frame may have
CYCLE = 5
INF = float("inf")
MAX_THRESHOLD = 1023
MAX_RESIDENT = 65535   # frames of one call of the library


def default_threshold(bits: int) -> int:
    """T of the comb test (u - m) * (d - m) > T * T: 12 at 8 bits, 48 at 10."""
    return 48 if bits == 10 else 12


def _parity(order) -> int:
    return 1 if choice("order", order, ORDERS) == "bff" else 0


def _check_frames(frames: torch.Tensor, bits: int):
    if frames.dim() != 2 or not frames.is_contiguous():
        raise ValueError("frames must be a contiguous [n, samples] tensor of tight frames")
    if bits_of(frames) != bits:
        raise ValueError(f"bits={bits!r} does not match frames of {frames.dtype}")
    return frames.shape


def _fit(planes, row):
    need = max(off + (h - 1) * pitch + (w - 1) * step + 1 for off, h, w, pitch, step in planes)
    if need > row:
        raise ValueError(f"the planes describe a frame of {need} samples, the rows have {row}")


def _window(first, count, n):
    first = int(first)
    count = n - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > n:
        raise ValueError(f"first={first} and count={count} do not name frames of a window of {n}")
    return first, count


def _metric_plane(layout_or_plane):
    """The plane the comb score is taken on: a Layout's first, or one plane [(name,) offset, h, w, pitch, step]."""
    if isinstance(layout_or_plane, Layout):
        pl = layout_or_plane.planes[0]
    else:
        pl = layout_or_plane
        if len(pl) and isinstance(pl[0], (tuple, list)):
            pl = pl[0]
    off, h, w, pitch, step = (int(v) for v in tuple(pl)[-5:])
    if h < 3:
        raise ValueError(f"a plane of {h} x {w} has no comb score: a sample needs a row above and below (h >= 3)")
    return off, h, w, pitch, step


def field_scores(frames: torch.Tensor, layout_or_plane, bits: int, order: str = "tff", first: int = 0,
                 count: int | None = None, threshold: int | None = None, out: torch.Tensor | None = None,
                 stream=None) -> torch.Tensor:
    """Device rows [n, samples] of a window -> the comb scores of frames first .. first + count - 1 as int32 [count, 3] on
    the device, columns p, c, n.  layout_or_plane: a `layout.Layout` (its first plane) or one plane (offset, h, w, pitch,
    step) in samples of a row.  threshold: T of the comb test (default 12 at 8 bits, 48 at 10).  out: a contiguous int32
    [count, 3] tensor the scores are MAX-ACCUMULATED into (the caller zeroed it; several planes may share it).  On the
    rows' current stream (or the raw handle `stream`), without allocation when `out` is given, without synchronisation."""
    parity = _parity(order)
    n, row = _check_frames(frames, bits)
    plane = _metric_plane(layout_or_plane)
    _fit([plane], row)
    first, count = _window(first, count, n)
    threshold = default_threshold(bits) if threshold is None else int(threshold)
    if not 0 <= threshold <= MAX_THRESHOLD:
        raise ValueError(f"threshold must lie in 0..{MAX_THRESHOLD}, got {threshold}")
    if out is None:
        out = torch.zeros((count, 3), dtype=torch.int32, device=frames.device)
    elif out.shape != (count, 3) or out.dtype != torch.int32 or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"out must be a contiguous int32 [{count}, 3] tensor on the frames' device")
    if count:
        _native.field_match(frames, n, plane + (row,), first, count, parity, threshold, out, bits, stream)
    return out


def weave(frames: torch.Tensor, layout_or_planes, bits: int, entries, order: str = "tff", out: torch.Tensor | None = None,
          stream=None) -> torch.Tensor:
    """Device rows [n, samples] of a window and (keep, other) pairs -> rows [len(entries), samples]: output j takes the
    rows of the first field's parity of every plane from frame keep_j and the others from frame other_j.  Bytes are
    moved; samples of a row that belong to no plane are not written (without `out` they are zero).  On the rows' current
    stream (or `stream`), without allocation when `out` is given, without synchronisation."""
    parity = _parity(order)
    n, row = _check_frames(frames, bits)
    planes = planes_of(layout_or_planes)
    _fit(planes, row)
    entries = [(int(k), int(o)) for k, o in entries]
    for k, o in entries:
        if not (0 <= k < n and 0 <= o < n):
            raise ValueError(f"entry {(k, o)} names a frame outside the window of {n}")
    if out is None:
        out = torch.zeros((len(entries), row), dtype=frames.dtype, device=frames.device)
    elif out.shape != (len(entries), row) or out.dtype != frames.dtype or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"out must be a contiguous [{len(entries)}, {row}] {frames.dtype} tensor on the frames' device")
    if entries:
        full = [p + (row,) for p in planes]
        for k in range(0, len(full), MAX_PLANES):
            _native.field_weave(frames, n, full[k:k + MAX_PLANES], out, full[k:k + MAX_PLANES], entries, parity, bits, stream)
    return out


# ---- host arithmetic ------------------------------------------------------------------------------------------------------
def choose(scores, combed: int = COMBED):
    """Scores [n, 3] (p, c, n; a tensor, an array or lists) -> (matches: a list of "p" / "c" / "n", flags: a list of
    bools).  c if sc <= min(sp, sn), else p if sp <= sn, else n; a frame is flagged iff its chosen score exceeds `combed`."""
    if isinstance(scores, torch.Tensor):
        scores = scores.cpu().numpy()
    matches, flags = [], []
    for sp, sc, sn in np.asarray(scores).reshape(-1, 3).tolist():
        m, s = ("c", sc) if sc <= min(sp, sn) else ("p", sp) if sp <= sn else ("n", sn)
        matches.append(m)
        flags.append(s > combed)
    return matches, flags


def _check_cycle(cycle) -> int:
    if not isinstance(cycle, int) or isinstance(cycle, bool) or cycle < 2:
        raise ValueError(f"cycle must be a whole number of frames, 2 or more, got {cycle!r}")
    return cycle


def _drop_of(peaks) -> int:
    """The position of the smallest peak of a cycle, the earliest of equals."""
    return min(range(len(peaks)), key=lambda i: (peaks[i], i))


def decimate_plan(peaks, cycle: int = CYCLE, start: int = 0):
    """peaks[i]: `scene.pair_peak` of clip frame start + i against the frame before it (INF for the clip's first frame)
    -> the clip indices that stay.  Cycles are aligned to the clip (t // cycle); of every cycle that lies whole inside
    start .. start + len(peaks) - 1 the frame with the smallest peak goes, the earliest of equals; an incomplete cycle at
    either end is kept whole."""
    cycle, n, start = _check_cycle(cycle), len(peaks), int(start)
    kept = []
    t = start
    while t < start + n:
        c0 = t // cycle * cycle
        if c0 == t and t + cycle <= start + n:
            drop = _drop_of([peaks[i - start] for i in range(t, t + cycle)])
            kept.extend(t + i for i in range(cycle) if i != drop)
            t += cycle
        else:
            kept.append(t)
            t += 1
    return kept


class Carry:
    """What a chunked run carries from one chunk to the next: the peaks of the unfinished cycle (`pending`: [(clip index,
    peak)]), the clip index of the next frame (`next`), the indices dropped so far, and for the caller's use `last`, the
    last output frame (the next chunk's first peak is taken against it) and `held`, the output frames of `pending`.
    `feed(peaks)` takes the peaks of the next frames and returns the clip indices that can be written now, in order;
    `finish()` returns the rest (a trailing incomplete cycle, kept whole).  Fed in any pieces, the indices are
    `decimate_plan` of the whole clip."""

    def __init__(self, cycle: int = CYCLE, decimate: bool = True):
        self.cycle, self.decimate = _check_cycle(cycle), bool(decimate)
        self.next = 0
        self.pending = []
        self.dropped = []
        self.last = None
        self.held = None

    def feed(self, peaks):
        emit = []
        for p in peaks:
            t = self.next
            self.next += 1
            if not self.decimate:
                emit.append(t)
                continue
            self.pending.append((t, p))
            if len(self.pending) == self.cycle:   # (the clip starts on a cycle boundary, so the pending ones are a cycle)
                drop = _drop_of([v for _, v in self.pending])
                self.dropped.append(self.pending[drop][0])
                emit.extend(i for k, (i, _) in enumerate(self.pending) if k != drop)
                self.pending = []
        return emit

    def finish(self):
        emit = [i for i, _ in self.pending]
        self.pending = []
        return emit


def out_rate(fps, cycle: int = CYCLE, decimate: bool = True) -> tuple[int, int]:
    """The rate (num, den) behind the decimation: rate * (cycle - 1) / cycle as an exact fraction in lowest terms."""
    f = Fraction(int(fps[0]), int(fps[1]))
    if decimate:
        f = f * (_check_cycle(cycle) - 1) / cycle
    return f.numerator, f.denominator


def telecine(progressive: torch.Tensor, layout, order: str = "tff", phase: int = 0) -> torch.Tensor:
    """2:3 pulldown, in torch, for tests and scoring: film frames [F, samples] -> hard-telecined frames.  Film frame f
    gives 2 fields (f even) or 3 (f odd); the fields alternate in parity, beginning with the first field's of `order`; the
    first 2 * phase fields are dropped and the rest paired into frames (an odd field left over is dropped): frame t takes
    the rows of the first field's parity of every plane from its first field's film frame and the others from its second's."""
    k = _parity(order)
    if progressive.dim() != 2:
        raise ValueError("progressive must be [F, samples]")
    if not isinstance(phase, int) or phase < 0:
        raise ValueError(f"phase must be a whole number >= 0, got {phase!r}")
    src = [f for f in range(progressive.shape[0]) for _ in range(2 if f % 2 == 0 else 3)][2 * phase:]
    n = len(src) // 2
    dev = progressive.device
    a = progressive[torch.tensor(src[0:2 * n:2], dtype=torch.long, device=dev)]
    b = progressive[torch.tensor(src[1:2 * n:2], dtype=torch.long, device=dev)]
    out = a.clone()
    for off, h, w, pitch, step in planes_of(layout):
        rows = torch.arange(1 - k, h, 2, device=dev)
        idx = (off + rows[:, None] * pitch + torch.arange(w, device=dev)[None, :] * step).reshape(-1)
        out[:, idx] = b[:, idx]
    return out


# ---- the pipeline ---------------------------------------------------------------------------------------------------------
def _check_options(order, fallback, combed, cycle, threshold):
    choice("order", order, ORDERS)
    choice("fallback", fallback, FALLBACKS)
    _check_cycle(cycle)
    if not isinstance(combed, int) or isinstance(combed, bool) or combed < 0:
        raise ValueError(f"combed must be a whole number >= 0, got {combed!r}")
    if threshold is not None and not 0 <= int(threshold) <= MAX_THRESHOLD:
        raise ValueError(f"threshold must lie in 0..{MAX_THRESHOLD}, got {threshold}")


class _Engine:
    """The steps of one run: `step` takes a window of device rows with the frames to do (first, count; their neighbours
    come from the window) and returns the output rows that can be written now (or None); `finish` returns the rest."""

    def __init__(self, lay, bits, order, threshold, combed, fallback, decimate, cycle):
        from . import scene
        self.scene = scene
        self.lay, self.bits, self.order = lay, bits, order
        self.threshold, self.combed, self.fallback = threshold, combed, fallback
        self.carry = Carry(cycle, decimate)
        self.matches = {c: 0 for c in CANDIDATES}
        self.combed_frames = []
        self.frames_out = 0

    def step(self, d: torch.Tensor, first: int, count: int):
        n, carry = d.shape[0], self.carry
        base = carry.next
        scores = field_scores(d, self.lay, self.bits, self.order, first, count, self.threshold)
        matches, flags = choose(scores, self.combed)          # (the chunk's one read of the scores)
        other = {"p": lambda t: max(t - 1, 0), "c": lambda t: t, "n": lambda t: min(t + 1, n - 1)}
        out = weave(d, self.lay, self.bits, [(first + i, other[m](first + i)) for i, m in enumerate(matches)], self.order)
        for i, m in enumerate(matches):
            self.matches[m] += 1
            if flags[i]:
                self.combed_frames.append(base + i)
                if self.fallback == "deinterlace":
                    deinterlace(d, self.lay, self.bits, self.order, "frame", "adaptive", True, first=first + i, count=1,
                                out=out[i:i + 1])
        if not carry.decimate:
            carry.feed([0] * count)
            self.frames_out += count
            return out
        stack = out if carry.last is None else torch.cat([carry.last[None], out])
        peaks = self.scene.pair_peak([stack], self.bits).cpu().tolist()   # (the chunk's one read of the peaks)
        if carry.last is None:
            peaks = [INF] + peaks
        carry.last = out[-1].clone()
        # the frames at hand: the ones held over from the chunk before, then this chunk's
        held_idx = [i for i, _ in carry.pending]
        pool = out if carry.held is None else torch.cat([carry.held, out])
        where = {t: k for k, t in enumerate(held_idx + list(range(base, base + count)))}
        emit = carry.feed(peaks)
        keep = [where[i] for i, _ in carry.pending]
        carry.held = pool[torch.tensor(keep, dtype=torch.long, device=pool.device)] if keep else None
        self.frames_out += len(emit)
        if not emit:
            return None
        return pool[torch.tensor([where[t] for t in emit], dtype=torch.long, device=pool.device)]

    def finish(self):
        emit = self.carry.finish()
        held, self.carry.held = self.carry.held, None
        self.frames_out += len(emit)
        return held if emit else None

    def report(self) -> dict:
        return {"frames_in": self.carry.next, "frames_out": self.frames_out, "matches": dict(self.matches),
                "combed": list(self.combed_frames), "dropped": list(self.carry.dropped)}


def ivtc(frames: torch.Tensor, layout, bits: int, order: str = "tff", decimate: bool = True, cycle: int = CYCLE,
         threshold: int | None = None, combed: int = COMBED, fallback: str = "deinterlace"):
    """A resident clip as device rows [n, samples] -> (rows, report): the matched (and, unless decimate=False, decimated)
    frames and {"frames_in", "frames_out", "matches": {"p", "c", "n": counts}, "combed": clip indices of the flagged
    frames, "dropped": clip indices of the dropped ones}.  The scores are taken on the layout's first plane.  The clip
    goes to the library in one call per kernel: at most 65535 frames (`MAX_RESIDENT`; ValueError beyond - `ivtc_video`
    streams a clip of any length)."""
    _check_options(order, fallback, combed, cycle, threshold)
    n, row = _check_frames(frames, bits)
    if n > MAX_RESIDENT:
        raise ValueError(f"a resident clip holds at most {MAX_RESIDENT} frames, got {n}: stream it through ivtc_video")
    eng = _Engine(layout, bits, order, threshold, combed, fallback, decimate, cycle)
    parts = [eng.step(frames, 0, n)] if n else []
    parts.append(eng.finish())
    parts = [p for p in parts if p is not None]
    rows = torch.cat(parts) if parts else torch.empty((0, row), dtype=frames.dtype, device=frames.device)
    return rows, eng.report()


def ivtc_video(src, dst, order: str = "auto", decimate: bool = True, cycle: int = CYCLE, threshold: int | None = None,
               combed: int = COMBED, fallback: str = "deinterlace", chunk_frames: int = 32, raw=None, width=None,
               height=None, src_fps=None, packing=None, device=None) -> dict:
    """Inverse telecine of a clip of any length in memory bounded by the chunk -> the report of `ivtc`.

    src / dst, raw=, width=, height=, packing=, src_fps= and order= are `deinterlace.deinterlace_video`'s: Y4M at 8 and 10
    bits or headerless raw frames of `layout.RAW_FORMATS`, "auto" reading `It` / `Ib` off the Y4M header.  The output
    has the input's format; a Y4M result carries `Ip` and, when decimating, the rate * (cycle - 1) / cycle as an exact
    fraction (30000/1001 becomes 24000/1001).

    Each step uploads a window of chunk_frames + 2 source frames - one context frame either side - and carries the
    unfinished cycle and the last output frame to the next, so memory depends on the chunk and not on the clip, and the
    bytes written are the same for every chunk_frames.  A step reads the scores and the peaks back once each."""
    from . import stream as _stream
    if order != "auto":
        choice("order", order, ["auto"] + list(ORDERS))
    _check_options("tff", fallback, combed, cycle, threshold)
    chunk = _stream.check_chunk_frames(chunk_frames)
    if raw is None and (width is not None or height is not None or packing is not None):
        raise ValueError("width, height and packing describe raw= video: a Y4M stream carries its own header")
    close_src = close_dst = None
    wire = None
    try:
        if raw is None:
            reader = imageio_lite.Y4MReader(src)
            close_src = reader.close
            hdr = reader.header
            order = order_of(order, reader.interlace, None)
            lay = frame_layout(("y4m", hdr["colourspace"]), hdr["height"], hdr["width"])
            in_row = lay.samples
        else:
            if raw not in RAW_FORMATS:
                raise ValueError(f"raw must be one of {list(RAW_FORMATS)}, got {raw!r}")
            order = order_of(order, None, raw)
            if width is None or height is None:
                raise ValueError("raw video has no header: pass width and height")
            lay = frame_layout(raw, int(height), int(width))
            wire = _stream.check_packing(packing, raw, int(height), int(width))
            in_row = lay.samples if wire is None else wire.in_row
            hdr = None
        planes_of(lay)
        _metric_plane(lay)   # (a first plane of fewer than three rows is refused before anything is opened for writing)
        ndtype = np.uint8 if lay.bits == 8 else np.dtype("<u2")
        row_bytes = in_row * np.dtype(ndtype).itemsize
        if raw is not None:
            if is_path(src):
                if not os.path.exists(src):
                    raise FileNotFoundError(f"Video file not found: {src}")
                fin = open(src, "rb")
                close_src = fin.close
            else:
                fin = src
            reader = _stream._RawReader(fin, row_bytes)
        dev = torch.device("cuda" if device is None else device)
        if hdr is not None:
            fps = hdr["fps"] if src_fps is None else fps_pair(src_fps)
            writer = imageio_lite.Y4MWriter(dst, hdr["width"], hdr["height"], out_rate(fps, cycle, decimate),
                                            hdr["colourspace"], hdr["colour_range"], lay.bits)
            close_dst, write = writer.close, writer.write
        else:
            fout = open(dst, "wb") if is_path(dst) else dst
            close_dst = fout.close if is_path(dst) else fout.flush

            def write(rows):
                fout.write(memoryview(np.ascontiguousarray(rows)).cast("B"))

        eng = _Engine(lay, lay.bits, order, threshold, combed, fallback, decimate, cycle)

        def emit(res):
            if res is None or not res.shape[0]:
                return
            if wire is not None:
                res = wire.pack(res)
            host = res.cpu().numpy()
            write(host.view(ndtype) if lay.bits == 10 else host)

        buf = np.empty((chunk + 2, in_row), dtype=ndtype)
        have = reader.read_into(buf, chunk + 1)
        eof = have < chunk + 1
        lead = 0
        while True:
            count = have - lead - (0 if eof else 1)   # the last frame of a window that goes on is context only
            if count > 0:
                d = torch.from_numpy(buf[:have].view(np.int16) if lay.bits == 10 else buf[:have]).to(dev)
                if wire is not None:
                    d = wire.unpack(d)
                emit(eng.step(d, lead, count))
            if eof:
                break
            buf[0:2] = buf[have - 2:have].copy()   # the last frame done and the one behind it
            lead = 1
            got = reader.read_into(buf[2:], chunk)
            have, eof = 2 + got, got < chunk
        emit(eng.finish())
        return eng.report()
    finally:
        for close in (close_src, close_dst):
            if close is not None:
                close()


__all__ = ["CANDIDATES", "FALLBACKS", "COMBED", "CYCLE", "INF", "Carry", "default_threshold", "field_scores", "weave",
           "choose", "decimate_plan", "out_rate", "telecine", "ivtc", "ivtc_video"]
