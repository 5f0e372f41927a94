"""Hold-out scoring of a checkpoint on real video: drop frames of a clip, rebuild each from its two
neighbours, and compare with the frame that was really there - plane by plane, on the device, in memory bounded by the
chunk.

  triplets   "disjoint": frames 0, 2, 4, ... are the inputs and 1, 3, 5, ... the held-out frames ((n-1)//2 of them).
             "sliding": the reference's triplet set (model/train.py: (f[i], f[i+2]) -> f[i+1]), every frame 1 .. n-2;
             it is the disjoint evaluation of the clip together with that of the clip without its first frame.
  methods    each turns a decimated chunk d [k, row] into [2k-1, out_row] rows whose odd rows are the predictions:
             "unet" is `route.run(d, 2)`, the forward of whatever route the clip takes (stream.py: the source is opened
             by the video routes' own openers `_open_y4m`, `_open_npy`, `_open_raw`, with their refusals); "linear" the project's integer average (a + b + 1) >> 1 of every
             sample of the row; "repeat" the earlier neighbour, which is what a frame duplicator shows.  Beyond the
             default three (ALL_METHODS), the classical motion-compensated baseline: Farneback flow
             between the two neighbours on the device (optical_flow.farneback_flow, the HIP kernels; its source is the Y
             plane of Y4M, the plane of a gray .npy, the rounded channel mean of an [N,H,W,C] .npy), in sub-batches of
             `batch` pairs, and every plane of the row warped along it (sub-sampled chroma along the resampled, rescaled
             flow): "optical_flow" is the reference evaluators' formula, frame 0 at p + flow / 2, which moves AGAINST
             the motion and is kept for comparison with them; "motion" the symmetric warp (frame 0 at p - flow / 2 +
             frame 1 at p + flow / 2 + 1) >> 1, the baseline a user wants to beat.
  planes     Y4M: "y", then "u" and "v" when the stream has chroma (on the grayscale route the chroma of an inserted
             frame is the neighbour average the route writes: that is what ends up in the file, so it is scored);
             .npy [N,H,W]: "gray"; .npy [N,H,W,C]: "c0".. (made planar by one permute per chunk).  The plane views
             go to `metrics.psnr_planes` / `ssim_planes` as they lie in the rows: no plane is copied.  A plane smaller
             than 7x7 gets PSNR only (its SSIM is NaN).
  raw        with `raw=` (one of stream.RAW_FORMATS, with width and height) the source is headerless tight frames, what
             `interpolate_raw_stream` takes, through `stream._open_raw`: "y" "u" "v" for nv12, the planar 4:2:2 /
             4:4:4 formats and uyvy422 / yuyv422, "r" "g" "b" (and "a": the alpha of an inserted frame is what the route
             writes, so it is scored) for packed RGB (the layout table, layout.py).  A plane is (name, offset, h, w, row
             pitch, sample step): interleaved planes (U V of nv12, the bytes of packed RGB, the byte positions of the
             capture formats) are scored where they lie - all components of a group in one `metrics.psnr_interleaved`
             call per method, SSIM plane by plane through the stepped kernel.  Contiguous copies of stepped planes exist
             for the flow methods only: the flow source (Y; for packed RGB the rounded mean of r, g, b) and the planes
             the warp kernel reads and writes, which are copied back into the prediction rows.
  scene cuts with `scene_cut=` (scene.py's threshold) every uploaded chunk also goes through `scene.pair_sad` - the whole
             frame as stored, the video loops' definition - and the interval sums are kept on the host by source
             interval: 8 bytes per source frame, the one quantity here that grows with the clip.  After the last chunk
             one `scene.score_window` over all of them gives the flags `scene.detect_cuts` gives on the whole clip.  A
             held-out frame t is EXCLUDED when interval t-1 (frames t-1, t) or interval t (frames t, t+1) is a cut: it
             is still predicted and scored (`per_frame` and `scored_frames` are those of a run without scene_cut), but
             `summary` is taken over the other targets.
  chunks     `chunk_spans` cuts the clip so that a chunk holds `chunk_frames` held-out frames, their neighbours
             included; the loop reads a chunk through the route's reader, uploads it, runs the methods, scores, keeps
             the few numbers per frame on the host and carries the overlap frames into the next chunk.  Every held-out
             frame is scored exactly once and a pair's forward does not depend on the pairs that share its call
             (`_padded_chunk`), so the result is the same to the last bit for every chunk_frames.

  resize     with `resize=` (resize.py) every uploaded chunk is resized on the device before frames are
             dropped: the held-out truth is the resized frame, the protocol of the reference's evaluator, and the route,
             planes, groups and pixel counts are those of the destination size; the host buffer keeps source frames.

Out of scope: pitched raw input, several GPUs.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import chroma as _chroma
from . import metrics, optical_flow, packed, scene
from . import resize as _resize
from . import retime as _retime
from .inference import _interleave_average_p10, _interleave_average_u8
from .layout import frame_layout
from .stream import _is_path, _open_npy, _open_raw, _open_y4m, check_chunk_frames, check_packing

TRIPLETS = ("sliding", "disjoint")
METHODS = ("unet", "linear", "repeat")
FLOW_METHODS = {"optical_flow": "reference", "motion": "motion"}   # method -> optical_flow.MODES
ALL_METHODS = METHODS + tuple(FLOW_METHODS)
FLOW_BACKEND = "hip (csrc/flow.hip.h, the definition of optical_flow.py; parity unpinned against OpenCV)"
STATS = ("average_psnr", "std_psnr", "min_psnr", "max_psnr", "average_ssim", "std_ssim", "min_ssim", "max_ssim",
         "psnr_of_mean_mse", "identical_frames")


# ---- the chunk arithmetic (pure) ----------------------------------------------------------------------------------
def _check_triplets(triplets) -> str:
    if triplets not in TRIPLETS:
        raise ValueError(f"triplets must be one of {list(TRIPLETS)}, got {triplets!r}")
    return triplets


def _step(triplets: str) -> int:
    return 2 if triplets == "disjoint" else 1


def _nominal(i: int, chunk_frames: int, triplets: str):
    """Chunk i of an endless clip -> (first source frame, frame count): `chunk_frames` held-out frames `step` apart,
    the frame before the first and the frame after the last."""
    step = _step(triplets)
    return i * chunk_frames * step, (chunk_frames - 1) * step + 3


def _span(i: int, n_frames: int, chunk_frames: int, triplets: str):
    """Chunk i of a clip of n_frames -> (first, count, targets), or None past the last held-out frame."""
    step = _step(triplets)
    first, count = _nominal(i, chunk_frames, triplets)
    count = min(count, n_frames - first)
    targets = list(range(first + 1, first + count - 1, step))
    if not targets:
        return None
    return first, targets[-1] + 2 - first, targets   # (a trailing frame no triplet uses is left out)


def chunk_spans(n_frames: int, chunk_frames: int, triplets: str = "sliding"):
    """The chunks of a hold-out run over n_frames source frames -> [(first source frame, frame count, target
    indices)], in order.  A chunk holds at most `chunk_frames` targets and both neighbours (target - 1, target + 1) of
    each; its frame count is at most chunk_frames + 2 ("sliding") or 2 x chunk_frames + 1 ("disjoint"); consecutive
    chunks share 2 / 1 frames; over all chunks every target appears exactly once."""
    c, triplets = check_chunk_frames(chunk_frames), _check_triplets(triplets)
    if isinstance(n_frames, bool) or not isinstance(n_frames, (int, np.integer)) or n_frames < 0:
        raise ValueError(f"n_frames must be a non-negative int, got {n_frames!r}")
    out, i = [], 0
    while True:
        s = _span(i, int(n_frames), c, triplets)
        if s is None:
            return out
        out.append(s)
        i += 1


# ---- sources ------------------------------------------------------------------------------------------------------
def _too_short(n):
    return ValueError(f"hold-out scoring needs at least 3 frames (two neighbours and the frame between them), the "
                      f"clip has {n}")


class _Source:
    """What scoring adds to an opened source (`stream._Opened`: the route, the reader, `upload`, `close`): the planes
    [(name, offset in the row, h, w, row pitch, sample step)] and the interleaved groups [(S, offset, h, w, row pitch,
    {plane name: component})], whose PSNR comes from one `psnr_interleaved` call (w: samples per component and row), both
    in samples as the layout table gives them; channels: the C of an [N,H,W,C] stack, whose planes are cut after a
    permute; lead: the plane names the flow is estimated on (one: that plane; three: their rounded mean); fps: the frame
    rate (a Fraction or None)."""

    def __init__(self, opened, planes, channels=0, groups=(), lead=None, fps=None):
        self.opened, self.channels, self.fps = opened, channels, fps
        self.planes, self.groups = [tuple(p) for p in planes], list(groups)
        self.lead = lead or (self.planes[0][0],)


def raw_planes(raw: str, height: int, width: int):
    """The planes and the interleaved groups of one tight frame of `raw` (stream.RAW_FORMATS), in samples: the layout
    table's (`layout.frame_layout`) -> (planes, groups)."""
    return frame_layout(raw, height, width)[:2]


def _open(model, src, batch, matrix, siting, src_fps, raw=None, width=None, height=None, size=None,
          rfilter="linear", packing=None, chroma="average") -> _Source:
    """The source of a scoring run through the video routes' openers, with their refusals; a clip whose frame count is
    known up front has at least three frames."""
    npy = _is_path(src) and os.fspath(src).lower().endswith(".npy")
    channels, lead, fps = 0, None, src_fps
    if raw is not None:
        if npy:
            raise ValueError(f"raw={raw!r} describes headerless video; a .npy stack carries its own shape (leave raw None)")
        _chroma.refuse_motion(chroma, f"raw {raw} video")
        opened = _open_raw(model, src, raw, width, height, False, batch, matrix, siting, size, rfilter, packing)
        if raw in packed.FORMATS:
            lead = ("r", "g", "b")
    else:
        check_packing(packing, raw)   # (refuses: Y4M and .npy video take no packing)
        if width is not None or height is not None:
            raise ValueError("width and height describe raw video: pass raw= with them")
        if npy:
            _chroma.refuse_motion(chroma, ".npy video")
            opened = _open_npy(model, src, batch, size, rfilter)
            channels = opened.shape[2] if len(opened.shape) == 3 else 0
        else:
            opened = _open_y4m(model, src, False, batch, matrix, siting, size, rfilter, count=True, chroma=chroma)
            if fps is None:
                try:
                    fps = _retime.parse_fps(tuple(int(v) for v in opened.fps))
                except ValueError:
                    pass
    if opened.count is not None and opened.count < 3:
        opened.close()
        raise _too_short(opened.count)
    return _Source(opened, opened.layout.planes, channels, opened.layout.groups, lead, fps)


# ---- one chunk on the device ----------------------------------------------------------------------------------------
def _predict(method: str, route, d: torch.Tensor) -> torch.Tensor:
    """The k-1 predicted rows of a decimated chunk d [k, row]."""
    if method == "unet":
        return route.run(d, 2)[1::2]
    if method == "repeat":
        return d[:-1]
    if route.bits == 10:   # (the 16-bit words as unsigned samples, as the grayscale route averages its chroma)
        return _interleave_average_p10(d.to(torch.int32) & 0xFFFF)[1::2].to(torch.int16)
    return _interleave_average_u8(d)[1::2]


def _predict_flow(methods, source: _Source, d: torch.Tensor, batch: int) -> dict:
    """The k-1 predicted rows of a decimated chunk d [k, row] for each of the flow methods asked for: one flow per
    pair, shared by the methods, `batch` pairs at a time (a pair's flow and warp do not depend on the pairs beside it)."""
    bits, k = source.opened.route.bits, d.shape[0]
    if source.channels:   # [N,H,W,C]: planar copies, flow on the rounded channel mean
        c = source.channels
        _, _, h, w = source.planes[0][:4]
        planar = d.reshape(k, h, w, c).permute(0, 3, 1, 2).contiguous()
        planes = [planar[:, i] for i in range(c)]
        lead = ((planar.sum(1, dtype=torch.int32) * 2 + c) // (2 * c)).to(torch.uint8)
        outs = {m: torch.empty((k - 1, c, h, w), dtype=d.dtype, device=d.device) for m in methods}
        dst = {m: [outs[m][:, i] for i in range(c)] for m in methods}
    else:
        views = _plane_views(d, source)
        stepped = [p[5] != 1 for p in source.planes]
        # (the warp kernel reads and writes rows of stride 1: a stepped plane goes through a contiguous copy)
        planes = [v.contiguous() if st else v for v, st in zip(views, stepped)]
        by_name = {p[0]: v for p, v in zip(source.planes, planes)}
        if len(source.lead) == 1:
            lead = by_name[source.lead[0]]
        else:   # packed RGB: the rounded mean of r, g and b (not alpha), the [N,H,W,C] .npy rule
            c = len(source.lead)
            total = sum(by_name[n].to(torch.int32) for n in source.lead)
            lead = ((total * 2 + c) // (2 * c)).to(torch.uint8)
        outs = {m: torch.empty_like(d[:-1]) for m in methods}
        back = {m: _plane_views(outs[m], source) for m in methods}
        dst = {m: [torch.empty_like(p[:-1]) if st else o for p, o, st in zip(planes, back[m], stepped)] for m in methods}
    for s in range(0, k - 1, batch):
        e = min(s + batch, k - 1)
        flow = optical_flow.farneback_flow(lead[s:e], lead[s + 1:e + 1], "hip", bits=bits)
        for m in methods:
            for p, o in zip(planes, dst[m]):
                optical_flow.warp(p[s:e], p[s + 1:e + 1], flow, FLOW_METHODS[m], "hip", bits=bits, out=o[s:e])
    if source.channels:
        return {m: outs[m].permute(0, 2, 3, 1).reshape(k - 1, -1) for m in methods}
    for m in methods:
        for o, b, st in zip(dst[m], back[m], stepped):
            if st:
                b.copy_(o)
    return outs


def _strided(rows: torch.Tensor, off: int, shape, strides):
    return rows.as_strided((rows.shape[0],) + tuple(shape), (rows.stride(0),) + tuple(strides), rows.storage_offset() + off)


def _plane_views(rows: torch.Tensor, source: _Source):
    """rows [m, row] (any row stride) -> the planes' [m, h, w] views, in the order of source.planes."""
    if source.channels:
        _, _, h, w = source.planes[0][:4]
        planar = rows.reshape(rows.shape[0], h, w, source.channels).permute(0, 3, 1, 2).contiguous()
        return [planar[:, c] for c in range(source.channels)]
    return [_strided(rows, off, (h, w), (pitch, step)) for _, off, h, w, pitch, step in source.planes]


def _group_views(rows: torch.Tensor, source: _Source):
    """rows [m, row] -> the interleaved groups' [m, h, w, S] views, in the order of source.groups."""
    return [_strided(rows, off, (h, w, comp), (pitch, comp, 1)) for comp, off, h, w, pitch, _ in source.groups]


def _score_chunk(source: _Source, methods, d_all: torch.Tensor, n_targets: int, step: int, batch: int = 8):
    """-> {method: {plane: (psnr, ssim, sse)}}, host arrays over the chunk's targets in order."""
    flow_methods = [m for m in methods if m in FLOW_METHODS]
    bits = source.opened.route.bits
    res = {m: {p[0]: (np.empty(n_targets), np.full(n_targets, np.nan), np.empty(n_targets, np.uint64))
               for p in source.planes} for m in methods}
    grouped = {name for g in source.groups for name in g[5]}
    for off in range(3 - step):   # sliding: the frames at even offsets, then those at odd offsets
        d = d_all[off::2].contiguous()
        k = d.shape[0]
        if k < 2:
            continue
        truth_rows = d_all[off + 1::2][:k - 1]
        truth, truth_groups = _plane_views(truth_rows, source), _group_views(truth_rows, source)
        where = slice(off, None, 2) if step == 1 else slice(None)
        flowed = _predict_flow(flow_methods, source, d, batch) if flow_methods else {}
        for m in methods:
            rows = flowed[m] if m in flowed else _predict(m, source.opened.route, d)
            # every component of an interleaved group in one pass over its samples
            for g, p, t in zip(source.groups, _group_views(rows, source), truth_groups):
                ps, sse = metrics.psnr_interleaved(p, t, bits, return_sse=True)
                ps, sse = ps.cpu().numpy(), sse.cpu().numpy().view(np.uint64)
                for name, comp in g[5].items():
                    res[m][name][0][where], res[m][name][2][where] = ps[:, comp], sse[:, comp]
            for (name, _, h, w, _, _), p, t in zip(source.planes, _plane_views(rows, source), truth):
                out = res[m][name]
                if name not in grouped:
                    ps, sse = metrics.psnr_planes(p, t, bits, return_sse=True)
                    out[0][where] = ps.cpu().numpy()
                    out[2][where] = sse.cpu().numpy().view(np.uint64)
                if h >= 7 and w >= 7:
                    out[1][where] = metrics.ssim_planes(p, t, bits).cpu().numpy()
    return res


# ---- the statistics ---------------------------------------------------------------------------------------------------
def _stats(psnr, ssim, sse, pixels: int, peak: int) -> dict:
    fin = psnr[np.isfinite(psnr)]
    out = {}
    for key, v in (("psnr", fin), ("ssim", ssim[~np.isnan(ssim)])):
        for stat, fn in (("average", np.mean), ("std", np.std), ("min", np.min), ("max", np.max)):
            # (every frame identical: no finite PSNR, the average is +inf; a plane below 7x7 has no SSIM)
            out[f"{stat}_{key}"] = float(fn(v)) if v.size else (float("nan") if key == "ssim" or stat == "std"
                                                                else float("inf"))
    mse = float(np.mean(sse.astype(np.float64))) / pixels
    out["psnr_of_mean_mse"] = float("inf") if mse == 0 else 10.0 * math.log10(peak * peak / mse)
    out["identical_frames"] = int((sse == 0).sum())
    return {k: out[k] for k in STATS}


def _kept_stats(a: dict, keep, pixels: int, peak: int) -> dict:
    """`_stats` over the targets of the mask `keep` (None: all of them); with none left every figure is NaN and
    identical_frames 0."""
    if keep is None:
        return _stats(a["psnr"], a["ssim"], a["sse"], pixels, peak)
    if not keep.any():
        return {k: 0 if k == "identical_frames" else float("nan") for k in STATS}
    return _stats(a["psnr"][keep], a["ssim"][keep], a["sse"][keep], pixels, peak)


def excluded_targets(cut_flags, scored_frames) -> np.ndarray:
    """bool mask over `scored_frames`: held-out frame t is excluded when interval t-1 (frames t-1, t) or interval t
    (frames t, t+1) is a cut.  cut_flags: one value per source interval."""
    cut = np.asarray(cut_flags).astype(bool)
    t = np.asarray(scored_frames, dtype=np.int64)
    return cut[t - 1] | cut[t] if t.size else np.zeros(0, bool)


@torch.no_grad()
def score_video(model, src, *, triplets: str = "sliding", methods=METHODS, batch: int = 8, chunk_frames: int = 32,
                matrix: str = "bt709", siting=None, src_fps=None, raw=None, width=None, height=None,
                scene_cut=None, resize=None, resize_filter: str = "linear", packing=None,
                chroma: str = "average") -> dict:
    """Hold-out scores of `model` on a clip (methods: any of ALL_METHODS; with "optical_flow" or "motion" the result
    also has "flow_backend").  src: a path (.y4m, or a uint8 .npy stack [N,H,W] / [N,H,W,C]) or a
    readable binary file object carrying Y4M (a pipe): what `interpolate_y4m_stream` / `interpolate_npy_stream` take
    for this model, with those routes' refusals; with raw (one of stream.RAW_FORMATS), width and height: a path or a
    readable binary file object of headerless tight frames, what `interpolate_raw_stream` takes, with that route's
    refusals (a grayscale model, a missing size, an odd width of uyvy422 / yuyv422).  batch / matrix / siting: the
    routes' arguments; chunk_frames: held-out
    frames per chunk (memory: chunk_frames + 2 source frames, "disjoint" 2 x chunk_frames + 1, on the host and on the
    device, beside each method's predictions); src_fps: the clip's frame rate where the stream carries none (kept in
    the result for time stamps); scene_cut: None, or scene.py's threshold in (0, 100]: held-out frames next to a cut
    are left out of the summary (8 bytes per source frame are kept for it).  resize: None, or (width, height) / "WxH":
    the clip is resized on the device (resize.py) before frames are dropped, so the held-out truth is the
    resized frame - the protocol of the reference's evaluator, which scores a checkpoint at its training size against a
    ground truth resized the same way; the route, planes and pixel counts are those of the new size, width / height stay
    the size of a raw source, and the result gains "resize" [W, H] and "source_size" [w, h].  resize_filter: "linear" or
    "area" (alias-free down-scaling; an error without `resize`, and where a plane would grow or shrink
    more than 64 times); with a filter other than "linear" the result also has "resize_filter".  packing: None, or with
    raw="yuv422p10le" one of wire10.PACKINGS ("v210", "y210le", "p210le"): the source is tight frames of
    that packing, unpacked on the device where a chunk is uploaded (before `resize`); the planes are scored where they
    lie in the working format, so the result equals that of the unpacked clip.  chroma: "average" or "motion", the
    chroma of the "unet" method's frames on colour Y4M video through the grayscale network (chroma.py; its
    `u` and `v` planes show what carrying the chroma along the motion buys on this footage); "motion" is refused for an
    RGB model, a .npy stack and raw video; the result names the mode as "chroma".  Every argument is
    checked before any GPU work.  Returns

      {"frames", "triplets", "bits", "peak", "planes", "methods", "fps", "scored_frames": int64 source frame indices,
       "per_frame": {method: {plane: {"psnr": f64[], "ssim": f64[], "sse": uint64[]}}},
       "summary": {method: {plane: {average_ / std_ / min_ / max_psnr over the finite values (numpy mean, population
                   std), the same of ssim, psnr_of_mean_mse, identical_frames}}}}

    and, with scene_cut, "scene_cut", "scene_scores" (float64 [frames - 1]), "cut_intervals" (int64), "excluded_frames"
    (int64 source indices) and "excluded" (bool, aligned with scored_frames); the summary is then over the targets
    that are not excluded (all NaN and identical_frames 0 if none is left)."""
    triplets = _check_triplets(triplets)
    methods = tuple([methods] if isinstance(methods, str) else methods)
    for m in methods:
        if m not in ALL_METHODS:
            raise ValueError(f"unknown method {m!r}; choose from {list(ALL_METHODS)}")
    if not methods or len(set(methods)) != len(methods):
        raise ValueError(f"methods: one or more of {list(ALL_METHODS)}, each once")
    c = check_chunk_frames(chunk_frames)
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError(f"batch must be a positive int, got {batch!r}")
    thr = scene.check_threshold(scene_cut)
    _chroma.check_mode(chroma)
    if src_fps is not None:
        src_fps = _retime.parse_fps(src_fps)
    size = None if resize is None else _resize.check_size(resize)
    rfilter = _resize.check_resize_filter(resize, resize_filter)
    source = _open(model, src, batch, matrix, siting, src_fps, raw, width, height, size, rfilter, packing, chroma)
    try:
        opened, step = source.opened, _step(triplets)
        route, rs = opened.route, opened.rs
        dev = next(model.parameters()).device

        def upload(a):   # (the host buffer holds frames as they are on the wire: the source size, the packing)
            return opened.upload(a, dev)
        buf = np.empty((_nominal(0, c, triplets)[1], opened.row), dtype=route.ndtype)
        have = frames = 0          # rows of buf carried over; frames read so far
        scored, parts = [], []
        sad = []                   # with scene_cut: (first interval, int64 sums) of every chunk: 8 bytes per frame
        i = 0
        while True:
            first, want = _nominal(i, c, triplets)
            got = opened.reader.read_into(buf[have:], want - have)
            frames += got
            span = _span(i, frames, c, triplets)
            count = 0 if span is None else span[1]
            d_up = None
            if thr is not None and got and have + got >= 2:
                # every frame read, a trailing one no triplet uses included: the flags are the whole clip's
                up = have + got
                d_up = upload(buf[:up])
                sums = scene.pair_sad(d_up, route.bits).cpu().numpy()
                # (an interval two chunks share has the same sum in both: only the new ones are kept)
                sad.append((first + max(have - 1, 0), sums[max(have - 1, 0):]))
            if span is None:
                break
            _, count, targets = span
            d_all = upload(buf[:count]) if d_up is None else d_up[:count]
            parts.append(_score_chunk(source, methods, d_all, len(targets), step, int(batch)))
            scored += targets
            if have + got < want:   # the stream ended inside this chunk
                break
            have = want - c * step
            buf[:have] = buf[c * step:want].copy()
            i += 1
        if frames < 3:
            raise _too_short(frames)
    finally:
        opened.close()
    peak = 255 if route.bits == 8 else 1023
    names = [p[0] for p in source.planes]
    per = {m: {p: {key: np.concatenate([part[m][p][j] for part in parts])
                   for j, key in enumerate(("psnr", "ssim", "sse"))} for p in names} for m in methods}
    pixels = {p[0]: p[2] * p[3] for p in source.planes}
    scored = np.asarray(scored, dtype=np.int64)
    cuts = keep = None
    if thr is not None:
        sums = np.empty(frames - 1, dtype=np.int64)
        for at, part in sad:
            sums[at:at + part.size] = part
        scores, flags = scene.score_window(torch.from_numpy(sums).to(dev), route.row, route.bits, thr)
        cuts = flags.cpu().numpy().astype(bool)
        excluded = excluded_targets(cuts, scored)
        keep = ~excluded
    out = {"frames": frames, "triplets": triplets, "bits": route.bits, "peak": peak, "planes": names,
           "methods": list(methods), "fps": None if source.fps is None else (source.fps.numerator,
                                                                             source.fps.denominator),
           "scored_frames": scored, "per_frame": per, "chroma": chroma,
           "summary": {m: {p: _kept_stats(per[m][p], keep, pixels[p], peak) for p in names} for m in methods}}
    if thr is not None:
        out.update({"scene_cut": thr, "scene_scores": scores.cpu().numpy(),
                    "cut_intervals": np.flatnonzero(cuts).astype(np.int64), "excluded_frames": scored[excluded],
                    "excluded": excluded})
    if any(m in FLOW_METHODS for m in methods):
        out["flow_backend"] = FLOW_BACKEND
    if rs is not None:
        out.update({"resize": list(rs.size), "source_size": list(rs.source_size)})
        if rs.filter != "linear":
            out["resize_filter"] = rs.filter
    return out


# ---- the result as text ---------------------------------------------------------------------------------------------
def _json_number(v):
    v = float(v)
    return v if math.isfinite(v) else ("nan" if math.isnan(v) else "inf" if v > 0 else "-inf")


def to_jsonable(result: dict) -> dict:
    """The result with arrays as lists and inf / NaN as the strings "inf" / "-inf" / "nan" (strict JSON has no such
    numbers); `float()` of an entry gives the value back."""
    def conv(v):
        if isinstance(v, dict):
            return {k: conv(x) for k, x in v.items()}
        if isinstance(v, np.ndarray):
            if v.dtype.kind == "b":
                return [bool(x) for x in v]
            return [int(x) for x in v] if v.dtype.kind in "iu" else [_json_number(x) for x in v]
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return _json_number(v)
        return int(v) if isinstance(v, np.integer) else v
    return conv(result)


def csv_lines(result: dict):
    """A header line, then one line per scored frame: frame, time (seconds; empty without a frame rate), excluded
    (0 / 1; only in a result of a scene_cut run), then psnr, ssim and sse of every method and plane."""
    cols = [(m, p) for m in result["methods"] for p in result["planes"]]
    excluded = result.get("excluded")
    yield ",".join(["frame", "time"] + (["excluded"] if excluded is not None else [])
                   + [f"{m}_{p}_{k}" for m, p in cols for k in ("psnr", "ssim", "sse")])
    fps = result["fps"]
    for j, f in enumerate(result["scored_frames"]):
        row = [str(int(f)), "" if fps is None else repr(int(f) * fps[1] / fps[0])]
        if excluded is not None:
            row.append(str(int(excluded[j])))
        for m, p in cols:
            a = result["per_frame"][m][p]
            row += [repr(float(a["psnr"][j])), repr(float(a["ssim"][j])), str(int(a["sse"][j]))]
        yield ",".join(row)


def summary_table(result: dict) -> str:
    mw = max([8] + [len(m) + 1 for m in result["methods"]])   # the method column fits "optical_flow"
    left_out = ""
    if "excluded" in result:
        n_cuts = len(result["cut_intervals"])
        left_out = f", {int(np.sum(result['excluded']))} left out at {n_cuts} scene cut{'' if n_cuts == 1 else 's'}"
    lines = [f"{result['frames']} frames, {len(result['scored_frames'])} held out ({result['triplets']}), "
             f"{result['bits']}-bit, peak {result['peak']}{left_out}"]
    if "resize" in result:
        (w, h), (sw, sh) = result["resize"], result["source_size"]
        how = f" with the {result['resize_filter']} filter" if "resize_filter" in result else ""
        lines.append(f"scored at {w}x{h} (the {sw}x{sh} clip resized on the device{how} before frames were held out)")
    lines += [f"{'method':<{mw}}{'plane':<6}{'PSNR mean':>11}{'std':>8}{'min':>9}{'max':>9}{'of mean MSE':>13}"
             f"{'SSIM mean':>11}{'min':>9}{'identical':>11}"]
    for m in result["methods"]:
        for p in result["planes"]:
            s = result["summary"][m][p]
            lines.append(f"{m:<{mw}}{p:<6}{s['average_psnr']:>11.3f}{s['std_psnr']:>8.3f}{s['min_psnr']:>9.3f}"
                         f"{s['max_psnr']:>9.3f}{s['psnr_of_mean_mse']:>13.3f}{s['average_ssim']:>11.5f}"
                         f"{s['min_ssim']:>9.5f}{s['identical_frames']:>11d}")
    return "\n".join(lines)
