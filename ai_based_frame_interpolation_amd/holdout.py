"""Hold-out scoring of a checkpoint on real video: drop frames of a clip, rebuild each from its two
neighbours, and compare with the frame that was really there - plane by plane, on the device, in memory bounded by the
chunk.

  triplets   "disjoint": frames 0, 2, 4, ... are the inputs and 1, 3, 5, ... the held-out frames ((n-1)//2 of them).
             "sliding": the reference's triplet set (model/train.py: (f[i], f[i+2]) -> f[i+1]), every frame 1 .. n-2;
             it is the disjoint evaluation of the clip together with that of the clip without its first frame.
  methods    each turns a decimated chunk d [k, row] into [2k-1, out_row] rows whose odd rows are the predictions:
             "unet" is `route.run(d, 2)`, the forward of whatever route the clip takes (stream.py: `_y4m_route`,
             `_npy_route`, with their refusals); "linear" the project's integer average (a + b + 1) >> 1 of every
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
  chunks     `chunk_spans` cuts the clip so that a chunk holds `chunk_frames` held-out frames, their neighbours
             included; the loop reads a chunk through the route's reader, uploads it, runs the methods, scores, keeps
             the few numbers per frame on the host and carries the overlap frames into the next chunk.  Every held-out
             frame is scored exactly once and a pair's forward does not depend on the pairs that share its call
             (`_padded_chunk`), so the result is the same to the last bit for every chunk_frames.

Out of scope: raw NV12 and packed-RGB input, leaving out triplets that straddle a scene cut (the per-frame arrays let a
caller filter), several GPUs.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

from . import imageio_lite, metrics, optical_flow
from . import retime as _retime
from .inference import _interleave_average_p10, _interleave_average_u8
from .stream import _NpyRows, _is_path, _npy_route, _y4m_route, check_chunk_frames

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
    """route, reader, the planes [(name, offset in the row, h, w)] (channels: the C of an [N,H,W,C] stack, whose planes
    are cut after a permute), the frame rate (a Fraction or None) and close()."""

    def __init__(self, route, reader, planes, channels, fps, close):
        self.route, self.reader, self.planes, self.channels, self.fps, self.close = (route, reader, planes, channels,
                                                                                     fps, close)


def _open(model, src, batch, matrix, siting, src_fps) -> _Source:
    if _is_path(src) and os.fspath(src).lower().endswith(".npy"):
        mm = np.load(src, mmap_mode="r")
        if mm.dtype != np.uint8 or mm.ndim not in (3, 4):
            raise ValueError("expected a uint8 .npy stack [N,H,W] or [N,H,W,3]")
        route = _npy_route(model, mm.shape[1:], batch)
        if mm.shape[0] < 3:
            raise _too_short(mm.shape[0])
        h, w = mm.shape[1:3]
        if mm.ndim == 3:
            planes, channels = [("gray", 0, h, w)], 0
        else:
            channels = mm.shape[3]
            planes = [(f"c{i}", i * h * w, h, w) for i in range(channels)]
        return _Source(route, _NpyRows(mm), planes, channels, src_fps, lambda: None)
    reader = imageio_lite.Y4MReader(src)
    try:
        hdr = reader.header
        route = _y4m_route(model, hdr, False, batch, matrix, siting)
        h, w, (hc, wc) = hdr["height"], hdr["width"], hdr["chroma"]
        planes = [("y", 0, h, w)]
        if hc * wc:
            planes += [("u", h * w, hc, wc), ("v", h * w + hc * wc, hc, wc)]
        fps = src_fps
        if fps is None:
            try:
                fps = _retime.parse_fps(tuple(int(v) for v in hdr["fps"]))
            except ValueError:
                fps = None
        if _is_path(src) and os.path.isfile(src):
            n = imageio_lite.y4m_frame_count(src)
            if n < 3:
                raise _too_short(n)
    except BaseException:
        reader.close()
        raise
    return _Source(route, reader, planes, 0, fps, reader.close)


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
    bits, k = source.route.bits, d.shape[0]
    if source.channels:   # [N,H,W,C]: planar copies, flow on the rounded channel mean
        c = source.channels
        _, _, h, w = source.planes[0]
        planar = d.reshape(k, h, w, c).permute(0, 3, 1, 2).contiguous()
        planes = [planar[:, i] for i in range(c)]
        lead = ((planar.sum(1, dtype=torch.int32) * 2 + c) // (2 * c)).to(torch.uint8)
        outs = {m: torch.empty((k - 1, c, h, w), dtype=d.dtype, device=d.device) for m in methods}
        dst = {m: [outs[m][:, i] for i in range(c)] for m in methods}
    else:
        planes = _plane_views(d, source)
        lead = planes[0]
        outs = {m: torch.empty_like(d[:-1]) for m in methods}
        dst = {m: _plane_views(outs[m], source) for m in methods}
    for s in range(0, k - 1, batch):
        e = min(s + batch, k - 1)
        flow = optical_flow.farneback_flow(lead[s:e], lead[s + 1:e + 1], "hip", bits=bits)
        for m in methods:
            for p, o in zip(planes, dst[m]):
                optical_flow.warp(p[s:e], p[s + 1:e + 1], flow, FLOW_METHODS[m], "hip", bits=bits, out=o[s:e])
    if source.channels:
        return {m: outs[m].permute(0, 2, 3, 1).reshape(k - 1, -1) for m in methods}
    return outs


def _plane_views(rows: torch.Tensor, source: _Source):
    """rows [m, row] (any row stride) -> the planes' [m, h, w] views, in the order of source.planes."""
    if source.channels:
        _, _, h, w = source.planes[0]
        planar = rows.reshape(rows.shape[0], h, w, source.channels).permute(0, 3, 1, 2).contiguous()
        return [planar[:, c] for c in range(source.channels)]
    return [rows[:, off:off + h * w].unflatten(1, (h, w)) for _, off, h, w in source.planes]


def _score_chunk(source: _Source, methods, d_all: torch.Tensor, n_targets: int, step: int, batch: int = 8):
    """-> {method: {plane: (psnr, ssim, sse)}}, host arrays over the chunk's targets in order."""
    flow_methods = [m for m in methods if m in FLOW_METHODS]
    bits = source.route.bits
    res = {m: {p[0]: (np.empty(n_targets), np.full(n_targets, np.nan), np.empty(n_targets, np.uint64))
               for p in source.planes} for m in methods}
    for off in range(3 - step):   # sliding: the frames at even offsets, then those at odd offsets
        d = d_all[off::2].contiguous()
        k = d.shape[0]
        if k < 2:
            continue
        truth = _plane_views(d_all[off + 1::2][:k - 1], source)
        where = slice(off, None, 2) if step == 1 else slice(None)
        flowed = _predict_flow(flow_methods, source, d, batch) if flow_methods else {}
        for m in methods:
            pred = _plane_views(flowed[m] if m in flowed else _predict(m, source.route, d), source)
            for (name, _, h, w), p, t in zip(source.planes, pred, truth):
                ps, sse = metrics.psnr_planes(p, t, bits, return_sse=True)
                out = res[m][name]
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


@torch.no_grad()
def score_video(model, src, *, triplets: str = "sliding", methods=METHODS, batch: int = 8, chunk_frames: int = 32,
                matrix: str = "bt709", siting=None, src_fps=None) -> dict:
    """Hold-out scores of `model` on a clip (methods: any of ALL_METHODS; with "optical_flow" or "motion" the result
    also has "flow_backend").  src: a path (.y4m, or a uint8 .npy stack [N,H,W] / [N,H,W,C]) or a
    readable binary file object carrying Y4M (a pipe): what `interpolate_y4m_stream` / `interpolate_npy_stream` take
    for this model, with those routes' refusals.  batch / matrix / siting: the routes' arguments; chunk_frames: held-out
    frames per chunk (memory: chunk_frames + 2 source frames, "disjoint" 2 x chunk_frames + 1, on the host and on the
    device, beside each method's predictions); src_fps: the clip's frame rate where the stream carries none (kept in
    the result for time stamps).  Every argument is checked before any GPU work.  Returns

      {"frames", "triplets", "bits", "peak", "planes", "methods", "fps", "scored_frames": int64 source frame indices,
       "per_frame": {method: {plane: {"psnr": f64[], "ssim": f64[], "sse": uint64[]}}},
       "summary": {method: {plane: {average_ / std_ / min_ / max_psnr over the finite values (numpy mean, population
                   std), the same of ssim, psnr_of_mean_mse, identical_frames}}}}"""
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
    if src_fps is not None:
        src_fps = _retime.parse_fps(src_fps)
    source = _open(model, src, batch, matrix, siting, src_fps)
    try:
        route, step = source.route, _step(triplets)
        dev = next(model.parameters()).device
        buf = np.empty((_nominal(0, c, triplets)[1], route.row), dtype=route.ndtype)
        have = frames = 0          # rows of buf carried over; frames read so far
        scored, parts = [], []
        i = 0
        while True:
            first, want = _nominal(i, c, triplets)
            got = source.reader.read_into(buf[have:], want - have)
            frames += got
            span = _span(i, frames, c, triplets)
            if span is None:
                break
            _, count, targets = span
            d_all = torch.from_numpy(buf[:count].view(np.int16) if route.bits == 10 else buf[:count]).to(dev)
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
        source.close()
    peak = 255 if route.bits == 8 else 1023
    names = [p[0] for p in source.planes]
    per = {m: {p: {key: np.concatenate([part[m][p][j] for part in parts])
                   for j, key in enumerate(("psnr", "ssim", "sse"))} for p in names} for m in methods}
    pixels = {p[0]: p[2] * p[3] for p in source.planes}
    out = {"frames": frames, "triplets": triplets, "bits": route.bits, "peak": peak, "planes": names,
           "methods": list(methods), "fps": None if source.fps is None else (source.fps.numerator,
                                                                             source.fps.denominator),
           "scored_frames": np.asarray(scored, dtype=np.int64), "per_frame": per,
           "summary": {m: {p: _stats(per[m][p]["psnr"], per[m][p]["ssim"], per[m][p]["sse"], pixels[p], peak)
                           for p in names} for m in methods}}
    if any(m in FLOW_METHODS for m in methods):
        out["flow_backend"] = FLOW_BACKEND
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
            return [int(x) for x in v] if v.dtype.kind in "iu" else [_json_number(x) for x in v]
        if isinstance(v, (list, tuple)):
            return [conv(x) for x in v]
        if isinstance(v, (float, np.floating)):
            return _json_number(v)
        return int(v) if isinstance(v, np.integer) else v
    return conv(result)


def csv_lines(result: dict):
    """A header line, then one line per scored frame: frame, time (seconds; empty without a frame rate), then psnr,
    ssim and sse of every method and plane."""
    cols = [(m, p) for m in result["methods"] for p in result["planes"]]
    yield ",".join(["frame", "time"] + [f"{m}_{p}_{k}" for m, p in cols for k in ("psnr", "ssim", "sse")])
    fps = result["fps"]
    for j, f in enumerate(result["scored_frames"]):
        row = [str(int(f)), "" if fps is None else repr(int(f) * fps[1] / fps[0])]
        for m, p in cols:
            a = result["per_frame"][m][p]
            row += [repr(float(a["psnr"][j])), repr(float(a["ssim"][j])), str(int(a["sse"][j]))]
        yield ",".join(row)


def summary_table(result: dict) -> str:
    mw = max([8] + [len(m) + 1 for m in result["methods"]])   # the method column fits "optical_flow"
    lines = [f"{result['frames']} frames, {len(result['scored_frames'])} held out ({result['triplets']}), "
             f"{result['bits']}-bit, peak {result['peak']}",
             f"{'method':<{mw}}{'plane':<6}{'PSNR mean':>11}{'std':>8}{'min':>9}{'max':>9}{'of mean MSE':>13}"
             f"{'SSIM mean':>11}{'min':>9}{'identical':>11}"]
    for m in result["methods"]:
        for p in result["planes"]:
            s = result["summary"][m][p]
            lines.append(f"{m:<{mw}}{p:<6}{s['average_psnr']:>11.3f}{s['std_psnr']:>8.3f}{s['min_psnr']:>9.3f}"
                         f"{s['max_psnr']:>9.3f}{s['psnr_of_mean_mse']:>13.3f}{s['average_ssim']:>11.5f}"
                         f"{s['min_ssim']:>9.5f}{s['identical_frames']:>11d}")
    return "\n".join(lines)
