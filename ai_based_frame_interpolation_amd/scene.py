"""Scene cuts in the video loops: detect a hard cut between two input frames and hold the frame before it.

The network sees only the two frames of a pair, so across a hard cut it would insert a double exposure of two
unrelated pictures.  With `scene_cut=<threshold>` the device-resident video loops (`inference.interpolate_sequence*`,
`FrameInterpolator.interpolate_video`) detect cuts once on the input frames and replace every frame they insert into
a cut interval by a byte copy of the frame before the cut (sample-and-hold), so the cut stays where the source has it.
The definition is our own (the reference has no video loop).  For N frames and the N-1 intervals i:

  sad[i]    sum over every sample of the frame as stored (all planes) of |F[i+1] - F[i]|, exact int64; 10-bit samples
            above 1023 read as 1023
  mafd[i]   sad[i] * 100.0 / count / 2**bits in float64, in that order (count = samples per frame): FFmpeg scdet's
            0-100 scale
  score[i]  min(mafd[i], |mafd[i] - mafd[i-1]|, |mafd[i] - mafd[i+1]|), a missing neighbour left out
  cut       score[i] >= threshold, a threshold in (0, 100]; 10 separates a cut from ordinary motion

The score is two-sided so that neither the first interval of a fast pan nor the interval after a cut in high-motion
footage is flagged.  Not flagged: a one-frame flash (two adjacent jumps) and fades (by design).

Every step is a HIP kernel (csrc/scene.hip.h): `fiunet_pair_sad_u8` / `fiunet_pair_sad_p10`, `fiunet_scene_cuts`,
`fiunet_hold_cut_frames`.  The flags stay on the device; the hold reads them there.
"""
from __future__ import annotations

import math
import numbers
from typing import Sequence, Tuple, Union

import torch

from . import _native

Stacks = Union[torch.Tensor, Sequence[torch.Tensor]]


def check_threshold(scene_cut) -> float | None:
    """None -> None (off); a real number in (0, 100] -> float; anything else (0, negative, above 100, NaN, bool, str)
    -> ValueError naming `scene_cut`.  Called before any GPU work."""
    if scene_cut is None:
        return None
    if isinstance(scene_cut, bool) or not isinstance(scene_cut, numbers.Real):
        raise ValueError(f"scene_cut must be None or a number in (0, 100], got {scene_cut!r}")
    v = float(scene_cut)
    if math.isnan(v) or not 0.0 < v <= 100.0:
        raise ValueError(f"scene_cut must be None or a number in (0, 100], got {scene_cut!r}")
    return v


def _stacks(stacks: Stacks, bits: int):
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    st = [stacks] if isinstance(stacks, torch.Tensor) else list(stacks)
    if not st:
        raise ValueError("pair_sad needs at least one frame stack")
    n, dev = st[0].shape[0], st[0].device
    want = (torch.uint8,) if bits == 8 else (torch.int16, torch.uint16)
    for s in st:
        if s.dtype not in want:
            raise ValueError(f"{bits}-bit frame stacks must be {' or '.join(str(d) for d in want)}, got {s.dtype}")
        if s.shape[0] != n or s.device != dev:
            raise ValueError("every frame stack must hold the same frames on the same device")
        if not s.is_cuda:
            raise RuntimeError("frame stacks must be on the GPU: there is no CPU path in this package")
        if not s.is_contiguous():
            raise ValueError("every frame stack must be contiguous")
    return st, n, dev


@torch.no_grad()
def pair_sad(stacks: Stacks, bits: int) -> torch.Tensor:
    """int64 [N-1] device tensor: sum |F[i+1] - F[i]| over every sample of every stack.  `stacks`: one contiguous device
    stack [N, ...] or several holding planes of the same N frames (Y, U, V); uint8 at 8 bits, the int16 (or uint16)
    words of 10-bit codes at 10."""
    st, n, dev = _stacks(stacks, bits)
    sums = torch.zeros(max(n - 1, 0), dtype=torch.int64, device=dev)
    if n >= 2:   # (an empty tensor has no data pointer to hand over)
        with torch.cuda.device(dev):
            for s in st:
                _native.pair_sad(s, sums, bits)
    return sums


PEAK_SEGMENT = 64   # samples per segment of `pair_peak`


@torch.no_grad()
def pair_peak(stacks: Stacks, bits: int) -> torch.Tensor:
    """int32 [N-1] device tensor: for every interval the largest sum of |F[i+1] - F[i]| over the aligned 64-sample
    segments of a frame as stored (counted from the frame's first sample; the last one may be short; 10-bit words above
    1023 read as 1023), the maximum taken over every stack.  The measure of repeated frames (retime.py):
    a small object moving in a static shot has a tiny frame mean and a large segment sum.  `stacks` as for `pair_sad`;
    the segments of each stack are counted from that stack's frames."""
    st, n, dev = _stacks(stacks, bits)
    peaks = torch.zeros(max(n - 1, 0), dtype=torch.int32, device=dev)
    if n >= 2:
        with torch.cuda.device(dev):
            for s in st:
                _native.pair_peak(s, peaks, bits)
    return peaks


@torch.no_grad()
def detect_cuts(stacks: Stacks, threshold: float, bits: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (scores float64 [N-1], flags uint8 [N-1]), both on the device: what `scene_cut=threshold` would hold."""
    thr = check_threshold(threshold)
    if thr is None:
        raise ValueError("detect_cuts needs a threshold in (0, 100]")
    st, n, dev = _stacks(stacks, bits)
    sums = pair_sad(st, bits)
    count = sum(s[0].numel() for s in st) if n else 0
    scores = torch.empty(max(n - 1, 0), dtype=torch.float64, device=dev)
    flags = torch.zeros(max(n - 1, 0), dtype=torch.uint8, device=dev)
    if n >= 2 and count:
        with torch.cuda.device(dev):
            _native.scene_cuts(sums, n, count, bits, thr, scores, flags)
    else:
        scores.zero_()
    return scores, flags


@torch.no_grad()
def score_window(sums: torch.Tensor, count: int, bits: int, threshold: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (scores float64 [K], flags uint8 [K]) on the device for a window of K consecutive interval sums (int64, as
    `pair_sad` returns them) of frames of `count` samples: `fiunet_scene_cuts` on the window alone, so the first and
    last interval of the window are scored without their outer neighbour.  The streaming loop (stream.py) passes the
    carried interval, a chunk's intervals and the lookahead interval, and keeps the chunk's own: each of those has both
    neighbours in the window (or sits at the clip's edge), so its score equals `detect_cuts` on the whole clip."""
    thr = check_threshold(threshold)
    if thr is None:
        raise ValueError("score_window needs a threshold in (0, 100]")
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    if sums.dtype != torch.int64 or sums.dim() != 1 or not sums.is_cuda:
        raise ValueError("sums must be an int64 [K] device tensor")
    k = sums.shape[0]
    sums = sums.contiguous()
    scores = torch.zeros(k, dtype=torch.float64, device=sums.device)
    flags = torch.zeros(k, dtype=torch.uint8, device=sums.device)
    if k and count:
        with torch.cuda.device(sums.device):
            _native.scene_cuts(sums, k + 1, int(count), bits, thr, scores, flags)
    return scores, flags


@torch.no_grad()
def hold_cut_frames(video: torch.Tensor, flags: torch.Tensor, factor: int) -> torch.Tensor:
    """In place on the contiguous interleaved result [(N-1)*factor + 1, ...] of a factor-`factor` loop (any dtype): for
    every flagged interval i, frames i*factor + 1 .. i*factor + factor - 1 become byte copies of frame i*factor.
    Returns `video`."""
    if factor < 2 or factor & (factor - 1):
        raise ValueError(f"factor must be a power of two >= 2, got {factor!r}")
    n_out = video.shape[0]
    if n_out < 1 or (n_out - 1) % factor:
        raise ValueError(f"video of {n_out} frames is not the result of a factor-{factor} loop")
    n = (n_out - 1) // factor + 1
    if flags.dtype != torch.uint8 or flags.numel() != n - 1 or flags.device != video.device:
        raise ValueError(f"flags must be uint8 [{n - 1}] on {video.device}")
    if not video.is_cuda:
        raise RuntimeError("video must be on the GPU: there is no CPU path in this package")
    if not video.is_contiguous():
        raise ValueError("video must be contiguous")
    if n >= 2:
        with torch.cuda.device(video.device):
            _native.hold_cut_frames(video, n, factor, flags.contiguous())
    return video


__all__ = ["check_threshold", "pair_sad", "pair_peak", "PEAK_SEGMENT", "detect_cuts", "score_window", "hold_cut_frames"]
