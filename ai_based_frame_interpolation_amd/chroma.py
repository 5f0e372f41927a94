"""Motion-guided chroma for the grayscale video route.

On that route the luma of an inserted frame comes from the network and its chroma has always been the rounded average
of its neighbours' (`inference._interleave_average_*`): whatever is coloured and moves gets a sharp luma and a
double-exposed chroma.  With `chroma="motion"` the chroma is carried along the motion instead, where the network's own
luma says the motion is known.

The definition is `guided_torch`, plain torch on any device, for ONE inserted frame M between the stored frames A and B
at one bisection level.  Inputs: the luma planes YA, YB [h, w], the network's luma YM for the inserted frame, the chroma
planes CA, CB [hc, wc] sub-sampled by (sy, sx), each 1 or 2, and the flow A -> B on the luma [h, w, 2]
(`optical_flow.farneback_flow`).  At 10 bits every word is read as min(word, 1023).

  1. Ym = `optical_flow._warp_time_torch(YA, YB, flow, 1, 2, bits)`, Ya = (YA + YB + 1) >> 1.
  2. For every 8x8 luma block (by, bx) of the ceil(h / 8) x ceil(w / 8) blocks: cost_m = sum |Ym - YM| over rows
     8 by - 4 .. 8 by + 11 and columns 8 bx - 4 .. 8 bx + 11, every index clamped to the plane (a clamped index counts
     again: 256 terms, which fit int32 at 10 bits); cost_a the same with Ya.  pick[by, bx] = 1 iff cost_m < cost_a: the
     comparison is strict, a tie takes the average.
  3. Chroma sample (cy, cx) of the inserted frame is, where pick[(cy * sy) >> 3, (cx * sx) >> 3] is 1,
     `_warp_time_torch(CA, CB, flow, 1, 2, bits)` there (the flow resampled to the chroma plane by that function's own
     rule: bit for bit what `fiunet_warp_table_*` writes for wn = 1, den = 2), else (CA + CB + 1) >> 1, the bytes of
     `chroma="average"`.

There are no thresholds and no tuning constants: the rule compares two candidates against the same evidence.

`pick` and `fill` run steps 1-2 and step 3 in HIP (csrc/chroma.hip.h: fiunet_chroma_pick_*, fiunet_chroma_fill_*), for
n frames a call, on planes where they lie; they are held to the definition bit for bit (tests/test_gpu_chroma.py).
There is no CPU fallback for them.
"""
from __future__ import annotations

import torch

from . import optical_flow as _of

MODES = ("average", "motion")
BLOCK = 8   # luma samples per block side


def check_mode(chroma) -> str:
    if chroma not in MODES:
        raise ValueError(f"chroma must be one of {list(MODES)}, got {chroma!r}")
    return chroma


def refuse_motion(chroma, what: str) -> str:
    """`check_mode`, then ValueError for "motion" on a route that has no separate chroma planes (`what` names it)."""
    if check_mode(chroma) == "motion":
        raise ValueError(f'chroma="motion" is not available for {what}: it carries the separate chroma planes of Y4M '
                         "video through the grayscale network along the motion, and there are none here")
    return chroma


def subsampling(luma_shape, chroma_shape):
    """(sy, sx) of an [hc, wc] chroma plane under an [h, w] luma plane: 1 where the sizes are equal, 2 where the chroma
    size is ceil(luma / 2); ValueError for anything else."""
    out = []
    for n, c in zip(luma_shape, chroma_shape):
        if c == n:
            out.append(1)
        elif c == (n + 1) // 2:
            out.append(2)
        else:
            raise ValueError(f"a chroma plane of {tuple(chroma_shape)} under a luma plane of {tuple(luma_shape)} is "
                             "sub-sampled by neither 1 nor 2")
    return tuple(out)


def pick_shape(h: int, w: int):
    return -(-h // BLOCK), -(-w // BLOCK)


def _average(a, b, bits):
    return (_of._codes(a, bits) + _of._codes(b, bits) + 1) >> 1


def _window_sums(d: torch.Tensor) -> torch.Tensor:
    """int64 [h, w] -> [ceil(h / 8), ceil(w / 8)]: the sum over each block's 16x16 window, indices clamped."""
    h, w = d.shape
    ph, pw = pick_shape(h, w)
    off = torch.arange(-4, 12, device=d.device)
    ry = (torch.arange(ph, device=d.device)[:, None] * BLOCK + off).clamp(0, h - 1)   # [ph, 16]
    rx = (torch.arange(pw, device=d.device)[:, None] * BLOCK + off).clamp(0, w - 1)   # [pw, 16]
    return d[ry.reshape(-1)][:, rx.reshape(-1)].reshape(ph, 16, pw, 16).sum(dim=(1, 3))


@torch.no_grad()
def pick_torch(ya, yb, ym, flow, bits: int = 8) -> torch.Tensor:
    """Steps 1-2 of the definition -> uint8 [ceil(h / 8), ceil(w / 8)]."""
    if not (ya.shape == yb.shape == ym.shape and ya.dim() == 2) or tuple(flow.shape) != tuple(ya.shape) + (2,):
        raise ValueError(f"expected three [h, w] luma planes and an [h, w, 2] flow, got {tuple(ya.shape)}, "
                         f"{tuple(yb.shape)}, {tuple(ym.shape)} and {tuple(flow.shape)}")
    warped = _of._warp_time_torch(ya, yb, flow, 1, 2, bits)
    m = _of._codes(ym, bits)
    cost_m = _window_sums((warped - m).abs())
    cost_a = _window_sums((_average(ya, yb, bits) - m).abs())
    return (cost_m < cost_a).to(torch.uint8)


@torch.no_grad()
def fill_torch(ca, cb, flow, pick, bits: int = 8, sub=None) -> torch.Tensor:
    """Step 3 of the definition for one chroma plane -> int64 [hc, wc].  sub: (sy, sx), or None: from the shapes."""
    h, w = flow.shape[:2]
    sy, sx = subsampling((h, w), ca.shape) if sub is None else sub
    if tuple(pick.shape) != pick_shape(h, w):
        raise ValueError(f"pick: expected {pick_shape(h, w)}, got {tuple(pick.shape)}")
    hc, wc = ca.shape
    by = (torch.arange(hc, device=pick.device) * sy) >> 3
    bx = (torch.arange(wc, device=pick.device) * sx) >> 3
    sel = pick[by][:, bx].bool()
    return torch.where(sel, _of._warp_time_torch(ca, cb, flow, 1, 2, bits), _average(ca, cb, bits))


@torch.no_grad()
def guided_torch(ya, yb, ym, ca, cb, flow, bits: int = 8, *, sub=None, pick=None):
    """THE DEFINITION (module docstring) -> (int64 [hc, wc] chroma of the inserted frame, uint8 pick map).  pick: a map
    to use instead of the computed one (all ones: the warp everywhere)."""
    if pick is None:
        pick = pick_torch(ya, yb, ym, flow, bits)
    return fill_torch(ca, cb, flow, pick, bits, sub), pick


# ---- the HIP entry points ---------------------------------------------------------------------------------------------
def _luma_plane(t: torch.Tensor, name: str):
    """[n, h, w] tensor or view -> its (offset, h, w, pitch, step, frame_stride), in samples from its first element."""
    if t.dim() != 3:
        raise ValueError(f"{name}: expected [n, h, w], got {tuple(t.shape)}")
    n, h, w = t.shape
    fs, pitch, step = t.stride()
    body = (h - 1) * pitch + (w - 1) * step + 1
    return (0, h, w, pitch, step, max(fs, body) if n > 1 else body)


def _chroma_planes(t: torch.Tensor, name: str):
    """[n, 2, hc, wc] tensor or view (U and V of n frames) -> its two planes."""
    if t.dim() != 4 or t.shape[1] != 2:
        raise ValueError(f"{name}: expected [n, 2, hc, wc] (U and V), got {tuple(t.shape)}")
    n, _, h, w = t.shape
    fs, ps, pitch, step = t.stride()
    body = (h - 1) * pitch + (w - 1) * step + 1
    fs = max(fs, ps + body) if n > 1 else ps + body
    return [(0, h, w, pitch, step, fs), (ps, h, w, pitch, step, fs)]


def _check_dtype(bits, *ts):
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    ok = (torch.uint8,) if bits == 8 else (torch.uint16, torch.int16)
    if any(t.dtype not in ok for t in ts):
        raise ValueError(f"{bits}-bit planes are {' or '.join(str(d) for d in ok)} tensors, got "
                         f"{[str(t.dtype) for t in ts]}")


@torch.no_grad()
def pick(ya: torch.Tensor, yb: torch.Tensor, ym: torch.Tensor, flow: torch.Tensor, bits: int = 8, *,
         out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
    """Steps 1-2 for n frames on the device (fiunet_chroma_pick_*): ya, yb, ym [n, h, w] tensors or views (three views of
    one buffer, as the route holds them, are read where they lie), flow float32 [n, h, w, 2] -> uint8 [n, ceil(h / 8),
    ceil(w / 8)] (`out`, or a new tensor)."""
    from . import _native
    _check_dtype(bits, ya, yb, ym)
    _of._need_gpu(ya, yb, ym, flow)
    if not ya.shape == yb.shape == ym.shape:
        raise ValueError(f"the luma planes differ in shape: {tuple(ya.shape)}, {tuple(yb.shape)}, {tuple(ym.shape)}")
    n, h, w = ya.shape
    if out is None:
        out = torch.empty((n,) + pick_shape(h, w), dtype=torch.uint8, device=ya.device)
    if n:
        with torch.cuda.device(ya.device):
            _native.chroma_pick(ya, _luma_plane(ya, "ya"), yb, _luma_plane(yb, "yb"), ym, _luma_plane(ym, "ym"),
                                flow.contiguous(), out, bits, stream)
    return out


@torch.no_grad()
def fill(ca: torch.Tensor, cb: torch.Tensor, flow: torch.Tensor, pick: torch.Tensor, out: torch.Tensor, bits: int = 8, *,
         sub=None, stream=None) -> torch.Tensor:
    """Step 3 for both chroma planes of n frames on the device (fiunet_chroma_fill_*): ca, cb, out [n, 2, hc, wc] tensors
    or views (U and V), flow float32 [n, h, w, 2] and pick uint8 [n, ceil(h / 8), ceil(w / 8)] of the luma.  sub: (sy,
    sx), or None: from the shapes.  Writes and returns `out`, which must not overlap ca or cb."""
    from . import _native
    _check_dtype(bits, ca, cb, out)
    _of._need_gpu(ca, cb, flow, pick, out)
    if not ca.shape == cb.shape == out.shape:
        raise ValueError(f"the chroma planes differ in shape: {tuple(ca.shape)}, {tuple(cb.shape)}, {tuple(out.shape)}")
    if sub is None:
        sub = subsampling(flow.shape[1:3], ca.shape[2:])
    if ca.shape[0]:
        with torch.cuda.device(ca.device):
            _native.chroma_fill(ca, _chroma_planes(ca, "ca"), cb, _chroma_planes(cb, "cb"), flow.contiguous(), pick, sub,
                                out, _chroma_planes(out, "out"), bits, stream)
    return out


__all__ = ["MODES", "check_mode", "pick", "fill", "guided_torch", "pick_torch", "fill_torch", "subsampling"]
