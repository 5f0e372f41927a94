"""Frame-rate conversion: any higher frame rate (24 -> 60, 23.976 -> 59.94, 25 -> 60 ...) from the frames of bisection.

The network gives the middle of a pair only, so the video loops reach the times i + m / G of a clip (G = 2**D, D levels
of bisection: the "grid", row i * G + m).  With `fps=` the video paths (`FrameInterpolator.interpolate_video`,
stream.py, the command line) build that grid as the `factor = G` run does and resample it on the device, in the wire
format, before the copy back to the host.  The definition is our own (the reference has no video loop).
Source rate Fi, target rate Fo > Fi, both exact rationals; Fi / Fo reduced is p / q (0 < p < q <= 2**20).  A clip of N
frames gives J = (N - 1) * q // p + 1 frames; output frame j sits at input time j * p / q:

  i  = (j * p) // q,  r = (j * p) % q          the input interval of frame j and its phase r / q
  lo = (r * G) // q,  wn = (r * G) % q         the grid row below the frame and the weight of the row above, wn / q
  blend    (A * (q - wn) + B * wn + q // 2) // q per sample in integers, A = grid[i * G + lo], B the row after it;
           10-bit words above 1023 read as 1023; wn == 0: a byte copy of A
  nearest  a byte copy of B if 2 * wn > q, else of A
  cut      interval i flagged (scene_cut) and r != 0: a byte copy of input frame i, so that no frame blends across a cut

Every plane of a frame as stored is resampled by the same rule.  One HIP kernel (csrc/retime.hip.h): `fiunet_retime_u8`
/ `fiunet_retime_p10`; the flags are read on the device.
"""
from __future__ import annotations

import numbers
from fractions import Fraction
from typing import Tuple

import torch

from . import _native

MAX_Q = 1 << 20
MODES = ("blend", "nearest")


def parse_fps(x) -> Fraction:
    """A frame rate as an exact rational: an int, a `Fraction`, an `(n, d)` pair of ints or an "n/d" / "n" string.
    Floats are refused: 59.94 is not 60000/1001."""
    if isinstance(x, float):
        raise ValueError(f"a frame rate must be exact, got the float {x!r}: pass a fraction as a string or a pair, "
                         'such as "60000/1001" for 59.94 or "24000/1001" for 23.976')
    try:
        if isinstance(x, bool):
            raise TypeError
        if isinstance(x, (numbers.Integral, Fraction)):
            f = Fraction(x)
        elif isinstance(x, (tuple, list)):
            n, d = x
            if any(isinstance(v, bool) or not isinstance(v, numbers.Integral) for v in (n, d)):
                raise TypeError
            f = Fraction(int(n), int(d))
        elif isinstance(x, str):
            parts = x.strip().split("/")
            if not 1 <= len(parts) <= 2 or not all(s.strip().isdigit() for s in parts):
                raise TypeError
            f = Fraction(int(parts[0]), int(parts[1]) if len(parts) == 2 else 1)
        else:
            raise TypeError
    except (TypeError, ValueError, ZeroDivisionError):
        raise ValueError(f'a frame rate is an int, a Fraction, an (n, d) pair or an "n/d" string, got {x!r}') from None
    if f <= 0:
        raise ValueError(f"a frame rate must be positive, got {x!r}")
    return f


def check_time_depth(time_depth) -> int:
    if isinstance(time_depth, bool) or not isinstance(time_depth, numbers.Integral) or not 1 <= time_depth <= 4:
        raise ValueError(f"time_depth must be an int in 1..4, got {time_depth!r}")
    return int(time_depth)


def check_mode(retime) -> str:
    if retime not in MODES:
        raise ValueError(f"retime must be one of {MODES}, got {retime!r}")
    return retime


class Plan:
    """Where the output frames of one (source rate, target rate, time_depth) sit.  p, q: source / target rate reduced;
    depth, G = 2**depth: the bisection the grid needs; fps: the target rate."""

    def __init__(self, src_fps: Fraction, fps: Fraction, time_depth: int):
        self.src_fps, self.fps, self.depth = src_fps, fps, time_depth
        ratio = src_fps / fps
        self.p, self.q, self.G = ratio.numerator, ratio.denominator, 1 << time_depth

    def __iter__(self):   # p, q, G = plan
        return iter((self.p, self.q, self.G))

    def n_out(self, n_frames: int) -> int:
        """J: output frames of a clip of `n_frames` (>= 1) frames."""
        return (n_frames - 1) * self.q // self.p + 1

    def frame(self, j: int) -> Tuple[int, int, int, int]:
        """(i, r, lo, wn) of output frame j."""
        i, r = divmod(j * self.p, self.q)
        lo, wn = divmod(r * self.G, self.q)
        return i, r, lo, wn

    def span(self, first_interval: int, n_intervals: int, last: bool = False) -> Tuple[int, int]:
        """(j0, n_out) of the chunk that holds intervals first_interval .. first_interval + n_intervals: the frames j
        with first_interval <= j * p / q < first_interval + n_intervals, and the frame at the chunk's end too when
        `last` (the clip's last frame).  A time belongs to exactly one chunk."""
        p, q = self.p, self.q
        j0 = -(-first_interval * q // p)
        end = (first_interval + n_intervals) * q
        j1 = -(-end // p)
        if last and end % p == 0:
            j1 += 1
        return j0, j1 - j0


def plan(src_fps, fps, time_depth: int = 2) -> Plan:
    """The plan of a conversion from `src_fps` to `fps` (anything `parse_fps` takes).  ValueError unless fps > src_fps
    and the reduced q fits 2**20."""
    depth = check_time_depth(time_depth)
    fi, fo = parse_fps(src_fps), parse_fps(fps)
    if fo <= fi:
        raise ValueError(f"fps must be above the source rate: fps {fo} <= source {fi} (lowering the frame rate, or "
                         "keeping it, is not interpolation)")
    pl = Plan(fi, fo, depth)
    if pl.q > MAX_Q:
        raise ValueError(f"source rate {fi} / fps {fo} reduces to {pl.p}/{pl.q}: the denominator must not exceed "
                         f"2**20 = {MAX_Q}")
    return pl


@torch.no_grad()
def resample(grid: torch.Tensor, plan: Plan, first_interval: int, j0: int, n_out: int, *, bits: int, flags=None,
             mode: str = "blend", out: torch.Tensor | None = None) -> torch.Tensor:
    """Output frames j0 .. j0 + n_out - 1 of the clip from `grid`: a contiguous device stack [n_intervals * G + 1, ...]
    (uint8 at 8 bits; 16-bit words, int16 or uint16, at 10) that covers clip intervals first_interval ..
    first_interval + n_intervals.  flags: uint8 [n_intervals] on the same device (the chunk's cut flags) or None.
    Returns `out` ([n_out, ...] of the grid's dtype; allocated when None)."""
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    mode = check_mode(mode)
    want = (torch.uint8,) if bits == 8 else (torch.int16, torch.uint16)
    if grid.dtype not in want:
        raise ValueError(f"a {bits}-bit grid must be {' or '.join(str(d) for d in want)}, got {grid.dtype}")
    rows = grid.shape[0]
    if rows < 1 or (rows - 1) % plan.G:
        raise ValueError(f"a grid of {rows} frames is not the result of a factor-{plan.G} loop")
    n_int = (rows - 1) // plan.G
    if not grid.is_cuda:
        raise RuntimeError("the grid must be on the GPU: there is no CPU path in this package")
    if not grid.is_contiguous():
        raise ValueError("the grid must be contiguous")
    if first_interval < 0 or j0 < 0 or n_out < 0:
        raise ValueError("first_interval, j0 and n_out must not be negative")
    if flags is not None:
        if flags.dtype != torch.uint8 or flags.numel() != n_int or flags.device != grid.device:
            raise ValueError(f"flags must be uint8 [{n_int}] on {grid.device}")
        flags = flags.contiguous()
    shape = (n_out,) + tuple(grid.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=grid.dtype, device=grid.device)
    elif tuple(out.shape) != shape or out.dtype != grid.dtype or out.device != grid.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {grid.dtype} {shape} tensor on {grid.device}")
    if n_out:
        with torch.cuda.device(grid.device):
            _native.retime(grid, n_int, plan.depth, first_interval, j0, n_out, plan.p, plan.q, MODES.index(mode),
                           flags if n_int else None, out, bits)
    return out


__all__ = ["MAX_Q", "MODES", "Plan", "parse_fps", "check_time_depth", "check_mode", "plan", "resample"]
