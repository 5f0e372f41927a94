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
  motion   (the video routes only, VIDEO_MODES; the last section of this file) blend's frames, but where
           wn != 0 A and B are first warped along the optical flow between them to the frame's time wn / q
  cut      interval i flagged (scene_cut) and r != 0: a byte copy of input frame i, so that no frame blends across a cut

Every plane of a frame as stored is resampled by the same rule.  One HIP kernel (csrc/retime.hip.h): `fiunet_retime_u8`
/ `fiunet_retime_p10`; the flags are read on the device.

Repeated frames (`dedup=`; the second half of this file): the spans of repeats are found on the host and
every output frame becomes one (row, wn, den) entry of a table that a second kernel, `fiunet_retime_table_u8` / `_p10`,
takes in its arguments.

Lower rates and a synthesized shutter (`shutter=`; the section after the repeated frames).  With
`plan(any_rate=True)` Fo is any positive rate, 1 <= p, q <= 2**20, and J and the frame times stay as above.  Dropping
to a lower rate by point sampling strobes: each frame keeps the source's short exposure.  So the exposure of the slower
camera is synthesized, by averaging the clip over a shutter window.  Exact rationals and Python integers only:

  time     grid time is u = t * G; grid row k sits at u = k.  Between rows the clip c(u) is the straight line between
           row floor(u) and the next row (blend before rounding); in an interval i flagged by scene_cut c(u) is row
           i * G throughout (the hold rule)
  shutter  s, an exact rational in [0, 1]: the fraction of the OUTPUT frame period the shutter is open (180 degrees =
           1/2); parsed like a frame rate (`check_shutter`), floats refused
  window   frame j opens at u0 = j p G / q and closes at u1 = u0 + s p G / q, cut short at the clip's last frame
           (u1 <= (N - 1) G) and at the end of the first flagged interval it touches (u1 <= (i + 1) G: no exposure
           crosses a cut).  Interval floor(u0 / G) is touched; a later interval i is where i G < u1
  weights  the frame is the mean of c(u) over [u0, u1]: W_k, the weight of row k, is the integral of its hat function
           over the window divided by u1 - u0 (a zero-width window: the two rows around u0 by its phase), the share
           inside a flagged interval i going to row i G.  Quantised to D = 2**20: w_k = floor(W_k D), and the
           D - sum w_k left-over units go one each to the rows with the largest fractional parts, ties to the lower
           row; sum w_k == D always; rows with w_k == 0 are dropped
  frame    out = (sum_k w_k x_k + D / 2) >> 20 per sample, 10-bit words above 1023 read as 1023 (the sum stays below
           2**30); a frame with a single tap is a byte copy of that row, as wn == 0 above
  limits   at most 48 rows from the first to the last tap of a frame (SHUTTER_MAX_TAPS); s p / q <= 8 source intervals

One HIP kernel (csrc/shutter.hip.h): `fiunet_shutter_u8` / `fiunet_shutter_p10`, the entries (first row, weights) in
its arguments.  shutter = 0 is point sampling and goes through `table_entries` / `resample_table`, whose rule holds for
p >= q as it stands.
"""
from __future__ import annotations

import math
import numbers
from fractions import Fraction
from typing import Tuple

import torch

from . import _native

MAX_Q = 1 << 20
MODES = ("blend", "nearest")
VIDEO_MODES = MODES + ("motion",)   # what the video routes take; MODES: what the retime kernels themselves know


def parse_fps(x) -> Fraction:
    """A frame rate as an exact rational: an int, a `Fraction`, an `(n, d)` pair of ints or an "n/d" / "n" string.
    Floats are refused: 59.94 is not 60000/1001."""
    f = _parse_rational(x, "a frame rate", 'such as "60000/1001" for 59.94 or "24000/1001" for 23.976')
    if f <= 0:
        raise ValueError(f"a frame rate must be positive, got {x!r}")
    return f


def _parse_rational(x, what: str, such_as: str) -> Fraction:
    """`x` as an exact rational >= 0 (what `parse_fps` and `check_shutter` share); `what` and `such_as` word the
    refusals."""
    if isinstance(x, float):
        raise ValueError(f"{what} must be exact, got the float {x!r}: pass a fraction as a string or a pair, {such_as}")
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
        raise ValueError(f'{what} is an int, a Fraction, an (n, d) pair or an "n/d" string, got {x!r}') from None
    return f


def check_time_depth(time_depth) -> int:
    if isinstance(time_depth, bool) or not isinstance(time_depth, numbers.Integral) or not 1 <= time_depth <= 4:
        raise ValueError(f"time_depth must be an int in 1..4, got {time_depth!r}")
    return int(time_depth)


def check_mode(retime) -> str:
    if retime not in VIDEO_MODES:
        raise ValueError(f"retime must be one of {VIDEO_MODES}, got {retime!r}")
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


def plan(src_fps, fps, time_depth: int = 2, any_rate: bool = False) -> Plan:
    """The plan of a conversion from `src_fps` to `fps` (anything `parse_fps` takes).  ValueError unless fps > src_fps
    and the reduced q fits 2**20.  any_rate (what `shutter=` asks for): any positive fps, a lower one and the source's
    own included; the reduced p must then fit 2**20 as q does."""
    depth = check_time_depth(time_depth)
    fi, fo = parse_fps(src_fps), parse_fps(fps)
    if fo <= fi and not any_rate:
        raise ValueError(f"fps must be above the source rate: fps {fo} <= source {fi} (lowering the frame rate, or "
                         "keeping it, is not interpolation)")
    pl = Plan(fi, fo, depth)
    if pl.q > MAX_Q:
        raise ValueError(f"source rate {fi} / fps {fo} reduces to {pl.p}/{pl.q}: the denominator must not exceed "
                         f"2**20 = {MAX_Q}")
    if pl.p > MAX_Q:
        raise ValueError(f"source rate {fi} / fps {fo} reduces to {pl.p}/{pl.q}: the numerator must not exceed "
                         f"2**20 = {MAX_Q}")
    return pl


@torch.no_grad()
def resample(grid: torch.Tensor, plan: Plan, first_interval: int, j0: int, n_out: int, *, bits: int, flags=None,
             mode: str = "blend", out: torch.Tensor | None = None, layout=None, batch: int = 8) -> torch.Tensor:
    """Output frames j0 .. j0 + n_out - 1 of the clip from `grid`: a contiguous device stack [n_intervals * G + 1, ...]
    (uint8 at 8 bits; 16-bit words, int16 or uint16, at 10) that covers clip intervals first_interval ..
    first_interval + n_intervals.  flags: uint8 [n_intervals] on the same device (the chunk's cut flags) or None.
    Returns `out` ([n_out, ...] of the grid's dtype; allocated when None).
    mode "motion" (the second half of this file's last section): the blend pass first, then every frame with wn != 0
    outside a flagged interval is warped to its time; layout: the `layout.Layout` of a frame (None: an [H, W] or
    [H, W, C] frame, from the grid's shape); batch: the pairs per flow call."""
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
            _native.retime(grid, n_int, plan.depth, first_interval, j0, n_out, plan.p, plan.q,
                           MODES.index("blend" if mode == "motion" else mode), flags if n_int else None, out, bits)
            if mode == "motion":
                entries = []
                for k in range(n_out):
                    i, _, lo, wn = plan.frame(j0 + k)
                    li = i - first_interval   # (wn != 0: the frame lies inside interval li, which the C call checked)
                    entries.append(((li << plan.depth) + lo, wn, plan.q, -1 if flags is None else li))
                _motion(grid, entries, bits, out, layout, flags, batch)
    return out


# ---- repeated frames -------------------------------------------------------------------------------
# Telecined film, animation on twos and threes, a stalled capture: A A A B.  The loops would ask the network for the
# middle of (A, A) twice and squeeze the motion from A to B into the last interval.  With `dedup=` the output times
# inside a run of repeats are mapped onto the grid of the one interval that carries the motion.  Integers and exact
# rationals only:
#
#   peak[i]  the largest sum of |F[i+1] - F[i]| over the aligned 64-sample segments of a frame as stored
#            (scene.pair_peak); interval i is DEAD iff peak[i] <= floor(dedup * 64), dedup a tolerance in code values
#   span     a maximal run of m >= 1 dead intervals a .. a+m-1 followed by a live interval i = a+m that is not a flagged
#            cut, with L = m + 1 <= max_gap: the intervals [a, i+1).  A longer hold, a run that reaches the clip's end,
#            a run before a cut and every interval outside a run form no span and behave as without dedup.
#   time     output frame j sits at t = j p / q; (a, i, L) the span that holds floor(t) (outside spans a = i = floor(t),
#            L = 1): num = j p - a q, den = q L, lo = num G // den, wn = num G % den; the frame is grid row (i, lo)
#            blended with the row after it by wn / den ("nearest": the closer of the two, a tie to the earlier one); an
#            interval floor(t) flagged as a cut, off a source frame, stays a copy of grid row (floor(t), 0).
#
# With L = 1 this is the rule at the top of this file bit for bit.  den <= 2**20 keeps the kernel's 32-bit arithmetic.
MAX_GAP_RANGE = (2, 8)
DEDUP_MAX_FACTOR = 16


def check_dedup(dedup, max_gap=4):
    """-> (dedup as a float or None, max_gap as an int).  dedup: None (off) or a finite real number >= 0 (not a bool);
    max_gap: an int in 2..8.  ValueError otherwise."""
    if isinstance(max_gap, bool) or not isinstance(max_gap, numbers.Integral) or \
            not MAX_GAP_RANGE[0] <= max_gap <= MAX_GAP_RANGE[1]:
        raise ValueError(f"max_gap must be an int in {MAX_GAP_RANGE[0]}..{MAX_GAP_RANGE[1]}, got {max_gap!r}")
    if dedup is None:
        return None, int(max_gap)
    if isinstance(dedup, bool) or not isinstance(dedup, numbers.Real):
        raise ValueError(f"dedup must be None or a number >= 0 (a tolerance in code values), got {dedup!r}")
    v = float(dedup)
    if not math.isfinite(v) or v < 0.0:
        raise ValueError(f"dedup must be None or a finite number >= 0 (a tolerance in code values), got {dedup!r}")
    return v, int(max_gap)


def dead_limit(dedup: float) -> int:
    """floor(dedup * 64): interval i is dead iff peak[i] <= this (a peak is below 2**16)."""
    return int(min(math.floor(dedup * 64), (1 << 31) - 1))


def dedup_plan(pl: "Plan | None", factor: int, max_gap: int) -> "Plan":
    """The plan a run with `dedup` goes through: `pl` (from fps), or p / q = 1 / factor, G = factor.  ValueError when
    factor > 16 (the grid's depth) or q * max_gap > 2**20 (the kernel's divisor)."""
    if pl is None:
        if factor > DEDUP_MAX_FACTOR:
            raise ValueError(f"dedup re-times on the grid of a factor run of at most {DEDUP_MAX_FACTOR}: got "
                             f"factor={factor!r}")
        pl = Plan(Fraction(1), Fraction(factor), factor.bit_length() - 1)
    if pl.q * max_gap > MAX_Q:
        raise ValueError(f"with dedup, q * max_gap must not exceed 2**20 = {MAX_Q}: the rates reduce to "
                         f"{pl.p}/{pl.q} and max_gap is {max_gap}")
    return pl


def dedup_spans(dead, cuts, max_gap: int):
    """The spans of a clip: `dead` (one truth value per interval), `cuts` (the same length, or None) -> a list of
    (a, L), first interval and length, in order."""
    n, spans, k = len(dead), [], 0
    while k < n:
        if not dead[k]:
            k += 1
            continue
        a = k
        while k < n and dead[k]:
            k += 1
        # k: the live interval after the run, or n when the run reaches the end
        if k < n and k - a + 1 <= max_gap and not (cuts is not None and cuts[k]):
            spans.append((a, k - a + 1))
            k += 1
    return spans


def classify_chunk(dead, cuts, carry: int, first_interval: int, c: int, max_gap: int):
    """The spans that touch a chunk's own intervals first_interval .. first_interval + c, from what the chunk sees:
    `dead` / `cuts` (or None) of the intervals from first_interval on (its own and the lookahead's: max_gap - 1 more, or
    as many as the clip has; with cuts one more still, whose own flag is not relied on), and `carry`, the number of
    dead intervals directly before first_interval, saturated at max_gap.  -> (spans as (a, L) with clip interval
    numbers, e: the intervals past the chunk's end that they need, the carry of the next chunk).  Equals `dedup_spans`
    on the whole clip (tests/test_dedup_host.py)."""
    s = first_interval
    local_dead = [True] * carry + [bool(v) for v in dead]
    local_cuts = None if cuts is None else [False] * carry + [bool(v) for v in cuts]
    spans = []
    for a, ln in dedup_spans(local_dead, local_cuts, max_gap):
        a += s - carry
        # a saturated carry stands for a run of max_gap or more: no span (L > max_gap), which dedup_spans has found
        if a + ln > s and a < s + c:
            spans.append((a, ln))
    e = max([a + ln - (s + c) for a, ln in spans] + [0])
    own = local_dead[:carry + c]
    trail = 0
    while trail < len(own) and own[len(own) - 1 - trail]:
        trail += 1
    return spans, e, min(trail, max_gap)


def table_entries(pl: Plan, spans, first_interval: int, j0: int, n_out: int, n_intervals: int, mode: str = "blend",
                  cuts=None):
    """(row, wn, den) of output frames j0 .. j0 + n_out - 1 on a grid of n_intervals * G + 1 rows that starts at clip
    interval first_interval: what `resample_table` takes.  spans: (a, L) with clip interval numbers; cuts: truth values
    of the grid's intervals (from first_interval), or None.  Python integers only; ValueError when a frame needs a row
    outside the grid."""
    mode = check_mode(mode)
    p, q, G = pl
    rows = n_intervals * G + 1
    where = {}
    for a, ln in spans:
        for f in range(a, a + ln):
            where[f] = (a, ln)
    out = []
    for j in range(j0, j0 + n_out):
        f, r = divmod(j * p, q)
        k = f - first_interval
        if r != 0 and cuts is not None and 0 <= k < len(cuts) and cuts[k]:
            row, wn, den = k * G, 0, 1
        else:
            a, ln = where.get(f, (f, 1))
            num, den = j * p - a * q, q * ln
            lo, wn = divmod(num * G, den)
            row = (a + ln - 1 - first_interval) * G + lo
            if mode == "nearest":
                row, wn = row + (1 if 2 * wn > den else 0), 0
            g = math.gcd(wn, den)
            wn, den = wn // g, den // g      # (wn == 0: den = 1)
        if k < 0 or row < 0 or row + (1 if wn else 0) >= rows:
            raise ValueError(f"output frame {j} needs grid row {row}{' and the next' if wn else ''}: the grid has "
                             f"{rows} rows from interval {first_interval}")
        out.append((row, wn, den))
    return out


@torch.no_grad()
def resample_table(grid: torch.Tensor, entries, bits: int, out: torch.Tensor | None = None, mode: str = "blend",
                   layout=None, batch: int = 8) -> torch.Tensor:
    """One output frame per entry (row, wn, den) from `grid`, a contiguous device stack [rows, ...] (uint8 at 8 bits;
    16-bit words at 10): a byte copy of grid[row] when wn == 0, else (A (den - wn) + B wn + den // 2) // den per sample
    with B = grid[row + 1].  The entries are read on the host during the call and go to the kernel in its arguments
    (`fiunet_retime_table_u8` / `_p10`).  Returns `out` ([len(entries), ...]; allocated when None).
    mode "motion": after that pass every entry with wn != 0 is warped to its time (layout, batch: as for `resample`);
    "blend" and "nearest" are resolved into the entries by `table_entries` and change nothing here."""
    mode = check_mode(mode)
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    want = (torch.uint8,) if bits == 8 else (torch.int16, torch.uint16)
    if grid.dtype not in want:
        raise ValueError(f"a {bits}-bit grid must be {' or '.join(str(d) for d in want)}, got {grid.dtype}")
    if not grid.is_cuda:
        raise RuntimeError("the grid must be on the GPU: there is no CPU path in this package")
    if not grid.is_contiguous():
        raise ValueError("the grid must be contiguous")
    entries = [tuple(int(v) for v in e) for e in entries]
    shape = (len(entries),) + tuple(grid.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=grid.dtype, device=grid.device)
    elif tuple(out.shape) != shape or out.dtype != grid.dtype or out.device != grid.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {grid.dtype} {shape} tensor on {grid.device}")
    if entries:
        with torch.cuda.device(grid.device):
            _native.retime_table(grid, entries, out, bits)
            if mode == "motion":
                _motion(grid, [e + (-1,) for e in entries], bits, out, layout, None, batch)
    return out


# ---- lower rates: a synthesized shutter ----------------------------------------------------------------
# The definition stands at the top of this file.  Everything here is Python integers and `Fraction`s; the device sees
# (first row, weights) entries whose weights sum to 2**20.
SHUTTER_ONE = 1 << 20            # D
SHUTTER_MAX_TAPS = 48            # csrc/shutter.hip.h: kShutterMaxTaps
SHUTTER_MAX_INTERVALS = 8        # s p / q: source intervals per window


def check_shutter(x):
    """-> None (no shutter asked for) or the shutter as an exact `Fraction` in [0, 1]: an int, a `Fraction`, an (n, d)
    pair or an "n/d" string, as a frame rate.  Floats are refused as `parse_fps` refuses them."""
    if x is None:
        return None
    s = _parse_rational(x, "a shutter", 'such as "1/2" for 180 degrees')
    if not 0 <= s <= 1:
        raise ValueError(f"a shutter is the fraction of the output frame period it is open, 0 to 1, got {x!r}")
    return s


def shutter_lookahead(pl: Plan, s: Fraction) -> int:
    """ceil(s p / q): the source frames behind a chunk's own that its frames' windows can reach."""
    return -((-s.numerator * pl.p) // (s.denominator * pl.q))


def check_shutter_plan(pl: Plan, s: Fraction) -> None:
    """The limits of a shutter `s` > 0 on plan `pl`, from the rates alone: ValueError when a window spans more than 8
    source intervals, or when a frame's taps can span more than 48 grid rows (the bound: a window of length
    L = s p G / q that opens at phase f of a grid cell covers the rows 0 .. ceil(f + L), and f takes every multiple of
    1 / q' below 1, q' the denominator of p G / q)."""
    p, q, G = pl
    if s * p > SHUTTER_MAX_INTERVALS * q:
        raise ValueError(f"a shutter of {s} at source / fps = {p}/{q} keeps the window open over {s * p / q} source "
                         f"intervals; at most {SHUTTER_MAX_INTERVALS} are supported: lower `shutter`, or convert in "
                         "two steps")
    length, unit = s * Fraction(p * G, q), Fraction(p * G, q).denominator
    top = Fraction(unit - 1, unit) + length
    taps = -((-top.numerator) // top.denominator) + 1
    if taps > SHUTTER_MAX_TAPS:
        raise ValueError(f"a shutter of {s} at source / fps = {p}/{q} and time_depth {pl.depth} averages up to {taps} "
                         f"grid rows per frame; at most {SHUTTER_MAX_TAPS} are supported: lower `time_depth` or "
                         "`shutter`")


def _flagged(cuts, k: int) -> bool:
    return cuts is not None and 0 <= k < len(cuts) and bool(cuts[k])


def shutter_window(pl: Plan, s: Fraction, j: int, first_interval: int = 0, cuts=None, clip_last=None):
    """(u0, u1) of output frame j in grid time, as `Fraction`s.  cuts: truth values of the intervals from
    first_interval on, or None; clip_last: the number of the clip's last frame, N - 1, or None where the clip is
    known to go on past every window."""
    p, q, G = pl
    u0 = Fraction(j * p * G, q)
    u1 = u0 + s * Fraction(p * G, q)
    if clip_last is not None:
        u1 = max(u0, min(u1, Fraction(clip_last * G)))
    if cuts is not None:
        i = u0.numerator // (u0.denominator * G)
        while True:
            if _flagged(cuts, i - first_interval):
                u1 = min(u1, Fraction((i + 1) * G))
                break
            i += 1
            if i * G >= u1:
                break
    return u0, u1


def shutter_weights(u0: Fraction, u1: Fraction, G: int, first_interval: int = 0, cuts=None):
    """{grid row of the clip: weight} of the window [u0, u1], quantised to 2**20 (the weights sum to SHUTTER_ONE; rows
    of weight 0 are left out)."""
    W = {}

    def add(k, v):
        if v:
            W[k] = W.get(k, 0) + v
    m = u0.numerator // u0.denominator
    if u0 == u1:
        if _flagged(cuts, m // G - first_interval):
            add(m // G * G, Fraction(1))
        else:
            add(m, 1 - (u0 - m))
            add(m + 1, u0 - m)
    else:
        while m < u1:
            x0, x1 = max(u0, Fraction(m)), min(u1, Fraction(m + 1))
            if _flagged(cuts, m // G - first_interval):
                add(m // G * G, x1 - x0)
            else:
                mid = (x0 + x1) / 2
                add(m, (x1 - x0) * (m + 1 - mid))
                add(m + 1, (x1 - x0) * (mid - m))
            m += 1
        W = {k: v / (u1 - u0) for k, v in W.items()}
    rows = sorted(W)
    w = {k: (W[k] * SHUTTER_ONE).numerator // (W[k] * SHUTTER_ONE).denominator for k in rows}
    left = SHUTTER_ONE - sum(w.values())
    # the left-over units: the largest fractional parts first, ties to the lower row
    for k in sorted(rows, key=lambda k: (-(W[k] * SHUTTER_ONE - w[k]), k))[:left]:
        w[k] += 1
    return {k: v for k, v in w.items() if v}


def shutter_reach(pl: Plan, s: Fraction, first_interval: int, n_own: int, j0: int, n_out: int, cuts=None,
                  clip_last=None) -> int:
    """How many intervals past first_interval + n_own the windows of frames j0 .. j0 + n_out - 1 reach: what a chunk's
    grid is extended by."""
    end = 0
    for j in range(j0, j0 + n_out):
        u1 = shutter_window(pl, s, j, first_interval, cuts, clip_last)[1] / pl.G
        end = max(end, -((-u1.numerator) // u1.denominator))
    return max(0, end - (first_interval + n_own))


def shutter_entries(pl: Plan, s: Fraction, first_interval: int, j0: int, n_out: int, n_intervals: int, cuts=None,
                    clip_last=None):
    """(first_row, [w ...]) of output frames j0 .. j0 + n_out - 1 on a grid of n_intervals * G + 1 rows that starts at
    clip interval first_interval: what `resample_shutter` takes.  The taps are consecutive grid rows from first_row, a
    row the definition dropped carrying weight 0.  cuts, clip_last: as for `shutter_window`.  Python integers only;
    ValueError when a frame needs a row outside the grid, or more than 48 rows."""
    G = pl.G
    rows = n_intervals * G + 1
    out = []
    for j in range(j0, j0 + n_out):
        u0, u1 = shutter_window(pl, s, j, first_interval, cuts, clip_last)
        w = shutter_weights(u0, u1, G, first_interval, cuts)
        lo, hi = min(w) - first_interval * G, max(w) - first_interval * G
        if lo < 0 or hi >= rows:
            raise ValueError(f"output frame {j} needs grid rows {lo} .. {hi}: the grid has {rows} rows from interval "
                             f"{first_interval}")
        if hi - lo + 1 > SHUTTER_MAX_TAPS:
            raise ValueError(f"output frame {j} averages {hi - lo + 1} grid rows; at most {SHUTTER_MAX_TAPS} are "
                             "supported: lower `time_depth` or `shutter`")
        out.append((lo, [w.get(k + first_interval * G, 0) for k in range(lo, hi + 1)]))
    return out


@torch.no_grad()
def resample_shutter(grid: torch.Tensor, entries, bits: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """One output frame per entry (first_row, weights) from `grid`, a contiguous device stack [rows, ...] (uint8 at 8
    bits; 16-bit words at 10): (sum_t w[t] grid[first_row + t] + 2**19) >> 20 per sample, a byte copy of the row where
    one weight is 2**20.  The entries are read on the host during the call and go to the kernel in its arguments
    (`fiunet_shutter_u8` / `_p10`).  Returns `out` ([len(entries), ...]; allocated when None)."""
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    want = (torch.uint8,) if bits == 8 else (torch.int16, torch.uint16)
    if grid.dtype not in want:
        raise ValueError(f"a {bits}-bit grid must be {' or '.join(str(d) for d in want)}, got {grid.dtype}")
    if not grid.is_cuda:
        raise RuntimeError("the grid must be on the GPU: there is no CPU path in this package")
    if not grid.is_contiguous():
        raise ValueError("the grid must be contiguous")
    entries = [(int(r), [int(v) for v in w]) for r, w in entries]
    shape = (len(entries),) + tuple(grid.shape[1:])
    if out is None:
        out = torch.empty(shape, dtype=grid.dtype, device=grid.device)
    elif tuple(out.shape) != shape or out.dtype != grid.dtype or out.device != grid.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous {grid.dtype} {shape} tensor on {grid.device}")
    if entries:
        with torch.cuda.device(grid.device):
            _native.shutter(grid, entries, out, bits)
    return out


# ---- motion-compensated resampling -----------------------------------------------------------------
# retime "motion": an output frame between two grid rows A and B (wn != 0) is not their cross-fade but both of them
# warped along the dense flow A -> B to the frame's own time wn / den (optical_flow._warp_time_torch is the definition,
# `fiunet_warp_table_u8` / `_p10` the kernel).  The blend pass runs first over the same output rows: it gives the
# wn == 0 copies and the held frames of flagged intervals, whose flags the warp reads on the device and leaves alone.
# The flow is Farneback's on the LEAD plane of the pair: the first plane of the layout, or the rounded mean of r, g and
# b (packed RGB) / of the channels of an [H, W, C] frame, hold-out scoring's rule.  Every plane of the layout is then
# warped where it lies, one call per plane.  A pair's flow does not depend on the pairs beside it (the C ABI says so),
# so neither does an output frame: a streamed run equals a resident one byte for byte.  At most `batch` flow fields
# (8 bytes a lead sample) and one flow workspace are alive at a time.
def _motion_layout(grid: torch.Tensor, layout, bits: int):
    from . import layout as _layout
    if layout is None:
        if grid.dim() == 3:
            layout = _layout.frame_layout("npy", grid.shape[1], grid.shape[2])
        elif grid.dim() == 4:
            layout = _layout.frame_layout(("npy", grid.shape[3]), grid.shape[1], grid.shape[2])
        else:
            raise ValueError(f'retime "motion" needs the layout of a frame: a grid {tuple(grid.shape)} does not say '
                             "where its planes lie (pass layout=layout.frame_layout(...))")
    planes = [tuple(p) for p in layout.planes]
    row = grid[0].numel()
    if _layout.frame_samples(planes) > row:
        raise ValueError(f"the layout's planes reach sample {_layout.frame_samples(planes)} of a frame of {row}")
    if bits == 10 and len(lead_planes(planes)) > 1:
        raise ValueError('retime "motion": the mean of several lead planes is defined for 8-bit frames only')
    return planes


def lead_planes(planes):
    """The names of the planes the flow is estimated on: r, g and b of packed RGB, every channel of an [H, W, C]
    frame (their rounded mean), else the first plane."""
    names = [p[0] for p in planes]
    if {"r", "g", "b"} <= set(names):
        return ["r", "g", "b"]
    if len(names) > 1 and all(n == f"c{i}" for i, n in enumerate(names)):
        return names
    return names[:1]


def _plane_rows(flat: torch.Tensor, plane, idx: torch.Tensor) -> torch.Tensor:
    """Plane `plane` of the rows `idx` of the [rows, row] buffer `flat` as a contiguous [len(idx), h, w] tensor."""
    _, off, h, w, pitch, step = plane
    view = flat.as_strided((flat.shape[0], h, w), (flat.stride(0), pitch, step), flat.storage_offset() + off)
    return view.index_select(0, idx)


def _motion(grid, entries, bits, out, layout, flags, batch):
    """Overwrite, in `out`, every plane of the frames whose entry (row, wn, den, flag) has wn != 0."""
    from . import optical_flow
    if isinstance(batch, bool) or not isinstance(batch, numbers.Integral) or batch < 1:
        raise ValueError(f"batch must be a positive int, got {batch!r}")
    planes = _motion_layout(grid, layout, bits)
    todo = [(k, e) for k, e in enumerate(entries) if e[1] != 0]
    if not todo:
        return
    rows, row = grid.shape[0], grid[0].numel()
    flat, oflat = grid.reshape(rows, row), out.reshape(out.shape[0], row)
    lead = [p for p in planes if p[0] in lead_planes(planes)]
    pairs = sorted({e[0] for _, e in todo})
    for s in range(0, len(pairs), batch):
        part = pairs[s:s + batch]
        idx = torch.tensor(part, dtype=torch.int64, device=grid.device)
        if len(lead) == 1:
            prev, nxt = _plane_rows(flat, lead[0], idx), _plane_rows(flat, lead[0], idx + 1)
        else:   # the rounded mean of the lead planes (8-bit formats only)
            c = len(lead)
            prev, nxt = (((sum(_plane_rows(flat, p, i).to(torch.int32) for p in lead) * 2 + c) // (2 * c)).to(torch.uint8)
                         for i in (idx, idx + 1))
        flow = optical_flow.farneback_flow(prev, nxt, "hip", bits=bits)
        where = {r: f for f, r in enumerate(part)}
        mine = [(k, e) for k, e in todo if e[0] in where]
        # runs of consecutive output frames: one call per run and plane (`out`'s plane starts at the run's first frame)
        runs, start = [], 0
        for n in range(1, len(mine) + 1):
            if n == len(mine) or mine[n][0] != mine[n - 1][0] + 1:
                runs.append(mine[start:n])
                start = n
        for run in runs:
            k0 = run[0][0]
            table = [(e[0], e[1], e[2], where[e[0]], e[3]) for _, e in run]
            for _, off, h, w, pitch, step in planes:
                _native.warp_table(flat, rows, (off, h, w, pitch, step, row), flow, flags, table, oflat[k0:k0 + len(run)],
                                   (off, h, w, pitch, step, row), bits)


__all__ = ["MAX_Q", "MODES", "VIDEO_MODES", "lead_planes", "Plan", "parse_fps", "check_time_depth", "check_mode", "plan", "resample",
           "check_dedup", "dead_limit", "dedup_plan", "dedup_spans", "classify_chunk", "table_entries",
           "resample_table", "SHUTTER_ONE", "SHUTTER_MAX_TAPS", "SHUTTER_MAX_INTERVALS", "check_shutter",
           "shutter_lookahead", "check_shutter_plan", "shutter_window", "shutter_weights", "shutter_reach",
           "shutter_entries", "resample_shutter"]
