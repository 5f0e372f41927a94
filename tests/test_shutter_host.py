"""CPU: conversion to any lower frame rate with a synthesized shutter (retime.py) where it needs no GPU -
the literal pins of the definition, the weights against the restatement of tests/shutter_ref.py, the chunk rule, every
refusal of the public call before any GPU work, the C ABI's host-side checks and the command line."""
import ctypes
import math
import os
import random
import re
import sys
from fractions import Fraction as F

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shutter_ref as SR  # noqa: E402
import shutter_stream_rows  # noqa: E402  (importing it adds the new entry points' rows to the stream contract's table)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli  # noqa: E402
from ai_based_frame_interpolation_amd import imageio_lite as IO  # noqa: E402
from ai_based_frame_interpolation_amd import retime as RT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 1 << 20
RATES = [(60, 24), (F(60000, 1001), 50), (120, 24), (60, 50), (24, 60)]


def _plan(src, dst, depth):
    return RT.plan(src, dst, depth, any_rate=True)


# ---- the literal pins ---------------------------------------------------------------------------------------------------
def test_literal_pins():
    half = F(1, 2)
    p24, p50 = _plan(60, 24, 2), _plan(60, 50, 2)
    assert tuple(p24) == (5, 2, 4) and tuple(p50) == (6, 5, 4)

    def frame(pl, j, cuts=None):
        u = RT.shutter_window(pl, half, j, 0, cuts)
        return u, RT.shutter_weights(*u, pl.G, 0, cuts)
    assert frame(p24, 1) == ((10, 15), {10: 104858, 11: 209715, 12: 209715, 13: 209715, 14: 209715, 15: 104858})
    # the tie rule: rows 5 and 7 have the same fractional part, the unit goes to the lower row
    assert frame(p50, 1) == ((F(24, 5), F(36, 5)), {4: 8738, 5: 297097, 6: 436907, 7: 297096, 8: 8738})
    assert frame(p24, 1, [0, 0, 0, 1, 0, 0]) == ((10, 15), {10: 104858, 11: 209715, 12: 734003})
    assert frame(p24, 1, [0, 0, 1, 0, 0, 0]) == ((10, 12), {8: 1048576})
    assert RT.shutter_weights(F(3), F(4), 4) == {3: 524288, 4: 524288}
    # ... which is, bit for bit, the (row, wn, den) = (3, 1, 2) of the table kernel: (A + B + 1) // 2
    a, b = np.arange(256)[:, None], np.arange(256)[None, :]
    assert np.array_equal((a * 524288 + b * 524288 + D // 2) >> 20, (a + b + 1) // 2)
    # the restatement agrees on all of them
    assert SR.weights(5, 2, 4, half, 1, 100) == frame(p24, 1)[1]
    assert SR.weights(6, 5, 4, half, 1, 100) == frame(p50, 1)[1]
    assert SR.weights(5, 2, 4, half, 1, 100, [0, 0, 0, 1, 0, 0]) == {10: 104858, 11: 209715, 12: 734003}
    assert SR.weights(5, 2, 4, half, 1, 100, [0, 0, 1, 0, 0, 0]) == {8: 1048576}


def test_the_window_ends_with_the_clip_and_a_last_frame_is_a_copy():
    pl = _plan(60, 24, 2)          # N = 6: J = 3, frame 2 opens at the last frame
    assert pl.n_out(6) == 3
    e = RT.shutter_entries(pl, F(1), 0, 0, 3, 5, None, 5)
    assert e[2] == (20, [D]) and [r for r, _ in e] == [0, 10, 20]
    assert e[0][1] == e[1][1] and len(e[0][1]) == 11
    # N = 5: frame 1 opens at u = 10 and is cut short at u = 16
    assert RT.shutter_window(pl, F(1), 1, 0, None, 4) == (10, 16)


# ---- the weights over a sweep -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 2, 4])
@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_weights_sum_to_one_and_taps_stay_within_48(rate, depth):
    pl = _plan(rate[0], rate[1], depth)
    p, q, G = pl
    n_frames = 40
    J = pl.n_out(n_frames)
    for k in range(1, 9):
        s = F(k, 8)
        try:
            RT.check_shutter_plan(pl, s)
        except ValueError as e:
            assert "time_depth" in str(e) and "shutter" in str(e)
            # the refusal is not idle: a window of that length, opened at the worst phase, spans more than 48 rows
            assert math.ceil(s * p * G / q) + 1 > 48 - 1
            continue
        entries = RT.shutter_entries(pl, s, 0, 0, J, n_frames - 1, None, n_frames - 1)
        assert len(entries) == J
        for j, (row, w) in enumerate(entries):
            assert sum(w) == D and 1 <= len(w) <= RT.SHUTTER_MAX_TAPS and w[0] and w[-1], (s, j)
            want = SR.weights(p, q, G, s, j, n_frames)
            assert {row + t: v for t, v in enumerate(w) if v} == want, (s, j)


def test_with_cuts_the_weights_are_the_restatements():
    rng = random.Random(5)
    for rate in RATES:
        for depth in (1, 2, 3):
            pl = _plan(rate[0], rate[1], depth)
            p, q, G = pl
            n_frames = 14
            cuts = [rng.random() < 0.3 for _ in range(n_frames - 1)]
            for s in (F(1, 8), F(1, 2), F(1)):
                J = pl.n_out(n_frames)
                entries = RT.shutter_entries(pl, s, 0, 0, J, n_frames - 1, cuts, n_frames - 1)
                for j, (row, w) in enumerate(entries):
                    assert sum(w) == D
                    assert {row + t: v for t, v in enumerate(w) if v} == SR.weights(p, q, G, s, j, n_frames, cuts)
                    u0, u1 = SR.window(p, q, G, s, j, n_frames, cuts)
                    first = math.floor(u0 / G)
                    # no exposure crosses a cut: past a flagged interval nothing is read
                    for i in range(first, n_frames - 1):
                        if cuts[i]:
                            assert row + len(w) - 1 <= i * G and u1 <= (i + 1) * G
                            break


def test_a_clip_linear_in_time_gives_the_value_at_the_windows_midpoint():
    """x(u) = u: the weighted mean of the rows' times against (u0 + u1) / 2.  The exact weights give the midpoint; a
    20-bit weight is off by less than 2**-20 and a row lies at most 47 rows from the first, so the mean is off by less
    than 48 * 47 / 2 * 2**-20 = 1.1e-3 < 2**-9 (6.5e-4 was the largest of 2000 random cases)."""
    rng = random.Random(11)
    worst = F(0)
    for _ in range(2000):
        q = rng.randint(1, 1200)
        p = rng.randint(max(1, q // 3), 6 * q)
        g = math.gcd(p, q)
        p, q, G = p // g, q // g, 1 << rng.randint(1, 4)
        s = F(rng.randint(1, 16), 16)
        if s * p > 8 * q or s * p * G / q > 45:
            continue
        j = rng.randint(0, 50)
        u0, u1 = SR.window(p, q, G, s, j, 10 ** 6)
        W = SR.exact_weights(u0, u1, G)
        assert sum(k * v for k, v in W.items()) == (u0 + u1) / 2
        w = RT.shutter_weights(u0, u1, G)
        assert w == SR.quantise(W)
        worst = max(worst, abs(F(sum(k * v for k, v in w.items()), D) - (u0 + u1) / 2))
    assert 0 < worst <= F(1, 512), float(worst)


# ---- chunks ---------------------------------------------------------------------------------------------------------------
def _chunks(n_frames, C, look):
    """(first interval, own intervals, frames read, last) of the chunks stream._run makes of a clip."""
    s, out = 0, []
    while n_frames - s >= C + 1 + look:
        out.append((s, C, C + 1 + look, False))
        s += C
    out.append((s, n_frames - 1 - s, n_frames - s, True))
    return out


@pytest.mark.parametrize("with_cuts", [False, True], ids=["no-cuts", "cuts"])
@pytest.mark.parametrize("C", [1, 2, 5])
@pytest.mark.parametrize("rate", RATES, ids=lambda r: f"{r[0]}to{r[1]}")
def test_the_entries_of_the_chunks_are_the_clips(rate, C, with_cuts):
    rng = random.Random(3)
    n_frames = 17
    for depth, s in ((2, F(1, 2)), (2, F(1)), (1, F(1, 8)), (3, F(3, 4))):
        pl = _plan(rate[0], rate[1], depth)
        G = pl.G
        cuts = [rng.random() < 0.25 for _ in range(n_frames - 1)] if with_cuts else None
        J = pl.n_out(n_frames)
        whole = RT.shutter_entries(pl, s, 0, 0, J, n_frames - 1, cuts, n_frames - 1)
        ahead = math.ceil(s * pl.p / pl.q)
        assert RT.shutter_lookahead(pl, s) == ahead
        look = ahead + (1 if with_cuts else 0)
        made = []
        for first, c, m, last in _chunks(n_frames, C, look):
            seen = None
            if with_cuts:   # the flags of every interval read; the last one read is not to be relied on: it lies
                seen = list(cuts[first:first + m - 1])
                if not last and seen:
                    seen[-1] = not seen[-1]
            j0, nj = pl.span(first, c, last)
            assert j0 == len(made)
            clip_last = first + c if last else None
            ext = RT.shutter_reach(pl, s, first, c, j0, nj, seen, clip_last)
            assert 0 <= ext <= ahead and c + 1 + ext <= m and (ext == 0 or not last)
            part = RT.shutter_entries(pl, s, first, j0, nj, c + ext, None if seen is None else seen[:c + ext], clip_last)
            made += [(row + first * G, w) for row, w in part]
        assert made == whole, (depth, s)
    # p > q with chunk_frames 1: a chunk without a frame of its own
    pl = _plan(60, 24, 2)
    assert [pl.span(i, 1)[1] for i in range(5)] == [1, 0, 1, 0, 0]


# ---- plans and parsing ------------------------------------------------------------------------------------------------------
def test_plan_any_rate():
    assert tuple(RT.plan(60, 24, 2, any_rate=True)) == (5, 2, 4) and tuple(RT.plan(60, 60, 1, any_rate=True)) == (1, 1, 2)
    assert tuple(RT.plan(24, 60, 2, any_rate=True)) == tuple(RT.plan(24, 60, 2))
    for fps in (24, 60):
        with pytest.raises(ValueError, match="fps must be above the source rate"):
            RT.plan(60, fps, 2)
    with pytest.raises(ValueError, match=r"numerator must not exceed 2\*\*20"):
        RT.plan((1 << 20) + 1, 1, 2, any_rate=True)
    with pytest.raises(ValueError, match=r"denominator must not exceed 2\*\*20"):
        RT.plan(1, (1 << 20) + 1, 2, any_rate=True)
    assert RT.plan(1 << 20, 1, 2, any_rate=True).p == 1 << 20


def test_check_shutter():
    assert RT.check_shutter(None) is None
    for x, want in ((0, 0), (1, 1), ("1/2", F(1, 2)), (" 3 / 8 ", F(3, 8)), ((1, 4), F(1, 4)), (F(2, 3), F(2, 3)), ("0", 0)):
        assert RT.check_shutter(x) == want and isinstance(RT.check_shutter(x), F)
    with pytest.raises(ValueError) as e:
        RT.check_shutter(0.5)
    with pytest.raises(ValueError) as f:
        RT.parse_fps(0.5)
    # the float refusal is parse_fps's sentence
    assert str(e.value).split("must be exact")[1].split("such as")[0] == str(f.value).split("must be exact")[1].split("such as")[0]
    assert "must be exact, got the float 0.5: pass a fraction as a string or a pair" in str(e.value)
    for bad in ("3/2", 2, (5, 4), "-1/2", "1/0", True, "half", [1, 2, 3], b"1/2"):
        with pytest.raises(ValueError, match="shutter"):
            RT.check_shutter(bad)


def test_command_line():
    ap = cli.parser()
    base = ["video", "--input", "a.y4m", "--output", "b.y4m"]
    assert ap.parse_args(base).shutter is None
    a = ap.parse_args(base + ["--fps", "50", "--shutter", "1/2"])
    assert a.shutter == F(1, 2) and a.fps == 50
    assert ap.parse_args(base + ["--shutter", "0"]).shutter == 0
    for bad in ("0.5", "3/2", "x"):
        with pytest.raises(SystemExit):
            ap.parse_args(base + ["--shutter", bad])
    assert "--shutter" in cli.__doc__ and "--fps 50 --shutter 1/2" in cli.__doc__


# ---- refusals before any GPU work ---------------------------------------------------------------------------------------------
def _cpu_model(channels=1):
    return P.FrameInterpolationUNet(bilinear=True, frame_channels=channels).eval()


REFUSALS = [
    (dict(shutter="1/2"), "fps.*shutter|shutter.*fps"),                                    # fps is required
    (dict(shutter=0), "fps.*shutter|shutter.*fps"),
    (dict(shutter="1/2", fps=12, dedup=0), "shutter.*dedup|dedup.*shutter"),
    (dict(shutter=0, fps=12, dedup=0), "shutter.*dedup|dedup.*shutter"),
    (dict(shutter="1/2", fps=12, retime="nearest"), "retime"),
    (dict(shutter="1/2", fps=12, retime="motion"), "retime"),
    (dict(shutter=0.5, fps=12), "must be exact"),
    (dict(shutter="3/2", fps=12), "shutter"),
    (dict(shutter=1, fps=2), "shutter"),                                                   # 12 source intervals per window
    (dict(shutter=1, fps=4, time_depth=4), "time_depth"),                                  # 6 x 16 grid rows
    (dict(shutter=0, fps="1/43691"), r"2\*\*20"),                                          # p = 24 * 43691 > 2**20
    (dict(fps=12), "fps must be above the source rate"),                                   # without shutter: as ever
    (dict(fps=24), "fps must be above the source rate"),
]


@pytest.mark.parametrize("chunk_frames", [None, 3])
@pytest.mark.parametrize("kw,match", REFUSALS)
def test_interpolate_video_refuses_before_gpu_work(tmp_path, kw, match, chunk_frames):
    npy, y4m, raw = (str(tmp_path / n) for n in ("in.npy", "in.y4m", "in.rgb"))
    np.save(npy, np.zeros((2, 16, 16), np.uint8))
    IO.write_y4m(y4m, np.zeros((2, 16, 16), np.uint8), (np.zeros((2, 8, 8), np.uint8),) * 2, fps=(24, 1))
    open(raw, "wb").write(bytes(2 * 16 * 16 * 3))
    for src, dst, ch, extra in ((npy, "out.npy", 1, dict(src_fps=24)), (y4m, "out.y4m", 1, {}), (y4m, "out.y4m", 3, {}),
                                (raw, "out.rgb", 3, dict(raw="rgb24", width=16, height=16, src_fps=24))):
        fi = P.FrameInterpolator(model=_cpu_model(ch), device="cuda")
        with pytest.raises(ValueError, match=match):
            fi.interpolate_video(src, str(tmp_path / dst), 2, chunk_frames=chunk_frames, **extra, **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.npy", "in.rgb", "in.y4m"]    # no output, no .part


def test_the_remedies_are_named():
    with pytest.raises(ValueError, match="lower `time_depth` or `shutter`"):
        RT.check_shutter_plan(_plan(120, 24, 4), F(1))
    with pytest.raises(ValueError, match="lower `shutter`"):
        RT.check_shutter_plan(_plan(120, 10, 1), F(1))
    RT.check_shutter_plan(_plan(120, 24, 3), F(1))
    RT.check_shutter_plan(_plan(60, 24, 4), F(1))
    with pytest.raises(ValueError, match="lower `time_depth` or `shutter`"):
        RT.shutter_entries(_plan(120, 24, 4), F(1), 0, 0, 1, 8, None, 8)
    with pytest.raises(ValueError, match="needs grid rows"):
        RT.shutter_entries(_plan(60, 24, 2), F(1), 0, 1, 1, 3)


# ---- the C ABI's checks, the header ------------------------------------------------------------------------------------------
def test_c_abi_refuses_bad_entries_without_gpu(hip_lib_built):
    lib = _native.lib()
    fake = ctypes.c_void_p(256)
    ok = [(0, [D]), (3, [D // 2, D // 2]), (1, [D - 1, 0, 1]), (0, [1] * 47 + [D - 47]), (4, [D])]   # a grid of 48 rows

    def call(fn, entries, grid=fake, n_rows=48, fs=0, n_out=None, out=fake):
        arr = _native.shutter_entries(entries)
        return fn(grid, n_rows, fs, arr, len(entries) if n_out is None else n_out, out, None)

    for fn in (lib.fiunet_shutter_u8, lib.fiunet_shutter_p10):
        assert call(fn, ok) == 0                                                  # (an empty frame: no launch)
        assert call(fn, []) == 0 and call(fn, ok, n_out=0, grid=None) == 1
        for bad in ((0, []), (0, [1] * 48 + [D - 48]),                            # n_taps outside 1 .. 48
                    (0, [D - 1]), (0, [D, 1]), (0, [0]), (0, [D + 1]), (2, [(1 << 32) - 1, D + 1]),   # sum w != 2**20
                    (48, [D]), (47, [D // 2, D // 2]), (47, [D, 0]), ((1 << 32) - 1, [D]), (1 << 31, [D])):   # rows
            for pos in (0, len(ok)):
                entries = ok[:pos] + [bad] + ok[pos:]
                assert call(fn, entries) == 1, bad
                assert lib.fiunet_last_error_string()
        assert call(fn, ok, grid=None) == 1 and call(fn, ok, out=None) == 1
        assert call(fn, ok, n_rows=-1) == 1 and call(fn, ok, n_out=-1) == 1
        assert fn(fake, 48, 0, None, 4, fake, None) == 1                          # entries NULL
        assert call(fn, [(0, [D // 2, D // 2])] * 70 + [(0, [1] * 47 + [D - 47])] * 40, n_rows=48) == 0   # several launches
    with pytest.raises(ValueError, match="32 bits"):
        _native.shutter_entries([(0, [-1])])
    assert _native.SHUTTER_MAX_TAPS == RT.SHUTTER_MAX_TAPS == 48


def test_header_symbols_and_the_kernels_constants():
    hdr = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    new = ["fiunet_shutter_p10", "fiunet_shutter_u8"]
    assert sorted(re.findall(r"\b(fiunet_shutter[a-z0-9_]*)\s*\(", code)) == new and set(new) <= set(_native.SYMBOLS)
    for name in new:
        assert name in hdr.split("enum fiunet_status")[0]     # the version comment names them
    assert re.search(r"#define FIUNET_ABI_VERSION 8\b", hdr)
    src = open(os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc", "shutter.hip.h")).read()
    assert re.search(r"kShutterMaxTaps = 48;", src) and re.search(r"kShutterOne = 1u << 20;", src)
    # the argument block: 32 frames and 864 weights stay below 4 KB
    frames, weights = (int(re.search(rf"{n} = (\d+);", src).group(1)) for n in ("kShutterMaxFrames", "kShutterMaxWeights"))
    assert frames * 8 + weights * 4 + 24 < 4096 and weights >= 48
    assert '#include "shutter.hip.h"' in open(os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc", "video.hip")).read()


def test_the_new_entry_points_are_rows_of_the_stream_contract():
    import stream_contract as SC
    rows = [r.entry for r in SC.ROWS]
    for r in shutter_stream_rows.ROWS:
        assert rows.count(r.entry) == 1, r.entry
    shutter_stream_rows.register()          # idempotent
    assert [r.entry for r in SC.ROWS] == rows


# ---- the restatement itself -------------------------------------------------------------------------------------------------
def test_reference_mix_and_point():
    g = np.array([[0, 10], [4, 20], [255, 255], [255, 255]], np.uint8)
    assert SR.mix(g, {0: D // 2, 1: D // 2}, 8).tolist() == [2, 15]
    assert SR.mix(g, {2: D - 1, 3: 1}, 8).tolist() == [255, 255]
    w = np.array([[1023, 5000], [1023, 7]], np.uint16)
    assert SR.mix(w, {0: D}, 10).tolist() == [1023, 5000]                     # one tap: a copy, the word as it is
    assert SR.mix(w, {0: D // 2, 1: D // 2}, 10).tolist() == [1023, 515]      # above 1023 reads as 1023
    assert SR.mix(w.view(np.int16), {0: D - 1, 1: 1}, 10).tolist() == [1023, 1023]
    assert SR.apply_entries(g, [(1, [0, D, 0]), (0, [D // 2, D // 2])], 8).tolist() == [[255, 255], [2, 15]]
    # point sampling for p > q: 60 -> 24 at G = 4 takes rows 0, 10, 20
    grid = np.arange(21, dtype=np.uint8)[:, None] * 10
    assert SR.convert(grid, 6, 60, 24, 4, 0, 8).ravel().tolist() == [0, 100, 200]
    assert SR.convert(grid, 6, 60, 50, 4, 0, 8).ravel().tolist() == [0, 48, 96, 144, 192]
    assert SR.convert(grid, 6, 60, 24, 4, F(1, 2), 8).ravel().tolist() == [25, 125, 200]
