"""CPU: the host side of the re-timing of repeated frames (retime.py's second half) against brute-force
Fraction arithmetic (tests/dedup_ref.py): spans, the entry table, the chunked classification that stream.py runs, the
argument checks, which come before any GPU work, the C entry points' host-side refusals and the command line."""
import ctypes
import os
import random
import sys
from fractions import Fraction
from math import gcd

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as D  # noqa: E402
import dedup_stream_rows  # noqa: E402  (importing it adds the new entry points' rows to the stream contract's table)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, imageio_lite as IO  # noqa: E402

RT = P.retime
GAPS = (2, 4, 8)


def _plans():
    """(name, plan): the issue's rate ratios, factor 2 and 4 as `dedup` without fps runs them."""
    return [("24->60", RT.plan("24", "60", 2)), ("23.976->59.94", RT.plan("24000/1001", "60000/1001", 3)),
            ("factor2", RT.dedup_plan(None, 2, 4)), ("factor4", RT.dedup_plan(None, 4, 4)),
            ("q*gap=2**20", RT.plan(Fraction(5), Fraction(1 << 17), 4))]


def _patterns(seed, n, count=40):
    """Random (dead, cuts) patterns over n intervals, dead runs of every length among them; and the named cases."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        pd, pc = rng.choice((0.3, 0.6, 0.85)), rng.choice((0.0, 0.15))
        out.append(([rng.random() < pd for _ in range(n)], [rng.random() < pc for _ in range(n)]))
    live = [False] * n
    if n < 12:
        return out
    for name, dead_at, cut_at in (("start", (0, 1), ()), ("end", (n - 2, n - 1), ()), ("long", tuple(range(2, 12)), ()),
                                  ("before a cut", (3, 4), (5,)), ("all dead", tuple(range(n)), ()),
                                  ("none", (), ())):
        dead, cuts = list(live), list(live)
        for k in dead_at:
            dead[k] = True
        for k in cut_at:
            cuts[k] = True
        out.append((dead, cuts))
    return out


N_INT = 17


@pytest.mark.parametrize("max_gap", GAPS)
def test_spans_against_the_definition(max_gap):
    for dead, cuts in _patterns(max_gap, N_INT):
        for use_cuts in (cuts, None):
            spans = RT.dedup_spans(dead, use_cuts, max_gap)
            where = {f: (a, a + ln - 1, ln) for a, ln in spans for f in range(a, a + ln)}
            assert len(where) == sum(ln for _, ln in spans)                   # disjoint
            for f in range(N_INT):
                assert where.get(f, (f, f, 1)) == D.span_of(f, dead, use_cuts, max_gap), (dead, use_cuts, f)
            for a, ln in spans:
                assert 2 <= ln <= max_gap and all(dead[a:a + ln - 1]) and not dead[a + ln - 1]
                assert (a == 0 or not dead[a - 1]) and not (use_cuts and use_cuts[a + ln - 1])


def test_named_cases():
    n = N_INT
    pats = _patterns(0, n)[-6:]
    (start, end, long, cut, alldead, none) = [RT.dedup_spans(d, c, 4) for d, c in pats]
    assert start == [(0, 3)]          # a run at clip start is a span
    assert end == []                  # a run that reaches the clip's end is not
    assert long == []                 # ten dead intervals: a hold
    assert cut == []                  # a run before a cut
    assert alldead == [] and none == []
    assert RT.dedup_spans(pats[2][0], None, 8) == []                     # 10 + 1 > 8
    assert RT.dedup_spans([True] * 7 + [False], None, 8) == [(0, 8)]     # L == max_gap is accepted
    assert RT.dedup_spans([True] * 8 + [False], None, 8) == []


def _eval(entry, G):
    row, wn, den = entry
    return row // G, row % G, Fraction(wn, den)


@pytest.mark.parametrize("max_gap", GAPS)
@pytest.mark.parametrize("name,pl", _plans(), ids=[n for n, _ in _plans()])
def test_entries_against_fraction_arithmetic(name, pl, max_gap):
    if name == "q*gap=2**20":
        pl = RT.plan(Fraction(5), Fraction((1 << 20) // max_gap), 4)
        assert pl.q * max_gap == 1 << 20
        with pytest.raises(ValueError, match=r"2\*\*20"):
            RT.dedup_plan(RT.plan(Fraction(1), Fraction((1 << 20) // max_gap + 1), 4), 2, max_gap)
    p, q, G = pl
    assert RT.dedup_plan(pl, 2, max_gap) is pl
    step, n_frames = Fraction(p, q), N_INT + 1
    J = pl.n_out(n_frames)
    assert J == D.n_out(n_frames, step)
    js = range(J) if J < 400 else sorted(random.Random(1).sample(range(J), 300) + [0, J - 1])
    for dead, cuts in _patterns(100 + max_gap, N_INT, count=12):
        for use_cuts in (cuts, None):
            spans = RT.dedup_spans(dead, use_cuts, max_gap)
            for mode in RT.MODES:
                for j in js:
                    (row, wn, den), = RT.table_entries(pl, spans, 0, j, 1, N_INT, mode, use_cuts)
                    assert 0 <= wn < den <= q * max_gap and gcd(wn, den) == 1 and 0 <= row < N_INT * G + 1
                    i, lo, w = D.place(j, step, G, dead, use_cuts, max_gap)
                    if w is None:
                        w = Fraction(0)
                    if mode == "nearest":
                        i, lo, w = (i + (lo + 1) // G, (lo + 1) % G, Fraction(0)) if w > Fraction(1, 2) else (i, lo, 0)
                    assert _eval((row, wn, den), G) == (i, lo, w), (name, j, mode)


@pytest.mark.parametrize("name,pl", _plans(), ids=[n for n, _ in _plans()])
def test_without_dead_intervals_the_entries_are_the_plan(name, pl):
    p, q, G = pl
    J = min(pl.n_out(N_INT + 1), 500)
    cuts = [k % 5 == 2 for k in range(N_INT)]
    for use_cuts in (None, cuts):
        entries = RT.table_entries(pl, [], 0, 0, J, N_INT, "blend", use_cuts)
        for j, e in enumerate(entries):
            i, r, lo, wn = pl.frame(j)
            if use_cuts and r and use_cuts[i]:
                lo = wn = 0
            assert _eval(e, G) == (i, lo, Fraction(wn, q))
    # a grid that starts at interval 5: rows count from there, and a frame outside it is refused
    j0, nj = pl.span(5, 3, False)
    for k, e in enumerate(RT.table_entries(pl, [], 5, j0, nj, 3)):
        i, r, lo, wn = pl.frame(j0 + k)
        assert _eval(e, G) == (i - 5, lo, Fraction(wn, q))
    with pytest.raises(ValueError, match="grid"):
        RT.table_entries(pl, [], 5, j0, nj + 1 + q // p, 3)
    with pytest.raises(ValueError, match="grid"):
        RT.table_entries(pl, [], 5, j0 - 1, 1, 3)


def _chunks(n_frames, C, look):
    """(s, frames read, c, last) of the chunks stream._run's reader makes."""
    s, out = 0, []
    while True:
        m = min(C + 1 + look, n_frames - s)
        if m == C + 1 + look:
            out.append((s, m, C, False))
            s += C
            continue
        out.append((s, m, m - 1, True))
        return out


@pytest.mark.parametrize("max_gap", GAPS)
@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6])
def test_chunked_classification_equals_the_whole_clip(C, max_gap):
    rng = random.Random(C * 10 + max_gap)
    pl = RT.plan("24", "60", 2)
    for n_int in (N_INT, 1, 2, max_gap, max_gap + 1):
        for dead, cuts in _patterns(C * 100 + max_gap, n_int, count=25)[:25] + (_patterns(0, n_int)[-6:] if
                                                                                  n_int == N_INT else []):
            for use_cuts in (cuts, None):
                look = max_gap if use_cuts is not None else max_gap - 1
                whole = RT.dedup_spans(dead, use_cuts, max_gap)
                want = RT.table_entries(pl, whole, 0, 0, pl.n_out(n_int + 1), n_int, "blend", use_cuts)
                carry, got, straddles = 0, [], 0
                for s, m, c, last in _chunks(n_int + 1, C, look):
                    assert c <= C + max(look - 1, 0)                      # what stream._run sizes its slots for
                    wd = dead[s:s + m - 1]
                    wc = None if use_cuts is None else list(use_cuts[s:s + m - 1])
                    if wc and not last:
                        wc[-1] = rng.random() < 0.5                       # scored without its neighbour: not relied on
                    if c == 0:
                        spans, e = [], 0
                    else:
                        spans, e, carry = RT.classify_chunk(wd, wc, carry, s, c, max_gap)
                    assert 0 <= e <= max_gap - 1 and c + e <= m - 1 and not (last and e)
                    assert spans == [sp for sp in whole if sp[0] + sp[1] > s and sp[0] < s + c]
                    straddles += bool(e)
                    true_carry = 0
                    while true_carry < s + c and dead[s + c - 1 - true_carry]:
                        true_carry += 1
                    assert carry == min(true_carry, max_gap)
                    j0, nj = pl.span(s, c, last)
                    assert j0 == len(got)
                    loc = RT.table_entries(pl, spans, s, j0, nj, c + e, "blend", None if wc is None else wc[:c + e])
                    got += [(row + s * pl.G, wn, den) for row, wn, den in loc]   # rows of the whole clip's grid
                assert got == want, (dead, use_cuts, C)


def test_a_span_straddles_a_chunk_edge():
    dead = [False, True, True, False, False, True, False]
    spans, e, carry = RT.classify_chunk(dead[0:5], None, 0, 0, 2, 4)
    assert (spans, e, carry) == ([(1, 3)], 2, 1)
    spans, e, carry = RT.classify_chunk(dead[2:7], None, 1, 2, 2, 4)
    assert (spans, e, carry) == ([(1, 3)], 0, 0)


# ---- refusals before any GPU work ------------------------------------------------------------------------------------
def test_check_dedup():
    assert RT.check_dedup(None) == (None, 4) and RT.check_dedup(0) == (0.0, 4) and RT.check_dedup(1.5, 8) == (1.5, 8)
    assert RT.check_dedup(np.float32(2), np.int64(2)) == (2.0, 2)
    for bad in (-1, -0.5, float("nan"), float("inf"), -float("inf"), True, "1", [1]):
        with pytest.raises(ValueError, match="dedup"):
            RT.check_dedup(bad)
    for bad in (1, 9, 0, -4, 4.0, True, "4", None):
        with pytest.raises(ValueError, match="max_gap"):
            RT.check_dedup(0, bad)
        with pytest.raises(ValueError, match="max_gap"):
            RT.check_dedup(None, bad)
    assert RT.dead_limit(0) == 0 and RT.dead_limit(1) == 64 and RT.dead_limit(0.99) == 63 and RT.dead_limit(1e30) > 1 << 16


def _cpu_model(channels=1):
    return P.FrameInterpolationUNet(bilinear=True, frame_channels=channels).eval()


REFUSALS = [
    (dict(dedup=-1), "dedup"),
    (dict(dedup=float("nan")), "dedup"),
    (dict(dedup=float("inf")), "dedup"),
    (dict(dedup=True), "dedup"),
    (dict(dedup="0"), "dedup"),
    (dict(dedup=0, max_gap=1), "max_gap"),
    (dict(dedup=0, max_gap=9), "max_gap"),
    (dict(max_gap=2.0), "max_gap"),
    (dict(dedup=0, factor=32), "factor"),
    (dict(dedup=0, fps="262145/2", max_gap=8), r"2\*\*20"),     # 24 / fps = 48 / 262145: q * 8 > 2**20
]


@pytest.mark.parametrize("chunk_frames", [None, 3])
@pytest.mark.parametrize("kw,match", REFUSALS)
def test_interpolate_video_refuses_before_gpu_work(tmp_path, kw, match, chunk_frames):
    npy, y4m, raw = (str(tmp_path / n) for n in ("in.npy", "in.y4m", "in.rgb"))
    np.save(npy, np.zeros((2, 16, 16), np.uint8))
    IO.write_y4m(y4m, np.zeros((2, 16, 16), np.uint8), (np.zeros((2, 8, 8), np.uint8),) * 2, fps=(24, 1))
    open(raw, "wb").write(bytes(2 * 16 * 16 * 3))
    kw = dict(kw)
    factor = kw.pop("factor", 2)
    for src, dst, ch, extra in ((npy, "out.npy", 1, dict(src_fps=24)), (y4m, "out.y4m", 1, {}), (y4m, "out.y4m", 3, {}),
                                (raw, "out.rgb", 3, dict(raw="rgb24", width=16, height=16, src_fps=24))):
        fi = P.FrameInterpolator(model=_cpu_model(ch), device="cuda")
        with pytest.raises(ValueError, match=match):
            fi.interpolate_video(src, str(tmp_path / dst), factor, chunk_frames=chunk_frames, **extra, **kw)
        assert sorted(os.listdir(tmp_path)) == ["in.npy", "in.rgb", "in.y4m"]    # no output, no .part


def test_c_abi_refuses_bad_tables_without_gpu(hip_lib_built):
    lib = _native.lib()
    fake = ctypes.c_void_p(256)
    ok = [(0, 0, 1), (3, 1, 2), (4, 0, 7), (3, (1 << 20) - 1, 1 << 20)]          # a grid of 5 rows

    def call(fn, entries, grid=fake, n_rows=5, fs=0, n_out=None, out=fake):
        arr = _native.retime_entries(entries)
        return fn(grid, n_rows, fs, arr, len(entries) if n_out is None else n_out, out, None)

    for fn in (lib.fiunet_retime_table_u8, lib.fiunet_retime_table_p10):
        assert call(fn, ok) == 0                                                  # (an empty frame: no launch)
        assert call(fn, []) == 0 and call(fn, ok, n_out=0, grid=None) == 1
        for bad in ((5, 0, 1), (1 << 31, 0, 1), ((1 << 32) - 1, 0, 1),            # row >= n_rows
                    (0, 1, 1), (0, 2, 2), (0, 5, 3),                              # wn >= den
                    (4, 1, 2),                                                    # wn > 0 needs the row after
                    (0, 0, 0), (0, 0, (1 << 20) + 1), (0, 1, (1 << 32) - 1)):     # den outside 1 .. 2**20
            for pos in (0, len(ok)):
                entries = ok[:pos] + [bad] + ok[pos:]
                assert call(fn, entries) == 1, bad
                assert lib.fiunet_last_error_string()
        assert call(fn, ok, grid=None) == 1 and call(fn, ok, out=None) == 1
        assert call(fn, ok, n_rows=-1) == 1 and call(fn, ok, n_out=-1) == 1
        assert fn(fake, 5, 0, None, 4, fake, None) == 1                           # entries NULL
        assert call(fn, [(0, 0, 1)] * 130, n_rows=1) == 0                         # more than one launch's worth
    for fn in (lib.fiunet_pair_peak_u8, lib.fiunet_pair_peak_p10):                # pair_sad's conventions
        assert fn(None, 2, 16, fake, None) == 1 and fn(fake, 2, 16, None, None) == 1 and fn(fake, -1, 16, fake, None) == 1
        assert fn(fake, 1, 16, fake, None) == 0 and fn(fake, 0, 16, fake, None) == 0 and fn(fake, 3, 0, fake, None) == 0
    with pytest.raises(ValueError, match="32 bits"):
        _native.retime_entries([(0, -1, 1)])


def test_the_new_entry_points_are_rows_of_the_stream_contract():
    import stream_contract as SC
    rows = [r.entry for r in SC.ROWS]
    for r in dedup_stream_rows.ROWS:
        assert rows.count(r.entry) == 1, r.entry
    dedup_stream_rows.register()          # idempotent
    assert [r.entry for r in SC.ROWS] == rows


def test_header_symbols_and_struct():
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "fiunet.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert sorted(set(re.findall(r"\b(fiunet_[a-z0-9_]+)\s*\(", code))) == sorted(_native.SYMBOLS)
    for name in ("fiunet_pair_peak_u8", "fiunet_pair_peak_p10", "fiunet_retime_table_u8", "fiunet_retime_table_p10"):
        assert name in _native.SYMBOLS and name in hdr.split("enum fiunet_status")[0]     # the version comment names them
    assert re.search(r"typedef struct fiunet_retime_entry \{\s*uint32_t row, wn, den;\s*\} fiunet_retime_entry;", code)
    assert ctypes.sizeof(_native.RetimeEntry) == 12


# ---- the reference peak, and the command line -------------------------------------------------------------------------
def test_reference_peak_is_a_maximum_over_segments():
    f = np.zeros((2, 130), np.uint8)
    f[1, 63], f[1, 64], f[1, 129] = 10, 20, 7          # either side of a segment edge, and the short last segment
    assert D.pair_peak(f).tolist() == [20]
    f[1, 129] = 30
    assert D.pair_peak(f).tolist() == [30]
    w = np.array([[0, 1023], [2000, 65535]], np.uint16)
    assert D.pair_peak(w, 10).tolist() == [1023] and D.pair_peak(w.view(np.int16), 10).tolist() == [1023]
    assert D.dead_of([0, 64, 65], 1) == [True, True, False] and D.dead_of([0, 1], 0) == [True, False]


def test_cli_flags():
    base = ["video", "--input", "a.y4m", "--output", "b.y4m"]
    a = cli.parse_args(base)
    assert a.dedup is None and a.max_gap == 4
    a = cli.parse_args(base + ["--dedup", "1.5", "--max-gap", "3"])
    assert a.dedup == 1.5 and a.max_gap == 3
    assert cli.parse_args(base + ["--dedup", "0"]).dedup == 0.0
    for bad in (["--dedup", "-1"], ["--dedup", "nan"], ["--dedup", "inf"], ["--dedup", "x"], ["--max-gap", "1"], ["--max-gap", "9"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)
    dead = np.array([0, 1, 1, 0, 1, 0, 1], bool)
    log = [(np.zeros(3), dead[:3]), (np.zeros(4), dead[3:])]
    assert cli.retimed_repeats(log, None, 4) == 3                     # the trailing run is not re-timed
    cuts = [(np.zeros(3), np.zeros(3, np.uint8)), (np.zeros(4), np.array([1, 0, 0, 0], np.uint8))]
    assert cli.retimed_repeats(log, cuts, 4) == 1 and cli.retimed_repeats(log, None, 2) == 1
