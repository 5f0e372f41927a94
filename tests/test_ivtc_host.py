"""CPU: inverse telecine's definition (tests/ivtc_ref.py) held to what it is for, the host arithmetic of
ai_based_frame_interpolation_amd.ivtc against it, and the argument checks of the four entry points.

  1. 2:3 pulldown of the film content of tests/ivtc_content.py (sizes 24x40, 34x70, 48x136; tff and bff; phases 0..4;
     motions (3,1), (5,3), (4,0); cut to whole cycles) comes back as the film frames, byte for byte, in order, each once
  2. the separation that makes 1. a statement about the definition and not about luck, on the reference's own scores
  3. `choose`'s ties, `decimate_plan` on hand-written peaks, the `Carry` fed in pieces
  4. two telecined clips joined mid-cycle: a flagged orphan at the join, film frames elsewhere
  5. one hand-computed comb score on a 5 x 70 plane
  6. the C ABI: names, struct, refusals before any launch; the stream-contract rows; the command line

Separation, measured with this file's content at T = 12 (8 bits) and T = 48 (10-bit codes = the 8-bit picture times four,
the same counts): a candidate that is a film frame scores at most 24 (24x40: 19, 34x70: 23, 48x136: 24), a candidate
woven from two film frames at least 248 (248 / 452 / 570), the best candidate of an orphan at least 327 (327 / 466 / 609),
against `combed` = 48.  The content is box-blurred TWICE: after one pass of 13 x 13 the curvature of the picture itself
reads as comb (film frames scored up to 257), so the content was changed and the defaults were not.

Phase 2.  The clip begins with an orphan and cycle 0 then holds five DIFFERENT pictures (orphan, film 2, 3, 4, 5) while
the repeat of film 5 opens cycle 1.  The definition drops one frame of every complete cycle, so cycle 0 loses the film
frame that moved least against its predecessor: a fixed-cycle decimation cannot do otherwise (ffmpeg's decimate has the
same property).  For phase 2 the test therefore asserts exactly that - the film frames in order, none twice, one frame of
cycle 0 missing - and "each once" for every other phase."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivtc_content as C  # noqa: E402
import ivtc_ref as R  # noqa: E402
import ivtc_stream_rows  # noqa: E402

from ai_based_frame_interpolation_amd import _native, cli, ivtc as I  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every film-frame candidate at or below, every other candidate at or above: just outside this content's recorded margins
# (24 and 248), inside the issue's own trial figures (29 and 78), far either side of `combed`
CLEAN_MAX, WRONG_MIN = 26, 240
COMBED = 48


def _plane(h, w):
    return [(0, h, w, w, 1)]


def _film_index(frame, film):
    hits = [f for f in range(film.shape[0]) if np.array_equal(frame, film[f])]
    return hits[0] if hits else None


def _clip(h, w, motion, order, phase):
    film = C.film(h, w, motion)
    tc, pairs = R.telecine(film, order, phase)
    n = len(tc) // 5 * 5
    return film, tc[:n], pairs[:n]


# ---- 1., 2. --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("size", C.SIZES)
def test_pulldown_comes_back_as_the_film_frames_and_the_scores_separate(size, order):
    h, w = size
    for motion in C.MOTIONS:
        for phase in range(5):
            film, tc, pairs = _clip(h, w, motion, order, phase)
            n = tc.shape[0]
            assert n == (20 if phase == 0 else 15)
            # the separation, on the reference's own scores
            scores = R.comb_scores(tc, order)
            orphans = []
            for t in range(n):
                second = {"p": pairs[max(t - 1, 0)][1], "c": pairs[t][1], "n": pairs[min(t + 1, n - 1)][1]}
                good = [c for c in R.CANDIDATES if second[c] == pairs[t][0]]
                for i, c in enumerate(R.CANDIDATES):
                    if c in good:
                        assert scores[t, i] <= CLEAN_MAX < COMBED, (motion, phase, t, c, scores[t])
                    else:
                        assert scores[t, i] >= WRONG_MIN > COMBED, (motion, phase, t, c, scores[t])
                if not good:
                    orphans.append(t)
            assert orphans == ([0] if phase in (2, 3) else []), (motion, phase)
            # the pipeline
            for fallback in ("deinterlace", "keep"):
                out, rep = R.ivtc(tc.reshape(n, -1), _plane(h, w), order=order, fallback=fallback)
                assert rep["frames_in"] == n and rep["frames_out"] == n * 4 // 5 == len(out)
                assert rep["combed"] == orphans and len(rep["dropped"]) == n // 5
                ids = [_film_index(f.reshape(h, w), film) for f in out]
                want = sorted({a for t, (a, b) in enumerate(pairs) if t not in orphans})
                if phase == 2:
                    body = ids[1:]
                    assert ids[0] is None and None not in body and body == sorted(set(body)), (motion, ids)
                    missing = sorted(set(want) - set(body))
                    assert len(missing) == 1 and missing[0] in (pairs[1][0], pairs[2][0], pairs[3][0], pairs[4][0])
                    assert set(body) <= set(want)
                elif phase == 3:
                    assert ids[0] is None and ids[1:] == want, (motion, ids)
                else:
                    assert ids == want, (motion, phase, ids)
            # without decimation: every frame matched, the repeats still there
            out, rep = R.ivtc(tc.reshape(n, -1), _plane(h, w), order=order, decimate=False)
            assert len(out) == n and rep["dropped"] == []
            assert [_film_index(f.reshape(h, w), film) for t, f in enumerate(out) if t not in orphans] == \
                [a for t, (a, b) in enumerate(pairs) if t not in orphans]


def test_the_package_telecine_is_the_reference_pulldown():
    h, w = 24, 40
    film = C.film(h, w)
    for order in R.ORDERS:
        for phase in range(5):
            want, _ = R.telecine(film, order, phase)
            got = I.telecine(torch.from_numpy(film.reshape(len(film), -1)), _plane(h, w), order, phase)
            assert np.array_equal(got.numpy().reshape(want.shape), want), (order, phase)
    with pytest.raises(ValueError, match="phase"):
        I.telecine(torch.zeros((4, h * w), dtype=torch.uint8), _plane(h, w), "tff", -1)
    with pytest.raises(ValueError, match="order"):
        I.telecine(torch.zeros((4, h * w), dtype=torch.uint8), _plane(h, w), "top")


def test_ten_bit_codes_score_as_the_eight_bit_picture_and_words_above_1023_read_as_1023():
    h, w = 24, 40
    f8, f10 = C.film(h, w), C.film(h, w, bits=10)
    t8, _ = R.telecine(f8, "tff", 1)
    t10, _ = R.telecine(f10, "tff", 1)
    assert np.array_equal(R.comb_scores(t8, "tff", 12, 8), R.comb_scores(t10, "tff", 48, 10))
    assert R.default_threshold(8) == I.default_threshold(8) == 12 and R.default_threshold(10) == I.default_threshold(10) == 48
    high = t10.copy()
    high[high >= 1020] = 60000
    assert np.array_equal(R.comb_scores(high, "tff", 48, 10), R.comb_scores(np.minimum(high, 1023), "tff", 48, 10))
    assert np.array_equal(R.comb_scores(high.view(np.int16), "tff", 48, 10), R.comb_scores(high, "tff", 48, 10))


# ---- 3. ------------------------------------------------------------------------------------------------------------------
def test_choose_prefers_c_then_p_on_ties_and_flags_above_combed():
    scores = [(5, 5, 5), (4, 5, 4), (6, 5, 4), (4, 5, 6), (5, 4, 4), (49, 50, 60), (48, 50, 60), (100, 0, 100), (3, 9, 3)]
    want = (["c", "p", "n", "p", "c", "p", "p", "c", "p"], [False, False, False, False, False, True, False, False, False])
    assert R.choose(scores) == want
    assert I.choose(scores) == want and I.choose(np.array(scores)) == want and I.choose(torch.tensor(scores)) == want
    assert I.choose(scores, combed=3)[1] == [True, True, True, True, True, True, True, False, False]
    assert I.choose([]) == ([], [])


@pytest.mark.parametrize("plan", [R.decimate_plan, I.decimate_plan])
def test_decimate_plan_on_hand_written_peaks(plan):
    inf = float("inf")
    assert plan([inf, 9, 0, 7, 8, 6, 5, 4, 3, 9]) == [0, 1, 3, 4, 5, 6, 7, 9]
    assert plan([inf, 3, 3, 3, 3]) == [0, 2, 3, 4]                       # ties: the earliest goes
    assert plan([inf, 5, 5, 2, 2, 0, 0, 0, 0, 0]) == [0, 1, 2, 4, 6, 7, 8, 9]
    assert plan([inf, 1, 2, 3, 4, 0, 0]) == [0, 2, 3, 4, 5, 6]           # an incomplete last cycle is kept whole
    assert plan([inf, 1, 2]) == [0, 1, 2] and plan([]) == []
    assert plan([1, 2, 3, 4], cycle=2) == [1, 3] and plan([inf, 1, 2, 3, 0, 1], cycle=3) == [0, 2, 3, 5]
    # start off a cycle boundary: frames 3, 4 are the tail of a cycle that is not whole here; 5..9 is; 10, 11 is not
    assert plan([9, 9, 4, 3, 2, 8, 9, 0, 0], start=3) == [3, 4, 5, 6, 8, 9, 10, 11]
    assert plan([7, 1, 5, 5, 5, 5], start=4) == [4, 6, 7, 8, 9]
    with pytest.raises((ValueError, AssertionError, ZeroDivisionError)):
        plan([1, 2, 3], cycle=0)


def test_the_carry_fed_in_pieces_gives_the_whole_clip_plan():
    rng = np.random.default_rng(5)
    for n in (0, 1, 4, 5, 6, 23, 40):
        peaks = [float("inf")] + [int(v) for v in rng.integers(0, 4, max(n - 1, 0))] if n else []
        want = R.decimate_plan(peaks)
        assert I.decimate_plan(peaks) == want
        for piece in (1, 2, 3, 7, 64):
            carry, got = I.Carry(), []
            for k in range(0, n, piece):
                got += carry.feed(peaks[k:k + piece])
                assert len(carry.pending) < 5 and carry.next == min(k + piece, n)
            got += carry.finish()
            assert got == want and carry.dropped == sorted(set(range(n)) - set(want)), (n, piece)
    carry = I.Carry(decimate=False)
    assert carry.feed([0, 0, 0]) + carry.feed([0, 0, 0, 0]) + carry.finish() == list(range(7)) and carry.dropped == []
    assert I.out_rate((30000, 1001)) == R.out_rate((30000, 1001)) == (24000, 1001)
    assert I.out_rate((30, 1)) == (24, 1) and I.out_rate((25, 1), 5, False) == (25, 1) and I.out_rate((30, 1), 6) == (25, 1)


# ---- 4. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", ["deinterlace", "keep"])
def test_two_clips_joined_mid_cycle_give_a_flagged_orphan_at_the_join(fallback):
    h, w = 34, 70
    film_a, film_b = C.film(h, w, (3, 1), seed=7), C.film(h, w, (5, 3), seed=8)
    a, pa = R.telecine(film_a, "tff", 0)
    b, pb = R.telecine(film_b, "tff", 0)
    # b begins with its frame 3 = (film 2, film 3): the other field of film 2 lay in b's frame 2, which the edit cut away
    tc = np.concatenate([a[:8], b[3:15]])
    pairs = [("a",) + p for p in pa[:8]] + [("b",) + p for p in pb[3:15]]
    n = len(tc)
    out, rep = R.ivtc(tc.reshape(n, -1), _plane(h, w), fallback=fallback, decimate=False)
    assert rep["combed"] == [8]
    for t in range(n):
        clip, first, _ = pairs[t]
        if t == 8:
            want = R.candidate(tc, t, R.choose(R.comb_scores(tc, first=8, count=1))[0][0]) if fallback == "keep" else None
            assert want is None or np.array_equal(out[t].reshape(h, w), want)
            assert _film_index(out[t].reshape(h, w), film_a) is None and _film_index(out[t].reshape(h, w), film_b) is None
        else:
            assert np.array_equal(out[t].reshape(h, w), (film_a if clip == "a" else film_b)[first]), t
    dec, rep = R.ivtc(tc.reshape(n, -1), _plane(h, w), fallback=fallback)
    assert rep["frames_out"] == 16 and rep["combed"] == [8] and rep["dropped"] == [2, 7, 12, 17]


# ---- 5. ------------------------------------------------------------------------------------------------------------------
def test_a_hand_computed_comb_score_with_a_partial_block_column():
    p = np.full((5, 70), 100, np.uint8)
    # row 2 lies 20 below its neighbours in columns 0..9 (block column 0) and 66..69 (the partial block column 1)
    p[2, 0:10] = 80
    p[2, 66:70] = 80
    # centre row 2: (100 - 80) * (100 - 80) = 400 > 144: 10 and 4 combed samples; centre rows 1 and 3 see one neighbour 20
    # below and one level: the product is 0
    assert R.comb_score(p, 12) == 10
    p[2, 0:10] = 100
    assert R.comb_score(p, 12) == 4
    assert R.comb_score(p, 20) == 0 and R.comb_score(p, 19) == 4        # 400 > T * T
    p[1, 60:66] = 130                                                     # row 1 above both neighbours, columns 60..65
    # centre row 1 in columns 60..63 (block column 0): (100 - 130)^2 = 900: 4 combed; columns 64, 65 (block column 1): 2,
    # beside the 4 of row 2: 6.  Centre row 2 at columns 60..65: (130 - 100) * (100 - 100) = 0
    assert R.comb_score(p, 12) == 6
    rows17 = np.full((17, 3), 50, np.uint8)
    rows17[15], rows17[16] = 90, 50         # centre row 15 (block row 0): (50 - 90) * (50 - 90) = 1600: 3 combed
    assert R.comb_score(rows17, 12) == 3    # (block row 1 holds row 16 alone, which has no row below it)
    with pytest.raises(AssertionError):
        R.comb_score(np.zeros((2, 8), np.uint8), 12)


# ---- 6. ------------------------------------------------------------------------------------------------------------------
NEW = ["fiunet_field_match_u8", "fiunet_field_match_p10", "fiunet_field_weave_u8", "fiunet_field_weave_p10"]
SRC, DST = 1 << 24, 1 << 28     # addresses that are never dereferenced: every refusal comes before a launch


def test_header_and_binding_name_the_entry_points(hip_lib_built):
    hdr = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW:
        assert name in _native.SYMBOLS and name + "(" in code and name in hdr.split("enum fiunet_status")[0]
    assert "#define FIUNET_ABI_VERSION 8" in hdr and _native.ABI_VERSION == 8
    assert re.search(r"typedef struct fiunet_weave_entry \{\s*uint32_t keep, other;\s*\} fiunet_weave_entry;", code)
    assert ctypes.sizeof(_native.WeaveEntry) == 8
    L = _native.lib()
    assert len(L.fiunet_field_match_u8.argtypes) == len(L.fiunet_field_match_p10.argtypes) == 9
    assert len(L.fiunet_field_weave_u8.argtypes) == len(L.fiunet_field_weave_p10.argtypes) == 10
    csrc = os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc")
    assert '#include "ivtc.hip.h"' in open(os.path.join(csrc, "video.hip")).read()
    assert {r.entry for r in ivtc_stream_rows.ROWS} == set(NEW) <= {r.entry for r in ivtc_stream_rows.SC.ROWS}


def _p(off=0, h=6, w=8, pitch=8, step=1, fs=48):
    return (off, h, w, pitch, step, fs)


def _match(L, name="fiunet_field_match_u8", src=SRC, n_src=3, plane=None, first=0, n_frames=3, order=0, threshold=12,
           scores=DST, filt=0):
    arr = None if plane == "null" else _native.resize_plane_array([_p() if plane is None else plane], filt)
    return getattr(L, name)(src, n_src, arr, first, n_frames, order, threshold, scores, None)


def _weave(L, name="fiunet_field_weave_u8", src=SRC, n_src=3, sp=None, dst=DST, dp=None, n_planes=None, entries=((0, 1),),
           n_out=None, parity=0, filt=0):
    sp = [_p()] if sp is None else sp
    dp = sp if dp is None else dp
    arr = _native.resize_plane_array
    ent = None if entries is None else _native.weave_entries(list(entries))
    return getattr(L, name)(src, n_src, arr(sp) if sp != "null" else None, dst, arr(dp, filt) if dp != "null" else None,
                            len(sp) if n_planes is None else n_planes, ent, len(entries or ()) if n_out is None else n_out,
                            parity, None)


def test_every_refusal_of_the_match_comes_before_a_launch(hip_lib_built):
    L = _native.lib()
    msg = L.fiunet_last_error_string
    for name in ("fiunet_field_match_u8", "fiunet_field_match_p10"):
        bad = [dict(src=None), dict(scores=None), dict(plane="null"), dict(order=2), dict(order=-1), dict(threshold=-1),
               dict(threshold=1024), dict(first=-1), dict(n_frames=-1), dict(first=1, n_frames=3), dict(first=4, n_frames=0),
               dict(n_src=-1, n_frames=0), dict(n_src=70000, n_frames=65536, plane=_p(fs=48)),
               dict(plane=_p(h=2, fs=48)), dict(plane=_p(h=0)), dict(plane=_p(w=0)), dict(plane=_p(step=5)), dict(plane=_p(step=0)),
               dict(plane=_p(pitch=7)), dict(plane=_p(fs=47)), dict(plane=_p(off=1)), dict(filt=1),
               dict(plane=_p(fs=1 << 63)), dict(scores=SRC + 16), dict(scores=SRC + 2)]
        for kw in bad:
            assert _match(L, name, **kw) == 1, (name, kw)
            assert msg(), kw
        assert _match(L, name, n_frames=0) == 0 and _match(L, name, first=3, n_frames=0) == 0
    assert _match(L, "fiunet_field_match_p10", src=SRC + 1) == 1 and b"misaligned" in msg()
    assert _match(L, plane=_p(h=2, fs=48)) == 1 and b"h < 3" in msg()
    assert _match(L, scores=SRC + 3 * 48 - 4) == 1 and b"overlap" in msg()
    assert _match(L, n_src=70000, n_frames=65536) == 1 and b"65535" in msg()


def test_every_refusal_of_the_weave_comes_before_a_launch(hip_lib_built):
    L = _native.lib()
    msg = L.fiunet_last_error_string
    for name in ("fiunet_field_weave_u8", "fiunet_field_weave_p10"):
        bad = [dict(src=None), dict(dst=None), dict(sp="null"), dict(dp="null"), dict(n_planes=0), dict(n_planes=5),
               dict(parity=2), dict(parity=-1), dict(n_src=-1), dict(n_out=-1), dict(entries=None, n_out=1),
               dict(entries=[(3, 0)]), dict(entries=[(0, 3)]), dict(entries=[(0, 0), (0, 1), (1 << 31, 0)]),
               dict(entries=[(0, 0)], n_src=0), dict(sp=[_p(h=1, fs=48)]), dict(sp=[_p(step=5)]), dict(sp=[_p(pitch=7)]),
               dict(sp=[_p(fs=47)]), dict(dp=[_p(h=8, fs=64)]), dict(dp=[_p(w=7)]), dict(filt=1),
               dict(sp=[_p(fs=1 << 63)]), dict(dst=SRC + 3 * 48 - 2), dict(dst=SRC), dict(dst=SRC - 46)]
        for kw in bad:
            assert _weave(L, name, **kw) == 1, (name, kw)
            assert msg(), kw
        assert _weave(L, name, entries=(), n_out=0) == 0 and _weave(L, name, entries=None, n_out=0) == 0
    assert _weave(L, "fiunet_field_weave_p10", dst=DST + 1) == 1 and b"misaligned" in msg()
    assert _weave(L, sp=[_p(h=1, fs=48)]) == 1 and b"h < 2" in msg()
    assert _weave(L, dst=SRC + 3 * 48 - 1) == 1 and b"overlap" in msg()
    assert _weave(L, entries=[(0, 0)] * 65536) == 1 and b"65535" in msg()
    with pytest.raises(ValueError, match="32 bits"):
        _native.weave_entries([(0, -1)])


def test_python_argument_checks_without_a_device():
    rows = torch.zeros((3, 6 * 8), dtype=torch.uint8)
    lay = [(0, 6, 8, 8, 1)]
    for call, kw, match in ((I.field_scores, dict(order="top"), "order"), (I.field_scores, dict(first=3, count=1), "window"),
                            (I.field_scores, dict(threshold=2000), "threshold"), (I.field_scores, dict(out=torch.zeros(3, 3)), "out must be"),
                            (I.weave, dict(entries=[(0, 3)]), "outside the window"), (I.weave, dict(entries=[(0, 0)], order="x"), "order")):
        with pytest.raises(ValueError, match=match):
            call(rows, lay, 8, **kw)
    with pytest.raises(ValueError, match="bits"):
        I.field_scores(rows, lay, 10)
    with pytest.raises(ValueError, match="h >= 3"):
        I.field_scores(rows, [(0, 2, 8, 8, 1)], 8)
    with pytest.raises(ValueError, match="the rows have"):
        I.weave(rows[:, :-1].contiguous(), lay, 8, [(0, 0)])
    with pytest.raises(ValueError, match="65535"):
        I.ivtc(torch.zeros((65536, 1), dtype=torch.uint8), [(0, 1, 1, 1, 1)], 8)
    for kw, match in ((dict(fallback="bob"), "fallback"), (dict(cycle=1), "cycle"), (dict(combed=-1), "combed"),
                      (dict(order="auto"), "order"), (dict(threshold=-1), "threshold")):
        with pytest.raises(ValueError, match=match):
            I.ivtc(rows, lay, 8, **kw)


def test_cli_ivtc_flags():
    a = cli.parse_args(["ivtc", "--input", "-", "--output", "-"])
    assert (a.order, a.no_decimate, a.cycle, a.comb_threshold, a.combed, a.fallback, a.chunk_frames, a.raw) == \
        ("auto", False, 5, None, 48, "deinterlace", 32, None)
    a = cli.parse_args(["ivtc", "--input", "a", "--output", "b", "--order", "bff", "--no-decimate", "--cycle", "6",
                        "--comb-threshold", "9", "--combed", "30", "--fallback", "keep", "--raw", "yuv422p10le", "--size",
                        "24x18", "--packing", "v210", "--chunk-frames", "3"])
    assert (a.order, a.no_decimate, a.cycle, a.comb_threshold, a.combed, a.fallback, a.chunk_frames) == \
        ("bff", True, 6, 9, 30, "keep", 3)
    assert (a.raw, a.size, a.packing) == ("yuv422p10le", (24, 18), "v210")
    for bad in (["--raw", "nv12"], ["--size", "8x6"], ["--packing", "v210"], ["--raw", "nv12", "--size", "8x6"],
                ["--fallback", "bob"], ["--model", "x.pth"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["ivtc", "--input", "-", "--output", "-"] + bad)
    assert cli.parse_args(["deinterlace", "--input", "-", "--output", "-"]).rate == "field"
