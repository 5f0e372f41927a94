"""GPU (MI355X): fiunet_field_match_u8 / _p10 and fiunet_field_weave_u8 / _p10 bit for bit against tests/ivtc_ref.py
(DESIGN.md 3.3x).

  1. the match: H x W of 3x1, 4x2, 17x64, 24x40, 34x70, 48x136 and 33x1030 (the smallest that reaches the vector path's
     per-lane tail plus a second wave), at 8 bits, 10-bit codes and 16-bit words above 1023, both orders; each clip tight
     and with an aligned pitch (the vector path with its tail)
  2. layouts: the Y of uyvy422, a byte of rgb24, the U of NV12, an unaligned base, `first` / `n_frames` inside a larger
     window with the clamps at both ends, two planes accumulated into one result, a frame stride that puts the last frame
     beyond 2^32 bytes
  3. the weave on the same layouts with 1..4 planes: 65 entries (two launches), keep == other, an output directly behind its
     input, guard bands
  4. the refusals launch nothing
  5. the stream-contract rows: side stream and captured graph"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivtc_content as C  # noqa: E402
import ivtc_ref as R  # noqa: E402
import ivtc_stream_rows as RS  # noqa: E402
import large_extent as LE  # noqa: E402
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native, ivtc as I  # noqa: E402
from ai_based_frame_interpolation_amd.layout import frame_layout  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((3, 1), (4, 2), (17, 64), (24, 40), (34, 70), (48, 136), (33, 1030))
KINDS = {"u8": (8, 256), "p10": (10, 1024), "words16": (10, 1400)}   # words16: a third of the words lie above 1023
ORDER = {"tff": _native.DEINT_TFF, "bff": _native.DEINT_BFF}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np_dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def _to_dev(a, dev):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _to_np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _clip(rng, n, h, w, top, dt):
    """Frames that share most of their rows, so that scores are neither zero nor saturated: a smooth ramp, noise on top,
    and every frame shifted a little against the one before."""
    base = (np.arange(h)[:, None] * 3 + np.arange(w)[None, :] * 2) % (top // 2)
    out = np.empty((n, h, w), np.int64)
    for f in range(n):
        out[f] = np.roll(base, f, axis=0) + rng.integers(0, top // 2, (h, w)) * (rng.random((h, w)) < 0.3)
    return out.astype(dt)


def _scores(dev, buf, n, plane, first, count, order, thr, bits, into=None):
    scores = torch.zeros((count, 3), dtype=torch.int32, device=dev) if into is None else into
    _native.field_match(buf, n, plane, first, count, ORDER[order], thr, scores, bits)
    return scores.cpu().numpy()


# ---- 1. the match ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", list(KINDS))
def test_match_against_the_reference(dev, kind, shape):
    bits, top = KINDS[kind]
    h, w = shape
    dt = _np_dtype(bits)
    vec = 16 // np.dtype(dt).itemsize
    rng = np.random.default_rng(h * 7 + w + bits + top % 5)
    n = 4
    clip = _clip(rng, n, h, w, top, dt)
    pitch = -(-w // vec) * vec
    padded = np.zeros((n, h, pitch), dt)
    padded[:, :, :w] = clip
    tight, pitched = _to_dev(clip.reshape(n, -1), dev), _to_dev(padded.reshape(n, -1), dev)
    for order in R.ORDERS:
        for thr in (R.default_threshold(bits), 3):
            want = R.comb_scores(clip, order, thr, bits)
            assert want.max() > 0 or h * w < 16
            got_t = _scores(dev, tight, n, (0, h, w, w, 1, h * w), 0, n, order, thr, bits)
            got_p = _scores(dev, pitched, n, (0, h, w, pitch, 1, h * pitch), 0, n, order, thr, bits)
            assert np.array_equal(got_t, want), ("tight", kind, shape, order, thr)
            assert np.array_equal(got_p, want), ("pitched", kind, shape, order, thr)


@pytest.mark.parametrize("bits", [8, 10])
def test_match_on_the_film_content(dev, bits):
    """What the scores are for: telecined film of tests/ivtc_content.py, through `fi.ivtc.field_scores`."""
    for h, w in C.SIZES:
        film = C.film(h, w, (5, 3), bits=bits)
        tc, _ = R.telecine(film, "bff", 2)
        got = I.field_scores(_to_dev(tc.reshape(len(tc), -1), dev), [(0, h, w, w, 1)], bits, "bff")
        assert np.array_equal(got.cpu().numpy(), R.comb_scores(tc, "bff", None, bits)), (h, w)


# ---- 2. layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,which", [("uyvy422", "y"), ("rgb24", 1), ("nv12", "u")])
def test_stepped_planes_where_they_lie(dev, fmt, which):
    h, w, n = 22, 70, 3
    lay = frame_layout(fmt, h, w)
    names = [p[0] for p in lay.planes]
    pl = lay.planes[names.index(which) if which in names else which]
    off, ph, pw, pitch, step = tuple(pl)[-5:]
    assert step > 1
    rng = np.random.default_rng(len(fmt))
    rows = rng.integers(0, 256, (n, lay.samples)).astype(np.uint8)
    rows[1:] = np.where(rng.random((n - 1, lay.samples)) < 0.5, rows[:-1], rows[1:])
    want = R.comb_scores(rows[:, R.plane_index(pl)], "tff", 12, 8)
    assert want.max() > 0
    got = _scores(dev, _to_dev(rows, dev), n, (off, ph, pw, pitch, step, lay.samples), 0, n, "tff", 12, 8)
    assert np.array_equal(got, want)
    assert np.array_equal(I.field_scores(_to_dev(rows, dev), pl, 8, "tff").cpu().numpy(), want)


@pytest.mark.parametrize("bits", [8, 10])
def test_an_unaligned_base_takes_the_per_sample_path(dev, bits):
    n, h, w = 3, 33, 64
    dt = _np_dtype(bits)
    clip = _clip(np.random.default_rng(bits), n, h, w, 1 << bits, dt)
    want = R.comb_scores(clip, "bff", None, bits)
    for shift in (1, 3, 5):
        buf = torch.zeros(n * h * w + 8, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
        buf[shift:shift + n * h * w] = _to_dev(clip.reshape(-1), dev)
        got = _scores(dev, buf[shift:], n, (0, h, w, w, 1, h * w), 0, n, "bff", R.default_threshold(bits), bits)
        assert np.array_equal(got, want), shift


@pytest.mark.parametrize("bits", [8, 10])
def test_every_position_of_a_five_frame_window_and_the_clamps(dev, bits):
    n, h, w = 5, 19, 37
    clip = _clip(np.random.default_rng(50 + bits), n, h, w, 1 << bits, _np_dtype(bits))
    d = _to_dev(clip.reshape(n, -1), dev)
    whole = R.comb_scores(clip, "tff", None, bits)
    assert (whole[0, 0] == whole[0, 1]) and (whole[-1, 2] == whole[-1, 1])     # the clamps: p of frame 0 and n of the last are c
    for first in range(n + 1):
        for count in range(n - first + 1):
            got = I.field_scores(d, [(0, h, w, w, 1)], bits, "tff", first=first, count=count).cpu().numpy()
            assert np.array_equal(got, whole[first:first + count]), (first, count)
            if count:   # a window of its own: one context frame either side where the clip has one
                lo, hi = max(first - 1, 0), min(first + count + 1, n)
                sub = I.field_scores(d[lo:hi].contiguous(), [(0, h, w, w, 1)], bits, "tff", first=first - lo, count=count)
                assert np.array_equal(sub.cpu().numpy(), whole[first:first + count]), (first, count, "sub-window")


def test_two_planes_accumulate_into_one_result(dev):
    n, h, w = 3, 20, 72
    rng = np.random.default_rng(9)
    a, b = _clip(rng, n, h, w, 256, np.uint8), _clip(rng, n, h, w // 2, 256, np.uint8)
    a[2] = (np.arange(h)[:, None] + np.arange(w)[None, :]).astype(np.uint8)    # a smooth last frame: there plane b scores higher
    rows = np.concatenate([a.reshape(n, -1), b.reshape(n, -1)], axis=1)
    d = _to_dev(rows, dev)
    fs = rows.shape[1]
    sa, sb = R.comb_scores(a, "tff", 12), R.comb_scores(b, "tff", 12)
    assert (sa > sb).any() and (sb > sa).any()
    acc = torch.zeros((n, 3), dtype=torch.int32, device=dev)
    _scores(dev, d, n, (0, h, w, w, 1, fs), 0, n, "tff", 12, 8, into=acc)
    got = _scores(dev, d, n, (h * w, h, w // 2, w // 2, 1, fs), 0, n, "tff", 12, 8, into=acc)
    assert np.array_equal(got, np.maximum(sa, sb))
    out = torch.full((n, 3), 2000, dtype=torch.int32, device=dev)          # larger than any score: nothing is lowered
    I.field_scores(d, (0, h, w, w, 1), 8, "tff", out=out)
    assert (out == 2000).all()


def test_a_frame_stride_that_puts_the_last_frame_beyond_2_to_the_32_bytes(dev):
    """Frames 2^31 + 64 samples apart: frame 1 starts past byte 2^31, frame 2 past 2^32.  On the vector path (offset 0) and
    on the per-sample path (offset 1); only the small planes are ever touched."""
    n, h, w, pitch, fs = 3, 33, 67, 80, (1 << 31) + 64
    need = (n - 1) * fs + h * pitch + 1
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need + LE.HEADROOM:
        pytest.skip(f"plans {need / LE.GIB:.1f} GiB + {LE.HEADROOM / LE.GIB:.0f} GiB headroom, the card has {free / LE.GIB:.1f} GiB free")
    try:
        src = torch.empty(need, dtype=torch.uint8, device=dev)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"the allocation failed: {e}")
    clip = _clip(np.random.default_rng(32), n, h, w, 256, np.uint8)
    want = R.comb_scores(clip, "tff", 12)
    assert len({tuple(r) for r in want.tolist()}) == n          # every frame scores differently: a wrong frame shows
    padded = np.zeros((n, h, pitch), np.uint8)
    padded[:, :, :w] = clip
    for off in (0, 1):
        for f in range(n):
            src[f * fs + off:f * fs + off + h * pitch] = _to_dev(padded[f].reshape(-1), dev)
        got = _scores(dev, src, n, (off, h, w, pitch, 1, fs), 0, n, "tff", 12, 8)
        assert np.array_equal(got, want), off


# ---- 3. the weave -----------------------------------------------------------------------------------------------------------
def _entries(rng, n, k):
    e = [(int(a), int(b)) for a, b in rng.integers(0, n, (k, 2))]
    e[0], e[1] = (1, 1), (n - 1, 0)          # keep == other: a copy; the two ends of the window
    return e


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("fmt", ["gray", "nv12", "uyvy422", "bgra", "i420-pitched"])
def test_weave_against_the_reference_with_65_entries(dev, fmt, bits):
    h, w, n = 22, 36, 4
    dt = _np_dtype(bits)
    rng = np.random.default_rng(len(fmt) + bits)
    if fmt == "gray":
        planes, samples = [(0, h, w, w, 1)], h * w
    elif fmt == "i420-pitched":          # three step-1 planes with 16-byte pitches: the vector path with its tail
        pitch, cp = 48, 32
        planes = [(0, h, w, pitch, 1), (h * pitch, h // 2, w // 2, cp, 1), (h * pitch + (h // 2) * cp, h // 2, w // 2, cp, 1)]
        samples = h * pitch + h * cp
    else:
        lay = frame_layout(fmt, h, w)
        planes, samples = [tuple(p)[-5:] for p in lay.planes], lay.samples
    assert 1 <= len(planes) <= 4
    rows = rng.integers(0, 65536 if bits == 10 else 256, (n, samples)).astype(dt)     # (words pass through unclamped)
    entries = _entries(rng, n, 65)
    for order in R.ORDERS:
        got = _to_np(I.weave(_to_dev(rows, dev), planes, bits, entries, order))
        assert np.array_equal(got, R.weave(rows, planes, entries, order)), order


@pytest.mark.parametrize("bits", [8, 10])
def test_weave_guard_bands_an_unaligned_base_and_an_output_directly_behind_its_input(dev, bits):
    n, h, w = 3, 9, 37
    dt = _np_dtype(bits)
    tdt = torch.uint8 if bits == 8 else torch.int16
    rng = np.random.default_rng(60 + bits)
    pa, off_a = 48, 32                               # plane a: step 1, pitch 48, from sample 32 of a frame
    off_b, pb = off_a + h * pa + 16 + 1, 2 * w + 3   # plane b: step 2, behind a gap
    fs = off_b + h * pb + 16
    fs += -fs % 16
    frame = rng.integers(0, 1 << bits, (n, fs)).astype(dt)
    planes5 = [(off_a, h, w, pa, 1), (off_b, h, w, pb, 2)]
    planes = [p + (fs,) for p in planes5]
    entries = [(0, 1), (2, 2), (1, 0), (2, 0)]
    want = R.weave(frame, planes5, entries, "bff")
    covered = np.zeros(fs, bool)
    for p in planes5:
        covered[R.plane_index(p).reshape(-1)] = True
    poison = 0xA5 if bits == 8 else 0x5AA5
    for shift in (0, 1):                             # 16-byte aligned: plane a takes the vector path; shifted: per sample
        guard = 64
        # one buffer: [shift | n source frames | the output directly behind them | guard]
        buf = torch.full((shift + n * fs + len(entries) * fs + guard,), poison, dtype=tdt, device=dev)
        buf[shift:shift + n * fs] = _to_dev(frame.reshape(-1), dev)
        src, dst = buf[shift:], buf[shift + n * fs:]
        _native.field_weave(src, n, planes, dst, planes, entries, 1, bits)
        got = _to_np(buf)
        body = got[shift + n * fs:shift + (n + len(entries)) * fs].reshape(len(entries), fs)
        assert np.array_equal(body[:, covered], want[:, covered]), shift
        assert (body[:, ~covered] == poison).all() and (got[shift + (n + len(entries)) * fs:] == poison).all()
        assert np.array_equal(got[shift:shift + n * fs].reshape(n, fs), frame) and (got[:shift] == poison).all()


def test_weave_beyond_2_to_the_32_bytes(dev):
    n, h, w, pitch, fs = 3, 9, 67, 80, (1 << 31) + 64
    need = 2 * ((n - 1) * fs + h * pitch + 1)
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need + LE.HEADROOM:
        pytest.skip(f"plans {need / LE.GIB:.1f} GiB + {LE.HEADROOM / LE.GIB:.0f} GiB headroom, the card has {free / LE.GIB:.1f} GiB free")
    try:
        src = torch.empty(need // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty(need // 2, dtype=torch.uint8, device=dev)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"the allocation failed: {e}")
    clip = np.random.default_rng(33).integers(0, 256, (n, h, pitch)).astype(np.uint8)
    entries = [(2, 1), (0, 2), (2, 2)]
    want = R.weave(clip.reshape(n, -1), [(0, h, w, pitch, 1)], entries, "tff").reshape(n, h, pitch)
    for off in (0, 1):
        for f in range(n):
            src[f * fs + off:f * fs + off + h * pitch] = _to_dev(clip[f].reshape(-1), dev)
            dst[f * fs + off:f * fs + off + h * pitch] = 0
        _native.field_weave(src, n, [(off, h, w, pitch, 1, fs)], dst, [(off, h, w, pitch, 1, fs)], entries, 0, 8)
        got = np.stack([dst[f * fs + off:f * fs + off + h * pitch].cpu().numpy().reshape(h, pitch) for f in range(n)])
        assert np.array_equal(got[:, :, :w], want[:, :, :w]) and not got[:, :, w:].any(), off


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_a_refused_call_launches_nothing(dev):
    n, h, w = 3, 6, 8
    src = torch.zeros(n * h * w, dtype=torch.uint8, device=dev)
    src[::3] = 200
    L = _native.lib()
    arr = _native.resize_plane_array
    ok = (0, h, w, w, 1, h * w)
    scores = torch.full((n, 3), -7, dtype=torch.int32, device=dev)
    for plane, first, count, order, thr in ((ok, 0, n, 2, 12), (ok, 1, n, 0, 12), (ok, 0, n, 0, 1024), ((0, 2, w, w, 1, h * w), 0, n, 0, 12),
                                            ((0, h, w, w - 1, 1, h * w), 0, n, 0, 12), ((0, h, w, w, 5, h * w), 0, n, 0, 12)):
        assert L.fiunet_field_match_u8(src.data_ptr(), n, arr([plane]), first, count, order, thr, scores.data_ptr(), None) == 1
        assert L.fiunet_last_error_string()
    # the scores inside the source's range
    assert L.fiunet_field_match_u8(src.data_ptr(), n, arr([ok]), 0, 1, 0, 12, src.data_ptr() + 16, None) == 1
    assert b"overlap" in L.fiunet_last_error_string()
    dst = torch.full((2 * h * w,), 0x5A, dtype=torch.uint8, device=dev)
    for planes, entries, parity in (([ok], [(0, 3)], 0), ([ok], [(0, 0), (3, 0)], 0), ([ok], [(0, 1)], 2),
                                    ([(0, 1, w, w, 1, h * w)], [(0, 1)], 0), ([ok] * 5, [(0, 1)], 0)):
        rc = L.fiunet_field_weave_u8(src.data_ptr(), n, arr(planes), dst.data_ptr(), arr(planes), len(planes),
                                     _native.weave_entries(entries), len(entries), parity, None)
        assert rc == 1 and L.fiunet_last_error_string(), (planes, entries, parity)
    rc = L.fiunet_field_weave_u8(src.data_ptr(), n, arr([ok]), src.data_ptr() + h * w, arr([ok]), 1, _native.weave_entries([(0, 1)]),
                                 1, 0, None)
    assert rc == 1 and b"overlap" in L.fiunet_last_error_string()
    torch.cuda.synchronize(dev)
    assert (scores == -7).all() and (dst == 0x5A).all()
    with pytest.raises(ValueError, match="reach"):
        _native.field_match(src, n + 1, ok, 0, 1, 0, 12, torch.zeros((1, 3), dtype=torch.int32, device=dev), 8)


# ---- 5. the stream contract -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", RS.ROWS, ids=lambda r: f"{r.entry}-{r.ident}")
def test_side_stream_and_captured_graph(dev, row):
    env = SC.Env(dev)
    try:
        SC.check_row(row, env)
    finally:
        env.close()
