"""GPU (MI355X): the two kernels of the re-timing of repeated frames (csrc/scene.hip.h pair_peak_kernel, csrc/retime.hip.h
retime_table_kernel).  Every comparison is exact.

  1. scene.pair_peak bit for bit against numpy (tests/dedup_ref.py): sizes around the 64-sample segment, 8 and 10 bits
     with words above 1023, the short last segment, a maximum and not a sum, the per-sample path of an unaligned base,
     accumulation over stacks, no frames
  2. retime.resample_table against Python integers: sizes around the 16-byte vector, the divisors 1, 3, 7 * 2**17 and
     2**20, copies, the first and the last grid row, 64 / 65 / 129 output frames (one, two and three launches); against
     fiunet_retime_* byte for byte on entries built from a plan; the refusals leave the output untouched
"""
import ctypes
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as D  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
RT = P.retime


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _stack(rng, rows, fs, bits):
    if bits == 8:
        return rng.integers(0, 256, (rows, fs), dtype=np.uint8)
    a = rng.integers(0, 1024, (rows, fs)).astype(np.uint16)
    over = rng.random((rows, fs)) < 0.1            # some words above 1023, the top bit among them
    a[over] = rng.choice(np.array([1024, 2000, 32768, 65535], np.uint16), int(over.sum()))
    return a.view(np.int16)


def _on_device(dev, a, offset=0):
    """`a` on the device in a buffer whose base is `offset` samples past an allocation's (16-byte aligned) start."""
    flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
    t = flat[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == (offset * a.itemsize) % 16
    return t


def _np(t):
    return t.cpu().numpy()


# ---- 1. pair_peak ------------------------------------------------------------------------------------------------------
SIZES = [1, 63, 64, 65, 4099]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("bits", [8, 10])
def test_pair_peak_matches_numpy(dev, bits, n, offset):
    """An odd n misaligns every second pair, so n = 63, 65 and 4099 take both paths in one call; offset 1 moves the
    base itself off the 16-byte boundary."""
    a = _stack(np.random.default_rng(bits * 10000 + n), 4, n, bits)
    got = P.scene.pair_peak(_on_device(dev, a, offset), bits)
    assert got.dtype == torch.int32 and got.shape == (3,)
    assert np.array_equal(_np(got), D.pair_peak(a, bits))


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("bits", [8, 10])
def test_pair_peak_segments(dev, bits, offset):
    dt = np.uint8 if bits == 8 else np.int16
    n = 4099
    f = np.zeros((2, n), dt)
    f[1, n - 1] = 9                                  # a lone differing sample in the short last segment
    assert _np(P.scene.pair_peak(_on_device(dev, f, offset), bits)).tolist() == [9]
    f = np.zeros((2, n), dt)
    f[1, 64 * 7 - 1], f[1, 64 * 7] = 100, 60         # either side of a segment edge: the maximum, not the sum
    assert _np(P.scene.pair_peak(_on_device(dev, f, offset), bits)).tolist() == [100]
    f[1, 64 * 7 + 63] = 50                           # the same segment as the 60
    assert _np(P.scene.pair_peak(_on_device(dev, f, offset), bits)).tolist() == [110]
    f = np.full((2, n), 3, dt)
    f[1] = 5                                         # every sample differs by 2: a full segment's sum
    assert _np(P.scene.pair_peak(_on_device(dev, f, offset), bits)).tolist() == [128]
    if bits == 10:                                   # words above 1023 read as 1023: equal after the clamp
        f = np.zeros((2, n), np.uint16)
        f[0], f[1] = 1023, 40000
        assert _np(P.scene.pair_peak(_on_device(dev, f.view(np.int16), offset), 10)).tolist() == [0]
        f[0] = 0
        assert _np(P.scene.pair_peak(_on_device(dev, f.view(np.int16), offset), 10)).tolist() == [64 * 1023]


@pytest.mark.parametrize("bits", [8, 10])
def test_pair_peak_accumulates_over_stacks_and_takes_no_frames(dev, bits):
    rng = np.random.default_rng(bits)
    planes = [_stack(rng, 5, n, bits) for n in (4099, 130)]
    got = _np(P.scene.pair_peak([_on_device(dev, p) for p in planes], bits))
    want = D.pair_peak(planes, bits)
    assert np.array_equal(got, want) and np.array_equal(got, np.maximum(*(D.pair_peak(p, bits) for p in planes)))
    # the C call MAX-accumulates into what it is given
    peaks = torch.full((4,), 1 << 20, dtype=torch.int32, device=dev)
    _native.pair_peak(_on_device(dev, planes[0]), peaks, bits)
    assert _np(peaks).tolist() == [1 << 20] * 4
    # n_frames < 2: nothing is written
    for k in (0, 1):
        assert P.scene.pair_peak(_on_device(dev, planes[0][:k]), bits).shape == (0,)
    one = _on_device(dev, planes[0][:1])
    guard = torch.full((2,), 7, dtype=torch.int32, device=dev)
    _native.pair_peak(one, guard, bits)
    assert _np(guard).tolist() == [7, 7]


# ---- 2. retime_table --------------------------------------------------------------------------------------------------
def _read(a, bits):
    a = a.view(np.uint16) if a.dtype == np.int16 else a
    return np.minimum(a.astype(np.int64), 1023) if bits == 10 else a.astype(np.int64)


def _want(grid, entries, bits):
    out = []
    for row, wn, den in entries:
        if wn == 0:
            out.append(grid[row].copy())
        else:
            v = (_read(grid[row], bits) * (den - wn) + _read(grid[row + 1], bits) * wn + den // 2) // den
            out.append(v.astype(np.uint16).view(np.int16) if bits == 10 else v.astype(np.uint8))
    return np.stack(out)


DENS = [1, 3, 7 << 17, 1 << 20]
ROWS = 6


def _entries(rng, n_out):
    """Copies of the first and the last row, every divisor at its smallest, largest and a middle weight, the last pair
    of rows among them; then random ones."""
    e = [(0, 0, 1), (ROWS - 1, 0, 1), (ROWS - 1, 0, 1 << 20), (0, 0, 3)]
    for den in DENS[1:]:
        e += [(0, 1, den), (ROWS - 2, den - 1, den), (2, den // 2, den), (ROWS - 2, den // 2 + 1, den)]
    while len(e) < n_out:
        den = DENS[int(rng.integers(0, 4))]
        wn = int(rng.integers(0, den))
        e.append((int(rng.integers(0, ROWS - (1 if wn else 0))), wn, den))
    return e[:n_out]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
@pytest.mark.parametrize("bits", [8, 10])
def test_table_matches_python_integers(dev, bits, n, offset):
    rng = np.random.default_rng(bits * 100000 + n)
    grid = _stack(rng, ROWS, n, bits)
    d = _on_device(dev, grid, offset)
    for n_out in (64, 65, 129):                      # one launch, two, three
        entries = _entries(rng, n_out)
        assert {den for _, _, den in entries} >= set(DENS)
        out = _on_device(dev, np.zeros((n_out, n), grid.dtype), offset)
        got = RT.resample_table(d, entries, bits, out=out)
        assert got is out
        want = _want(grid, entries, bits)
        got = _np(got)
        for k in range(n_out):
            assert np.array_equal(got[k], want[k]), (k, entries[k])
    assert RT.resample_table(d, [], bits).shape == (0, n)


@pytest.mark.parametrize("bits", [8, 10])
def test_table_from_a_plan_equals_the_plan_kernel(dev, bits):
    """Entries built from a plan without spans: byte for byte what fiunet_retime_* writes, in both modes, with flags."""
    rng = np.random.default_rng(bits)
    for p, q, depth in ((2, 5, 2), (1001, 2500, 3), (1, 4, 2), ((1 << 20) - 1, 1 << 20, 1)):
        pl = RT.plan(Fraction(p), Fraction(q), depth)
        for first, n_int, last in ((0, 3, False), (7, 3, True)):
            grid = _stack(rng, n_int * pl.G + 1, 4099, bits)
            d = _on_device(dev, grid)
            j0, n_out = pl.span(first, n_int, last)
            for flags in (None, np.array([0, 1, 0], np.uint8), np.ones(3, np.uint8)):
                dflags = None if flags is None else torch.from_numpy(flags).to(dev)
                for mode in RT.MODES:
                    want = RT.resample(d, pl, first, j0, n_out, bits=bits, flags=dflags, mode=mode)
                    entries = RT.table_entries(pl, [], first, j0, n_out, n_int, mode, flags)
                    got = RT.resample_table(d, entries, bits)
                    assert torch.equal(got, want), (p, q, first, mode)


@pytest.mark.parametrize("bits", [8, 10])
def test_table_refusals_leave_the_output_untouched(dev, bits):
    lib = _native.lib()
    fn = lib.fiunet_retime_table_p10 if bits == 10 else lib.fiunet_retime_table_u8
    grid = _on_device(dev, _stack(np.random.default_rng(3), 5, 64, bits))
    ok = [(0, 0, 1), (3, 1, 2), (4, 0, 7)]
    s = torch.cuda.current_stream(dev).cuda_stream
    for bad in ((5, 0, 1),                            # row >= n_rows
                (0, 2, 2), (0, 5, 3),                 # wn >= den
                (4, 1, 2),                            # wn > 0 with row + 1 >= n_rows
                (0, 0, 0), (0, 0, (1 << 20) + 1)):    # den outside 1 .. 2**20
        for entries in ([bad] + ok, ok + [bad], ok * 30 + [bad]):     # (the last: in the second launch's share)
            out = torch.full((len(entries), 64), 77, dtype=grid.dtype, device=dev)
            arr = _native.retime_entries(entries)
            assert fn(grid.data_ptr(), 5, 64, arr, len(entries), out.data_ptr(), s) == 1, bad
            torch.cuda.synchronize(dev)
            assert bool((out == 77).all()), bad
        with pytest.raises(_native.NativeError):
            RT.resample_table(grid, ok + [bad], bits)
    out = torch.full((3, 64), 77, dtype=grid.dtype, device=dev)
    assert fn(grid.data_ptr(), 5, 64, None, 3, out.data_ptr(), s) == 1
    assert fn(None, 5, 64, _native.retime_entries(ok), 3, out.data_ptr(), s) == 1
    assert fn(grid.data_ptr(), 5, 64, _native.retime_entries(ok), 3, None, s) == 1
    torch.cuda.synchronize(dev)
    assert bool((out == 77).all())
    assert ctypes.sizeof(_native.RetimeEntry) == 12
