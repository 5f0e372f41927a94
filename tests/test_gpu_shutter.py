"""GPU (MI355X): fiunet_shutter_u8 / fiunet_shutter_p10 (csrc/shutter.hip.h), bit for bit against the numpy
restatement of tests/shutter_ref.py (`apply_entries`: int64 accumulation, words above 1023 read as 1023, one live tap a
copy).  No tolerance anywhere.

  shapes     frame_samples 1, 15, 16, 17, 4099 and 32000 (the vector path's grid-stride loop), the grid's and the output's
             base each on and one sample off a 16-byte boundary (off: the per-sample path); taps 1, 2, 3 and 48, zero-weight
             holes at either end and inside, weights (D - 1, 1) on all-255 / all-1023 rows, 10-bit words above 1023, and 70
             output frames with 20 of 48 taps among them: more frames and more weights than one launch holds
  kernels    (2**19, 2**19) against `resample_table`'s entry (row, 1, 2); a single tap against a byte copy
  streams    once on a side stream; once warmed up, captured into a graph and replayed on other data over poisoned
             outputs (the instrument of tests/stream_contract.py on the rows of tests/shutter_stream_rows.py)
  extent     one case whose tap rows begin past bytes 2**31 and 2**32 of the grid (5 rows of 2**30 + 3 samples), against
             torch in int64 on the device, chunk by chunk

measured on an MI355X: the whole file (20 cases) 3.0 s; the far rows 0.6 s at a peak of 12.1 GiB, every other case under 0.2 s
"""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_extent as L  # noqa: E402
import shutter_ref as SR  # noqa: E402
import shutter_stream_rows as RS  # noqa: E402
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402
from ai_based_frame_interpolation_amd import retime as RT  # noqa: E402

pytestmark = pytest.mark.gpu
D = 1 << 20
ROWS = 50
SIZES = [1, 15, 16, 17, 4099, 32000]
W48 = [21845] * 47 + [D - 47 * 21845]
#: (first row, weights) on a grid of 50 rows whose rows 0 to 2 are all 255 / all 1023
ENTRIES = ([(0, [D - 1, 1]), (1, [1, D - 1]), (5, [D]), (49, [D]), (3, [D // 2, D // 2]), (48, [D - 7, 7]),
            (7, [D // 4, D // 2, D // 4]), (2, W48), (0, W48[::-1]), (9, [0, D // 2, 0, 0, D // 2, 0]), (11, [0, D, 0]),
            (20, [0, 0, 0, 0, 1, D - 1]), (30, [D // 8] * 8), (31, [3] * 5 + [D - 15]), (12, [D - 1, 0, 0, 0, 1])]
           + [(k % 3, W48) for k in range(20)] + [(k, [D // 4, D // 4, D // 2]) for k in range(35)])


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _grid(bits, fs, seed=1):
    rng = np.random.default_rng(seed)
    if bits == 8:
        g = rng.integers(0, 256, (ROWS, fs)).astype(np.uint8)
        g[:3] = 255
    else:   # 10-bit codes, every fourth word anything up to 65535, rows 0 to 2 all 1023
        g = rng.integers(0, 1024, (ROWS, fs)).astype(np.uint16)
        wild = rng.integers(0, 4, (ROWS, fs)) == 0
        g[wild] = rng.integers(1024, 65536, int(wild.sum())).astype(np.uint16)
        g[:3] = 1023
    return g


def _dev_rows(a, dev, off):
    """The rows of numpy array `a` on the device as a contiguous tensor whose base lies `off` samples past an allocation's
    start (0: 16-byte aligned; 1: not)."""
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    buf = torch.zeros(a.size + off, dtype=t.dtype, device=dev)
    view = buf[off:].view(a.shape)
    view.copy_(t)
    assert view.is_contiguous() and (view.data_ptr() % 16 == 0) == (off == 0)
    return view


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("fs", SIZES)
def test_kernel_equals_the_restatement(dev, bits, fs):
    """0.2 s for the twelve cases together."""
    g = _grid(bits, fs)
    want = SR.apply_entries(g, ENTRIES, bits)
    assert want.shape == (len(ENTRIES), fs)
    if fs > 1:
        assert (want[0] == (255 if bits == 8 else 1023)).all() and (want[1] == want[0]).all()
    for goff, ooff in ((0, 0), (1, 0), (0, 1), (1, 1)):
        grid = _dev_rows(g, dev, goff)
        out = _dev_rows(np.full_like(want, 0x55), dev, ooff)
        got = RT.resample_shutter(grid, ENTRIES, bits, out=out)
        assert got.data_ptr() == out.data_ptr()
        bad = np.argwhere(_np(got) != want)
        assert bad.size == 0, (bits, fs, goff, ooff, "first difference at (frame, sample)", bad[0].tolist(),
                               ENTRIES[bad[0][0]][0], len(ENTRIES[bad[0][0]][1]))
    # allocated by the call
    assert np.array_equal(_np(RT.resample_shutter(_dev_rows(g, dev, 0), ENTRIES[:3], bits)), want[:3])
    assert RT.resample_shutter(_dev_rows(g, dev, 0), [], bits).shape == (0, fs)


@pytest.mark.parametrize("bits", [8, 10])
def test_against_the_table_kernel_and_a_copy(dev, bits):
    fs = 4099
    g = _grid(bits, fs, seed=2)
    grid = _dev_rows(g, dev, 0)
    rows = [2, 7, 30, 48]
    halves = RT.resample_shutter(grid, [(r, [D // 2, D // 2]) for r in rows], bits)
    table = RT.resample_table(grid, [(r, 1, 2) for r in rows], bits)
    assert torch.equal(halves, table)
    # a single tap, with or without holes beside it: the bytes of the row, words above 1023 as they are
    one = RT.resample_shutter(grid, [(r, [D]) for r in rows] + [(r - 1, [0, D, 0]) for r in rows], bits)
    assert torch.equal(one[:4], grid[rows]) and torch.equal(one[4:], grid[rows])
    if bits == 10:
        assert (g[rows] > 1023).any()


@pytest.mark.parametrize("bits", [8, 10])
def test_on_a_side_stream(dev, bits):
    fs = 4112
    g = _grid(bits, fs, seed=3)
    want = SR.apply_entries(g, ENTRIES, bits)
    grid = _dev_rows(g, dev, 0)
    out = torch.zeros((len(ENTRIES), fs), dtype=grid.dtype, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        _native.shutter(grid, ENTRIES, out, bits, stream=side.cuda_stream)
    side.synchronize()
    assert np.array_equal(_np(out), want)


@pytest.mark.parametrize("row", RS.ROWS, ids=[r.entry for r in RS.ROWS])
def test_captured_replay_equals_the_eager_call(dev, row):
    env = SC.Env(dev)
    try:
        SC.check_row(row, env)
    finally:
        env.close()


def test_refusals_reach_python(dev):
    grid = torch.zeros((4, 16), dtype=torch.uint8, device=dev)
    for bad, text in (((0, [D - 1]), "sum"), ((3, [D // 2, D // 2]), "outside the grid"), ((0, [1] * 48 + [D - 48]), "n_taps")):
        with pytest.raises(_native.NativeError, match=text):
            RT.resample_shutter(grid, [(0, [D]), bad], 8)
    with pytest.raises(ValueError, match="8 or 10"):
        RT.resample_shutter(grid, [(0, [D])], 12)
    with pytest.raises(ValueError, match="10-bit grid"):
        RT.resample_shutter(grid, [(0, [D])], 10)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RT.resample_shutter(grid.cpu(), [(0, [D])], 8)
    with pytest.raises(ValueError, match="out must be"):
        RT.resample_shutter(grid, [(0, [D])], 8, out=torch.zeros((2, 16), dtype=torch.uint8, device=dev))


def test_tap_rows_past_2_32_bytes_of_the_grid(dev):
    """5 rows of 2**30 + 3 samples: rows 2 .. 4 begin past byte 2**31, row 4 past 2**32.  One frame of three taps over rows
    2 .. 4, one copy of row 4, one two-tap frame over rows 3 and 4; against torch in int64, 2**27 samples at a time.
    12.1 GiB at the peak (the stack, the three frames, the int64 pieces of the comparison)."""
    from test_gpu_large_extent import Case
    n, chunk = (1 << 30) + 3, 1 << 27
    entries = [(2, [D // 4, D // 4 + 1, D // 2 - 1]), (4, [D]), (3, [D - 3, 3])]
    nothing = types.SimpleNamespace(_ws=None, precision="fp32", set_options=lambda: None)   # (Case releases a model's workspace)
    with Case("shutter over rows of 2^30 + 3 samples", 14 * L.GIB, nothing):
        g = torch.Generator(device=dev).manual_seed(61)
        stack = torch.randint(0, 256, (5, n), dtype=torch.uint8, device=dev, generator=g)
        assert 4 * n > 1 << 32
        got = RT.resample_shutter(stack, entries, 8)
        for k, (row, w) in enumerate(entries):
            for c in range(0, n, chunk):
                if len(w) == 1:
                    want = stack[row, c:c + chunk]
                else:
                    acc = sum(stack[row + t, c:c + chunk].to(torch.int64) * v for t, v in enumerate(w))
                    want = ((acc + D // 2) >> 20).to(torch.uint8)
                assert torch.equal(got[k, c:c + chunk], want), (k, c)
        del got, stack
