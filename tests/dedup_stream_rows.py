"""The stream-contract rows of the four entry points of the re-timing of repeated frames, for the
instrument of tests/stream_contract.py: fiunet_pair_peak_u8 / _p10 and fiunet_retime_table_u8 / _p10.

They are rows like that module's own (`_pair_sad`, `_retime`).  They stand in a file of their own so that the existing table stays as it
was when this feature was added.
IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`), so that
tests/test_stream_contract_host.py (every declared function that takes a `void* stream` is a row or excluded) and
tests/test_gpu_stream_contract.py (every row through the instrument) see them whenever the suite is collected:
tests/test_dedup_host.py and tests/test_gpu_dedup_stream.py import it, and pytest imports both before those two files.

What this cannot do: run ALONE, tests/test_stream_contract_host.py and tests/test_gpu_stream_contract.py import nothing
that knows of this module, do not see these rows, and the first of them fails on the four new names.
tests/test_gpu_dedup_stream.py puts the rows through the instrument itself, so the GPU check does not depend on what
else is collected.  The rows' home is the table: whoever may edit tests/stream_contract.py moves the two functions and
the four rows there and deletes `register()`; nothing else changes (`register()` skips names that are rows already)."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402


def _pair_peak(entry, bits_):
    n, fs = 5, 1003

    def build(env):
        L = _native.lib()
        frames = SC._inp(SC._samples(env, bits_, 1, n, fs, top=1100), SC._samples(env, bits_, 2, n, fs, top=1100))
        # the call MAX-ACCUMULATES (the header has the caller zero the peaks): in place, so an input and the output; the
        # values it starts from lie among the peaks of these frames, so that some win and some lose
        base = [torch.from_numpy(np.random.default_rng(k).integers(0, 64 * (450 if bits_ == 10 else 120), n - 1)
                                 .astype(np.int32)).to(env.dev) for k in (3, 4)]
        peaks = SC._inp(*base)
        return SC.Buffers(lambda s: getattr(L, entry)(SC._p(frames[0]), n, fs, SC._p(peaks[0]), s), [frames, peaks],
                          [peaks[0]], [])
    return SC.Row(entry, f"{n}x{fs}-accumulating", None, None, None, build)


def _retime_table(entry, bits_):
    fs, rows = 1003, 5
    entries = [(0, 0, 1), (3, 2, 5), (1, 4, 5), (4, 0, 1), (2, (1 << 20) - 1, 1 << 20), (3, 1, 3)]

    def build(env):
        L = _native.lib()
        grid = SC._inp(SC._samples(env, bits_, 1, rows, fs, top=1100), SC._samples(env, bits_, 2, rows, fs, top=1100))
        out = SC._empty(env, grid[0].dtype, len(entries), fs)

        def call(s):   # the entries are host memory that lives for the call alone: they travel in the kernel's arguments
            arr = _native.retime_entries(entries)
            rc = getattr(L, entry)(SC._p(grid[0]), rows, fs, arr, len(entries), SC._p(out), s)
            ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))
            return rc
        return SC.Buffers(call, [grid], [out], [])
    return SC.Row(entry, f"{len(entries)}-entries-from-host-memory", None, None, None, build)


ROWS = [_pair_peak("fiunet_pair_peak_u8", 8), _pair_peak("fiunet_pair_peak_p10", 10),
        _retime_table("fiunet_retime_table_u8", 8), _retime_table("fiunet_retime_table_p10", 10)]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
