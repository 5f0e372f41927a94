"""The stream-contract rows of the two entry points of the synthesized shutter, for the instrument of
tests/stream_contract.py: fiunet_shutter_u8 / fiunet_shutter_p10 (as tests/dedup_stream_rows.py, tests/ivtc_stream_rows.py
and the other *_stream_rows.py files add theirs).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_shutter_host.py and
tests/test_gpu_shutter.py import it, and pytest imports both before tests/test_stream_contract_host.py and
tests/test_gpu_stream_contract.py run.  Run ALONE those two files do not see these rows; tests/test_gpu_shutter.py puts them
through the instrument itself.  The rows' home is the table: whoever may edit tests/stream_contract.py moves `_shutter` and
the rows there and deletes `register()`."""
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

D = 1 << 20
#: a copy, two taps, a hole, 48 taps, and enough frames (40) for a second launch; a grid of 50 rows
ENTRIES = [(0, [D]), (3, [D // 2, D // 2]), (1, [D - 1, 0, 1]), (2, [21845] * 47 + [D - 47 * 21845]),
           (7, [0, D, 0])] + [(k, [D // 4, D // 4, D // 2]) for k in range(35)]


def _shutter(entry, bits_):
    fs, rows = 1003, 50

    def build(env):
        L = _native.lib()
        grid = SC._inp(SC._samples(env, bits_, 1, rows, fs, top=1100), SC._samples(env, bits_, 2, rows, fs, top=1100))
        out = SC._empty(env, grid[0].dtype, len(ENTRIES), fs)

        def call(s):   # the entries are host memory that lives for the call alone: they travel in the kernel's arguments
            arr = _native.shutter_entries(ENTRIES)
            rc = getattr(L, entry)(SC._p(grid[0]), rows, fs, arr, len(ENTRIES), SC._p(out), s)
            ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))
            return rc
        return SC.Buffers(call, [grid], [out], [])
    return SC.Row(entry, f"{len(ENTRIES)}-entries-from-host-memory", None, None, None, build)


ROWS = [_shutter("fiunet_shutter_u8", 8), _shutter("fiunet_shutter_p10", 10)]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
