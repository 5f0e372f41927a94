"""The stream-contract rows of fiunet_warp_table_u8 / fiunet_warp_table_p10, for the instrument of
tests/stream_contract.py, in a file of their own so that the existing table stays as it was (the way
tests/wire10_stream_rows.py, tests/resize_stream_rows.py and tests/dedup_stream_rows.py add theirs).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_retime_motion_host.py and
tests/test_gpu_retime_motion.py import it, and pytest imports both before it runs tests/test_stream_contract_host.py
(every declared function that takes a `void* stream` is a row or excluded).  tests/test_gpu_retime_motion.py puts the
rows through the instrument itself.  Their home is the table: whoever may edit tests/stream_contract.py moves `_build`
and the rows there and deletes `register()`.

A row warps the one plane of 70 tight frames (two launches of 64 entries at most) from a grid of four rows along three
flow fields that the entries share; no entry carries a flag and the plane covers the frame, so every byte of the output
is written by every replay (the instrument poisons it in between)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

H, W, ROWS_IN, N_OUT = 33, 47, 4, 70
ENTRIES = [(k % 3, 1 + k % 15, 16, k % 3, -1) for k in range(N_OUT)]


def _build(bits):
    def build(env):
        grid = SC._inp(SC._samples(env, bits, 1, ROWS_IN, H * W), SC._samples(env, bits, 2, ROWS_IN, H * W))
        flow = SC._inp(SC._f32(env, 3, 3, H, W, 2, lo=-4.0, hi=4.0), SC._f32(env, 4, 3, H, W, 2, lo=-4.0, hi=4.0))
        out = SC._empty(env, torch.uint8 if bits == 8 else torch.int16, N_OUT, H * W)
        plane = (0, H, W, W, 1, H * W)
        return SC.Buffers(lambda s: (_native.warp_table(grid[0], ROWS_IN, plane, flow[0], None, ENTRIES, out, plane, bits,
                                                        stream=s), 0)[1], [grid, flow], [out], [])
    return build


ROWS = [SC.Row(f"fiunet_warp_table_{'u8' if bits == 8 else 'p10'}", f"{N_OUT}x{H}x{W}", None, None, None, _build(bits))
        for bits in (8, 10)]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
