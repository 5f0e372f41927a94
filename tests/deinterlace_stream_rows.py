"""The stream-contract rows of fiunet_deinterlace_u8 / fiunet_deinterlace_p10, for the instrument of
tests/stream_contract.py, in a file of their own so that the existing table stays as it was (the way
tests/chroma_stream_rows.py and tests/retime_motion_stream_rows.py add theirs).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_deinterlace_host.py and
tests/test_gpu_deinterlace.py import it, and pytest imports both before it runs tests/test_stream_contract_host.py (every
declared function that takes a `void* stream` is a row or excluded).  tests/test_gpu_deinterlace.py puts the rows through
the instrument itself.  Their home is the table: whoever may edit tests/stream_contract.py moves `_build` and the rows
there and deletes `register()`.

A row deinterlaces the middle three frames of a window of five at the field rate: six output frames of 18 x 32 in the
nv12 arrangement, whose luma takes the vector path and whose interleaved U and V take the per-sample path, all three in
one call.  The planes cover the frame, so every byte of the output is written by every replay (the instrument poisons it
in between)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

N_SRC, FIRST, COUNT, H, W = 5, 1, 3, 18, 32
ROW = H * W + (H // 2) * W
PLANES = [(0, H, W, W, 1, ROW), (H * W, H // 2, W // 2, W, 2, ROW), (H * W + 1, H // 2, W // 2, W, 2, ROW)]


def _build(bits):
    def build(env):
        src = SC._inp(SC._samples(env, bits, 21, N_SRC, ROW), SC._samples(env, bits, 22, N_SRC, ROW))
        out = SC._empty(env, torch.uint8 if bits == 8 else torch.int16, 2 * COUNT, ROW)

        def call(s):
            _native.deinterlace(src[0], N_SRC, PLANES, out, PLANES, FIRST, COUNT, _native.DEINT_BFF, _native.DEINT_FIELD_RATE,
                                _native.DEINT_ADAPTIVE, bits, stream=s)
            return 0
        return SC.Buffers(call, [src], [out], [])
    return build


ROWS = [SC.Row(f"fiunet_deinterlace_{'u8' if bits == 8 else 'p10'}", f"{COUNT}of{N_SRC}x{H}x{W}", None, None, None, _build(bits))
        for bits in (8, 10)]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
