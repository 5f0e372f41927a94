"""The stream-contract rows of the four entry points of inverse telecine, for the instrument of
tests/stream_contract.py, in a file of their own so that the existing table stays as it was (the way
tests/deinterlace_stream_rows.py and tests/dedup_stream_rows.py add theirs).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_ivtc_host.py and
tests/test_gpu_ivtc.py import it, and pytest imports both before it runs tests/test_stream_contract_host.py (every
declared function that takes a `void* stream` is a row or excluded).  tests/test_gpu_ivtc.py puts the rows through the
instrument itself.  Their home is the table: whoever may edit tests/stream_contract.py moves the builders and the rows
there and deletes `register()`.

The match rows score the middle three frames of a window of five in the nv12 arrangement of 18 x 32: the luma (the vector
path) and, into the same scores, the interleaved U (the per-sample path).  The call MAX-ACCUMULATES, so the scores are an
input and the output at once, and they start from values among the scores of these frames so that some win and some
lose.  The weave rows write six frames of all three planes from host entries that are overwritten right after the call."""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

N_SRC, FIRST, COUNT, H, W = 5, 1, 3, 18, 32
ROW = H * W + (H // 2) * W
PLANES = [(0, H, W, W, 1, ROW), (H * W, H // 2, W // 2, W, 2, ROW), (H * W + 1, H // 2, W // 2, W, 2, ROW)]
ENTRIES = [(0, 0), (1, 0), (2, 3), (4, 4), (3, 2), (0, 4)]


def _match(bits):
    def build(env):
        src = SC._inp(SC._samples(env, bits, 31, N_SRC, ROW, top=1100), SC._samples(env, bits, 32, N_SRC, ROW, top=1100))
        base = [torch.from_numpy(np.random.default_rng(k).integers(0, 200, (COUNT, 3)).astype(np.int32)).to(env.dev)
                for k in (33, 34)]
        scores = SC._inp(*base)

        def call(s):
            for plane in PLANES[:2]:
                _native.field_match(src[0], N_SRC, plane, FIRST, COUNT, _native.DEINT_BFF, 12 if bits == 8 else 48, scores[0],
                                    bits, stream=s)
            return 0
        return SC.Buffers(call, [src, scores], [scores[0]], [])
    return build


def _weave(bits):
    def build(env):
        src = SC._inp(SC._samples(env, bits, 35, N_SRC, ROW, top=65536), SC._samples(env, bits, 36, N_SRC, ROW, top=65536))
        out = SC._empty(env, torch.uint8 if bits == 8 else torch.int16, len(ENTRIES), ROW)
        L = _native.lib()
        fn = L.fiunet_field_weave_p10 if bits == 10 else L.fiunet_field_weave_u8

        def call(s):   # the entries are host memory that lives for the call alone: they travel in the kernel's arguments
            arr = _native.weave_entries(ENTRIES)
            planes = _native.resize_plane_array(PLANES)
            rc = fn(SC._p(src[0]), N_SRC, planes, SC._p(out), planes, len(PLANES), arr, len(ENTRIES), 1, s)
            ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))
            return rc
        return SC.Buffers(call, [src], [out], [])
    return build


ROWS = [SC.Row("fiunet_field_match_u8", f"{COUNT}of{N_SRC}x{H}x{W}-accumulating", None, None, None, _match(8)),
        SC.Row("fiunet_field_match_p10", f"{COUNT}of{N_SRC}x{H}x{W}-accumulating", None, None, None, _match(10)),
        SC.Row("fiunet_field_weave_u8", f"{len(ENTRIES)}-entries-from-host-memory", None, None, None, _weave(8)),
        SC.Row("fiunet_field_weave_p10", f"{len(ENTRIES)}-entries-from-host-memory", None, None, None, _weave(10))]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
