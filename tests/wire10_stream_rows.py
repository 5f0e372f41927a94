"""The stream-contract rows of fiunet_unpack_422p10 / fiunet_pack_422p10, for the instrument of
tests/stream_contract.py, in a file of their own so that the existing table stays as it was (the way
tests/resize_stream_rows.py and tests/dedup_stream_rows.py add theirs).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_wire10_host.py and
tests/test_gpu_wire10.py import it, and pytest imports both before it runs tests/test_stream_contract_host.py (every
declared function that takes a `void* stream` is a row or excluded).  tests/test_gpu_wire10.py puts the rows through the
instrument itself.  Their home is the table: whoever may edit tests/stream_contract.py moves `_build` and the rows there
and deletes `register()`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402
import wire10_ref as R  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

SHAPES = {"vector": (2, 3, 48), "scalar": (2, 3, 50)}    # W % 8 == 0 and tight aligned frames; a partial last group


def _words(env, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)


def _build(direction, packing, b, h, w):
    code, n = R.CODES[packing], R.planar_samples(h, w)

    def build(env):
        lib = _native.lib()
        planar = [np.random.default_rng(s).integers(0, 1024, (b, n)).astype(np.uint16) for s in (1, 2)]
        if direction == "unpack":
            inp = SC._inp(*[_words(env, R.pack(p, h, w, packing)) for p in planar])
            out = SC._empty(env, torch.int16, b, n)
            return SC.Buffers(lambda s: lib.fiunet_unpack_422p10(inp[0].data_ptr(), code, None, None, out.data_ptr(), 0, b,
                                                                 h, w, s), [inp], [out], [])
        inp = SC._inp(*[_words(env, p) for p in planar])
        out = SC._empty(env, torch.int16, b, R.frame_bytes(packing, h, w) // 2)
        return SC.Buffers(lambda s: lib.fiunet_pack_422p10(inp[0].data_ptr(), 0, out.data_ptr(), code, None, None, b, h, w,
                                                           s), [inp], [out], [])
    return build


ROWS = [SC.Row(f"fiunet_{d}_422p10", f"{p}-{path}-{b}x{h}x{w}", None, None, None, _build(d, p, b, h, w))
        for d in ("unpack", "pack") for p in R.PACKINGS for path, (b, h, w) in SHAPES.items()]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
