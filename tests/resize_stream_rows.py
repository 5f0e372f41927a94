"""The stream-contract rows of fiunet_resize_planes_u8 / _p10, for the instrument of
tests/stream_contract.py, in a file of their own so that the existing table stays as it was (the way
tests/dedup_stream_rows.py adds its four).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_resize_host.py and
tests/test_gpu_resize_contract.py import it, and pytest imports both before tests/test_stream_contract_host.py (every
declared function that takes a `void* stream` is a row or excluded) and tests/test_gpu_stream_contract.py (every row
through the instrument).  Run alone, those two files do not see these rows and the first fails on the two new names;
tests/test_gpu_resize_contract.py puts the rows through the instrument itself.  Their home is the table: whoever may edit
tests/stream_contract.py moves `_build` and the two rows there and deletes `register()`."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as C  # noqa: E402
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402


def _up(a, dev):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _build(bits, size, sstep, dstep, n_planes):
    def build(env):
        lib = _native.lib()
        a, sp, dst, dp, n = C.case(1, bits, size, sstep, dstep, n_planes)
        b = C.case(2, bits, size, sstep, dstep, n_planes)[0]
        inp = SC._inp(_up(a, env.dev), _up(b, env.dev))
        out = _up(dst, env.dev)
        fn = lib.fiunet_resize_planes_p10 if bits == 10 else lib.fiunet_resize_planes_u8
        s_arr, d_arr = _native.resize_plane_array(sp), _native.resize_plane_array(dp)   # (host memory, read during the call)
        # the outputs are the destination planes as they lie in the buffer; the buffer itself is scratch (what lies
        # between the planes keeps each run's poison, which differs from run to run)
        views = [out.as_strided((n, h, w), (fs, pitch, step), off) for off, h, w, pitch, step, fs in dp]
        return SC.Buffers(lambda s: fn(inp[0].data_ptr(), s_arr, out.data_ptr(), d_arr, len(sp), n, s), [inp], views, [out])
    return build


ROWS = [SC.Row("fiunet_resize_planes_u8", "37x53-18x26-nv12-like", None, None, None, _build(8, (37, 53, 18, 26), 2, 1, 2)),
        SC.Row("fiunet_resize_planes_p10", "18x26-37x53-four-planes", None, None, None, _build(10, (18, 26, 37, 53), 1, 4, 4))]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
