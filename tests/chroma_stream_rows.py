"""The stream-contract rows of fiunet_chroma_pick_* and fiunet_chroma_fill_* (DESIGN.md 3.3u), for the instrument of
tests/stream_contract.py, in a file of their own so that the existing table stays as it was (the way
tests/retime_motion_stream_rows.py adds its rows).

IMPORTING THIS MODULE APPENDS THEM TO `stream_contract.ROWS`, once (`register()`): tests/test_chroma_host.py and
tests/test_gpu_chroma.py import it, and pytest imports both before it runs tests/test_stream_contract_host.py (every
declared function that takes a `void* stream` is a row or excluded).  tests/test_gpu_chroma.py puts the rows through the
instrument itself.  Their home is the table: whoever may edit tests/stream_contract.py moves the rows there and deletes
`register()`.

A pick row makes the map of 3 frames of 37 x 51 luma (partial last blocks) from A, B and M at three offsets of one
buffer; a fill row makes both 19 x 26 chroma planes of 3 frames under that luma.  The planes cover the outputs, so every
byte is written by every replay (the instrument poisons them in between).  The pick map of a fill row is an input: random
bits, so that both branches run."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

N, H, W, HC, WC = 3, 37, 51, 19, 26
PH, PW = 5, 7


def _pick(bits):
    def build(env):
        luma = SC._inp(SC._samples(env, bits, 1, 3 * N, H * W), SC._samples(env, bits, 2, 3 * N, H * W))
        flow = SC._inp(SC._f32(env, 3, N, H, W, 2, lo=-6.0, hi=6.0), SC._f32(env, 4, N, H, W, 2, lo=-6.0, hi=6.0))
        out = SC._empty(env, torch.uint8, N, PH, PW)
        buf = luma[0]
        planes = [(k * H * W, H, W, W, 1, 3 * H * W) for k in range(3)]   # frame f: A, B, M side by side

        def call(s):
            _native.chroma_pick(buf, planes[0], buf, planes[1], buf, planes[2], flow[0], out, bits, stream=s)
            return 0
        return SC.Buffers(call, [luma, flow], [out], [])
    return build


def _fill(bits):
    def build(env):
        ca = SC._inp(SC._samples(env, bits, 5, N, 2 * HC * WC), SC._samples(env, bits, 6, N, 2 * HC * WC))
        cb = SC._inp(SC._samples(env, bits, 7, N, 2 * HC * WC), SC._samples(env, bits, 8, N, 2 * HC * WC))
        flow = SC._inp(SC._f32(env, 9, N, H, W, 2, lo=-6.0, hi=6.0), SC._f32(env, 10, N, H, W, 2, lo=-6.0, hi=6.0))
        pick = SC._inp(SC._u8(env, 11, N, PH, PW) & 1, SC._u8(env, 12, N, PH, PW) & 1)
        out = SC._empty(env, torch.uint8 if bits == 8 else torch.int16, N, 2 * HC * WC)
        planes = [(p * HC * WC, HC, WC, WC, 1, 2 * HC * WC) for p in range(2)]

        def call(s):
            _native.chroma_fill(ca[0], planes, cb[0], planes, flow[0], pick[0], (2, 2), out, planes, bits, stream=s)
            return 0
        return SC.Buffers(call, [ca, cb, flow, pick], [out], [])
    return build


ROWS = [SC.Row(f"fiunet_chroma_{kind}_{'u8' if bits == 8 else 'p10'}", f"{N}x{H}x{W}", None, None, None, make(bits))
        for kind, make in (("pick", _pick), ("fill", _fill)) for bits in (8, 10)]


def register():
    """Append ROWS to the table of tests/stream_contract.py; an entry point that is a row there already is left alone."""
    have = {r.entry for r in SC.ROWS}
    SC.ROWS.extend(r for r in ROWS if r.entry not in have)


register()
