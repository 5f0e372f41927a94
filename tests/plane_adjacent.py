"""Layouts at the edge of refusal (tests/test_gpu_plane_adjacent.py, tests/test_plane_check_host.py): in ONE dense buffer
the output begins at the sample directly behind the last sample the call reads, which csrc/plane_check.h must accept; one
sample earlier it must refuse.  N = 2 frames of H x W = 5 x 6 samples `step` apart, tight: rows W * step samples apart, a
frame as long as its body, so frame 1 begins directly behind frame 0 too.

A call is `CALLS[name](L, base, item, step, shift, flow, pick)`: `base` the buffer's address, `item` the bytes of a
sample, `shift` how many samples before the adjacent place the output begins, `flow` / `pick` the addresses of the
operands that lie elsewhere -> the status.  `spans(name, step)` says where in the buffer the operands lie."""
from ai_based_frame_interpolation_amd import _native

H, W, N = 5, 6, 2
DH, DW = 4, 9                               # the resize's destination size
ENTRIES = [(0, 1, 3, 0, -1), (0, 2, 3, 0, -1)]   # the warp's (row, wn, den, flow, flag)


def body(step, h=H, w=W):
    return (h - 1) * w * step + (w - 1) * step + 1


def plane(step, off=0, per_frame=1, h=H, w=W):
    """Plane (offset, h, w, pitch, step, frame_stride) of frames that hold `per_frame` tight planes."""
    return (off, h, w, w * step, step, per_frame * body(step, h, w))


def uv(step):
    return [plane(step, 0, 2), plane(step, body(step), 2)]


def spans(name, step):
    """-> ({operand: first sample}, first sample of the output when adjacent, samples the output spans)."""
    b = body(step)
    if "resize" in name:
        return {"src": 0}, N * b, N * body(step, DH, DW)
    if "warp" in name:
        return {"grid": 0}, N * b, N * b
    if "fill" in name:
        return {"a": 0, "b": 2 * N * b}, 4 * N * b, 2 * N * b
    return {"a": 0, "b": N * b, "m": 2 * N * b}, 3 * N * b, N   # the pick map: one block a frame, bytes


def _arr(planes):
    return _native.resize_plane_array(list(planes))


def _resize(L, base, item, step, shift, flow, pick):
    _, out, _ = spans("resize", step)
    return L.fiunet_resize_planes_u8(base, _arr([plane(step)]), base + (out - shift) * item,
                                     _arr([plane(step, h=DH, w=DW)]), 1, N, None)


def _warp(fn):
    def call(L, base, item, step, shift, flow, pick):
        _, out, _ = spans("warp", step)
        return getattr(L, fn)(base, N, _arr([plane(step)]), flow, 1, H, W, None, 0, _native.warp_entries(ENTRIES),
                              len(ENTRIES), base + (out - shift) * item, _arr([plane(step)]), None)
    return call


def _fill(L, base, item, step, shift, flow, pick):
    at, out, _ = spans("fill", step)
    return L.fiunet_chroma_fill_u8(base, _arr(uv(step)), base + at["b"] * item, _arr(uv(step)), flow, 2 * H, 2 * W, pick, 2, 2,
                                   N, base + (out - shift) * item, _arr(uv(step)), None)


def _pick(L, base, item, step, shift, flow, pick):
    at, out, _ = spans("pick", step)
    return L.fiunet_chroma_pick_u8(base, _arr([plane(step)]), base + at["b"] * item, _arr([plane(step)]),
                                   base + at["m"] * item, _arr([plane(step)]), flow, N, base + (out - shift) * item, None)


#: entry point -> (bytes of a sample, the call)
CALLS = {
    "fiunet_resize_planes_u8": (1, _resize), "fiunet_warp_table_u8": (1, _warp("fiunet_warp_table_u8")),
    "fiunet_warp_table_p10": (2, _warp("fiunet_warp_table_p10")), "fiunet_chroma_fill_u8": (1, _fill),
    "fiunet_chroma_pick_u8": (1, _pick),
}
