"""The single-fault refusal table of the frame-format forwards (tests/test_gpu_format_refusals.py on the device, the NULL
context rows also in tests/test_format_refusals_host.py): a valid call of each entry point, B = 1, 32 x 32, bf16, made
wrong in exactly one way, and the fiunet_status (include/fiunet.h) it then returns.  The calls go through ctypes with raw
pointers, so the same rows run with device buffers or - where the refusal comes before any pointer is used - fake ones."""
import ctypes

from ai_based_frame_interpolation_amd import _native

B, H, W = 1, 32, 32
BF16 = _native.BF16
INVALID_ARG, BAD_SHAPE, NOT_LOADED, UNSUPPORTED = 1, 2, 4, 7   # include/fiunet.h: enum fiunet_status
ELEMS = 8 * 34 * 34   # samples in every frame buffer of the tests: more than any format here needs at 32 x 33

# entry point -> (sample bits, argument form)
ENTRIES = {
    "fiunet_forward_yuv420": (8, "i420"), "fiunet_forward_yuv420p10": (10, "i420"),
    "fiunet_forward_nv12": (8, "surface"), "fiunet_forward_p010": (10, "surface"),
    "fiunet_forward_yuv": (8, "yuv"), "fiunet_forward_yuv_p10": (10, "yuv"),
    "fiunet_forward_rgb_packed": (8, "packed"), "fiunet_forward_p10": (10, "plain"),
}
YUV_422P, YUV_UYVY422 = 0, 2   # enum fiunet_yuv_format; 4 is neither one of it nor a fiunet_packed_format


def valid_args(ctx, frame1, frame2, out, ws, ws_bytes):
    """The valid call, as the dict `call` marshals: tight layouts, yuv422p / rgb24, BT.601 limited range."""
    return dict(ctx=ctx, frame1=frame1, frame2=frame2, out=out, ws=ws, ws_bytes=ws_bytes, B=B, H=H, W=W, precision=BF16,
                colour=0, format=0, out_stride=0, in_layout=None, out_layout=None, in_row_pitch=0, in_frame_stride=0,
                out_row_pitch=0)


def workspace_bytes(lib, name, ctx, a):
    """The entry point's own workspace query for the shape and precision of `a` (0: it refuses them)."""
    bits, form = ENTRIES[name]
    if form == "yuv":
        return lib.fiunet_workspace_bytes_yuv(ctx, a["B"], a["H"], a["W"], a["precision"], bits)
    query = {"fiunet_forward_yuv420": lib.fiunet_workspace_bytes_yuv420, "fiunet_forward_p10": lib.fiunet_workspace_bytes_p10,
             "fiunet_forward_yuv420p10": lib.fiunet_workspace_bytes_yuv420p10, "fiunet_forward_nv12": lib.fiunet_workspace_bytes_nv12,
             "fiunet_forward_p010": lib.fiunet_workspace_bytes_p010, "fiunet_forward_rgb_packed": lib.fiunet_workspace_bytes_rgb_packed}
    return query[name](ctx, a["B"], a["H"], a["W"], a["precision"])


def _layout(form, fields):
    if fields is None:
        return None
    return ctypes.byref((_native.SurfaceLayout if form == "surface" else _native.PackedLayout)(*fields))


def call(lib, name, a):
    """-> the status of entry point `name` on the arguments `a` (null stream)."""
    form = ENTRIES[name][1]
    head, tail = (a["ctx"], a["frame1"], a["frame2"]), (a["precision"], a["ws"], a["ws_bytes"], None)
    shape = (a["B"], a["H"], a["W"])
    fn = getattr(lib, name)
    if form == "i420":
        return fn(*head, a["out"], a["out_stride"], *shape, a["colour"], *tail)
    if form == "plain":
        return fn(*head, a["out"], a["out_stride"], *shape, *tail)
    if form == "yuv":
        return fn(*head, a["format"], a["in_row_pitch"], a["in_frame_stride"], a["out"], a["out_row_pitch"], a["out_stride"],
                  *shape, a["colour"], *tail)
    layouts = _layout(form, a["in_layout"]), _layout(form, a["out_layout"])
    return fn(*head, layouts[0], a["out"], layouts[1], *shape, a["format"] if form == "packed" else a["colour"], *tail)


def _tight(name):
    """Samples of one tight 32 x 32 frame of the valid call's format."""
    form = ENTRIES[name][1]
    return {"i420": H * W * 3 // 2, "surface": H * W * 3 // 2, "yuv": 2 * H * W, "packed": 3 * H * W, "plain": 3 * H * W}[form]


def _short_out_stride(name, a):
    form = ENTRIES[name][1]
    if form in ("surface", "packed"):
        a["out_layout"] = (0, 0, 0, _tight(name) - 1) if form == "surface" else (0, _tight(name) - 1)
    else:
        a["out_stride"] = _tight(name) - 1


def _uncovered_in_layout(name, a):
    form = ENTRIES[name][1]
    if form == "surface":
        a["in_layout"] = (W - 1, 0, 0, 0)          # luma_pitch < W
    elif form == "packed":
        a["in_layout"] = (3 * W - 1, 0)            # row_pitch < W * bpp
    else:
        a["in_frame_stride"] = _tight(name) - 1    # a yuv422p frame is 2*H*W samples


def _set(**kw):
    return lambda name, a: a.update(kw)


def _has_colour(name):
    return ENTRIES[name][1] in ("i420", "surface", "yuv")


def _is(*forms):
    return lambda name: ENTRIES[name][1] in forms


# fault -> (what to change in the valid call, the entry points it applies to, status, {entry point: another status}).
# "ctx" faults replace the context: "null", "gray" (a loaded grayscale network), "unloaded" (RGB, created, nothing loaded).
FAULTS = {
    "null-ctx": ("null", lambda n: True, INVALID_ARG, {}),
    "null-frame1": (_set(frame1=None), lambda n: True, INVALID_ARG, {}),
    "null-frame2": (_set(frame2=None), lambda n: True, INVALID_ARG, {}),
    "null-out": (_set(out=None), lambda n: True, INVALID_ARG, {}),
    "null-workspace": (_set(ws=None), lambda n: True, INVALID_ARG, {}),
    "gray-ctx": ("gray", lambda n: n != "fiunet_forward_p10", UNSUPPORTED, {}),   # (fiunet_forward_p10 takes both networks)
    "unloaded-ctx": ("unloaded", lambda n: True, NOT_LOADED, {}),
    "precision-99": (_set(precision=99), lambda n: True, INVALID_ARG, {}),
    "unknown-colour-bit": (_set(colour=16), _has_colour, INVALID_ARG, {}),
    "bt2020-at-8-bits": (_set(colour=_native.YUV_BT2020), lambda n: _has_colour(n) and ENTRIES[n][0] == 8, INVALID_ARG, {}),
    "bt709-with-bt2020": (_set(colour=_native.YUV_BT709 | _native.YUV_BT2020),
                          lambda n: _has_colour(n) and ENTRIES[n][0] == 10, INVALID_ARG, {}),
    "unknown-format": (_set(format=4), _is("packed", "yuv"), INVALID_ARG, {}),
    "one-plane-format-at-10-bits": (_set(format=YUV_UYVY422), lambda n: n == "fiunet_forward_yuv_p10", INVALID_ARG, {}),
    "odd-width-uyvy422": (_set(format=YUV_UYVY422, W=33), lambda n: n == "fiunet_forward_yuv", INVALID_ARG, {}),
    "short-out-stride": (_short_out_stride, lambda n: True, INVALID_ARG, {}),
    "uncovered-in-layout": (_uncovered_in_layout, _is("surface", "packed", "yuv"), INVALID_ARG, {}),
    "height-8": (_set(H=8), lambda n: True, BAD_SHAPE, {}),
    "batch-0": (_set(B=0), lambda n: True, INVALID_ARG, {"fiunet_forward_yuv": BAD_SHAPE, "fiunet_forward_yuv_p10": BAD_SHAPE}),
}

# The one behavioural tightening since these entry points were written: before the staged-RGB forward was shared, they
# found out that the context had no weights only from the inner forward, after their two input conversions had been
# launched into the workspace (fiunet_forward_p10 itself has always refused up front).  There the status was already
# this table's; only the nothing-launched assertion of test_gpu_format_refusals.py failed.
LAUNCHED_BEFORE_REFUSING_ONCE = {(n, "unloaded-ctx") for n in ENTRIES if n != "fiunet_forward_p10"}

CASES = [(name, fault) for name in ENTRIES for fault, (_, applies, _, _) in FAULTS.items() if applies(name)]


def expected(name, fault):
    return FAULTS[fault][3].get(name, FAULTS[fault][2])


def faulty_args(name, fault, valid):
    """A copy of the valid call's arguments with `fault` applied (a "ctx" fault is the caller's: it owns the contexts)."""
    a = dict(valid)
    change = FAULTS[fault][0]
    if not isinstance(change, str):
        change(name, a)
    return a
