"""What the motion-guided chroma tests share (tests/test_chroma_host.py, tests/test_gpu_chroma.py,
tests/test_gpu_chroma_video.py): the scenes of the quality bounds, the stored samples, and the refusals of
the C ABI.  The yardstick itself is the package's definition, `chroma.guided_torch`.

  scenes     a band-limited texture (tests/retime_motion_ref.py) at 96 x 128, luma seed 1 moving by `step` pixels per
             interval, 4:2:0 chroma seed 5 at 48 x 64 moving by half of it; the truth is the analytic middle frame.
             GAIN: steps where the guided chroma must be at least 3 dB above the average (measured gaps 12.9, 15.6 and
             5.5 dB; the margin of tests/test_retime_motion_host.py).  HOLD: steps with sub-pixel chroma motion or a flow
             that fails at this size, where it must be no more than 2 dB below the average (measured worst case 1.4 dB).
  psnr       of a chroma plane without a 6-sample border
"""
import math

import numpy as np
import torch

import retime_motion_ref as R

from ai_based_frame_interpolation_amd import _native

H, W = 96, 128
GAIN = [(4, 2), (6, -2), (3, 1)]
HOLD = [(1, 0.5), (0.4, 0.2), (8, 4), (12, 0)]
GAIN_DB, HOLD_DB, BORDER = 3.0, 2.0, 6


def scene(step):
    """-> (YA, YB, YM, CA, CB, CM): uint8 luma [96, 128] at times 0, 1, 1/2 and 4:2:0 chroma [48, 64] likewise."""
    luma = [R.texture(H, W, t, step, seed=1) for t in (0, 1, 0.5)]
    chroma = [R.texture(H // 2, W // 2, t, (step[0] / 2, step[1] / 2), seed=5) for t in (0, 1, 0.5)]
    return tuple(luma + chroma)


def psnr(a, b, peak=255.0):
    a, b = (t[BORDER:-BORDER, BORDER:-BORDER].to(torch.float64) for t in (a, b))
    mse = float(((a - b) ** 2).mean())
    return math.inf if mse == 0 else 10 * math.log10(peak * peak / mse)


def average(a, b, bits=8):
    return (R.codes(a, bits) + R.codes(b, bits) + 1) >> 1


def stored(rng, bits, *shape):
    """Random samples as stored: uint8, or int16 words of which some lie above 1023 (and some above 32767)."""
    if bits == 8:
        return torch.from_numpy(rng.integers(0, 256, shape).astype(np.uint8))
    a = rng.integers(0, 1024, shape)
    a = np.where(rng.random(shape) < 0.05, rng.integers(1024, 65536, shape), a)
    return torch.from_numpy(a.astype(np.uint16).view(np.int16))


# ---- the refusals of fiunet_chroma_pick_* / fiunet_chroma_fill_* (include/fiunet.h), every one before a launch -----------
def _plane(h, w, **k):
    d = dict(off=0, h=h, w=w, pitch=w, step=1, fs=h * w)
    d.update(k)
    return (d["off"], d["h"], d["w"], d["pitch"], d["step"], d["fs"])


def _arr(planes, filt=0):
    return None if planes is None else _native.resize_plane_array(list(planes), filt)


def pick_refusals(fn, a=1 << 20, b=1 << 22, m=1 << 24, flow=1 << 28, pick=1 << 30, h=20, w=28):
    """-> [(what, status)] of fiunet_chroma_pick_* calls that must all be refused, on pointers that are never
    dereferenced (tight h x w planes, 2 frames)."""
    ok = _plane(h, w)

    def call(**k):
        v = dict(a=a, ap=ok, b=b, bp=ok, m=m, mp=ok, flow=flow, n=2, pick=pick, filt=0)
        v.update(k)
        return fn(v["a"], _arr(None if v["ap"] is None else [v["ap"]], v["filt"]), v["b"],
                  _arr(None if v["bp"] is None else [v["bp"]]), v["m"], _arr(None if v["mp"] is None else [v["mp"]]),
                  v["flow"], v["n"], v["pick"], None)
    cases = {
        "NULL a": dict(a=None), "NULL b": dict(b=None), "NULL m": dict(m=None), "NULL flow": dict(flow=None),
        "NULL pick": dict(pick=None), "NULL a plane": dict(ap=None), "NULL b plane": dict(bp=None),
        "NULL m plane": dict(mp=None), "negative n": dict(n=-1), "n above 4096": dict(n=4097),
        "planes of different sizes": dict(mp=_plane(h - 1, w)), "b wider": dict(bp=_plane(h, w + 1)),
        "plane outside its frame stride": dict(ap=_plane(h, w, off=1)), "pitch below a row": dict(bp=_plane(h, w, pitch=w - 1)),
        "step 0": dict(mp=_plane(h, w, step=0)), "step 5": dict(ap=_plane(h, w, step=5, pitch=5 * w, fs=5 * h * w)),
        "h 0": dict(ap=_plane(0, w), bp=_plane(0, w), mp=_plane(0, w)),
        "a side above 32768": dict(**{k: _plane(h, 32769, fs=32769 * h) for k in ("ap", "bp", "mp")}),
        "a filter in a plane": dict(filt=1), "flow not 8-byte aligned": dict(flow=flow + 4),
        "a frame stride that leaves the address space": dict(ap=_plane(h, w, fs=1 << 63)),
        "pick inside a": dict(pick=a + 5), "pick inside m's second frame": dict(pick=m + h * w + 3),
    }
    # (the call with no case applied is valid, so it is never made here: it would launch on these pointers)
    return [(what, call(**k)) for what, k in cases.items()]


def fill_refusals(fn, a=1 << 20, b=1 << 22, flow=1 << 28, pick=1 << 30, out=1 << 24, h=10, w=14, fh=20, fw=28):
    """The same for fiunet_chroma_fill_*: two tight h x w planes a frame, 4:2:0 under an fh x fw luma, 2 frames."""
    ok = [_plane(h, w, fs=2 * h * w), _plane(h, w, off=h * w, fs=2 * h * w)]

    def two(**k):
        return [_plane(h, w, fs=2 * h * w), _plane(**dict(dict(h=h, w=w, off=h * w, fs=2 * h * w), **k))]

    def call(**k):
        v = dict(a=a, ap=ok, b=b, bp=ok, flow=flow, fh=fh, fw=fw, pick=pick, sy=2, sx=2, n=2, out=out, op=ok, filt=0)
        v.update(k)
        return fn(v["a"], _arr(v["ap"], v["filt"]), v["b"], _arr(v["bp"]), v["flow"], v["fh"], v["fw"], v["pick"],
                  v["sy"], v["sx"], v["n"], v["out"], _arr(v["op"]), None)
    cases = {
        "NULL a": dict(a=None), "NULL b": dict(b=None), "NULL flow": dict(flow=None), "NULL pick": dict(pick=None),
        "NULL out": dict(out=None), "NULL a planes": dict(ap=None), "NULL b planes": dict(bp=None),
        "NULL out planes": dict(op=None), "negative n": dict(n=-1), "n above 4096": dict(n=4097),
        "sy 0": dict(sy=0), "sx 3": dict(sx=3), "sy 4": dict(sy=4),
        "the second plane is checked too": dict(ap=two(pitch=w - 1)), "V of another size": dict(bp=two(h=h - 1)),
        "out planes of another size": dict(op=[_plane(h, w - 1, fs=2 * h * w), _plane(h, w - 1, off=h * w, fs=2 * h * w)]),
        "plane outside its frame stride": dict(op=two(off=h * w + 1)), "step 5": dict(ap=two(step=5, pitch=5 * w, fs=9 * h * w)),
        "a filter in a plane": dict(filt=1), "flow_h 0": dict(fh=0), "flow_w above 32768": dict(fw=32769),
        "flow not 8-byte aligned": dict(flow=flow + 4),
        "chroma rows reach past the luma": dict(fh=2 * h - 2), "chroma columns reach past the luma": dict(fw=2 * w - 2),
        "4:4:4 planes under a luma of half the size": dict(sy=1, sx=1, fh=h // 2, fw=w // 2),
        "out overlaps A": dict(out=a + h * w), "out overlaps B's last frame": dict(out=b + 4 * h * w - 1),
        "out's planes overlap": dict(op=two(off=h * w - 1)),
        "a frame stride that leaves the address space": dict(bp=[_plane(h, w, fs=1 << 63), _plane(h, w, off=h * w, fs=1 << 63)]),
    }
    return [(what, call(**k)) for what, k in cases.items()]
