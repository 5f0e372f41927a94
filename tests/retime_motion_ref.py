"""The yardstick of the retime "motion" tests (tests/test_retime_motion_host.py, tests/test_gpu_retime_motion.py): the
definition `optical_flow._warp_time_torch` applied to whole frames as stored, the inputs, and the refusals of the C ABI.

  frames    `warp_rows`: every output frame of a list of (row, wn, den, flag) entries from a grid of rows as stored, plane
            by plane of a layout (offset, pitch, step: the samples are read and written where they lie), on the CPU, in
            torch; wn == 0 and a set flag leave the frame to the caller's blend pass, as the kernel does
  blend     `blend_rows`: the integer formula of retime.py, 10-bit words above 1023 read as 1023
  dedup     `dedup_entries`: the entries of a clip with repeated frames and flagged cuts, from tests/dedup_ref.py's `place`
            (Fractions, Python ints): "motion" under dedup with scene cuts, which neither restatement had on its own (an
            extension for tests/test_gpu_video_matrix.py; without dead intervals it is the rule of tests/retime_ref.py)
  lead      `lead_of`: the plane the flow is estimated on (retime.lead_planes' rule, stated again)
  texture   `texture(h, w, t, step, seed)`: a band-limited picture (24 sinusoids, angular frequency up to 0.8 rad / px on
            each axis, 8 bits) moved by t * step pixels, evaluated analytically: the true frame at any time
  psnr      over the frame without an 8-pixel border (where content enters that no flow can know)
"""
import math

import numpy as np
import torch

from ai_based_frame_interpolation_amd import _native
from ai_based_frame_interpolation_amd import optical_flow as OF

BORDER = 8


def texture(h, w, t, step, seed=1):
    """uint8 [h, w]: the picture at time t of a texture that moves by `step` = (dx, dy) pixels per unit of time."""
    rng = np.random.default_rng(seed)
    fx, fy = rng.uniform(-0.8, 0.8, 24), rng.uniform(-0.8, 0.8, 24)
    ph, amp = rng.uniform(0, 2 * math.pi, 24), rng.uniform(0.5, 1.0, 24)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    xs, ys = xs - t * step[0], ys - t * step[1]
    v = sum(a * np.sin(kx * xs + ky * ys + p) for a, kx, ky, p in zip(amp, fx, fy, ph))
    v = 127.5 + v * (110.0 / np.abs(amp).sum())
    return torch.from_numpy(np.clip(np.rint(v), 0, 255).astype(np.uint8))


def psnr(a, b, peak=255.0):
    a, b = (t[BORDER:-BORDER, BORDER:-BORDER].to(torch.float64) for t in (a, b))
    mse = float(((a - b) ** 2).mean())
    return math.inf if mse == 0 else 10 * math.log10(peak * peak / mse)


def codes(t, bits):
    """int64 codes of stored samples (10 bits: the words unsigned, above 1023 read as 1023)."""
    return t.long() if bits == 8 else (t.view(torch.int16).long() & 0xFFFF).clamp(max=1023)


def plane_of(row, plane):
    """The [h, w] view of plane (name, offset, h, w, pitch, step) in the flat frame `row`."""
    _, off, h, w, pitch, step = plane
    return row.as_strided((h, w), (pitch, step), row.storage_offset() + off)


def lead_of(row, planes, bits):
    """The lead plane of a frame as stored, in the frame's dtype."""
    names = [p[0] for p in planes]
    if {"r", "g", "b"} <= set(names):
        pick = [p for p in planes if p[0] in "rgb"]
    elif len(names) > 1 and all(n == f"c{i}" for i, n in enumerate(names)):
        pick = planes
    else:
        return plane_of(row, planes[0]).contiguous()
    c = len(pick)
    total = sum(plane_of(row, p).to(torch.int32) for p in pick)
    return ((total * 2 + c) // (2 * c)).to(torch.uint8)


def blend_rows(a, b, wn, den, bits):
    """(A (den - wn) + B wn + den // 2) // den on stored rows -> the stored dtype."""
    v = ((den - wn) * codes(a, bits) + wn * codes(b, bits) + den // 2) // den
    return v.to(a.dtype)


def warp_rows(grid, entries, flows, planes, bits, out, flags=None):
    """Overwrite in `out` [len(entries), row] the planes of every frame whose entry (row, wn, den, flag) has wn != 0 and
    no set flag; flows: {grid row: float32 [h, w, 2] flow from it to the row after it}.  CPU tensors."""
    for k, (r, wn, den, flag) in enumerate(entries):
        if wn == 0 or (flag >= 0 and flags is not None and int(flags[flag])):
            continue
        for p in planes:
            v = OF._warp_time_torch(plane_of(grid[r], p), plane_of(grid[r + 1], p), flows[r], wn, den, bits)
            plane_of(out[k], p).copy_(v.to(out.dtype))
    return out


def plan_entries(plan, n_out, flagged=False):
    """(row, wn, den, flag) of output frames 0 .. n_out - 1 of a plan on the grid of the whole clip."""
    out = []
    for j in range(n_out):
        i, _, lo, wn = plan.frame(j)
        out.append((i * plan.G + lo, wn, plan.q, i if flagged else -1))
    return out


def dedup_entries(n_out, step, G, dead, cuts, max_gap):
    """(row, wn, den, -1) of output frames 0 .. n_out - 1 at times j * step on the factor-G grid of the whole clip:
    `dedup_ref.place` gives the interval, the row below and the weight of the row above as a Fraction, whose numerator and
    denominator are the time wn / den of the warp (`_warp_time_torch` rounds wn / den once, so the reduced fraction is the
    time itself); a frame held by the cut rule, and one that sits on a grid row, has wn == 0: a copy, never warped."""
    import dedup_ref
    out = []
    for j in range(n_out):
        i, lo, w = dedup_ref.place(j, step, G, dead, cuts, max_gap)
        if w is None or w == 0:
            out.append((i * G + lo, 0, 1, -1))
        else:
            out.append((i * G + lo, w.numerator, w.denominator, -1))
    return out


# ---- the refusals of fiunet_warp_table_* (include/fiunet.h), every one before a launch and before a pointer is used ----
def refusals(fn, grid=1 << 20, out=1 << 24, flow=1 << 28, flags=1 << 30, h=8, w=12):
    """-> [(what, status)] of calls that must all be refused, on pointers that are never dereferenced (any integers that
    keep the alignment rules; the planes are tight h x w frames, 4 grid rows, 2 flows, 3 flags, 2 output frames)."""
    ok_plane = (0, h, w, w, 1, h * w)
    ok_entries = [(0, 1, 5, 0, -1), (2, 2, 5, 1, 2)]

    def call(**k):
        a = dict(grid=grid, n_rows=4, gp=ok_plane, flow=flow, n_flows=2, fh=h, fw=w, flags=flags, n_flags=3,
                 entries=ok_entries, n_out=None, out=out, op=ok_plane, gfilter=0)
        a.update(k)
        ent = a["entries"]
        n_out = len(ent) if a["n_out"] is None else a["n_out"]
        arr = None if ent is None else _native.warp_entries(ent)
        gp = None if a["gp"] is None else _native.resize_plane_array([a["gp"]], a["gfilter"])
        op = None if a["op"] is None else _native.resize_plane_array([a["op"]])
        return fn(a["grid"], a["n_rows"], gp, a["flow"], a["n_flows"], a["fh"], a["fw"], a["flags"], a["n_flags"], arr,
                  n_out, a["out"], op, None)

    def plane(**k):
        d = dict(off=0, h=h, w=w, pitch=w, step=1, fs=h * w)
        d.update(k)
        return (d["off"], d["h"], d["w"], d["pitch"], d["step"], d["fs"])
    cases = {
        "NULL grid": dict(grid=None), "NULL out": dict(out=None), "NULL flow": dict(flow=None),
        "NULL grid plane": dict(gp=None), "NULL out plane": dict(op=None), "NULL entries": dict(entries=None, n_out=2),
        "NULL flags with n_flags": dict(flags=None), "negative n_rows": dict(n_rows=-1),
        "negative n_out": dict(n_out=-1), "negative n_flows": dict(n_flows=-1), "negative n_flags": dict(n_flags=-1),
        "row + 1 == n_rows": dict(entries=[(3, 1, 5, 0, -1)]), "row past the grid": dict(entries=[(9, 1, 5, 0, -1)]),
        "row + 1 == n_rows at wn 0": dict(entries=[(3, 0, 1, 0, -1)]),
        "flow == n_flows": dict(entries=[(0, 1, 5, 2, -1)]), "wn == den": dict(entries=[(0, 5, 5, 0, -1)]),
        "den 0": dict(entries=[(0, 0, 0, 0, -1)]), "den above 2^20": dict(entries=[(0, 1, (1 << 20) + 1, 0, -1)]),
        "flag == n_flags": dict(entries=[(0, 1, 5, 0, 3)]), "flag below -1": dict(entries=[(0, 1, 5, 0, -2)]),
        "a flag without flags": dict(flags=None, n_flags=0, entries=[(0, 1, 5, 0, 0)]),
        "the second entry is checked too": dict(entries=[(0, 1, 5, 0, -1), (0, 1, 5, 2, -1)]),
        "plane outside its frame stride": dict(gp=plane(off=1)), "out plane outside its stride": dict(op=plane(fs=h * w - 1)),
        "pitch below a row": dict(gp=plane(pitch=w - 1)), "step 0": dict(gp=plane(step=0)), "step 5": dict(op=plane(step=5, pitch=5 * w, fs=5 * h * w)),
        "h 0": dict(gp=plane(h=0)), "w 0": dict(op=plane(w=0)), "a side above 32768": dict(gp=plane(w=32769, pitch=32769, fs=32769 * h), op=plane(w=32769, pitch=32769, fs=32769 * h)),
        "a filter in a plane": dict(gfilter=1), "planes of different sizes": dict(op=plane(h=h - 1)),
        "flow_h 0": dict(fh=0), "flow_w above 32768": dict(fw=32769), "flow not 8-byte aligned": dict(flow=flow + 4),
        "out overlaps the grid": dict(out=grid + 2 * h * w), "out inside the grid's last row": dict(out=grid + 4 * h * w - 1),
    }
    # (the call with no case applied is valid, so it is never made here: it would launch on these pointers)
    return [(what, call(**k)) for what, k in cases.items()]
