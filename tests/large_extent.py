"""Shapes, zone arithmetic and window picks of the large-extent tests (test_large_extent_host.py, test_gpu_large_extent.py).

The kernels address a pixel record inside one plane with 32 bits (make_plan: H*W < 2^26, 64-B records).  "The zone" is the
part of a level-0 plane whose byte offset is at least 2^31: the pixels whose index y*W + x is at least 2^25.  Only level 0
can reach it, and only a frame of 2^25 pixels or more has one, so the shapes below are the smallest that can show a signed
32-bit offset, an offset truncated to 32 bits or a sign-extended lane offset; nothing bigger than B is accepted at all.
"""
import ctypes

import numpy as np

from ai_based_frame_interpolation_amd import _native, tiling
from oracle import stage_oracle as S

GIB = 1 << 30
ZONE_PIXEL = 1 << 25            # first pixel index whose 64-B record starts at byte 2^31 of its plane
#: name -> (B, H, W).  A: the smallest useful crossing (H and W odd: the floor-pool and the F.pad row of up4 lie in the zone,
#: the last tile column is 9 wide); B: 81 pixels below 2^26, offsets reach 2^32 - 5 KB; C: narrow pitch, the crossing falls
#: mid-row at another phase and the upsample grid has 5000 row groups.
SHAPES = {"A": (1, 4603, 8201), "B": (1, 8183, 8201), "C": (1, 40000, 1000)}
N_BANDS = {"A": 2, "B": 3, "C": 2}
BANDS = {"A": [(0, 2416), (2192, 4603)], "B": [(0, 2848), (2624, 5584), (5360, 8183)], "C": [(0, 20112), (19888, 40000)]}
VARIANTS = {"gray": (1, True), "rgb": (3, True), "convt": (1, False)}          # (channels per frame, bilinear decoder)
PRECISIONS = {"fp32": _native.FP32, "bf16": _native.BF16, "bf16x2": _native.BF16X2, "fp16": _native.FP16}
LEVEL = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0)
CASE_CAP, WINDOW_CAP = 64 * GIB, 80 * GIB    # peak allocation a whole-against-bands case / the window case may plan for
HEADROOM = 4 * GIB                           # what a GPU test wants free beyond its planned need before it starts

#: default-plan workspace in GiB (the table of the issue these tests answer; the host test holds the plan to it within 1 %)
PLAN_GIB = {("bf16", 0, "A"): 13.0, ("bf16", 0, "B"): 23.1, ("bf16", 0, "C"): 13.8,
            ("fp16", 0, "A"): 13.0, ("fp16", 0, "B"): 23.1, ("fp16", 0, "C"): 13.8,
            ("bf16x2", 0, "A"): 34.9,
            ("bf16", _native.OPT_UNFUSED, "A"): 22.6, ("bf16", _native.OPT_KEEP_ALL, "A"): 35.9}
#: the figures the issue gives to two digits ("about 27 GiB"): held to half a unit of their last digit
PLAN_GIB_ROUND = {("fp32", 0, "A"): 27, ("fp32", 0, "B"): 48, ("fp32", 0, "C"): 29, ("bf16x2", 0, "B"): 62,
                  ("bf16x2", 0, "C"): 37}

#: part 1: (id, variant, precision, shape name, unfused)
WHOLE_VS_BANDS = [("gray-bf16-A", "gray", "bf16", "A", False), ("gray-bf16-B", "gray", "bf16", "B", False),
                  ("gray-bf16-C", "gray", "bf16", "C", False), ("gray-fp16-A", "gray", "fp16", "A", False),
                  ("gray-fp32-A", "gray", "fp32", "A", False), ("gray-bf16x2-A", "gray", "bf16x2", "A", False),
                  ("gray-bf16-unfused-A", "gray", "bf16", "A", True), ("rgb-bf16-A", "rgb", "bf16", "A", False),
                  ("convt-bf16-A", "convt", "bf16", "A", False)]
FORCED_STAGES = (1, 16, 17)      # the level-0 convs, forced to either tile family at far offsets
WINDOW_STAGES = [0, 1, 2, 16, 17, S.HEAD]     # part 2: the level-0 stages, and stage 2, which reads the pooled level-0 tensor


def zone_start(w):
    """(row, column) of the first pixel of the zone in a plane `w` pixels wide."""
    return divmod(ZONE_PIXEL, w)


def full_zone_rows(h, w):
    """Rows of an h x w plane that lie in the zone from their first pixel on."""
    y, x = zone_start(w)
    return max(h - (y + (1 if x else 0)), 0)


def in_zone(y, x, w):
    return y * w + x >= ZONE_PIXEL


def bands(name):
    """[(first input row, one past the last)] of the row bands tiling.forward_tiled cuts the shape into, halo included."""
    return [(s.ext0, s.ext1) for s in tiling.strip_plan(SHAPES[name][1], N_BANDS[name]) if s.core1 > s.core0]


def stage_cfg(cf, bilinear, flags, precision, b, h, w, stage):
    """fiunet_debug_stage_cfg under `flags`: (small tile, K slices, in-workgroup cut, materialised half, form, epilogue)."""
    fn = _native.lib().fiunet_debug_stage_cfg
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 6)()
    assert fn(cf, int(bilinear), flags, PRECISIONS[precision], b, h, w, stage, out) == 0
    return tuple(out)


def plan_bytes(variant, precision, flags, b, h, w):
    cf, bil = VARIANTS[variant]
    return _native.debug_plan(cf, bil, flags, PRECISIONS[precision], b, h, w)[1]


def whole_vs_bands_need(variant, precision, name, unfused):
    """Planned peak allocation of one part-1 case: the whole frame's workspace (the bands reuse it), the two frames, the
    two results, one band's contiguous frame copies and result (under 6 frames; 7.5 measured at the peak), and half as
    much again for torch's temporaries."""
    b, h, w = SHAPES[name]
    frame = 4 * b * VARIANTS[variant][0] * h * w
    return plan_bytes(variant, precision, _native.OPT_UNFUSED if unfused else 0, b, h, w) + 12 * frame


def u8_need(name):
    """forward_u8 against the three-step route, gray bf16: the plan, fp32 frames and result (3 x 4 B a pixel), four uint8
    images, and as much again for torch's temporaries."""
    b, h, w = SHAPES[name]
    return plan_bytes("gray", "bf16", 0, b, h, w) + 32 * b * h * w


def window_need(name):
    """Part 2, gray bf16 under KEEP_ALL: the plan with every stage kept, the read-back taps one stage holds at once at
    most (stage 16: its own output, its skip, the low-res tensor it lerps - fp32 NCHW), one more tap being read, frames
    and result."""
    b, h, w = SHAPES[name]
    tap0, tap1 = 4 * 64 * b * h * w, 4 * 64 * b * (h // 2) * (w // 2)
    return (plan_bytes("gray", "bf16", _native.OPT_KEEP_ALL | _native.OPT_NO_DITHER, b, h, w) + 3 * tap0 + tap1
            + 4 * 4 * b * h * w)


def zone_windows(stage, th, tw, b, h, w, full_w):
    """Tile windows (image, y0, y1, x0, x1) of one stage at far offsets: h x w is the stage's level of a frame `full_w`
    pixels wide, (th, tw) its tile.  Each window is one whole tile of the stage's grid plus the 2-pixel ring: the tile that
    holds the pixel where byte 2^31 falls, its left and right neighbours, the tile below it, the bottom-left corner tile,
    the bottom-right one (partial both ways), two seeded tiles below row 4100 of level 0, and the top-left tile as a
    control."""
    lv = 0 if stage == S.HEAD else LEVEL[stage]
    zy, zx = zone_start(full_w)
    tys, txs = -(-h // th), -(-w // tw)
    ty, tx = (zy >> lv) // th, (zx >> lv) // tw
    assert 0 < tx < txs - 1 and ty < tys - 2, (stage, ty, tx, tys, txs)
    picks = [(ty, tx), (ty, tx - 1), (ty, tx + 1), (ty + 1, tx), (tys - 1, 0), (tys - 1, txs - 1)]
    rng = np.random.default_rng([2031, 18 if stage == S.HEAD else stage])
    first = -(-(4100 >> lv) // th)                 # first tile row that starts at or below level-0 row 4100
    picks += [(int(rng.integers(first, tys)), int(rng.integers(txs))) for _ in range(2)]
    picks.append((0, 0))
    return [(b - 1,) + S.tile_window(y, x, th, tw, h, w) for y, x in dict.fromkeys(picks)]
