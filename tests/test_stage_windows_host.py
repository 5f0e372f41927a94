"""CPU: the windowed stage reference (oracle.stage_oracle.stage_reference_window / check_stage_windows), and the shape at
which tests/test_gpu_stage_windows.py runs it.

The dense layer-local check needs a float64 reference of whole tensors, so it stops at small shapes, where the plan
launches the small-problem kernels.  The windowed reference recomputes a stage on a window of one image from crops of the
taps, which costs the same at any frame size.  Here, without a GPU:
  - on taps of emulate_forward at 1x34x52, 2x45x71 RGB, 1x70x86 and 1x34x52 ConvTranspose2d (odd levels: F.pad is live),
    every window - the four corners, both partial edges, an interior one - of all 18 stages (stage 1 through the tap and
    through the fused stem), the head and the `.up` halves equals the dense reference cropped, in y, M and E, within
    1e-12 M (the conv library's summation order), for weights exact, bf16_feedback and fp16_rne;
  - the untouched emulation passes check_stage_windows, and a column at a tile seam taken from its neighbour, a non-zero
    F.pad row or column of an upsampled half, a shift added twice and a lerp row taken one low-res row off are rejected;
  - the bf16 stem's dither: stage 0 and the fused stage 1 checked against frames carrying stem_dither reject a stem that
    omits the dither, swaps its sign between the frames or anchors the pattern at the window;
  - PINNED = 8 x 552 x 1000 is a shape at which the default plan launches what B = 8 at 1080p launches, stage by stage
    (fiunet_debug_stage_cfg under OPT_KEEP_ALL | OPT_NO_DITHER: form, epilogue, one K slice, no in-workgroup cut, the
    materialise flag, TH x TW), except the tile FAMILY of the stages in FORCED, which the GPU test forces.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import stage_oracle as S
from oracle import unet_oracle as O

VARIANTS = {"gray": (2, 1, True), "rgb": (6, 3, True), "convt": (2, 1, False)}
SHAPES = [("gray", 1, 34, 52), ("rgb", 2, 45, 71), ("gray", 1, 70, 86), ("convt", 1, 34, 52)]
MODES = {"exact": "fp32", "bf16_feedback": "bf16", "fp16_rne": "fp16"}     # weight mode -> the precision emulated


@pytest.fixture(scope="module")
def sds():
    return {v: (O.make_trained_like_state_dict(*a), {}) for v, a in VARIANTS.items()}


def _windows(nb, h, w):
    """Windows of an h x w level: the four corners, a window on each far (partial) edge away from the corners, one in
    the interior; over the images of the batch in turn."""
    a, c = min(h, 5), min(w, 7)
    ym, xm = min(max(h // 3, 0), h - a), min(max(w // 3, 0), w - c)
    wins = [(0, a, 0, c), (0, a, w - c, w), (h - a, h, 0, c), (h - a, h, w - c, w), (h - a, h, xm, xm + c), (ym, ym + a, w - c, w),
            ((1, h - 1) if h >= 3 else (0, h)) + ((1, w - 1) if w >= 3 else (0, w))]
    wins = list(dict.fromkeys(wins))
    return [(i % nb,) + win for i, win in enumerate(wins)]


def _stages(variant):
    return list(range(18)) + [S.HEAD] + ([] if VARIANTS[variant][2] else S.UP)


def _out_shape(taps, stage):
    if stage == S.HEAD:
        return taps[S.TAP[17]].shape
    if isinstance(stage, str):
        return taps[S.TAP[S.SKIP_OF_CONCAT[10 + 2 * S.UP.index(stage)]]].shape
    return taps[S.TAP[stage]].shape


@pytest.mark.parametrize("weights", list(MODES))
@pytest.mark.parametrize("variant,b,h,w", SHAPES)
def test_every_window_equals_the_dense_reference_cropped(sds, variant, b, h, w, weights):
    sd, cache = sds[variant]
    f1, f2 = O.make_frames(71, b, h, w, c=VARIANTS[variant][1])
    taps = {}
    S.emulate_forward(sd, f1, f2, MODES[weights], dither=False, dtype=torch.float32, keep=taps)
    bilinear_taps = {k: v for k, v in taps.items() if not (VARIANTS[variant][2] and k in S.UP)}   # (the reference lerps itself)
    n = 0
    for st in _stages(variant):
        for stem in (("tap", "fused") if st == 1 and weights != "exact" else ("tap",)):
            y, m, e = S.stage_reference(sd, st, bilinear_taps, weights, stem, with_slack=True, cache=cache)
            if isinstance(st, str) and st != S.HEAD:
                y, m, e = (S._pad_to(t, torch.empty(_out_shape(taps, st))) for t in (y, m, e))
            nb, _, hh, ww = y.shape
            assert tuple(y.shape[2:]) == tuple(_out_shape(taps, st)[2:])
            wins = _windows(nb, hh, ww)
            assert len(wins) == 7 or hh < 15 or ww < 21, (st, wins)     # (small levels: some of the seven coincide)
            for win in wins:
                i, y0, y1, x0, x1 = win
                yw, mw, ew = S.stage_reference_window(sd, st, bilinear_taps, win, weights, stem, True, cache)
                for name, got, want in (("y", yw, y), ("M", mw, m), ("E", ew, e)):
                    want = want[i:i + 1, :, y0:y1, x0:x1]
                    assert got.shape == want.shape, (st, win, name)
                    tol = 1e-12 * m[i:i + 1, :, y0:y1, x0:x1]
                    assert bool(((got - want).abs() <= tol).all()), (variant, st, stem, win, name,
                                                                     ((got - want).abs() - tol).max().item())
                n += 1
        if st in S.SKIP_OF_CONCAT and weights != "exact" and VARIANTS[variant][2]:
            assert e.any(), (variant, st)                     # (the slack band is live in what was compared)
    assert n >= 5 * 19


# ---- mutations -------------------------------------------------------------------------------------------------------------
MUT_SHAPE = (1, 70, 86)       # levels 70x86, 35x43, 17x21, 8x10, 4x5: F.pad adds a row and a column in up2 and up3
TILE = (8, 32)


@pytest.fixture(scope="module")
def emulated(sds):
    """variant -> (state dict, bf16 emulation taps with fp32 accumulation and the head, weight cache) at MUT_SHAPE."""
    out = {}
    for v in ("gray", "convt"):
        sd, cache = sds[v]
        f1, f2 = O.make_frames(71, *MUT_SHAPE, c=1)
        taps = {}
        taps[S.HEAD] = S.emulate_forward(sd, f1, f2, "bf16", dither=False, dtype=torch.float32, keep=taps)
        out[v] = (sd, taps, cache)
    return out


def _bf16(t):
    return torch.from_numpy(S.bf16_rne(t.numpy().astype(np.float32)).astype(np.float64))


def _tile_windows(h, w):
    th, tw = TILE
    tys, txs = (h + th - 1) // th, (w + tw - 1) // tw
    tiles = {(0, 0), (0, txs - 1), (tys - 1, 0), (tys - 1, txs - 1), (tys // 2, txs // 2)}
    return [(0,) + S.tile_window(ty, tx, th, tw, h, w) for ty, tx in sorted(tiles)]


def _check(sd, stage, acts, cache, stem="tap"):
    shape = _out_shape(acts, stage)
    S.check_stage_windows(sd, stage, acts, _tile_windows(shape[2], shape[3]), "bf16", "bf16_feedback", stem, "mutation",
                          cache, tile=TILE)


def _without_up(taps, bilinear):
    return {k: v for k, v in taps.items() if not (bilinear and k in S.UP)}


@pytest.mark.parametrize("variant", ["gray", "convt"])
def test_the_untouched_emulation_passes_on_tile_windows(emulated, variant):
    sd, taps, cache = emulated[variant]
    acts = _without_up(taps, variant == "gray")
    for st in _stages(variant):
        _check(sd, st, acts, cache)


@pytest.mark.parametrize("variant,stage", [("gray", 1), ("gray", 3), ("gray", 16), ("gray", S.HEAD), ("convt", "unet.up4.up")])
def test_a_seam_column_taken_from_its_neighbour_is_rejected(emulated, variant, stage):
    sd, taps, cache = emulated[variant]
    name = stage if isinstance(stage, str) else S.TAP[stage]
    acts = _without_up(taps, variant == "gray")
    t = taps[name].clone()
    assert t.shape[3] > 33
    t[..., 32] = t[..., 31]
    acts[name] = t
    with pytest.raises(AssertionError, match=r"x=32\).*x%32=0\)"):
        _check(sd, stage, acts, cache)


def test_a_nonzero_pad_row_or_column_of_an_upsampled_half_is_rejected(emulated):
    # ConvTranspose2d: the half is a stage of its own, and its F.pad band must read exactly zero
    sd, taps, cache = emulated["convt"]
    for k, (row, col) in ((2, (16, None)), (3, (None, 42))):
        name = S.UP[k - 1]
        t = taps[name].clone()
        assert t.shape[2:] == ((17, 21) if k == 2 else (35, 43)) and not t[:, :, -1].any() and not t[..., -1].any()
        if row is not None:
            t[:, :, row] = t[:, :, row - 1]
        else:
            t[..., col] = t[..., col - 1]
        with pytest.raises(AssertionError, match="over the bound"):
            _check(sd, name, {**taps, name: t}, cache)
    # bilinear: a concat conv that reads the band as a copy of its neighbour instead of zero
    sd, taps, cache = emulated["gray"]
    for stage, k, (row, col) in ((12, 2, (16, None)), (14, 3, (None, 42))):
        up = taps[S.UP[k - 1]].clone()
        if row is not None:
            up[:, :, row] = up[:, :, row - 1]
        else:
            up[..., col] = up[..., col - 1]
        y = S.stage_reference(sd, stage, {**taps, S.UP[k - 1]: up}, "bf16_feedback", cache=cache)[0]
        acts = _without_up(taps, True)
        acts[S.TAP[stage]] = _bf16(y)
        with pytest.raises(AssertionError, match="over the bound"):
            _check(sd, stage, acts, cache)


@pytest.mark.parametrize("stage", [1, 6, 12, 17])
def test_a_shift_added_twice_is_rejected(emulated, stage):
    sd, taps, cache = emulated["gray"]
    w, sh = S.stage_weights(sd, stage, "bf16_feedback", cache)
    y = S.stage_reference(sd, stage, taps, "bf16_feedback", cache={(stage, "bf16_feedback"): (w, 2 * sh)})[0]
    acts = _without_up(taps, True)
    acts[S.TAP[stage]] = y if stage == 17 else _bf16(y)
    with pytest.raises(AssertionError, match="over the bound"):
        _check(sd, stage, acts, cache)


@pytest.mark.parametrize("stage,k", [(10, 1), (12, 2), (16, 4)])
def test_a_lerp_row_taken_one_low_res_row_off_is_rejected(emulated, stage, k):
    sd, taps, cache = emulated["gray"]
    low = taps[S.TAP[stage - 1]]
    up = taps[S.UP[k - 1]].clone()
    off = S._pad_to(S.upsample_fp32(torch.roll(low, -1, 2)), up)       # every row lerped from the low-res rows one below
    row = min(9, up.shape[2] - 3)                                      # inside the first tile row's window, off the F.pad band
    up[:, :, row] = _bf16(off)[:, :, row]
    y = S.stage_reference(sd, stage, {**taps, S.UP[k - 1]: up}, "bf16_feedback", cache=cache)[0]
    acts = _without_up(taps, True)
    acts[S.TAP[stage]] = _bf16(y)
    with pytest.raises(AssertionError, match="over the bound"):
        _check(sd, stage, acts, cache)


# ---- the bf16 stem's dither ---------------------------------------------------------------------------------------------
DITHER_WINDOW = (0, 19, 45, 37, 75)      # origin (19, 37): not a multiple of the pattern's period 8 on either axis


def _dithered_stem(sd, kind, cache):
    """Taps 0 and 1 of a bf16 stem that dithers as `kind` says, and the frames carrying the dither as it should be."""
    f1, f2 = O.make_frames(71, *MUT_SHAPE, c=1)
    d = S.stem_dither(*MUT_SHAPE[1:])
    _, y0, _, x0, _ = DITHER_WINDOW
    dev = {"right": d, "omitted": torch.zeros_like(d), "swapped": -d,
           "anchored at the window": torch.roll(d, (y0, x0), (0, 1))}[kind]
    t0 = _bf16(S.stage_reference(sd, 0, {"frame1": (f1 + dev).double(), "frame2": (f2 - dev).double()})[0])
    t1 = _bf16(S.stage_reference(sd, 1, {S.TAP[0]: t0}, "bf16_feedback", cache=cache)[0])
    return {"frame1": (f1 + d).double(), "frame2": (f2 - d).double(), S.TAP[0]: t0, S.TAP[1]: t1}


@pytest.mark.parametrize("stage,stem", [(0, "tap"), (1, "fused")])
def test_a_wrong_stem_dither_is_rejected(sds, stage, stem):
    sd, cache = sds["gray"]
    wins = [DITHER_WINDOW, (0, 0, 10, 0, 34)]
    S.check_stage_windows(sd, stage, _dithered_stem(sd, "right", cache), wins, "bf16", "bf16_feedback", stem, "dither", cache)
    for kind in ("omitted", "swapped", "anchored at the window"):
        with pytest.raises(AssertionError, match="over the bound"):
            S.check_stage_windows(sd, stage, _dithered_stem(sd, kind, cache), wins[:1], "bf16", "bf16_feedback", stem, kind, cache)


# ---- the shape of the GPU test, pinned --------------------------------------------------------------------------------
# 8 x 552 x 984 was the first candidate; it fails at one stage: up3.3 (64 couts at level 1, 276 x 492) takes the narrow 32x16
# tile there (prefer_wide: 288 x 512 * 32 > 288 x 496 * 33), where 1080p runs 16x32.  The nearest shape (|dH| + |dW|, any
# H in 530..574 and W in 950..1019) that passes everything below is 16 columns wider.
PINNED = (8, 552, 1000)         # levels 552x1000, 276x500, 138x250, 69x125, 34x62
BENCH = (8, 1080, 1920)
#: stages whose tile FAMILY at PINNED differs from BENCH's (fewer tuned workgroups: choose_conv_cfg's partial-round rule
#: picks the small tile), per decoder: stage -> force_cfg tile code of BENCH's family (1 tuned, 2 small).  The GPU test
#: forces exactly these; every precision and both frame formats agree on them.
FORCED = {True: {6: 1, 7: 1, 10: 1, 11: 1, 13: 1}, False: {6: 1, 7: 1, 8: 1, 9: 1, 10: 1, 11: 1}}
LEVEL = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0)
COUT = {True: (64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 256, 256, 128, 128, 64, 64, 64),
        False: (64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64)}


def stage_plan(frame_channels, bilinear, precision, b, h, w, stage):
    """fiunet_debug_stage_cfg: (small tile, K slices, in-workgroup cut, materialised half, form, epilogue)."""
    from ai_based_frame_interpolation_amd import _native
    fn = _native.lib().fiunet_debug_stage_cfg
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 6)()
    code = {"fp32": _native.FP32, "bf16": _native.BF16, "bf16x2": _native.BF16X2, "fp16": _native.FP16}[precision]
    assert fn(frame_channels, int(bilinear), _native.OPT_KEEP_ALL | _native.OPT_NO_DITHER, code, b, h, w, stage, out) == 0
    return tuple(out)


def level_shape(h, w, level):
    return h >> level, w >> level


def tile_shape(small, cout, h, w):
    """(TH, TW) of a conv launch on an h x w level, restated from csrc/fiunet.hip (kSmallTile, big_tile) and
    csrc/fiunet_internal.h (prefer_wide): the 32-wide tile unless the narrow one saves more than 1/32 of the padded area."""
    def padded(th, tw):
        return -(-h // th) * th * (-(-w // tw) * tw)

    def prefer_wide(thw, tww, thn, twn):
        return padded(thw, tww) * 32 <= padded(thn, twn) * 33
    if small:
        return 8, 32
    if cout == 64:
        return (16, 32) if prefer_wide(16, 32, 32, 16) else (32, 16)
    return (8, 32) if prefer_wide(8, 32, 16, 16) else (16, 16)


def stage_tile(bilinear, shape, stage, small):
    return tile_shape(small, COUT[bilinear][stage], *level_shape(shape[1], shape[2], LEVEL[stage]))


def test_the_pinned_shape_is_just_past_the_materialise_gate_and_partial_everywhere():
    b, h, w = PINNED
    assert b * h * w <= 3 * 1080 * 1920
    h3, w3 = level_shape(h, w, 3)
    assert 65536 <= b * h3 * w3 < 1.06 * 65536            # materialise_up's gate at level 3, with under 6 % to spare
    assert (h3, w3) == (69, 125) and level_shape(h, w, 4) == (34, 62)       # F.pad adds a row and a column in up1
    for bilinear in (True, False):
        for stage in range(1, 18):                        # a partial last tile row and column in every stage's own tiling
            small = stage_plan(1, bilinear, "bf16", *BENCH, stage)[0]
            th, tw = stage_tile(bilinear, PINNED, stage, small)
            hl, wl = level_shape(h, w, LEVEL[stage])
            assert hl % th and wl % tw, (bilinear, stage, (hl, wl), (th, tw))
    # the persistent RGB stem loops (8 960 16x32 tiles on 768 resident workgroups), and level 4 fills the chip with tuned
    # tiles (320 workgroups of 128 couts x 8x32), so its K loop is whole
    assert b * -(-h // 16) * -(-w // 32) == 8960
    assert b * -(-34 // 8) * -(-62 // 32) * (512 // 128) == 320


@pytest.mark.parametrize("bilinear,frame_channels", [(True, 1), (True, 3), (False, 1)])
@pytest.mark.parametrize("precision", ["fp32", "bf16", "bf16x2", "fp16"])
def test_the_pinned_shape_launches_what_batch_8_at_1080p_launches(precision, bilinear, frame_channels):
    forced = {}
    for stage in range(18):
        small, k, kwave, mat, form, epi = stage_plan(frame_channels, bilinear, precision, *PINNED, stage)
        small_b, k_b, kwave_b, mat_b, form_b, epi_b = stage_plan(frame_channels, bilinear, precision, *BENCH, stage)
        assert (form, epi, mat) == (form_b, epi_b, mat_b), (stage, (form, epi, mat), (form_b, epi_b, mat_b))
        assert k == k_b == 1 and kwave == kwave_b == 0, stage
        if stage == 0:
            continue
        if small != small_b:
            forced[stage] = 2 if small_b else 1
        # with BENCH's family (forced where the rule differs), the tile is the same TH x TW at both shapes
        assert stage_tile(bilinear, PINNED, stage, small_b) == stage_tile(bilinear, BENCH, stage, small_b), stage
    assert forced == FORCED[bilinear], forced
    if bilinear and precision != "fp32":
        assert stage_plan(frame_channels, True, precision, *PINNED, 10)[3] == 1        # up1.0 and up2.0: materialised halves
        assert stage_plan(frame_channels, True, precision, *PINNED, 12)[3] == 1
    if bilinear:                                              # the two level-4 convs: the small tile by the partial-round rule
        assert [stage_plan(frame_channels, True, precision, *PINNED, s)[0] for s in (8, 9)] == [1, 1]
