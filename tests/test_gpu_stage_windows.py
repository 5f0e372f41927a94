"""GPU (MI355X): every stage of the full-chip launches, per element, on tile windows.

tests/test_gpu_bn_stats.py holds each stage to oracle.stage_oracle.stage_bound against a dense float64 reference, which
is affordable only at shapes where the plan launches the small-problem kernels.  Here the same bound - unchanged - is
applied at 8 x 552 x 1000 (tests/test_stage_windows_host.py pins that its plan is the one of B = 8 at 1080p: tuned 128x8x32
and 64x16x32 tiles, whole K loops, the materialised upsampled halves of up1.0 and up2.0, the wide in-gather lerp of up3.0
and up4.0, the fused gray stem, the fused head, the persistent RGB stem over 8 960 tiles), on windows: the reference is
oracle.stage_oracle.stage_reference_window on crops of the device's own taps, cut on the device.

Per stage - all 18, the head, the ConvTranspose2d halves - the windows are whole tiles of the stage's own tile grid plus a
2-pixel ring of their neighbours (every in-tile position, all four seams): the four corner tiles (the far ones partial),
one interior tile and seeded ones, from image 0, image 7 and images in between.  Stages whose tile family the partial-round
rule picks differently at this size are forced to the family 1080p runs (the host test lists them); the K cut is the plan's
own.  The kernel names of one profiled forward must show those forms.

bf16 with the default options: stages 0 and 1 against frames carrying the ordered stem dither (+d frame 1, -d frame 2,
anchored at the image origin), at this shape and on the second of two row bands of 1x135x240 through forward_strip.

Worst error / bound (and error / M) per precision and stage family, measured on an MI355X at 8 x 552 x 1000:
  precision                stem             inc.3          pool-fed            direct            concat             convt              head
  fp32          0.016 (2.5e-07)   0.143 (2.2e-06)   0.448 (6.8e-06)   0.440 (6.7e-06)   0.505 (7.7e-06)                 -   0.017 (2.6e-07)
  bf16x2        0.087 (6.5e-06)   0.116 (7.6e-06)   0.130 (9.8e-06)   0.136 (1.0e-05)   0.134 (1.0e-05)                 -   0.075 (5.1e-06)
  bf16          0.972 (3.5e-03)   0.956 (3.7e-03)   0.976 (3.8e-03)   0.979 (3.8e-03)   0.977 (3.8e-03)   0.979 (3.6e-03)   0.868 (3.4e-03)
  fp16          0.863 (4.2e-04)   0.801 (4.5e-04)   0.879 (4.8e-04)   0.882 (4.8e-04)   0.856 (4.6e-04)                 -   0.670 (3.3e-04)
  bf16, dither on: stem 0.968 (3.5e-03), inc.3 0.926 (3.5e-03); on the band 64:135 of 1x135x240: stem 0.974 (3.6e-03), inc.3 0.931 (3.5e-03)
  (bf16 and fp16 sit near 1 by construction: the store's own rounding is up to half an ulp, 2^-8 / 2^-11 of a value just
  above a power of two, which is the bound's first term.)
"""
import numpy as np
import pytest

from ai_based_frame_interpolation_amd import _native
from oracle import stage_oracle as S
from oracle import unet_oracle as O
from test_gpu_bn_stats import VARIANTS, WEIGHTS, _REPORT, _stage1_fused, caches, dev, dev_of, models, sds  # noqa: F401
from test_stage_windows_host import BENCH, COUT, FORCED, LEVEL, PINNED, level_shape, stage_plan, stage_tile

pytestmark = pytest.mark.gpu

CASES = [("gray", "fp32"), ("gray", "bf16x2"), ("gray", "bf16"), ("gray", "fp16"), ("rgb", "fp32"), ("rgb", "bf16"),
         ("convt", "bf16")]
ELEM = {"fp32": "f32", "bf16": "bf16", "bf16x2": "bf16", "fp16": "f16"}
SEEDED_TILES = 3
_FRAMES = {}


def frames_for(cf):
    """The frame pair of the pinned shape, made once per channel count and left unchanged."""
    if cf not in _FRAMES:
        _FRAMES[cf] = O.make_frames(79, *PINNED, c=cf)
    return _FRAMES[cf]


def bench_tile(variant, prec, stage):
    """(small family, TH, TW) of the launch B = 8 at 1080p gives this stage (the head: the last conv's; a ConvTranspose2d
    half: the concat conv's it feeds; the stem: the RGB stem's 16x32 tile)."""
    _, cf, bil = VARIANTS[variant]
    if stage == 0:
        return False, 16, 32
    i = 17 if stage == S.HEAD else 10 + 2 * S.UP.index(stage) if isinstance(stage, str) else stage
    small = bool(stage_plan(cf, bil, prec, *BENCH, i)[0])
    return (small,) + stage_tile(bil, PINNED, i, small)


def stage_windows(stage, th, tw, b, h, w, seeded=SEEDED_TILES):
    """Tile windows of one stage: the four corner tiles, one interior tile, `seeded` tiles drawn from a fixed seed; images
    0 and b - 1 at the corners, one in between for the interior tile, drawn ones for the rest."""
    tys, txs = -(-h // th), -(-w // tw)
    idx = 18 if stage == S.HEAD else 19 + S.UP.index(stage) if isinstance(stage, str) else stage
    rng = np.random.default_rng([2025, idx])
    picks = [(0, 0, 0), (b - 1, 0, txs - 1), (b - 1, tys - 1, 0), (0, tys - 1, txs - 1), (b // 2, tys // 2, txs // 2)]
    picks += [(int(rng.integers(b)), int(rng.integers(tys)), int(rng.integers(txs))) for _ in range(seeded)]
    return [(i,) + S.tile_window(ty, tx, th, tw, h, w) for i, ty, tx in dict.fromkeys(picks)]


def taps_needed(stage, bilinear, fused):
    """Read-back tap numbers (0..17 conv stages, 18..21 upsampled halves) a stage's check reads, its own output included."""
    if stage == S.HEAD:
        return [17]
    if isinstance(stage, str):
        k = S.UP.index(stage)
        return [18 + k, 9 + 2 * k, S.SKIP_OF_CONCAT[10 + 2 * k]]
    if stage == 0 or (stage == 1 and fused):
        return [stage]
    if stage in S.POOL_OF:
        return [stage, S.POOL_OF[stage]]
    if stage in S.SKIP_OF_CONCAT:   # the bilinear half is lerped by the reference itself; a ConvTranspose2d half is a stage of its own
        return [stage, S.SKIP_OF_CONCAT[stage], stage - 1 if bilinear else 18 + (stage - 10) // 2]
    return [stage, stage - 1]


def tap_name(t):
    return S.TAP[t] if t < 18 else S.UP[t - 18]


def check_forms(variant, prec, names):
    """The kernel names of one profiled forward show the forms of B = 8 at 1080p."""
    _, cf, bil = VARIANTS[variant]
    for i in range(1, 18):
        name = names[i]
        small, th, tw = bench_tile(variant, prec, i)
        bn = 64 if small or COUT[bil][i] == 64 else 128
        assert name.startswith(f"conv3x3_mfma_kernel<{ELEM[prec]},{bn},{th},{tw},"), (i, name)
        assert "kwave" not in name and "+splitk" not in name, (i, name)
        mode, epi = (int(v) for v in name[name.index("<") + 1:name.index(">")].split(",")[4:6])
        _, _, _, mat, form, epi_plan = stage_plan(cf, bil, prec, *PINNED, i)
        assert epi == epi_plan, (i, name)
        if i in S.SKIP_OF_CONCAT:   # a materialised half: the conv gathers two direct sources (mode 0, bf16x2: 4); else it lerps (2)
            assert mode == ((4 if prec == "bf16x2" else 0) if mat else 2), (i, name)
        else:                       # the gray stem evaluated in the gather (form 6: mode 3, bf16x2: 5), or a direct source
            assert mode == {6: 5 if prec == "bf16x2" else 3}.get(form, 4 if prec == "bf16x2" else 0), (i, name)
    if bil and prec in ("bf16", "fp16"):
        assert all(stage_plan(cf, bil, prec, *PINNED, i)[3] for i in (10, 12))      # upsample_kernel writes their halves


def run_windows(model, sd, variant, prec, frames, cache, stages, dither=False, strip=None, forms=False, label=""):
    """One forward with every stage kept; then each stage of `stages` on its windows, reading only the taps it needs.
    strip: (y_origin, image height) - the frames are that band, through forward_strip."""
    _, cf, bil = VARIANTS[variant]
    f1, f2 = frames
    b, _, h, w = f1.shape
    d = dev_of(model)
    model.precision = prec
    model.set_options(no_dither=not dither)
    ctx = model._context(d)
    try:
        if (b, h, w) == PINNED:
            for layer, tile in FORCED[bil].items():
                ctx.force_cfg(layer, tile, 1)          # (1 = the whole K loop, which is the plan's own choice at both shapes)
        ctx.profile_enable(forms)
        with model.debug_taps(f1.to(d), f2.to(d), strip=strip) as (read, out):
            if forms:
                check_forms(variant, prec, [r[0] for r in ctx.profile_read()[1]])
                ctx.profile_enable(False)
                if bil and prec != "fp32":     # the halves upsample_kernel / x2_upsample_kernel wrote are tensors of their own
                    assert read(18) is not None and read(19) is not None
            flags = _native.OPT_KEEP_ALL | (0 if dither else _native.OPT_NO_DITHER)
            fused = _stage1_fused(prec, cf, bil, flags, b, h, w)
            if dither:      # the frames as the stem must see them: the pattern of the whole image, in fp32
                hg, y0 = (h, 0) if strip is None else (strip[1], strip[0])
                pattern = S.stem_dither(hg, w)[y0:y0 + h]
                f1, f2 = f1 + pattern, f2 - pattern
            held = {"frame1": f1, "frame2": f2, S.HEAD: out}
            for st in stages:
                need = {tap_name(t): t for t in taps_needed(st, bil, fused)}
                held = {k: v for k, v in held.items() if k in need or k in ("frame1", "frame2", S.HEAD)}
                for name, t in need.items():
                    if name not in held:
                        held[name] = read(t)
                        assert held[name] is not None, (st, name)
                if (b, h, w) == PINNED:
                    _, th, tw = bench_tile(variant, prec, st)
                else:
                    i = 17 if st == S.HEAD else max(st, 1)      # (the head: the last conv's tile; the stem: conv 1's)
                    th, tw = stage_tile(bil, (b, h, w), i, bool(stage_plan(cf, bil, prec, b, h, w, i)[0]))
                lv = 0 if st == S.HEAD else LEVEL[10 + 2 * S.UP.index(st)] if isinstance(st, str) else LEVEL[st]
                hl, wl = level_shape(h, w, lv)
                wins = stage_windows(st, th, tw, b, hl, wl)
                S.check_stage_windows(sd, st, held, wins, prec, WEIGHTS[prec], "fused" if st == 1 and fused else "tap",
                                      f"{variant} {b}x{h}x{w}{label}", cache, _REPORT, (th, tw),
                                      S.stage_family(st) + (" dither" if dither else "") + " @%dx%dx%d" % (b, h, w))
    finally:
        ctx.profile_enable(False)
        ctx.force_cfg(-1)
        model.set_options()
        model.precision = "fp32"


@pytest.mark.parametrize("variant,prec", CASES)
def test_every_stage_of_the_full_chip_launches_on_tile_windows(models, sds, caches, variant, prec):
    bil = VARIANTS[variant][2]
    stages = list(range(18)) + [S.HEAD]
    if not bil:
        for k, name in enumerate(S.UP):     # each half right before the concat conv it feeds
            stages.insert(stages.index(10 + 2 * k), name)
    run_windows(models[variant], sds[variant], variant, prec, frames_for(VARIANTS[variant][1]), caches[variant], stages,
                forms=True)


def test_bf16_stem_dither_per_element_at_the_pinned_shape(models, sds, caches):
    run_windows(models["gray"], sds["gray"], "gray", "bf16", frames_for(1), caches["gray"], [0, 1], dither=True)


def test_bf16_stem_dither_per_element_on_the_second_row_band(models, sds, caches):
    """1x135x240 cut at row 64: the band [64, 135) through forward_strip carries the pattern of rows 64.. of the image."""
    f1, f2 = O.make_frames(83, 1, 135, 240)
    run_windows(models["gray"], sds["gray"], "gray", "bf16", (f1[:, :, 64:].contiguous(), f2[:, :, 64:].contiguous()),
                caches["gray"], [0, 1], dither=True, strip=(64, 135), label=" band 64:135")
