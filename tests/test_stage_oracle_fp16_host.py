"""CPU: the fp16 mode of oracle/stage_oracle.py, and that its per-element stage bound is not vacuous.

tests/test_gpu_bn_stats.py holds every fp16 stage of the device to
    |y - y_ref| <= 2^-11 |y_ref| + 2^-25 + 2^-14 M + E        (oracle.stage_oracle.stage_bound)
with y_ref from the device's own fp16 weights, subnormals kept.  Here, on the trained-like checkpoints at 1x32x48 and
without a GPU:
  - f16_rne_sat restates pack_f16x2 (clamp, round to nearest even, subnormals kept) on every half value, every
    midpoint between neighbours and values beyond the range;
  - the taps of the fp16 emulation (fp32 accumulation) and the rounded reference itself stay within the bound;
  - a "device" whose matrix unit reads every subnormal fp16 weight as zero breaks it, in every conv stage of every
    variant (4-25 % of a stage's folded weights are subnormal; the least affected stage, down4.3 of gray, still has
    over 400 of its 3 072 elements over the bound, by up to 80x) - so the GPU test does decide whether the subnormal weights
    reach the products;
  - one pixel column of a tap copied from its neighbour at x = 32, a tile seam, is rejected.
"""
import numpy as np
import pytest
import torch

from oracle import stage_oracle as S
from oracle import unet_oracle as O

VARIANTS = {"gray": (2, 1, True), "rgb": (6, 3, True), "convt": (2, 1, False)}
FRAME_SEED = 71


# ---- f16_rne_sat ---------------------------------------------------------------------------------------------------------
def _halves():
    h = np.arange(65536, dtype=np.uint16).view(np.float16)
    return h[np.isfinite(h)]


def test_f16_rne_sat_is_the_identity_on_every_half_value():
    h = _halves()
    got = S.f16_rne_sat(h.astype(np.float32))
    assert got.dtype == np.float32
    assert np.array_equal(got.astype(np.float16).view(np.uint16), h.view(np.uint16))      # bit for bit, -0 and subnormals too
    assert np.array_equal(got, h.astype(np.float32))
    inf = np.array([np.inf, -np.inf], dtype=np.float32)
    assert np.array_equal(S.f16_rne_sat(inf), np.array([65504.0, -65504.0], dtype=np.float32))


def test_f16_rne_sat_rounds_midpoints_to_even_and_their_neighbours_to_nearest():
    bits = np.arange(0x7BFF, dtype=np.uint16)                   # every non-negative finite half but the largest
    lo, hi = bits.view(np.float16).astype(np.float32), (bits + 1).view(np.float16).astype(np.float32)
    mid = (lo + hi) / np.float32(2)                             # exact in fp32: 12 significant bits
    assert np.array_equal(mid.astype(np.float64), (lo.astype(np.float64) + hi) / 2)
    even = np.where(bits & 1, hi, lo)
    for sign in (np.float32(1), np.float32(-1)):
        assert np.array_equal(S.f16_rne_sat(sign * mid), sign * even)
        assert np.array_equal(S.f16_rne_sat(sign * np.nextafter(mid, np.float32(0))), sign * lo)
        assert np.array_equal(S.f16_rne_sat(sign * np.nextafter(mid, np.float32(np.inf))), sign * hi)
        # numpy.float16 itself, where it does not overflow
        assert np.array_equal(S.f16_rne_sat(sign * mid), (sign * mid).astype(np.float16).astype(np.float32))
    # subnormals are kept, fp32 values below half the subnormal spacing go to zero
    tiny = np.array([2.0 ** -24, 2.0 ** -25, np.nextafter(np.float32(2.0 ** -25), np.float32(1)), 3 * 2.0 ** -25, 1e-40],
                    dtype=np.float32)
    assert np.array_equal(S.f16_rne_sat(tiny), np.array([2.0 ** -24, 0.0, 2.0 ** -24, 2.0 ** -23, 0.0], dtype=np.float32))


def test_f16_rne_sat_saturates_beyond_the_range():
    big = np.array([65504.0, np.nextafter(np.float32(65504), np.float32(1e9)), 65519.0, 65520.0, 65536.0, 1e5, 2e5, 3.4e38],
                   dtype=np.float32)
    for sign in (1.0, -1.0):
        got = S.f16_rne_sat(np.float32(sign) * big)
        assert np.array_equal(got, np.full_like(big, sign * 65504.0)), got
    # numpy alone would overflow to inf from 65520 on: the clamp is what pack_f16x2's v_med3_f32 does
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(65520.0).astype(np.float16))


def test_fp16_weights_are_the_fp32_fold_rounded_and_the_stem_stays_exact():
    sd = O.make_trained_like_state_dict(*VARIANTS["convt"])
    for stage in (1, 9, 16):
        w, sh = S.stage_weights(sd, stage, "fp16_rne")
        wb, shb = S.stage_weights(sd, stage, "bf16_rne")
        sc, _ = S.fold_bn(sd, stage, exact=False)
        p, ci, _ = S.STAGES[stage]
        w32 = sd[f"{p}.double_conv.{ci}.weight"].numpy().astype(np.float32) * sc.astype(np.float32)[:, None, None, None]
        assert np.array_equal(w, np.clip(w32, -65504, 65504).astype(np.float16).astype(np.float64))
        assert np.array_equal(sh, shb)                                       # the shift stays fp32
        sub = (np.abs(w) < 2.0 ** -14) & (w != 0)
        assert sub.any() and np.abs(w).max() < 65504                          # subnormals kept, nothing saturates
    w0, sh0 = S.stage_weights(sd, 0, "fp16_rne")
    e0, eh0 = S.stage_weights(sd, 0, "exact")
    assert np.array_equal(w0, e0) and np.array_equal(sh0, eh0)
    wt, _ = S.convt_weights(sd, 2, "fp16_rne")
    we, _ = S.convt_weights(sd, 2, "exact")
    assert wt.shape == we.shape
    assert np.array_equal(wt, we.astype(np.float32).astype(np.float16).astype(np.float64))


# ---- the stage bound on the emulation's taps -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emulated():
    """variant -> (state dict, taps of emulate_forward(..., "fp16") with fp32 accumulation + the head, weight cache)."""
    out = {}
    for v, (nc, ncl, bil) in VARIANTS.items():
        sd = O.make_trained_like_state_dict(nc, ncl, bil)
        f1, f2 = O.make_frames(FRAME_SEED, 1, 32, 48, c=ncl)
        taps = {}
        taps[S.HEAD] = S.emulate_forward(sd, f1, f2, "fp16", dtype=torch.float32, keep=taps)
        out[v] = (sd, taps, {})
    return out


def _stages(variant):
    return list(range(18)) + [S.HEAD] + ([] if VARIANTS[variant][2] else S.UP)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_emulation_taps_and_the_rounded_reference_are_within_the_fp16_bound(emulated, variant):
    sd, taps, cache = emulated[variant]
    for st in _stages(variant):
        S.check_stage(sd, st, taps, "fp16", "fp16_rne", label=f"{variant} emulation", cache=cache)
        y = S.stage_reference(sd, st, taps, "fp16_rne", cache=cache)[0]
        if isinstance(st, str) and st != S.HEAD:
            y = S._pad_to(y, taps[st])
        acts = dict(taps)
        acts[st if isinstance(st, str) else S.TAP[st]] = torch.from_numpy(S.f16_rne_sat(y.numpy().astype(np.float32)))
        _, _, _, ratio, _ = S.stage_error(sd, st, acts, "fp16", "fp16_rne", cache=cache)
        assert ratio.max().item() <= 1.0, (variant, st, ratio.max().item())


def test_emulation_stores_fp16_values_without_dither(emulated):
    sd, taps, _ = emulated["gray"]
    for i in range(17):
        t = taps[S.TAP[i]].numpy()
        assert np.array_equal(t, t.astype(np.float16).astype(np.float64)), S.TAP[i]
    f1, f2 = O.make_frames(FRAME_SEED, 1, 32, 48)
    assert torch.equal(taps["frame1"], f1.double())                          # no dither


def _flushed_stage(sd, st, taps, cache):
    """Elements over the bound when stage `st` is recomputed with every subnormal fp16 weight read as zero."""
    w, sh = S.stage_weights(sd, st, "fp16_rne", cache)
    sub = (np.abs(w) < 2.0 ** -14) & (w != 0)
    y = S.stage_reference(sd, st, taps, "fp16_rne", cache={(st, "fp16_rne"): (np.where(sub, 0.0, w), sh)})[0]
    acts = dict(taps)
    acts[S.TAP[st]] = torch.from_numpy(S.f16_rne_sat(y.numpy().astype(np.float32)))
    _, _, _, ratio, _ = S.stage_error(sd, st, acts, "fp16", "fp16_rne", cache=cache)
    return int((ratio > 1).sum()), float(sub.mean())


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_flushed_subnormal_weights_break_the_bound(emulated, variant):
    """Every conv stage 1-17 of every variant proves it at 32x48, frame seed 71 (the stem has exact weights): at least
    100 elements over the bound in each, where one stage per variant would do."""
    sd, taps, cache = emulated[variant]
    over = {}
    for st in range(1, 18):
        over[st], frac = _flushed_stage(sd, st, taps, cache)
        assert frac >= 0.03, (variant, st, frac)
    print(f"{variant}: elements over the fp16 bound with subnormal weights flushed, per stage: {over}")
    assert all(n >= 100 for n in over.values()), (variant, over)


@pytest.mark.parametrize("variant,stage", [("gray", 1), ("gray", 16), ("rgb", 17), ("convt", "unet.up4.up")])
def test_a_wrong_column_at_a_tile_seam_is_rejected(emulated, variant, stage):
    sd, taps, cache = emulated[variant]
    name = stage if isinstance(stage, str) else S.TAP[stage]
    acts = dict(taps)
    t = taps[name].clone()
    assert t.shape[3] == 48
    t[..., 32] = t[..., 31]
    acts[name] = t
    with pytest.raises(AssertionError, match=r"x=32\)"):
        S.check_stage(sd, stage, acts, "fp16", "fp16_rne", label="seam", cache=cache)
    S.check_stage(sd, stage, taps, "fp16", "fp16_rne", label="intact", cache=cache)
