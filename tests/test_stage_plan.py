"""CPU: the launch configuration of the conv stages as the forward launches them (csrc/fiunet.hip `plan_stages`: source
form, epilogue, tile family, K cut over workgroups, K cut over the waves of a workgroup) through the diagnostic entry point
`fiunet_debug_stage_cfg` - pure host arithmetic, no device call.  tests/test_cfg_rule.py pins the rule `choose_conv_cfg`
with its inputs given; this file pins the inputs the forward gives it.  What is pinned here is what callers rely on:
  * a problem that fills the chip keeps the whole K loop, and the tuned tiles except where their last partial round of
    workgroups would cost a whole one (direct convs and the >= 256-cout concat convs: levels 3-4 of one to four 1080p pairs,
    level 4 at eight);
  * a pair's K cuts never depend on the batch for frames of >= 1080p (bitwise batch invariance, include/fiunet.h);
  * ONE 256x256 pair - the reference's own operating point, /root/reference/model/inference.py:29,101-122 - takes the small
    tile on every layer, the in-workgroup cut on the direct convs with >= 4 planes in bf16, and in fp32 on the direct
    convs where it beats the best cut over workgroups (a concat conv through its materialised upsampled half);
  * every K cut is a power of two, at most the number of planes, and its slab fits - for both decoders, gray and RGB, and
    the option sets that change the launches."""
import ctypes

import pytest

from ai_based_frame_interpolation_amd import _native

FP32, BF16, BF16X2 = _native.FP32, _native.BF16, _native.BF16X2
# source forms (csrc/fiunet.hip SrcForm)
DIRECT, POOL, GATHER, UP, CONVT, UPCAT, STEM = range(7)
# output channels of convs 0..17 (csrc/fiunet_internal.h kCoutBil / kCoutCT: /root/reference/model/unet.py:65-82) and their level
COUT = {True: [64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 256, 256, 128, 128, 64, 64, 64],
        False: [64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64]}
LEVEL = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]
SKIP = {10: 7, 12: 5, 14: 3, 16: 1}   # concat convs: skip source; the low-res source is conv i - 1


def _cin(bilinear, i):
    cout = COUT[bilinear]
    if i in SKIP:
        return cout[SKIP[i]] + (cout[i - 1] if bilinear else cout[i - 1] // 2)
    return cout[i - 1]


@pytest.fixture(scope="module")
def stage():
    fn = _native.lib().fiunet_debug_stage_cfg
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]

    def call(prec, b, h, w, i, cf=1, bilinear=True, flags=0):
        out = (ctypes.c_int * 6)()
        assert fn(cf, int(bilinear), flags, prec, b, h, w, i, out) == 0
        return {"small": bool(out[0]), "ksplit": out[1], "kwave": bool(out[2]), "materialise": bool(out[3]),
                "form": out[4]}
    return call


def _levels(h, w):
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append(hs[-1] // 2); ws.append(ws[-1] // 2)
    return hs, ws


@pytest.mark.parametrize("prec", [FP32, BF16, BF16X2])
def test_stages_at_1080p_never_cut_k_and_tiles_follow_the_round_count(stage, prec):
    for b in (1, 2, 3, 4, 8, 16):
        for i in range(1, 18):
            lv, cout, cs = LEVEL[i], COUT[True][i], i in SKIP
            c = stage(prec, b, 1080, 1920, i)
            assert c["ksplit"] == 1 and not c["kwave"], (prec, b, i, c)     # bitwise batch invariance from B = 1
            # the tile never changes a bit, so it may follow the workgroup count: tuned tiles wherever the chip is full,
            # except where the tuned tile's last, partial round of workgroups would cost a whole one - the 512-cout concat
            # conv at level 3 included (two pairs: 1 088 tuned workgroups, 2.1 rounds)
            if b >= 2 and (lv <= 2 or cs):
                assert c["small"] == (b == 2 and i == 10), (prec, b, i, c)
            if b == 8 and lv == 4:
                assert c["small"], (b, i, c)      # 1 152 tuned workgroups = 2.25 rounds; 2 304 small ones = 3 full rounds
            if b == 1 and lv == 3 and not cs and cout == 512:
                assert c["small"], (b, i, c)      # 544 tuned workgroups on 512 slots


def test_stages_of_one_256x256_pair(stage):
    hs, ws = _levels(256, 256)
    n_kwave = n_kwave_fp32 = 0
    for i in range(1, 18):
        lv, cin, cout, cs = LEVEL[i], _cin(True, i), COUT[True][i], i in SKIP
        head_or_stem = i in (1, 17)
        for prec in (FP32, BF16, BF16X2):
            c = stage(prec, 1, 256, 256, i)
            assert c["small"], (i, prec, c)
            if prec == FP32 and cs:   # an fp32 concat conv is launched in the direct form exactly where that form takes the in-workgroup cut
                assert c["materialise"] == c["kwave"], (i, c)
            assert not (head_or_stem and (c["ksplit"] > 1 or c["kwave"]))
            k = c["ksplit"]
            assert k >= 1 and k & (k - 1) == 0 and k <= max(1, cin // (16 if prec == FP32 else 32) * (3 if prec == BF16X2 else 1))
            assert not (c["kwave"] and k > 1)
            if prec == BF16:
                n_kwave += c["kwave"]
                if cs:   # a concat conv takes the in-workgroup cut through its materialised upsampled half - or keeps the fused gather
                    assert c["materialise"] == c["kwave"], (i, c)
            if prec == FP32:
                n_kwave_fp32 += c["kwave"]
                if not head_or_stem and cin >= 128:   # one workgroup per CU, not more; two where the gather interpolates
                    assert c["ksplit"] * _small_blocks(1, hs[lv], ws[lv], cout) <= (512 if c["form"] == GATHER else 256)
    assert n_kwave >= 10 and n_kwave_fp32 >= 3


def _small_blocks(b, h, w, cout):
    return b * ((h + 7) // 8) * ((w + 31) // 32) * (cout // 64)


_FLAGS = {"default": 0, "unfused": _native.OPT_UNFUSED, "keep_all": _native.OPT_KEEP_ALL,
          "gather_upsample": _native.OPT_GATHER_UPSAMPLE}
_ARCHS = {"gray": (1, True), "gray_convt": (1, False), "rgb": (3, True)}
_SWEEP = [pytest.param(prec, *_ARCHS[a], _FLAGS[f], id=f"{prec}-{a}-{f}")
          for prec in (FP32, BF16, BF16X2) for a in _ARCHS for f in _FLAGS]


@pytest.mark.parametrize("prec,cf,bilinear,flags", _SWEEP)
def test_stage_cuts_are_sane_over_shapes_architectures_and_options(stage, prec, cf, bilinear, flags):
    for b in (1, 2, 5, 16):
        for h, w in ((16, 16), (17, 31), (64, 96), (135, 240), (270, 480), (360, 640), (720, 1280)):
            hs, ws = _levels(h, w)
            for i in range(2, 17):
                lv, cin, cout = LEVEL[i], _cin(bilinear, i), COUT[bilinear][i]
                c = stage(prec, b, h, w, i, cf, bilinear, flags)
                k = c["ksplit"]
                planes = cin // (16 if prec == FP32 else 32) * (3 if prec == BF16X2 else 1)
                assert k >= 1 and k & (k - 1) == 0 and k <= planes, (b, h, w, i, c)
                blocks = _small_blocks(b, hs[lv], ws[lv], cout) if c["small"] else None
                if c["small"] and k > 1:
                    assert k * blocks * 64 * 256 * 4 <= 64 << 20                          # the slab fits
                    # nobody cuts a launch that fills the chip (fp32 concat gathers - and the ablation path's concat convs
                    # that keep their configuration - two workgroups per CU)
                    assert blocks < (512 if prec == FP32 and c["form"] in (GATHER, UPCAT) else 256)
                if c["kwave"]:
                    assert cin // (16 if prec == FP32 else 32) >= 4 and c["form"] != GATHER
                    # one workgroup per CU (fp32: up to two rounds of them)
                    assert b * ((hs[lv] + 1) // 2) * ((ws[lv] + 31) // 32) * (cout // 64) <= (512 if prec == FP32 else 256)
