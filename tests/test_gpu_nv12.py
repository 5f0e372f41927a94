"""GPU (MI355X): NV12 / P010 decoder surfaces through the RGB (6->3) network.

Every comparison is bitwise.  The expected values come from the I420 / C420p10 path - tests/colour_ref.py,
tests/colour10_ref.py and the 4:2:0 entry points - and a numpy repack (tests/nv12_ref.py), never from the new kernels.

  1. fiunet_nv12_to_rgb_u8 / fiunet_rgb_to_nv12_u8 and the P010 pair against the references through the repack: every
     siting x matrix x range combination of the 4:2:0 tests, B = 3, at 49x67 (odd: the per-sample path, 2x1 / 1x2 / 1x1
     edge blocks), 48x64 (the 4-sample path), 5x1030 and 4x1032 (two workgroups along x, both paths)
  2. pitched surfaces: 48x64 at pitch 96 with an aligned chroma offset (4-sample path) and 49x67 at odd pitches; the
     encode leaves every sample outside the frame untouched
  3. P010 words: the low six bits of the input are ignored; every output word is code << 6
  4. forward_nv12 / forward_p010 == the repack of forward_yuv420 / forward_yuv420p10, tight and pitched, with and
     without out=; a gray context is refused
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour10_ref as C10  # noqa: E402
import colour_ref as C8  # noqa: E402
import nv12_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native  # noqa: E402
from ai_based_frame_interpolation_amd.colour import SurfaceLayout  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [(bits, dict(siting=s, matrix=m, colour_range=r))
          for bits, mats in ((8, ("bt601", "bt709")), (10, ("bt601", "bt709", "bt2020")))
          for s in ("jpeg", "mpeg2") for m in mats for r in ("limited", "full")]
COMBO_IDS = [f"{b}bit-{c['siting']}-{c['matrix']}-{c['colour_range']}" for b, c in COMBOS]
SHAPES = [(49, 67), (48, 64), (5, 1030), (4, 1032)]
TWO = [dict(siting="mpeg2", matrix="bt709", colour_range="limited"), dict(siting="jpeg", matrix="bt601", colour_range="full")]
GUARD = {8: 0xA5, 10: 0xA5A5}
# (h, w, layout): a decoder's padded surface (everything a multiple of 4: the 4-sample path) and odd pitches
PITCHED = [(48, 64, (96, 96 * 56, 96, 96 * 84 + 128)), (49, 67, (71, 49 * 71 + 3, 69, 49 * 71 + 3 + 24 * 69 + 68 + 5))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _api(bits):
    """(dtype, max code + 1, reference decode, reference encode, decode, encode, word shift)"""
    if bits == 8:
        return np.uint8, 256, C8.yuv420_to_rgb, C8.rgb_to_yuv420, P.nv12_to_rgb, P.rgb_to_nv12, 0
    return np.uint16, 1024, C10.yuv420p10_to_rgb, C10.rgb_to_yuv420p10, P.p010_to_rgb, P.rgb_to_p010, 6


def _random_i420(rng, b, h, w, hi, dt):
    """Random codes with a flat-chroma rectangle and a flat luma patch in every frame."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y = rng.integers(0, hi, (b, h, w)).astype(dt)
    u = rng.integers(0, hi, (b, hc, wc)).astype(dt)
    v = rng.integers(0, hi, (b, hc, wc)).astype(dt)
    u[:, hc // 4:hc // 2, wc // 4:wc // 2] = hi * 90 // 256
    v[:, hc // 4:hc // 2, wc // 4:wc // 2] = hi * 170 // 256
    y[:, h // 2:h // 2 + 8, w // 2:w // 2 + 8] = hi // 2
    return np.concatenate([y.reshape(b, -1), u.reshape(b, -1), v.reshape(b, -1)], axis=1)


def _random_rgb(rng, b, h, w, hi, dt):
    x = rng.integers(0, hi, (b, 3, h, w)).astype(dt)
    x[:, :, h // 4:h // 2, w // 4:w // 2] = (np.array([200, 40, 120]) * hi // 256).astype(dt)[:, None, None]
    x[:, :, h // 2:, :w // 8] = hi * 77 // 256   # grey
    return x


# ---- 1. the conversions, tight frames a stride apart ------------------------------------------------------------
@pytest.mark.parametrize("bits,opts", COMBOS, ids=COMBO_IDS)
def test_conversions_bit_exact_through_the_repack(dev, bits, opts):
    dt, hi, ref_dec, ref_enc, dec, enc, sh = _api(bits)
    for h, w in SHAPES:
        rng = np.random.default_rng(h * 7 + w + bits)
        b, fs = 3, R.tight(h, w)[3]
        # the 4-sample path needs a stride of a multiple of 4; the odd shapes get an odd one
        pad = 64 if w % 4 == 0 else 67
        codes = _random_i420(rng, b, h, w, hi, dt)
        src = np.full((b, fs + pad), GUARD[bits], dt)
        src[:, :fs] = R.i420_to_nv12(codes, h, w) << sh
        got = _np(dec(_dev(src, dev)[:, :fs], h, w, **opts))
        want = ref_dec(codes, h, w, **opts)
        assert got.dtype == dt and np.array_equal(got, want), (h, w, np.argwhere(got != want)[:5])
        rgb = _random_rgb(rng, b, h, w, hi, dt)
        dst = _dev(np.full((b, fs + pad), GUARD[bits], dt), dev)
        enc(_dev(rgb, dev), out=dst[:, :fs], **opts)
        res = _np(dst)
        want = R.i420_to_nv12(ref_enc(rgb, **opts), h, w) << sh
        assert np.array_equal(res[:, :fs], want), (h, w, np.argwhere(res[:, :fs] != want)[:5])
        assert (res[:, fs:] == GUARD[bits]).all(), (h, w)
        # no `out`: a new tight tensor
        assert np.array_equal(_np(enc(_dev(rgb, dev), **opts)), want), (h, w)


# ---- 2. pitched surfaces --------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,lay", PITCHED, ids=["48x64-pitch96", "49x67-odd-pitches"])
@pytest.mark.parametrize("bits", [8, 10])
def test_pitched_surfaces(dev, bits, h, w, lay):
    dt, hi, ref_dec, ref_enc, dec, enc, sh = _api(bits)
    rng = np.random.default_rng(h + w + bits)
    b = 3
    used = R.used_mask(h, w, lay)
    for opts in TWO:
        codes = _random_i420(rng, b, h, w, hi, dt)
        tight = R.i420_to_nv12(codes, h, w) << sh
        # the samples outside the frame hold noise: a kernel that read one would show it
        surf = rng.integers(0, 65536 if bits == 10 else 256, (b, lay[3])).astype(dt)
        surf[:, used] = tight
        got = _np(dec(_dev(surf, dev), h, w, layout=SurfaceLayout(*lay), **opts))
        want = ref_dec(codes, h, w, **opts)
        assert np.array_equal(got, want), np.argwhere(got != want)[:5]
        assert np.array_equal(got, _np(dec(_dev(tight, dev), h, w, **opts)))   # the tight result
        rgb = _random_rgb(rng, b, h, w, hi, dt)
        dst = _dev(np.full((b, lay[3]), GUARD[bits], dt), dev)
        enc(_dev(rgb, dev), out=dst, layout=SurfaceLayout(*lay), **opts)
        res = _np(dst)
        want = R.i420_to_nv12(ref_enc(rgb, **opts), h, w) << sh
        assert np.array_equal(res[:, used], want), np.argwhere(res[:, used] != want)[:5]
        assert (res[:, ~used] == GUARD[bits]).all(), np.argwhere(res[:, ~used] != GUARD[bits])[:5]
        # a surface made by the call: zeros outside the frame
        made = _np(enc(_dev(rgb, dev), layout=SurfaceLayout(*lay), **opts))
        assert np.array_equal(made[:, used], want) and not made[:, ~used].any()


def test_bad_layout_raises_before_any_launch(dev):
    f = torch.zeros(1, 96 * 84, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="luma_pitch"):
        P.nv12_to_rgb(f, 48, 64, layout=SurfaceLayout(60, 96 * 56, 96, 96 * 84))
    with pytest.raises(ValueError, match="frames must be uint8"):
        P.nv12_to_rgb(f, 48, 64)   # a pitched tensor without its layout
    with pytest.raises(_native.NativeError, match="surface layout"):
        _native.surface_to_rgb(f, SurfaceLayout(96, 100, 96, 96 * 84), torch.empty(1, 3, 48, 64, dtype=torch.uint8,
                                                                                     device=dev), 48, 64, 0, 8)


# ---- 3. P010 words --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(49, 67), (48, 64)])
def test_p010_bit_handling(dev, h, w):
    rng = np.random.default_rng(h * w)
    opts = dict(siting="mpeg2", matrix="bt2020", colour_range="limited")
    b = 2
    codes = _random_i420(rng, b, h, w, 1024, np.uint16)
    clean = R.i420_to_nv12(codes, h, w) << 6
    dirty = clean | rng.integers(0, 64, clean.shape).astype(np.uint16)
    assert (dirty != clean).any() and np.array_equal(dirty >> 6, clean >> 6)
    want = C10.yuv420p10_to_rgb(codes, h, w, **opts)
    assert np.array_equal(_np(P.p010_to_rgb(_dev(dirty, dev), h, w, **opts)), want)
    assert np.array_equal(_np(P.p010_to_rgb(_dev(clean | 63, dev), h, w, **opts)), want)
    rgb = _random_rgb(rng, b, h, w, 1024, np.uint16)
    words = _np(P.rgb_to_p010(_dev(rgb, dev), **opts))
    planar = _np(P.rgb_to_yuv420p10(_dev(rgb, dev), **opts))   # the C420p10 path's codes
    assert not (words & 63).any()
    assert np.array_equal(words >> 6, R.i420_to_nv12(planar, h, w))


# ---- 4. the forwards ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rgb_model(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield m
    del m
    torch.cuda.empty_cache()


IN_LAY, OUT_LAY = (96, 96 * 56, 96, 96 * 84), (80, 80 * 48 + 16, 72, 80 * 48 + 16 + 72 * 24 + 40)


@pytest.mark.parametrize("bits,prec", [(8, "bf16"), (8, "fp32"), (10, "fp16"), (10, "fp32")])
def test_forward_equals_the_repacked_420_forward(dev, rgb_model, bits, prec):
    dt, hi, _, _, _, _, sh = _api(bits)
    m = rgb_model
    m.precision = prec
    fwd = m.forward_nv12 if bits == 8 else m.forward_p010
    fwd420 = m.forward_yuv420 if bits == 8 else m.forward_yuv420p10
    try:
        for (b, h, w), lay, olay in (((2, 49, 67), None, None), ((1, 48, 64), IN_LAY, OUT_LAY)):
            rng = np.random.default_rng(b * h + w + bits)
            c1, c2 = (_random_i420(rng, b, h, w, hi, dt) for _ in range(2))
            for opts in TWO:
                want = R.i420_to_nv12(_np(fwd420(_dev(c1, dev), _dev(c2, dev), h, w, **opts)), h, w) << sh
                f1, f2 = (R.i420_to_nv12(c, h, w) << sh for c in (c1, c2))
                kw = dict(opts)
                if lay is not None:
                    f1, f2 = (R.to_surface(f, h, w, lay, 0x5A) for f in (f1, f2))
                    kw.update(layout=SurfaceLayout(*lay), out_layout=SurfaceLayout(*olay))
                else:
                    lay_t = olay_t = R.tight(h, w)
                used = R.used_mask(h, w, olay or olay_t)
                got = _np(fwd(_dev(f1, dev), _dev(f2, dev), h, w, **kw))
                assert got.shape == (b, (olay or olay_t)[3])
                assert np.array_equal(got[:, used], want), (prec, opts, int((got[:, used] != want).sum()))
                assert not got[:, ~used].any()
                out = _dev(np.full(got.shape, GUARD[bits], dt), dev)
                assert fwd(_dev(f1, dev), _dev(f2, dev), h, w, out=out, **kw) is out
                res = _np(out)
                assert np.array_equal(res[:, used], want) and (res[:, ~used] == GUARD[bits]).all()
        # siting None is "mpeg2"
        h, w = 48, 64
        f = _dev(R.i420_to_nv12(_random_i420(np.random.default_rng(1), 1, h, w, hi, dt), h, w) << sh, dev)
        assert torch.equal(fwd(f, f, h, w), fwd(f, f, h, w, siting="mpeg2"))
    finally:
        m.precision = "fp32"


def test_forward_nv12_into_every_second_frame(dev, rgb_model):
    """`out` as the video loop passes it: rows 2F apart."""
    b, h, w = 3, 48, 64
    rng = np.random.default_rng(3)
    f1, f2 = (_dev(R.i420_to_nv12(_random_i420(rng, b, h, w, 256, np.uint8), h, w), dev) for _ in range(2))
    first = rgb_model.forward_nv12(f1, f2, h, w)
    inter = torch.full((2 * b, f1.shape[1]), 0xA5, dtype=torch.uint8, device=dev)
    rgb_model.forward_nv12(f1, f2, h, w, out=inter[1::2])
    assert torch.equal(inter[1::2], first) and (inter[0::2] == 0xA5).all()


def test_gray_context_is_rejected(dev, seeded_sd):
    g = P.FrameInterpolationUNet(bilinear=True).to(dev).eval()
    g.load_state_dict(seeded_sd)
    f8 = torch.zeros(1, R.tight(32, 32)[3], dtype=torch.uint8, device=dev)
    f16 = torch.zeros(1, R.tight(32, 32)[3], dtype=torch.uint16, device=dev)
    with pytest.raises(RuntimeError, match="RGB"):
        g.forward_nv12(f8, f8, 32, 32)
    with pytest.raises(RuntimeError, match="RGB"):
        g.forward_p010(f16, f16, 32, 32)
    ctx = g._context(dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    lib = _native.lib()
    for fn, f in ((lib.fiunet_forward_nv12, f8), (lib.fiunet_forward_p010, f16)):
        rc = fn(ctx._h, f.data_ptr(), f.data_ptr(), None, f.data_ptr(), None, 1, 32, 32, 0, 0, ws.data_ptr(),
                ws.numel(), None)
        assert rc == _native.ERR_UNSUPPORTED
        assert b"RGB" in lib.fiunet_last_error_string()


def test_forward_refuses_a_bad_out_layout_before_the_first_launch(dev, rgb_model):
    f = torch.zeros(1, R.tight(32, 32)[3], dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="chroma_pitch"):
        rgb_model.forward_nv12(f, f, 32, 32, out_layout=SurfaceLayout(0, 0, 30, 0))
    ctx = rgb_model._context(dev)
    ws = rgb_model._workspace(ctx, dev, 1, 32, 32, 0, yuv=True)
    bad = ctypes.byref(_native.SurfaceLayout(0, 0, 30, 0))
    rc = _native.lib().fiunet_forward_nv12(ctx._h, f.data_ptr(), f.data_ptr(), None, f.data_ptr(), bad, 1, 32, 32, 0,
                                           0, ws.data_ptr(), ws.numel(), None)
    assert rc == 1 and b"chroma_pitch" in _native.lib().fiunet_last_error_string()
