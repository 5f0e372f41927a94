"""GPU (MI355X): 10-bit video through both networks.

  1. pre10 bit for bit against numpy over all 65536 uint16 inputs; post10 over 100k values and the u8 test's edges
  2. fiunet_yuv420p10_to_rgb_p10 / fiunet_rgb_p10_to_yuv420p10 bit for bit against tests/colour10_ref.py (2 sitings x
     3 matrices x 2 ranges; odd sizes and 48x64, where the 8-byte vector path runs; frames further apart than one
     frame, with the guard samples between them untouched; samples above 1023 in the input)
  3. forward_p10 == postprocess_p10(forward(preprocess_p10(a), preprocess_p10(b))) bit for bit (gray and RGB; fp32,
     bf16, bf16x2; one unfused run; 2x530x950 RGB, where the persistent RGB stem runs several tiles per workgroup; a
     strided `out`), and forward_yuv420p10 == its chain of public calls
  4. fp32 and bf16x2 against the CPU oracle through pre10 / post10; bf16 by the rel-L2 bound of the bf16 tests
  5. FrameInterpolator.interpolate_video on C420p10 / Cmono10 (gray model) and C420p10 with bt2020 (RGB model)
  6. a sequence's middles do not depend on its length
Comparisons run on host copies: torch's uint16 has limited GPU support, so nothing here asks for a uint16 GPU kernel.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour10_ref as C  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [dict(siting=s, matrix=m, colour_range=r) for s in ("jpeg", "mpeg2") for m in ("bt601", "bt709", "bt2020")
          for r in ("limited", "full")]
COMBO_IDS = [f"{c['siting']}-{c['matrix']}-{c['colour_range']}" for c in COMBOS]
GUARD = 0xA5A5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---- 1. pre10 / post10 ----------------------------------------------------------------------------------------
def test_pre10_post10_bit_exact(dev):
    allv = np.arange(65536, dtype=np.uint16)
    pre = _np(_native.preprocess_p10(_dev(allv, dev)))
    assert np.array_equal(pre.view(np.uint32), C.pre10(allv).view(np.uint32))
    gen = torch.Generator().manual_seed(10)
    x = torch.cat([torch.rand(100000, generator=gen) * 3 - 1.5,
                   torch.tensor([-1.0, 1.0, 0.0, 0.999, -0.999, 1.5, -1.5, 0.0039, 0.00392157,
                                 1 / 1023, -1 + 2 / 1023, float("nan"), float("inf"), float("-inf")])])
    post = _np(_native.postprocess_p10(x.to(dev)))
    assert post.dtype == np.uint16 and np.array_equal(post, C.post10(x.numpy()))


# ---- 2. the conversion kernels --------------------------------------------------------------------------------
def _random_p10_frames(rng, b, h, w):
    """Random 10-bit planes with a flat-chroma rectangle, a flat luma patch and a few out-of-range samples."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y = rng.integers(0, 1024, (b, h, w), dtype=np.uint16)
    u = rng.integers(0, 1024, (b, hc, wc), dtype=np.uint16)
    v = rng.integers(0, 1024, (b, hc, wc), dtype=np.uint16)
    u[:, hc // 4:hc // 2, wc // 4:wc // 2] = 360
    v[:, hc // 4:hc // 2, wc // 4:wc // 2] = 680
    y[:, h // 2:h // 2 + 8, w // 2:w // 2 + 8] = 512
    f = np.concatenate([y.reshape(b, -1), u.reshape(b, -1), v.reshape(b, -1)], axis=1)
    f[:, ::97] = rng.integers(1024, 65536, f[:, ::97].shape, dtype=np.uint16)
    return f


def _random_rgb10(rng, b, h, w):
    x = rng.integers(0, 1024, (b, 3, h, w), dtype=np.uint16)
    x[:, :, h // 4:h // 2, w // 4:w // 2] = np.array([800, 160, 480], np.uint16)[:, None, None]
    x[:, :, h // 2:, :w // 8] = 300   # grey
    x[:, :, 0, ::13] = 2000
    return x


@pytest.mark.parametrize("h,w", [(49, 67), (48, 64), (17, 5)])
@pytest.mark.parametrize("opts", COMBOS, ids=COMBO_IDS)
def test_kernels_bit_exact_against_colour10_ref(dev, opts, h, w):
    rng = np.random.default_rng(h * 7 + w + COMBOS.index(opts))
    b, fs = 3, C.frame_samples(h, w)
    pad = 64 + 3 * (w & 1)   # frames further apart than one frame; odd sizes also get an odd stride
    yuv = _random_p10_frames(rng, b, h, w)
    src = np.full((b, fs + pad), GUARD, np.uint16)
    src[:, :fs] = yuv
    got = _np(P.yuv420p10_to_rgb(_dev(src, dev)[:, :fs], h, w, **opts))
    want = C.yuv420p10_to_rgb(yuv, h, w, **opts)
    assert got.dtype == np.uint16 and np.array_equal(got, want), np.argwhere(got != want)[:5]
    rgb = _random_rgb10(rng, b, h, w)
    dst = _dev(np.full((b, fs + pad), GUARD, np.uint16), dev)
    P.rgb_to_yuv420p10(_dev(rgb, dev), out=dst[:, :fs], **opts)
    res = _np(dst)
    want = C.rgb_to_yuv420p10(rgb, **opts)
    assert np.array_equal(res[:, :fs], want), np.argwhere(res[:, :fs] != want)[:5]
    assert (res[:, fs:] == GUARD).all()


# ---- 3. the forwards against their chains of public calls ------------------------------------------------------
@pytest.fixture(scope="module")
def models(dev):
    out = {}
    for cf, seed in ((1, 1234), (3, 77)):
        m = P.FrameInterpolationUNet(bilinear=True, frame_channels=cf)
        sd = O.make_seeded_state_dict(seed, n_channels=2 * cf, n_classes=cf)
        m.load_state_dict(sd)
        out[cf] = (m.to(dev).eval(), sd)
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _chain_p10(m, a, b):
    return _native.postprocess_p10(m(_native.preprocess_p10(a), _native.preprocess_p10(b)))


@pytest.mark.parametrize("prec", ["bf16", "bf16x2", "fp32"])
@pytest.mark.parametrize("cf,shape", [(1, (2, 48, 64)), (3, (1, 49, 67)), (3, (2, 530, 950))],
                         ids=["gray-2x48x64", "rgb-1x49x67", "rgb-2x530x950"])
def test_forward_p10_equals_public_chain(dev, models, prec, cf, shape):
    b, h, w = shape
    rng = np.random.default_rng(b * h + w + cf)
    a = rng.integers(0, 1024, (b, cf, h, w), dtype=np.uint16)
    c = rng.integers(0, 1024, (b, cf, h, w), dtype=np.uint16)
    a[..., 0, :7] = 4000   # above 1023: read as 1023 on both sides
    m = models[cf][0]
    m.precision = prec
    try:
        fa, fb = _dev(a, dev), _dev(c, dev)
        got = _np(m.forward_p10(fa, fb))
        want = _np(_chain_p10(m, fa, fb))
        assert got.dtype == np.uint16 and np.array_equal(got, want), (prec, int((got != want).sum()))
        assert got.max() <= 1023
        # every second image of an interleaved buffer, as the video loop passes it; the others stay untouched
        inter = _dev(np.full((2 * b, cf, h, w), GUARD, np.uint16), dev)
        m.forward_p10(fa, fb, out=inter[1::2])
        res = _np(inter)
        assert np.array_equal(res[1::2], want) and (res[0::2] == GUARD).all()
    finally:
        m.precision = "fp32"


@pytest.mark.parametrize("cf", [1, 3])
def test_forward_p10_unfused_equals_chain(dev, models, cf):
    b, h, w = 1, 48, 64
    rng = np.random.default_rng(cf)
    fa, fb = (_dev(rng.integers(0, 1024, (b, cf, h, w), dtype=np.uint16), dev) for _ in range(2))
    m = models[cf][0]
    m.precision = "bf16"
    m.set_options(unfused=True)
    try:
        assert np.array_equal(_np(m.forward_p10(fa, fb)), _np(_chain_p10(m, fa, fb)))
    finally:
        m.set_options()
        m.precision = "fp32"


def _yuv_chain(m, f1, f2, h, w, opts):
    a = P.yuv420p10_to_rgb(f1, h, w, **opts)
    b = P.yuv420p10_to_rgb(f2, h, w, **opts)
    return P.rgb_to_yuv420p10(m.forward_p10(a, b), **opts)


@pytest.mark.parametrize("prec", ["bf16", "bf16x2", "fp32"])
@pytest.mark.parametrize("shape", [(1, 48, 64), (2, 49, 67)], ids=["1x48x64", "2x49x67"])
def test_forward_yuv420p10_equals_public_chain(dev, models, prec, shape):
    b, h, w = shape
    rng = np.random.default_rng(b * h + w)
    f1, f2 = (_dev(_random_p10_frames(rng, b, h, w), dev) for _ in range(2))
    m = models[3][0]
    m.precision = prec
    try:
        for opts in (dict(siting="mpeg2", matrix="bt2020", colour_range="limited"),
                     dict(siting="jpeg", matrix="bt709", colour_range="full")):
            got = _np(m.forward_yuv420p10(f1, f2, h, w, **opts))
            want = _np(_yuv_chain(m, f1, f2, h, w, opts))
            assert got.shape == (b, C.frame_samples(h, w)) and np.array_equal(got, want), (prec, opts)
        fs = C.frame_samples(h, w)
        inter = _dev(np.full((2 * b, fs), GUARD, np.uint16), dev)
        m.forward_yuv420p10(f1, f2, h, w, out=inter[1::2])
        res = _np(inter)
        assert np.array_equal(res[1::2], _np(m.forward_yuv420p10(f1, f2, h, w))) and (res[0::2] == GUARD).all()
    finally:
        m.precision = "fp32"


def test_gray_context_is_rejected_by_forward_yuv420p10(dev, models):
    g = models[1][0]
    f = _dev(np.zeros((1, C.frame_samples(32, 32)), np.uint16), dev)
    with pytest.raises(RuntimeError, match="RGB"):
        g.forward_yuv420p10(f, f, 32, 32)
    ctx = g._context(dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    rc = _native.lib().fiunet_forward_yuv420p10(ctx._h, f.data_ptr(), f.data_ptr(), f.data_ptr(), 0, 1, 32, 32, 0, 0,
                                                ws.data_ptr(), ws.numel(), None)
    assert rc == _native.ERR_UNSUPPORTED
    # a short out_image_stride is an invalid argument (checked before any launch)
    fr = _dev(np.zeros((2, 1, 32, 32), np.uint16), dev)
    rc = _native.lib().fiunet_forward_p10(ctx._h, fr.data_ptr(), fr.data_ptr(), fr.data_ptr(), 100, 2, 32, 32, 0,
                                          ws.data_ptr(), ws.numel(), None)
    assert rc == 1


# ---- 4. against the CPU oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cf", [1, 3])
def test_against_oracle_through_pre10_post10(dev, models, cf):
    b, h, w = 1, 64, 96
    rng = np.random.default_rng(6496 + cf)
    a, c = (rng.integers(0, 1024, (b, cf, h, w), dtype=np.uint16) for _ in range(2))
    m, sd = models[cf]
    ref = O.unet_forward(sd, torch.from_numpy(C.pre10(a)), torch.from_numpy(C.pre10(c))).numpy()
    want = C.post10(ref).astype(int)
    yref = np.clip((ref.astype(np.float64) + 1) / 2, 0, 1) * 1023   # where the oracle sits between two codes
    try:
        for prec in ("fp32", "bf16x2", "bf16"):
            m.precision = prec
            got = _np(m.forward_p10(_dev(a, dev), _dev(c, dev))).astype(int)
            diff = np.abs(got - want)
            if prec == "fp32":
                assert diff.max() <= 1, prec
                # only pixels within a hair of a truncation boundary flip
                near = np.abs(yref - np.rint(yref)) <= 0.02
                assert near[diff != 0].all(), (prec, int((diff != 0).sum()))
            elif prec == "bf16x2":
                assert diff.max() <= 1, prec
            else:
                x_got = got / 1023.0 * 2 - 1
                x_ref = np.clip(ref, -1, 1)
                rel = np.linalg.norm(x_got - x_ref) / np.linalg.norm(x_ref)
                assert rel <= 2e-2, rel
    finally:
        m.precision = "fp32"


# ---- 5. the video path -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interps(dev):
    out = {}
    for cf in (1, 3):
        m = P.FrameInterpolationUNet(bilinear=True, frame_channels=cf, precision="bf16x2")
        m.load_state_dict(O.make_interpolating_state_dict(n_channels=2 * cf, n_classes=cf))
        out[cf] = P.FrameInterpolator(model=m.to(dev).eval(), device="cuda")
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _moving_texture10(n, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        x = xx - 2 * t
        r = 512 + 400 * np.sin(x / 5.0) * np.cos(yy / 7.0)
        g = 512 + 360 * np.cos((x + yy) / 6.0)
        b = 512 + 320 * np.sin((x - 0.5 * yy) / 4.0)
        out.append(np.stack([r, g, b]))
    return np.clip(np.rint(np.stack(out)), 0, 1023).astype(np.uint16)


def _expected(fwd, frames, model, h, w, batch):
    """`fwd` of every pair, batched as the sequence loops batch them (a ragged chunk padded by its last pair up to
    model.batch_invariant_from(h, w), or to `batch` where that is larger)."""
    out = []
    n = frames.shape[0] - 1
    for s in range(0, n, batch):
        cnt = min(batch, n - s)
        a, b = frames[s:s + cnt], frames[s + 1:s + cnt + 1]
        if cnt < batch:
            bmin = model.batch_invariant_from(h, w)
            target = batch if bmin > batch else max(cnt, bmin)
            if target > cnt:
                a = np.concatenate([a, np.repeat(a[-1:], target - cnt, axis=0)])
                b = np.concatenate([b, np.repeat(b[-1:], target - cnt, axis=0)])
        out.append(fwd(a, b)[:cnt])
    return np.concatenate(out)


def _split(packed, h, w, tag):
    ny = h * w
    n = packed.shape[0]
    if tag == "mono10":
        return packed[:, :ny].reshape(n, h, w), None
    hc, wc = (h + 1) // 2, (w + 1) // 2
    nc = hc * wc
    return packed[:, :ny].reshape(n, h, w), (packed[:, ny:ny + nc].reshape(n, hc, wc),
                                             packed[:, ny + nc:].reshape(n, hc, wc))


@pytest.mark.parametrize("h,w,tag,rng", [(48, 64, "420p10", None), (49, 67, "420p10", "FULL"),
                                         (48, 64, "mono10", "LIMITED")])
def test_interpolate_video_p10_gray(tmp_path, dev, interps, h, w, tag, rng):
    interp = interps[1]
    m = interp.model
    n = 5
    texture = _moving_texture10(n, h, w)
    packed = C.rgb_to_yuv420p10(texture, "mpeg2", "bt2020")
    if tag == "mono10":
        packed = packed[:, :h * w]
    src = tmp_path / "in.y4m"
    y, ch = _split(packed, h, w, tag)
    IO.write_y4m_p10(str(src), y, ch, fps=(24, 1), colourspace=tag, colour_range=rng)
    mids = _expected(lambda a, b: _np(m.forward_p10(_dev(a[:, None], dev), _dev(b[:, None], dev)))[:, 0],
                     y, m, h, w, interp.batch)
    for factor in (2, 4):
        dst = tmp_path / f"out{factor}.y4m"
        cnt = interp.interpolate_video(str(src), str(dst), factor)
        yo, cho, fps, cs = IO.read_y4m_p10(str(dst))
        _, hdr = IO.read_y4m_packed_p10(str(dst))
        assert cnt == yo.shape[0] == factor * (n - 1) + 1
        assert fps == (24 * factor, 1) and cs == tag and hdr["colour_range"] == rng
        assert np.array_equal(yo[0::factor], y)
        if ch is not None:
            for c, co in zip(ch, cho):
                assert np.array_equal(co[0::factor], c)
                if factor == 2:
                    avg = (c[:-1].astype(np.int32) + c[1:].astype(np.int32) + 1) >> 1
                    assert np.array_equal(co[1::2], avg)
        if factor == 2:
            assert np.array_equal(yo[1::2], mids)


def test_interpolate_video_p10_rgb_bt2020(tmp_path, dev, interps):
    interp = interps[3]
    m = interp.model
    h, w, n = 49, 67, 5
    opts = dict(siting="mpeg2", matrix="bt2020", colour_range="limited")
    packed = C.rgb_to_yuv420p10(_moving_texture10(n, h, w), **opts)
    src = tmp_path / "in.y4m"
    y, ch = _split(packed, h, w, "420p10")
    IO.write_y4m_p10(str(src), y, ch, fps=(50, 1))
    mids = _expected(lambda a, b: _np(m.forward_yuv420p10(_dev(a, dev), _dev(b, dev), h, w, **opts)),
                     packed, m, h, w, interp.batch)
    for factor in (2, 4):
        dst = tmp_path / f"out{factor}.y4m"
        cnt = interp.interpolate_video(str(src), str(dst), factor, matrix="bt2020")
        out, hdr = IO.read_y4m_packed_p10(str(dst))
        assert cnt == out.shape[0] == factor * (n - 1) + 1
        assert hdr["fps"] == (50 * factor, 1) and hdr["colourspace"] == "420p10" and hdr["colour_range"] is None
        assert np.array_equal(out[0::factor], packed)
        if factor == 2:
            assert np.array_equal(out[1::2], mids)
            res2 = out
    # siting="jpeg" reaches the conversion
    jp = tmp_path / "jpeg.y4m"
    interp.interpolate_video(str(src), str(jp), 2, matrix="bt2020", siting="jpeg")
    outj, _ = IO.read_y4m_packed_p10(str(jp))
    assert np.array_equal(outj[0::2], packed) and not np.array_equal(outj[1::2], res2[1::2])


# ---- 6. independence of the sequence length ------------------------------------------------------------------------
def test_sequence_middles_do_not_depend_on_length(dev, interps):
    h, w = 48, 64
    texture = _moving_texture10(7, h, w)
    m3 = interps[3].model
    packed = _dev(C.rgb_to_yuv420p10(texture, "mpeg2", "bt709"), dev)
    long = _np(P.interpolate_sequence_yuv420p10(m3, packed, h, w, batch=4, siting="mpeg2"))
    for n in (2, 3, 5):
        short = _np(P.interpolate_sequence_yuv420p10(m3, packed[:n].contiguous(), h, w, batch=4, siting="mpeg2"))
        assert np.array_equal(short, long[:2 * n - 1]), n
    m1 = interps[1].model
    luma = _dev(texture[:, 1], dev)
    long = _np(P.interpolate_sequence_p10(m1, luma, batch=4))
    assert long.shape == (13, h, w) and np.array_equal(long[0::2], texture[:, 1])
    for n in (2, 5):
        assert np.array_equal(_np(P.interpolate_sequence_p10(m1, luma[:n].contiguous(), batch=4)), long[:2 * n - 1]), n
