"""GPU (MI355X): 4:2:2 / 4:4:4 YUV frames - the conversions bit for bit against the numpy restatement
(tests/yuv4xx_ref.py) and against the 4:2:0 kernels where the identities hold, and `forward_yuv` bit for bit against the
public chain.

Sizes are the smallest that reach each path of csrc/yuv4xx.hip.h (a thread covers 4 luma columns, 128 threads a
workgroup): 49x67 odd, per-sample path, clamped last chroma column; 48x64 the vector path; 5x2050 more than one
workgroup across with a ragged last thread; the one-plane formats 50x66 (W % 4 == 2), 48x64 and 4x2052 (vector path, more
than one workgroup across), and a pitched layout whose unused bytes must stay untouched."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour10_ref as C10  # noqa: E402
import colour_ref as C8  # noqa: E402
import yuv4xx_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import colour, packed  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

PLANAR = ["yuv422p", "yuv444p", "yuv422p10le", "yuv444p10le"]
PACKED = ["uyvy422", "yuyv422"]
PLANAR_SIZES = [(49, 67), (48, 64), (5, 2050)]
PACKED_SIZES = [(50, 66), (48, 64), (4, 2052)]
SENTINEL = 0xA5


def _opts(fmt):
    """One matrix / range combination per depth: bt709 limited at 8 bits, bt2020 full at 10."""
    return dict(matrix="bt2020", colour_range="full") if R.FORMATS[fmt][0] == 10 else \
        dict(matrix="bt709", colour_range="limited")


def _sitings(fmt):
    return ["mpeg2"] if R.FORMATS[fmt][1] == "444" else ["jpeg", "mpeg2"]


CASES = [(f, s, h, w) for f in PLANAR for s in _sitings(f) for h, w in PLANAR_SIZES] + \
        [(f, s, h, w) for f in PACKED for s in _sitings(f) for h, w in PACKED_SIZES]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _rand(rng, shape, bits):
    """Random samples over the full code range; at 10 bits also words above 1023 (read as 1023)."""
    if bits == 8:
        return rng.integers(0, 256, shape).astype(np.uint8)
    x = rng.integers(0, 1024, shape)
    hot = rng.random(shape) < 0.05
    x[hot] = rng.integers(1024, 65536, int(hot.sum()))
    return x.astype(np.uint16)


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _np(t):
    return t.cpu().numpy()


# ---- decode and encode against the numpy restatement ---------------------------------------------------------------
@pytest.mark.parametrize("fmt,siting,h,w", CASES)
def test_decode_bitwise(dev, fmt, siting, h, w):
    bits = R.FORMATS[fmt][0]
    rng = np.random.default_rng(h * 1000 + w)
    fr = _rand(rng, (2, R.frame_samples(fmt, h, w)), bits)
    got = colour.yuv_to_rgb(_dev(fr, dev), h, w, fmt, siting=siting, **_opts(fmt))
    want = R.yuv_to_rgb(fr, h, w, fmt, siting, **_opts(fmt))
    assert got.shape == (2, 3, h, w) and np.array_equal(_np(got), want)


@pytest.mark.parametrize("fmt,siting,h,w", CASES)
def test_encode_bitwise(dev, fmt, siting, h, w):
    bits = R.FORMATS[fmt][0]
    rng = np.random.default_rng(h * 1000 + w + 1)
    rgb = _rand(rng, (2, 3, h, w), bits)
    got = colour.rgb_to_yuv(_dev(rgb, dev), fmt, siting=siting, **_opts(fmt))
    want = R.rgb_to_yuv(rgb, fmt, siting, **_opts(fmt))
    assert got.shape == want.shape and got.dtype == (torch.uint16 if bits == 10 else torch.uint8)
    assert np.array_equal(_np(got), want)


def test_planar_frame_stride(dev):
    """Frames further apart than one frame: the decode reads them where they are, the encode leaves the gap untouched
    (a stride that is no multiple of 4 samples also takes the per-sample path at a vector width)."""
    h, w = 6, 8
    rng = np.random.default_rng(3)
    for fmt in PLANAR:
        bits = R.FORMATS[fmt][0]
        f = R.frame_samples(fmt, h, w)
        for gap in (4, 3):
            buf = _rand(rng, (2, f + gap), bits)
            d = _dev(buf, dev)
            got = colour.yuv_to_rgb(d[:, :f], h, w, fmt, **_opts(fmt))
            assert np.array_equal(_np(got), R.yuv_to_rgb(buf[:, :f], h, w, fmt, **_opts(fmt)))
            rgb = _rand(rng, (2, 3, h, w), bits)
            out = _dev(buf, dev)
            colour.rgb_to_yuv(_dev(rgb, dev), fmt, out=out[:, :f], **_opts(fmt))
            res = _np(out)
            assert np.array_equal(res[:, :f], R.rgb_to_yuv(rgb, fmt, **_opts(fmt)))
            assert np.array_equal(res[:, f:], buf[:, f:])


@pytest.mark.parametrize("fmt", PACKED)
@pytest.mark.parametrize("siting", ["jpeg", "mpeg2"])
@pytest.mark.parametrize("h,w,pitch,extra", [(6, 64, 2 * 64 + 8, 12), (5, 66, 2 * 66 + 5, 3)])
def test_packed_pitched_layout(dev, fmt, siting, h, w, pitch, extra):
    """A capture buffer: rows a pitch apart (a multiple of 4: the vector path; odd: the per-sample path), frames a stride
    apart.  The decode reads only the used columns; the encode leaves every byte outside them as it was."""
    stride = h * pitch + extra
    lay = packed.PackedLayout(pitch, stride)
    rng = np.random.default_rng(w + pitch)
    y, u, v = (_rand(rng, s, 8) for s in ((2, h, w), (2, h, w // 2), (2, h, w // 2)))
    fr = R.pack422(y, u, v, fmt, pitch, stride, fill=SENTINEL)
    got = colour.yuv_to_rgb(_dev(fr, dev), h, w, fmt, siting=siting, layout=lay)
    assert np.array_equal(_np(got), R.planes_to_rgb(y, u, v, "422", 8, siting))
    rgb = _rand(rng, (2, 3, h, w), 8)
    out = torch.full((2, stride), SENTINEL, dtype=torch.uint8, device=dev)
    colour.rgb_to_yuv(_dev(rgb, dev), fmt, siting=siting, layout=lay, out=out)
    want = R.rgb_to_yuv(rgb, fmt, siting, row_pitch=pitch, frame_stride=stride, fill=SENTINEL)
    assert np.array_equal(_np(out), want)
    used = np.zeros(stride, bool)
    for r in range(h):
        used[r * pitch:r * pitch + 2 * w] = True
    assert (_np(out)[:, ~used] == SENTINEL).all() and (~used).sum() == stride - 2 * h * w
    # a tensor made by the call starts as zeros outside the used columns
    made = colour.rgb_to_yuv(_dev(rgb, dev), fmt, siting=siting, layout=lay)
    assert np.array_equal(_np(made), R.rgb_to_yuv(rgb, fmt, siting, row_pitch=pitch, frame_stride=stride, fill=0))


# ---- cross-checks with the kernels already trusted -----------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("siting", ["jpeg", "mpeg2"])
@pytest.mark.parametrize("h,w", [(49, 67), (48, 64)])
def test_422_decode_equals_the_420_kernel_on_column_constant_chroma(dev, bits, siting, h, w):
    rng = np.random.default_rng(h + w + bits)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y = _rand(rng, (2, h, w), bits)
    u1, v1 = _rand(rng, (2, 1, wc), bits), _rand(rng, (2, 1, wc), bits)
    f420 = R.join_planar(y, np.repeat(u1, hc, 1), np.repeat(v1, hc, 1))
    f422 = R.join_planar(y, np.repeat(u1, h, 1), np.repeat(v1, h, 1))
    fmt, dec420 = ("yuv422p10le", P.yuv420p10_to_rgb) if bits == 10 else ("yuv422p", P.yuv420_to_rgb)
    want = dec420(_dev(f420, dev), h, w, siting=siting, **_opts(fmt))
    got = colour.yuv_to_rgb(_dev(f422, dev), h, w, fmt, siting=siting, **_opts(fmt))
    assert np.array_equal(_np(got), _np(want))


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("siting", ["jpeg", "mpeg2"])
@pytest.mark.parametrize("h,w", [(50, 67), (48, 64)])
def test_422_encode_equals_the_420_kernel_on_equal_row_pairs(dev, bits, siting, h, w):
    rng = np.random.default_rng(h + w + bits)
    rgb = np.repeat(_rand(rng, (2, 3, h // 2, w), bits), 2, axis=2)
    fmt, enc420 = ("yuv422p10le", P.rgb_to_yuv420p10) if bits == 10 else ("yuv422p", P.rgb_to_yuv420)
    f420 = _np(enc420(_dev(rgb, dev), siting=siting, **_opts(fmt)))
    y, u, v = R.split_planar(_np(colour.rgb_to_yuv(_dev(rgb, dev), fmt, siting=siting, **_opts(fmt))), "422", h, w)
    hc, wc = h // 2, (w + 1) // 2
    assert np.array_equal(y.reshape(2, -1), f420[:, :h * w])
    assert np.array_equal(u[:, 0::2].reshape(2, -1), f420[:, h * w:h * w + hc * wc])
    assert np.array_equal(v[:, 0::2].reshape(2, -1), f420[:, h * w + hc * wc:])


@pytest.mark.parametrize("fmt", PACKED)
@pytest.mark.parametrize("siting", ["jpeg", "mpeg2"])
@pytest.mark.parametrize("h,w", [(50, 66), (48, 64)])
def test_packed_equals_planar_through_the_repack(dev, fmt, siting, h, w):
    rng = np.random.default_rng(h + w)
    planar = _rand(rng, (2, R.frame_samples("yuv422p", h, w)), 8)
    fr = R.pack422(*R.split_planar(planar, "422", h, w), fmt)
    a = colour.yuv_to_rgb(_dev(fr, dev), h, w, fmt, siting=siting)
    b = colour.yuv_to_rgb(_dev(planar, dev), h, w, "yuv422p", siting=siting)
    assert torch.equal(a, b)
    rgb = _dev(_rand(rng, (2, 3, h, w), 8), dev)
    p = _np(colour.rgb_to_yuv(rgb, fmt, siting=siting))
    q = _np(colour.rgb_to_yuv(rgb, "yuv422p", siting=siting))
    assert np.array_equal(R.join_planar(*R.unpack422(p, fmt, h, w)), q)


# ---- the forward ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rgb_model(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield m
    del m
    torch.cuda.empty_cache()


def _precisions(fmt):
    return ["bf16", "fp32"] + (["fp16"] if R.FORMATS[fmt][0] == 10 else [])


def _shapes(fmt):
    return [(1, 48, 64), (2, 38, 54) if R.FORMATS[fmt][1] == "packed" else (2, 37, 53)]


@pytest.mark.parametrize("fmt,prec", [(f, p) for f in PLANAR + PACKED for p in _precisions(f)])
def test_forward_yuv_equals_the_public_chain(dev, rgb_model, fmt, prec):
    """forward_yuv is bit for bit yuv_to_rgb x2 -> forward_u8 / forward_p10 -> rgb_to_yuv, fused and unfused."""
    bits = R.FORMATS[fmt][0]
    m = rgb_model
    m.precision = prec
    net = m.forward_p10 if bits == 10 else m.forward_u8
    try:
        for unfused in (False, True):
            m.set_options(unfused=unfused)
            for b, h, w in _shapes(fmt):
                rng = np.random.default_rng(b * 100 + h)
                f1, f2 = (_dev(_rand(rng, (b, R.frame_samples(fmt, h, w)), bits), dev) for _ in range(2))
                o = _opts(fmt)
                got = m.forward_yuv(f1, f2, h, w, format=fmt, **o)
                mid = net(colour.yuv_to_rgb(f1, h, w, fmt, **o), colour.yuv_to_rgb(f2, h, w, fmt, **o))
                want = colour.rgb_to_yuv(mid, fmt, **o)
                assert got.shape == f1.shape and got.dtype == f1.dtype
                assert np.array_equal(_np(got), _np(want)), (fmt, prec, unfused, b, h, w)
                assert not np.array_equal(_np(got), _np(f1))
    finally:
        m.set_options()
        m.precision = "fp32"


@pytest.mark.parametrize("fmt", ["yuv422p", "yuv444p10le", "uyvy422"])
def test_forward_yuv_into_every_second_frame(dev, rgb_model, fmt):
    """`out`: every second row of an interleaved result, as the sequence loop passes it; the rows between are untouched."""
    bits = R.FORMATS[fmt][0]
    m = rgb_model
    m.precision = "fp16" if bits == 10 else "bf16"
    try:
        b, h, w = 2, 38, 54
        f = R.frame_samples(fmt, h, w)
        rng = np.random.default_rng(5)
        f1, f2 = (_dev(_rand(rng, (b, f), bits), dev) for _ in range(2))
        keep = _rand(rng, (2 * b + 1, f), bits)
        video = _dev(keep.view(np.int16) if bits == 10 else keep, dev)
        view = video.view(torch.uint16) if bits == 10 else video
        res = m.forward_yuv(f1, f2, h, w, format=fmt, out=view[1::2])
        assert res.data_ptr() == view[1].data_ptr()
        got = _np(video).view(keep.dtype)
        assert np.array_equal(got[1::2], _np(m.forward_yuv(f1, f2, h, w, format=fmt)))
        assert np.array_equal(got[0::2], keep[0::2])
    finally:
        m.precision = "fp32"


def test_forward_yuv_pitched_out_layout(dev, rgb_model):
    m = rgb_model
    m.precision = "bf16"
    try:
        b, h, w = 1, 38, 54
        lay = packed.PackedLayout(2 * w + 12, h * (2 * w + 12) + 8)
        rng = np.random.default_rng(6)
        tight = [_rand(rng, (b, 2 * h * w), 8) for _ in range(2)]
        pitched = [R.pack422(*R.unpack422(t, "yuyv422", h, w), "yuyv422", lay.row_pitch, lay.frame_stride, SENTINEL)
                   for t in tight]
        want = m.forward_yuv(_dev(tight[0], dev), _dev(tight[1], dev), h, w, format="yuyv422")
        out = torch.full((b, lay.frame_stride), SENTINEL, dtype=torch.uint8, device=dev)
        m.forward_yuv(_dev(pitched[0], dev), _dev(pitched[1], dev), h, w, format="yuyv422", layout=lay, out_layout=lay,
                      out=out)
        y, u, v = R.unpack422(_np(want), "yuyv422", h, w)
        assert np.array_equal(_np(out), R.pack422(y, u, v, "yuyv422", lay.row_pitch, lay.frame_stride, SENTINEL))
    finally:
        m.precision = "fp32"


def test_grayscale_model_and_context_are_refused(dev):
    from ai_based_frame_interpolation_amd import _native
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=1).to(dev).eval()
    x = torch.zeros((1, 2 * 48 * 64), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="grayscale"):
        m.forward_yuv(x, x, 48, 64, format="yuv422p")
    ctx = _native.Context(dev.index or 0, frame_channels=1)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    lay = packed.PackedLayout(0, x.shape[1])
    for bits, t in ((8, x), (10, torch.zeros((1, 2 * 48 * 64), dtype=torch.int16, device=dev).view(torch.uint16))):
        with pytest.raises(_native.NativeError) as e:
            ctx.forward_yuv(t, t, 0, lay, t, lay, 48, 64, 0, _native.BF16, ws, bits)
        assert e.value.status == _native.ERR_UNSUPPORTED
    ctx.close()
