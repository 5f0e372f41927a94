"""GPU (MI355X): packed RGB frames - rgb24, bgr24, rgba, bgra - through the RGB (6->3) network.

Every comparison is bitwise against tests/packed_ref.py, index shuffles in numpy plus the rounded alpha average; the
forward is compared with the chain of entry points it is defined as.

  1. packed_to_rgb / rgb_to_packed, all four formats, B = 3, at 3x5 (W just above one thread's 4 pixels), 37x53 (the
     byte path, an odd tail), 40x56 (the vector path), 6x1030 and 4x1028 (a second workgroup along x, both paths)
  2. pitched layouts: pitch W*bpp + 4 (the vector path stays), W*bpp + 3 and a frame stride that is no multiple of 4
     (both must take the byte path), frames further apart than a frame; every byte outside the pixels keeps its
     sentinel; a new pitched result starts as zeros
  3. bases one byte off a dword, W % 4 == 0: each pointer in turn - the choice of path includes the pointers
  4. alpha: 255, a copy, the rounded average; sources in a layout of their own; return_alpha
  5. bgr24 is rgb24 with the planes flipped
  6. forward_rgb_packed == packed_to_rgb x 2 -> forward_u8 -> rgb_to_packed(alpha_from=(f1, f2)), bf16 and fp16, tight and
     pitched, into every second row of a larger tensor
  7. refusals: dtype, shape, device, a gray model
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, packed  # noqa: E402
from ai_based_frame_interpolation_amd.packed import PackedLayout  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

FORMATS = list(R.BPP)
SHAPES = [(3, 5), (37, 53), (40, 56), (6, 1030), (4, 1028)]
B = 3
# (h, w, bytes added to the pitch, bytes added to the frame stride)
PITCHED = [(40, 56, 4, 8), (40, 56, 3, 5), (40, 56, 4, 6), (37, 53, 3, 0), (37, 53, 4, 8)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _rand(rng, *shape):
    return rng.integers(0, 256, shape).astype(np.uint8)


def _off_by_one(a, dev):
    """`a` on the device, contiguous, its first byte one past a dword boundary."""
    buf = torch.zeros(a.size + 8, dtype=torch.uint8, device=dev)
    v = buf[1:1 + a.size].view(a.shape)
    v.copy_(_dev(a, dev))
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


# ---- 1. tight frames ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("fmt", FORMATS)
def test_tight_frames(dev, fmt, h, w):
    rng = np.random.default_rng(h * 7 + w)
    fr = _rand(rng, B, h * w * R.BPP[fmt])
    want, want_a = R.unpack(fr, fmt, h, w)
    got = packed.packed_to_rgb(_dev(fr, dev), h, w, fmt)
    assert got.shape == (B, 3, h, w) and got.dtype == torch.uint8 and np.array_equal(_np(got), want)
    if want_a is not None:
        got, alpha = packed.packed_to_rgb(_dev(fr, dev), h, w, fmt, return_alpha=True)
        assert np.array_equal(_np(got), want) and np.array_equal(_np(alpha), want_a)
    rgb = _rand(rng, B, 3, h, w)
    out = packed.rgb_to_packed(_dev(rgb, dev), fmt)
    assert out.shape == (B, packed.frame_bytes(fmt, h, w)) and np.array_equal(_np(out), R.pack(rgb, fmt))
    # and the two are inverses
    assert np.array_equal(_np(packed.packed_to_rgb(out, h, w, fmt)), rgb)


# ---- 2. pitched layouts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,dp,ds", PITCHED, ids=[f"{h}x{w}+{dp}+{ds}" for h, w, dp, ds in PITCHED])
@pytest.mark.parametrize("fmt", FORMATS)
def test_pitched_layouts(dev, fmt, h, w, dp, ds):
    bpp = R.BPP[fmt]
    rp = w * bpp + dp
    lay = (rp, h * rp + ds)
    L = PackedLayout(*lay)
    rng = np.random.default_rng(h + w + dp + ds)
    rgb, alpha = _rand(rng, B, 3, h, w), (_rand(rng, B, h, w) if bpp == 4 else None)
    src = R.pack(rgb, fmt, lay, alpha, fill=0xA5)
    res = packed.packed_to_rgb(_dev(src, dev), h, w, fmt, layout=L, return_alpha=bpp == 4)
    if bpp == 4:
        assert np.array_equal(_np(res[1]), alpha)
        res = res[0]
    assert np.array_equal(_np(res), rgb)
    # into a sentinel-filled tensor whose frames lie further apart still
    big = torch.full((B, lay[1] + 12), 0x5A, dtype=torch.uint8, device=dev)
    out = big[:, :lay[1]]
    assert packed.rgb_to_packed(_dev(rgb, dev), fmt, layout=L, out=out) is out
    assert np.array_equal(_np(out), R.pack(rgb, fmt, lay, None, fill=0x5A))
    assert (big[:, lay[1]:] == 0x5A).all()
    # frames read from such a view
    big[:, :lay[1]] = _dev(src, dev)
    assert np.array_equal(_np(packed.packed_to_rgb(big[:, :lay[1]], h, w, fmt, layout=L)), rgb)
    # a result made by the call starts as zeros
    assert np.array_equal(_np(packed.rgb_to_packed(_dev(rgb, dev), fmt, layout=L)), R.pack(rgb, fmt, lay, None, fill=0))
    # the smallest stride: the last frame ends with its last pixel
    edge = (rp, (h - 1) * rp + w * bpp)
    got = packed.rgb_to_packed(_dev(rgb, dev), fmt, layout=PackedLayout(*edge))
    assert got.shape == (B, edge[1]) and np.array_equal(_np(got), R.pack(rgb, fmt, edge, None, fill=0))


# ---- 3. bases off a dword -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_misaligned_bases(dev, fmt):
    h, w = 40, 56
    bpp = R.BPP[fmt]
    rng = np.random.default_rng(11)
    fr, rgb = _rand(rng, B, h * w * bpp), _rand(rng, B, 3, h, w)
    want, _ = R.unpack(fr, fmt, h, w)
    assert np.array_equal(_np(packed.packed_to_rgb(_off_by_one(fr, dev), h, w, fmt)), want)          # the packed input
    out = _off_by_one(np.zeros((B, 3, h, w), np.uint8), dev)
    assert np.array_equal(_np(packed.packed_to_rgb(_dev(fr, dev), h, w, fmt, out=out)), want)         # the planes
    assert np.array_equal(_np(packed.rgb_to_packed(_off_by_one(rgb, dev), fmt)), R.pack(rgb, fmt))    # the planar input
    out = _off_by_one(np.full((B, h * w * bpp), 0x5A, np.uint8), dev)
    assert np.array_equal(_np(packed.rgb_to_packed(_dev(rgb, dev), fmt, out=out)), R.pack(rgb, fmt))  # the packed output
    if bpp == 4:                                                                                       # an alpha source
        a1, a2 = _rand(rng, B, h * w * 4), _rand(rng, B, h * w * 4)
        want = R.pack(rgb, fmt, alpha=R.alpha_average(R.unpack(a1, fmt, h, w)[1], R.unpack(a2, fmt, h, w)[1]))
        got = packed.rgb_to_packed(_dev(rgb, dev), fmt, alpha_from=(_dev(a1, dev), _off_by_one(a2, dev)))
        assert np.array_equal(_np(got), want)


# ---- 4. alpha -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(37, 53), (40, 56)], ids=["37x53", "40x56"])
@pytest.mark.parametrize("fmt", ["rgba", "bgra"])
def test_alpha_rules(dev, fmt, h, w):
    rng = np.random.default_rng(h)
    rgb, a1, a2 = _rand(rng, B, 3, h, w), _rand(rng, B, h * w * 4), _rand(rng, B, h * w * 4)
    a1[:, 3:64:4], a2[:, 3:64:4] = [255, 255, 0, 0] * 4, [255, 254, 1, 0] * 4   # the ends of the range, a tie that rounds up
    p1, p2 = R.unpack(a1, fmt, h, w)[1], R.unpack(a2, fmt, h, w)[1]
    d = _dev(rgb, dev)
    assert np.array_equal(_np(packed.rgb_to_packed(d, fmt)), R.pack(rgb, fmt, alpha=None))
    assert (_np(packed.rgb_to_packed(d, fmt))[:, 3::4] == 255).all()
    assert np.array_equal(_np(packed.rgb_to_packed(d, fmt, alpha_from=_dev(a1, dev))), R.pack(rgb, fmt, alpha=p1))
    assert np.array_equal(_np(packed.rgb_to_packed(d, fmt, alpha_from=(_dev(a2, dev),))), R.pack(rgb, fmt, alpha=p2))
    avg = R.alpha_average(p1, p2)
    assert avg[0, 0, :4].tolist() == [255, 255, 1, 0]
    got = packed.rgb_to_packed(d, fmt, alpha_from=(_dev(a1, dev), _dev(a2, dev)))
    assert np.array_equal(_np(got), R.pack(rgb, fmt, alpha=avg))
    # the sources in a layout of their own, the result in another
    for dp, ds in ((4, 8), (3, 1)):
        alay = (w * 4 + dp, h * (w * 4 + dp) + ds)
        olay = (w * 4 + 8, h * (w * 4 + 8))
        s1, s2 = (_dev(R.pack(R.unpack(a, fmt, h, w)[0], fmt, alay, p, fill=0xA5), dev) for a, p in ((a1, p1), (a2, p2)))
        got = packed.rgb_to_packed(d, fmt, layout=PackedLayout(*olay), alpha_from=(s1, s2), alpha_layout=PackedLayout(*alay))
        assert np.array_equal(_np(got), R.pack(rgb, fmt, olay, avg, fill=0))
    with pytest.raises(ValueError, match="alpha"):
        packed.rgb_to_packed(d, "rgb24", alpha_from=_dev(a1, dev))
    with pytest.raises(ValueError, match="alpha_from"):
        packed.rgb_to_packed(d, fmt, alpha_from=_dev(a1, dev)[:, :-4])


# ---- 5. the two byte orders ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", [("rgb24", "bgr24"), ("rgba", "bgra")], ids=["24", "32"])
def test_swapped_order_is_the_flipped_planes(dev, pair):
    h, w = 37, 53
    x = _dev(_rand(np.random.default_rng(5), B, h * w * R.BPP[pair[0]]), dev)
    assert torch.equal(packed.packed_to_rgb(x, h, w, pair[1]), packed.packed_to_rgb(x, h, w, pair[0]).flip(1))


# ---- 6. the forward -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rgb_model(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield m
    del m
    torch.cuda.empty_cache()


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_forward_is_the_chain(dev, rgb_model, fmt, prec):
    m = rgb_model
    m.precision = prec
    bpp = R.BPP[fmt]
    try:
        for (b, h, w), dp, ds in (((2, 40, 56), 0, 0), ((1, 33, 47), 0, 0), ((2, 40, 56), 4, 8), ((1, 33, 47), 3, 5)):
            rng = np.random.default_rng(b * h + w)
            lay = (w * bpp + dp, h * (w * bpp + dp) + ds)
            olay = (w * bpp + 2 * dp, h * (w * bpp + 2 * dp) + ds)
            pitched = bool(dp or ds)
            kw = dict(layout=PackedLayout(*lay), out_layout=PackedLayout(*olay)) if pitched else {}
            ckw = dict(layout=PackedLayout(*lay)) if pitched else {}
            f1, f2 = (_dev(R.pack(_rand(rng, b, 3, h, w), fmt, lay, _rand(rng, b, h, w), fill=0xA5), dev) for _ in range(2))
            mid = m.forward_u8(packed.packed_to_rgb(f1, h, w, fmt, **ckw), packed.packed_to_rgb(f2, h, w, fmt, **ckw))
            want = packed.rgb_to_packed(mid, fmt, layout=PackedLayout(*olay) if pitched else None,
                                        alpha_from=(f1, f2) if bpp == 4 else None,
                                        alpha_layout=PackedLayout(*lay) if pitched and bpp == 4 else None)
            got = m.forward_rgb_packed(f1, f2, h, w, format=fmt, **kw)
            assert got.shape == (b, olay[1]) and torch.equal(got, want), (fmt, prec, h, w, dp)
            # the pixels are the network's and the alpha the neighbours' rounded average, by the numpy restatement
            a = R.alpha_average(R.unpack(_np(f1), fmt, h, w, lay)[1], R.unpack(_np(f2), fmt, h, w, lay)[1]) if bpp == 4 else None
            assert np.array_equal(_np(got), R.pack(_np(mid), fmt, olay, a, fill=0))
            # into every second row of a larger sentinel-filled tensor, as the video loop passes `out`
            inter = torch.full((2 * b, olay[1] + 4), 0x5A, dtype=torch.uint8, device=dev)
            view = inter[1::2, :olay[1]]
            assert m.forward_rgb_packed(f1, f2, h, w, format=fmt, out=view, **kw) is view
            assert np.array_equal(_np(view), R.pack(_np(mid), fmt, olay, a, fill=0x5A))
            assert (inter[0::2] == 0x5A).all() and (inter[:, olay[1]:] == 0x5A).all()
        assert not torch.equal(mid, packed.packed_to_rgb(f1, h, w, fmt, **ckw))   # (the network did run)
    finally:
        m.precision = "fp32"


def test_forward_default_format_is_rgb24(dev, rgb_model):
    h, w = 32, 32
    f = _dev(_rand(np.random.default_rng(2), 1, h * w * 3), dev)
    assert torch.equal(rgb_model.forward_rgb_packed(f, f, h, w), rgb_model.forward_rgb_packed(f, f, h, w, format="rgb24"))


# ---- 7. refusals --------------------------------------------------------------------------------------------------
def test_bad_arguments_raise(dev, rgb_model):
    h, w = 32, 32
    f = torch.zeros(2, h * w * 3, dtype=torch.uint8, device=dev)
    rgb = torch.zeros(2, 3, h, w, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="uint8"):
        packed.packed_to_rgb(f.to(torch.int16), h, w, "rgb24")
    with pytest.raises(ValueError, match="frames of 32x32"):
        packed.packed_to_rgb(f, h, w, "rgba")
    with pytest.raises(ValueError, match="contiguous"):
        packed.packed_to_rgb(torch.zeros(h * w * 3, 2, dtype=torch.uint8, device=dev).t(), h, w, "rgb24")
    with pytest.raises(RuntimeError, match="GPU"):
        packed.packed_to_rgb(f.cpu(), h, w, "rgb24")
    with pytest.raises(ValueError, match="format"):
        packed.packed_to_rgb(f, h, w, "gbrp")
    with pytest.raises(ValueError, match="out must be"):
        packed.packed_to_rgb(f, h, w, "rgb24", out=torch.zeros(2, 3, h, w + 1, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match=r"\[B, 3, H, W\]"):
        packed.rgb_to_packed(rgb[:, :2], "rgb24")
    with pytest.raises(ValueError, match="uint8"):
        packed.rgb_to_packed(rgb.float(), "rgb24")
    with pytest.raises(RuntimeError, match="GPU"):
        packed.rgb_to_packed(rgb.cpu(), "rgb24")
    with pytest.raises(ValueError, match="out"):
        packed.rgb_to_packed(rgb, "rgb24", out=torch.zeros(2, h * w * 4, dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="row_pitch"):
        packed.rgb_to_packed(rgb, "rgb24", layout=PackedLayout(w * 3 - 1))
    m = rgb_model
    with pytest.raises(RuntimeError, match="expected two"):
        m.forward_rgb_packed(f, f[:1], h, w)
    with pytest.raises(RuntimeError, match="expected two"):
        m.forward_rgb_packed(f, f, h, w, format="bgra")
    with pytest.raises(RuntimeError, match="dtype"):
        m.forward_rgb_packed(f.to(torch.int8), f.to(torch.int8), h, w)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.forward_rgb_packed(f.cpu(), f.cpu(), h, w)
    with pytest.raises(ValueError, match="format"):
        m.forward_rgb_packed(f, f, h, w, format="rgb48le")
    with pytest.raises(ValueError, match="frame_stride"):
        m.forward_rgb_packed(f, f, h, w, out_layout=PackedLayout(w * 3 + 4, 100))
    with pytest.raises(ValueError, match="out must be"):
        m.forward_rgb_packed(f, f, h, w, out=torch.zeros(2, h * w * 3 + 1, dtype=torch.uint8, device=dev))


def test_gray_model_is_rejected(dev, seeded_sd):
    g = P.FrameInterpolationUNet(bilinear=True).to(dev).eval()
    g.load_state_dict(seeded_sd)
    f = torch.zeros(1, 32 * 32 * 3, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="RGB"):
        g.forward_rgb_packed(f, f, 32, 32)
    ctx = g._context(dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    lib = _native.lib()
    rc = lib.fiunet_forward_rgb_packed(ctx._h, f.data_ptr(), f.data_ptr(), None, f.data_ptr(), None, 1, 32, 32, 0, 0,
                                       ws.data_ptr(), ws.numel(), None)
    assert rc == _native.ERR_UNSUPPORTED and b"RGB" in lib.fiunet_last_error_string()
