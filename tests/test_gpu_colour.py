"""GPU (MI355X): colour 4:2:0 video through the RGB (6->3) network.

  1. fiunet_yuv420_to_rgb_u8 / fiunet_rgb_to_yuv420_u8 bit for bit against tests/colour_ref.py (all 8 siting x matrix x
     range combinations; odd sizes, where every edge rule is in play, and 48x64, where the 4-byte vector path runs;
     frames further apart than one frame, with the guard bytes between them untouched)
  2. fiunet_forward_yuv420 == yuv420_to_rgb -> forward_u8 -> rgb_to_yuv420 bit for bit (bf16, bf16x2, fp32; default
     options and unfused; 1x48x64, 2x530x950 where the persistent RGB stem runs several tiles per workgroup, and the
     benchmark's 8x1080x1920 in bf16, deterministic over two calls); a gray context is rejected
  3. fp32 against the CPU oracle through colour_ref's conversion (truncation-boundary flips only)
  4. FrameInterpolator.interpolate_video on colour Y4M with an RGB checkpoint
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_ref as C  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

COMBOS = [dict(siting=s, matrix=m, colour_range=r) for s in ("jpeg", "mpeg2") for m in ("bt601", "bt709")
          for r in ("limited", "full")]
COMBO_IDS = [f"{c['siting']}-{c['matrix']}-{c['colour_range']}" for c in COMBOS]
GUARD = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _random_i420(rng, b, h, w):
    """Random planes with a flat-chroma rectangle (and a flat luma patch) in every frame."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y = rng.integers(0, 256, (b, h, w), dtype=np.uint8)
    u = rng.integers(0, 256, (b, hc, wc), dtype=np.uint8)
    v = rng.integers(0, 256, (b, hc, wc), dtype=np.uint8)
    u[:, hc // 4:hc // 2, wc // 4:wc // 2] = 90
    v[:, hc // 4:hc // 2, wc // 4:wc // 2] = 170
    y[:, h // 2:h // 2 + 8, w // 2:w // 2 + 8] = 128
    return np.concatenate([y.reshape(b, -1), u.reshape(b, -1), v.reshape(b, -1)], axis=1)


def _random_rgb(rng, b, h, w):
    x = rng.integers(0, 256, (b, 3, h, w), dtype=np.uint8)
    x[:, :, h // 4:h // 2, w // 4:w // 2] = np.array([200, 40, 120], np.uint8)[:, None, None]
    x[:, :, h // 2:, :w // 8] = 77   # grey
    return x


# ---- 1. the conversion kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(49, 67), (48, 64), (1081, 1921)])
@pytest.mark.parametrize("opts", COMBOS, ids=COMBO_IDS)
def test_kernels_bit_exact_against_colour_ref(dev, opts, h, w):
    rng = np.random.default_rng(h * 7 + w + COMBOS.index(opts))
    b, fb = 3, C.frame_bytes(h, w)
    pad = 64 + 3 * (w & 1)   # frames further apart than one frame; odd sizes also get an odd stride
    # YUV -> RGB from frames `fb + pad` bytes apart
    yuv = _random_i420(rng, b, h, w)
    src = torch.full((b, fb + pad), GUARD, dtype=torch.uint8)
    src[:, :fb] = torch.from_numpy(yuv)
    got = P.yuv420_to_rgb(src.to(dev)[:, :fb], h, w, **opts).cpu().numpy()
    want = C.yuv420_to_rgb(yuv, h, w, **opts)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    # RGB -> YUV into frames `fb + pad` bytes apart: the guard bytes stay untouched
    rgb = _random_rgb(rng, b, h, w)
    dst = torch.full((b, fb + pad), GUARD, dtype=torch.uint8, device=dev)
    P.rgb_to_yuv420(torch.from_numpy(rgb).to(dev), out=dst[:, :fb], **opts)
    res = dst.cpu().numpy()
    want = C.rgb_to_yuv420(rgb, **opts)
    assert np.array_equal(res[:, :fb], want), np.argwhere(res[:, :fb] != want)[:5]
    assert (res[:, fb:] == GUARD).all()


# ---- 2. forward_yuv420 against the chain of the public calls ----------------------------------------------------
@pytest.fixture(scope="module")
def rgb_sd():
    return O.make_seeded_state_dict(77, n_channels=6, n_classes=3)


@pytest.fixture(scope="module")
def rgb_model(dev, rgb_sd):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(rgb_sd)
    m = m.to(dev).eval()
    yield m
    del m
    torch.cuda.empty_cache()


def _chain(m, f1, f2, h, w, opts):
    a = P.yuv420_to_rgb(f1, h, w, **opts)
    b = P.yuv420_to_rgb(f2, h, w, **opts)
    return P.rgb_to_yuv420(m.forward_u8(a, b), **opts)


CHAIN_OPTS = [dict(siting="jpeg", matrix="bt709", colour_range="limited"),
              dict(siting="mpeg2", matrix="bt601", colour_range="full")]


@pytest.mark.parametrize("unfused", [False, True], ids=["fused", "unfused"])
@pytest.mark.parametrize("shape", [(1, 48, 64), (2, 530, 950)], ids=["1x48x64", "2x530x950"])
@pytest.mark.parametrize("prec", ["bf16", "bf16x2", "fp32"])
def test_forward_yuv420_equals_public_chain(dev, rgb_model, prec, shape, unfused):
    b, h, w = shape
    rng = np.random.default_rng(b * h + w)
    f1 = torch.from_numpy(_random_i420(rng, b, h, w)).to(dev)
    f2 = torch.from_numpy(_random_i420(rng, b, h, w)).to(dev)
    m = rgb_model
    m.precision = prec
    m.set_options(unfused=unfused)
    try:
        for opts in CHAIN_OPTS:
            got = m.forward_yuv420(f1, f2, h, w, **opts)
            want = _chain(m, f1, f2, h, w, opts)
            assert got.shape == (b, C.frame_bytes(h, w))
            assert torch.equal(got, want), (prec, opts, int((got != want).sum()))
    finally:
        m.set_options()
        m.precision = "fp32"


def test_forward_yuv420_benchmark_shape_bf16_deterministic(dev, rgb_model):
    b, h, w = 8, 1080, 1920
    rng = np.random.default_rng(1080)
    f1 = torch.from_numpy(_random_i420(rng, b, h, w)).to(dev)
    f2 = torch.from_numpy(_random_i420(rng, b, h, w)).to(dev)
    m = rgb_model
    m.precision = "bf16"
    try:
        first = m.forward_yuv420(f1, f2, h, w).clone()
        assert torch.equal(m.forward_yuv420(f1, f2, h, w), first)
        assert torch.equal(_chain(m, f1, f2, h, w, dict()), first)
        # every second frame of an interleaved buffer, as the video loop passes it
        inter = torch.full((2 * b, C.frame_bytes(h, w)), GUARD, dtype=torch.uint8, device=dev)
        m.forward_yuv420(f1, f2, h, w, out=inter[1::2])
        assert torch.equal(inter[1::2], first) and (inter[0::2] == GUARD).all()
    finally:
        m.precision = "fp32"


def test_gray_context_is_rejected(dev, seeded_sd):
    g = P.FrameInterpolationUNet(bilinear=True).to(dev).eval()
    g.load_state_dict(seeded_sd)
    f = torch.zeros(1, C.frame_bytes(32, 32), dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="RGB"):
        g.forward_yuv420(f, f, 32, 32)
    ctx = g._context(dev)
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev)
    rc = _native.lib().fiunet_forward_yuv420(ctx._h, f.data_ptr(), f.data_ptr(), f.data_ptr(), 0, 1, 32, 32, 0, 0,
                                             ws.data_ptr(), ws.numel(), None)
    assert rc == _native.ERR_UNSUPPORTED
    assert b"RGB" in _native.lib().fiunet_last_error_string()


# ---- 3. against the CPU oracle -----------------------------------------------------------------------------------
def test_fp32_against_oracle_through_colour_ref(dev, rgb_model, rgb_sd):
    b, h, w = 1, 64, 96
    opts = dict(siting="jpeg", matrix="bt709", colour_range="limited")
    rng = np.random.default_rng(6496)
    y1, y2 = _random_i420(rng, b, h, w), _random_i420(rng, b, h, w)
    m = rgb_model
    m.precision = "fp32"
    got = m.forward_yuv420(torch.from_numpy(y1).to(dev), torch.from_numpy(y2).to(dev), h, w, **opts).cpu().numpy()

    def pre(rgb):
        return torch.from_numpy(2.0 * (rgb.astype(np.float32) / 255.0) - 1.0)

    ref = O.unet_forward(rgb_sd, pre(C.yuv420_to_rgb(y1, h, w, **opts)), pre(C.yuv420_to_rgb(y2, h, w, **opts)))
    rgb_out = (torch.clamp((ref + 1.0) / 2.0, 0.0, 1.0).numpy() * 255).astype(np.uint8)   # the oracle's truncating cast
    want = C.rgb_to_yuv420(rgb_out, **opts)
    diff = np.abs(got.astype(int) - want.astype(int))
    assert diff.max() <= 1 and (diff != 0).mean() <= 1e-3, (diff.max(), (diff != 0).mean())


# ---- 4. the video path -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interp(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(O.make_interpolating_state_dict(n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield P.FrameInterpolator(model=m, device="cuda")
    torch.cuda.empty_cache()


def _moving_texture(n, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        x = xx - 2 * t
        r = 128 + 100 * np.sin(x / 5.0) * np.cos(yy / 7.0)
        g = 128 + 90 * np.cos((x + yy) / 6.0)
        b = 128 + 80 * np.sin((x - 0.5 * yy) / 4.0)
        out.append(np.stack([r, g, b]))
    return np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)


def _write(path, packed, h, w, tag, rng):
    ny, nc = h * w, ((h + 1) // 2) * ((w + 1) // 2)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    IO.write_y4m(str(path), packed[:, :ny].reshape(-1, h, w),
                 (packed[:, ny:ny + nc].reshape(-1, hc, wc), packed[:, ny + nc:].reshape(-1, hc, wc)),
                 fps=(24, 1), colourspace=tag, colour_range=rng)


def _expected_middles(model, frames, h, w, batch, opts):
    """forward_yuv420 of every pair, batched as the sequence loop batches them: chunks of `batch` pairs, a ragged chunk
    padded (last pair repeated) to model.batch_invariant_from(h, w) pairs, or to `batch` where that is larger."""
    out = []
    n = frames.shape[0] - 1
    for s in range(0, n, batch):
        cnt = min(batch, n - s)
        a, b = frames[s:s + cnt], frames[s + 1:s + cnt + 1]
        if cnt < batch:
            bmin = model.batch_invariant_from(h, w)
            target = batch if bmin > batch else max(cnt, bmin)
            if target > cnt:
                a = torch.cat([a, a[-1:].repeat(target - cnt, 1)])
                b = torch.cat([b, b[-1:].repeat(target - cnt, 1)])
        out.append(model.forward_yuv420(a, b, h, w, **opts)[:cnt])
    return torch.cat(out)


VIDEO_CASES = [(48, 64, "420jpeg", None), (49, 67, "420jpeg", None), (48, 64, "420mpeg2", None),
               (49, 67, "420mpeg2", "FULL"), (48, 64, "420jpeg", "FULL")]


@pytest.mark.parametrize("h,w,tag,rng", VIDEO_CASES,
                         ids=[f"{h}x{w}-{t}-{r or 'norange'}" for h, w, t, r in VIDEO_CASES])
def test_interpolate_video_colour_y4m(tmp_path, dev, interp, h, w, tag, rng):
    opts = dict(siting="mpeg2" if tag == "420mpeg2" else "jpeg", matrix="bt709",
                colour_range="full" if rng == "FULL" else "limited")
    n = 5
    packed = C.rgb_to_yuv420(_moving_texture(n, h, w), **opts)
    src = tmp_path / "in.y4m"
    _write(src, packed, h, w, tag, rng)
    m = interp.model
    frames = torch.from_numpy(packed).to(dev)
    mids = _expected_middles(m, frames, h, w, interp.batch, opts).cpu().numpy()
    for factor in (2, 4):
        dst = tmp_path / f"out{factor}.y4m"
        cnt = interp.interpolate_video(str(src), str(dst), factor)
        out, hdr = IO.read_y4m_packed(str(dst))
        assert cnt == out.shape[0] == factor * (n - 1) + 1
        assert hdr["fps"] == (24 * factor, 1) and hdr["colourspace"] == tag and hdr["colour_range"] == rng
        assert (hdr["width"], hdr["height"]) == (w, h)
        assert np.array_equal(out[0::factor], packed)             # the originals, byte for byte
        if factor == 2:
            assert np.array_equal(out[1::2], mids)                # each middle is forward_yuv420 of its pair
            res2 = out
    # one pair shorter: the same frames (the ragged last chunk is padded, so no pair depends on the clip length)
    short = tmp_path / "short.y4m"
    _write(short, packed[:n - 1], h, w, tag, rng)
    interp.interpolate_video(str(short), str(tmp_path / "short_out.y4m"), 2)
    out_s, _ = IO.read_y4m_packed(str(tmp_path / "short_out.y4m"))
    assert np.array_equal(out_s, res2[:2 * (n - 1) - 1])
    # the bt601 keyword reaches the conversion
    bt601 = tmp_path / "bt601.y4m"
    interp.interpolate_video(str(src), str(bt601), 2, matrix="bt601")
    out6, _ = IO.read_y4m_packed(str(bt601))
    assert np.array_equal(out6[0::2], packed) and not np.array_equal(out6[1::2], mids)
