"""GPU (MI355X): 4:2:2 / 4:4:4 YUV video - the raw route of `interpolate_video` byte for byte against
`interpolate_sequence_yuv` (and the resampling) on the same frames.

The clip is 7 frames of 37x53 (38x54 for the one-plane formats) with a hard cut before frame 4, made from an RGB clip by
the numpy restatement (tests/yuv4xx_ref.py).  For yuv422p10le (fp16), uyvy422 and yuv444p (bf16), at factor 2 and at
24 -> 60 fps with scene_cut 10: the whole-clip run and chunk_frames 3 write the same bytes; the originals are in them
byte for byte; the cut interval is held; the middles are `interpolate_sequence_yuv`'s."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import yuv4xx_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import retime, scene  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

N, CUT = 7, 4
CASES = [("yuv422p10le", "fp16", 37, 53), ("uyvy422", "bf16", 38, 54), ("yuv444p", "bf16", 37, 53)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def interp(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(O.make_interpolating_state_dict(n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield P.FrameInterpolator(model=m, device="cuda", batch=2)
    torch.cuda.empty_cache()


def _clip(fmt, h, w):
    """[N, F] frames of `fmt`: a moving texture with a hard cut (another texture) before frame CUT."""
    bits = R.FORMATS[fmt][0]
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(N):
        x = xx - 2 * t
        if t < CUT:
            r, g, b = (128 + 100 * np.sin(x / 5.0) * np.cos(yy / 7.0), 128 + 90 * np.cos((x + yy) / 6.0),
                       128 + 80 * np.sin((x - 0.5 * yy) / 4.0))
        else:
            r, g, b = (40 + 30 * np.cos(x / 3.0), 200 + 40 * np.sin(yy / 2.0), 60 + 50 * np.sin((x + 2 * yy) / 9.0))
        out.append(np.stack([r, g, b]))
    scale, top, dt = (1023 / 255, 1023, np.uint16) if bits == 10 else (1, 255, np.uint8)
    rgb = np.clip(np.rint(np.stack(out) * scale), 0, top).astype(dt)
    return R.rgb_to_yuv(rgb, fmt)


def _run(interp, d, name, fmt, **kw):
    n = interp.interpolate_video(str(d / "in.yuv"), str(d / name), **kw)
    data = np.frombuffer((d / name).read_bytes(), "<u2" if R.FORMATS[fmt][0] == 10 else np.uint8)
    return n, data.reshape(n, -1)


@pytest.mark.parametrize("fmt,prec,h,w", CASES)
def test_raw_route(interp, dev, tmp_path, fmt, prec, h, w):
    bits = R.FORMATS[fmt][0]
    m = interp.model
    m.precision = prec
    try:
        src = _clip(fmt, h, w)
        assert src.shape == (N, R.frame_samples(fmt, h, w))
        (tmp_path / "in.yuv").write_bytes(src.astype("<u2" if bits == 10 else np.uint8).tobytes())
        raw = dict(raw=fmt, width=w, height=h, src_fps=24)
        frames = torch.from_numpy(src.view(np.int16) if bits == 10 else src).to(dev)   # (the loops' device dtype)
        as_model = (lambda t: t.view(torch.uint16)) if bits == 10 else (lambda t: t)
        as_loop = (lambda t: t.view(torch.int16)) if bits == 10 else (lambda t: t)
        host = lambda t: as_loop(t).cpu().numpy().view(src.dtype)   # noqa: E731
        flags = scene.detect_cuts([frames], 10, bits)[1]
        assert flags.cpu().tolist() == [int(i == CUT - 1) for i in range(N - 1)]

        # factor 2
        want = host(P.interpolate_sequence_yuv(m, as_model(frames), h, w, fmt, 2, scene_cut=10))
        n, got = _run(interp, tmp_path, "f2.yuv", fmt, factor=2, scene_cut=10, **raw)
        assert n == 2 * N - 1 and got.shape == (n, src.shape[1])
        assert np.array_equal(got[0::2], src)                                  # the originals, byte for byte
        assert np.array_equal(got[2 * CUT - 1], src[CUT - 1])                  # the cut interval is held ...
        assert not np.array_equal(got[1], src[0])                              # ... the others are interpolated
        assert np.array_equal(got, want)
        free = host(P.interpolate_sequence_yuv(m, as_model(frames), h, w, fmt, 2))
        keep = [i for i in range(n) if i != 2 * CUT - 1]
        assert np.array_equal(got[keep], free[keep])                           # the middles are the sequence loop's
        n3, got3 = _run(interp, tmp_path, "f2_c3.yuv", fmt, factor=2, scene_cut=10, chunk_frames=3, **raw)
        assert n3 == n and np.array_equal(got3, got)

        # 24 -> 60 fps: the frames of a factor-4 bisection, the cut held, resampled to the times j * 2/5
        plan = retime.plan(24, 60, 2)
        t = as_model(frames)
        for _ in range(2):
            t = P.interpolate_sequence_yuv(m, t, h, w, fmt, 2)
        grid = scene.hold_cut_frames(as_loop(t), flags, 4)
        rows = retime.resample(grid, plan, 0, 0, plan.n_out(N), bits=bits, flags=flags)
        want = rows.cpu().numpy().view(src.dtype)
        n, got = _run(interp, tmp_path, "fps.yuv", fmt, fps=60, scene_cut=10, **raw)
        assert n == 16 == plan.n_out(N)
        assert np.array_equal(got[0::5], src[0::2])                            # times 0, 2, 4, 6 are source frames
        assert np.array_equal(got, want)
        n3, got3 = _run(interp, tmp_path, "fps_c3.yuv", fmt, fps=60, scene_cut=10, chunk_frames=3, **raw)
        assert n3 == n and np.array_equal(got3, got)
        assert not [p for p in tmp_path.iterdir() if p.name.endswith(".part")]
    finally:
        m.precision = "fp32"
