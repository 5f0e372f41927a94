"""GPU (MI355X): packed RGB video - the sequence loop and the raw route of `interpolate_video`, byte for
byte against the planar loops on the de-interleaved frames, re-interleaved in numpy (tests/packed_ref.py).

The clip is 7 frames of 37x53 with a hard cut before frame 4.
  8. interpolate_video(raw="rgb24") at factor 2 and at 24 -> 60 fps with scene_cut 10: the whole-clip run and
     chunk_frames 3 write the same bytes; the originals are in them byte for byte; they are `interpolate_sequence` (and
     the resampling) on the planar frames, re-interleaved
  9. the same for bgra at factor 4: the alpha of the inserted frames is the levelwise rounded average, the cut interval
     is held, alpha included
 10. the scene-cut scores of rgb24 frames are those of the planar stack; the sequence loop holds what they flag
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import retime, scene  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

H, W, N, CUT = 37, 53, 7, 4


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


@pytest.fixture(scope="module")
def clip():
    """(planar RGB [N, 3, H, W], alpha [N, H, W]): a moving texture with a hard cut (another texture) before frame CUT;
    the alpha is a ramp that moves too."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out, alpha = [], []
    for t in range(N):
        x = xx - 2 * t
        if t < CUT:
            r, g, b = (128 + 100 * np.sin(x / 5.0) * np.cos(yy / 7.0), 128 + 90 * np.cos((x + yy) / 6.0),
                       128 + 80 * np.sin((x - 0.5 * yy) / 4.0))
        else:
            r, g, b = (40 + 30 * np.cos(x / 3.0), 200 + 40 * np.sin(yy / 2.0), 60 + 50 * np.sin((x + 2 * yy) / 9.0))
        out.append(np.stack([r, g, b]))
        alpha.append(255 - 3 * np.abs(x) - t)
    as_u8 = lambda a: np.clip(np.rint(np.stack(a)), 0, 255).astype(np.uint8)   # noqa: E731
    return as_u8(out), as_u8(alpha)


def _planar_run(interp, dev, rgb, levels):
    """`levels` factor-2 passes of the planar loop, no cut handling: [(N-1) * 2**levels + 1, 3, H, W] on the device."""
    t = torch.from_numpy(rgb).to(dev)
    for _ in range(levels):
        t = P.interpolate_sequence(interp.model, t, 2)
    return t


def _run(interp, d, src, name, **kw):
    n = interp.interpolate_video(str(d / src), str(d / name), **kw)
    data = np.frombuffer((d / name).read_bytes(), np.uint8)
    return n, data


# ---- 8. rgb24 -----------------------------------------------------------------------------------------------------
def test_rgb24_raw_route(interp, dev, clip, tmp_path):
    rgb, _ = clip
    src = R.pack(rgb, "rgb24")
    (tmp_path / "in.rgb").write_bytes(src.tobytes())
    raw = dict(raw="rgb24", width=W, height=H, src_fps=24)
    planar = torch.from_numpy(rgb).to(dev)
    flags = scene.detect_cuts([planar], 10, 8)[1]
    assert flags.cpu().tolist() == [int(i == CUT - 1) for i in range(N - 1)]

    # factor 2
    want = R.pack(P.interpolate_sequence(interp.model, planar, 2, scene_cut=10).cpu().numpy(), "rgb24")
    n, got = _run(interp, tmp_path, "in.rgb", "f2.rgb", factor=2, scene_cut=10, **raw)
    assert n == 2 * N - 1 and got.size == n * src.shape[1]
    got = got.reshape(n, -1)
    assert np.array_equal(got[0::2], src)                                  # the originals, byte for byte
    assert np.array_equal(got[2 * CUT - 1], src[CUT - 1])                  # the cut interval is held ...
    assert not np.array_equal(got[1], src[0])                              # ... the others are interpolated
    assert np.array_equal(got, want)
    n3, got3 = _run(interp, tmp_path, "in.rgb", "f2_c3.rgb", factor=2, scene_cut=10, chunk_frames=3, **raw)
    assert n3 == n and np.array_equal(got3.reshape(n, -1), got)

    # 24 -> 60 fps: the frames of a factor-4 bisection, the cut held, resampled to the times j * 2/5
    plan = retime.plan(24, 60, 2)
    grid = scene.hold_cut_frames(_planar_run(interp, dev, rgb, 2), flags, 4)
    rows = retime.resample(grid, plan, 0, 0, plan.n_out(N), bits=8, flags=flags)
    want = R.pack(rows.cpu().numpy(), "rgb24")
    n, got = _run(interp, tmp_path, "in.rgb", "fps.rgb", fps=60, scene_cut=10, **raw)
    assert n == 16 == plan.n_out(N)
    got = got.reshape(n, -1)
    assert np.array_equal(got[0::5], src[0::2])                            # times 0, 2, 4, 6 are source frames
    assert np.array_equal(got, want)
    n3, got3 = _run(interp, tmp_path, "in.rgb", "fps_c3.rgb", fps=60, scene_cut=10, chunk_frames=3, **raw)
    assert n3 == n and np.array_equal(got3.reshape(n, -1), got)
    assert not [p for p in tmp_path.iterdir() if p.name.endswith(".part")]


# ---- 9. bgra ------------------------------------------------------------------------------------------------------
def test_bgra_raw_route_at_factor_4(interp, dev, clip, tmp_path):
    rgb, alpha = clip
    src = R.pack(rgb, "bgra", alpha=alpha)
    (tmp_path / "in.bgra").write_bytes(src.tobytes())
    raw = dict(raw="bgra", width=W, height=H, src_fps=24)
    # the scores count the alpha bytes: the cut is found on the packed frames
    flags = scene.detect_cuts([torch.from_numpy(src).to(dev)], 10, 8)[1].cpu().tolist()
    assert flags == [int(i == CUT - 1) for i in range(N - 1)]
    a = alpha
    for _ in range(2):   # levelwise: every inserted alpha plane is the rounded average of its two neighbours
        nxt = np.empty((2 * a.shape[0] - 1,) + a.shape[1:], np.uint8)
        nxt[0::2], nxt[1::2] = a, R.alpha_average(a[:-1], a[1:])
        a = nxt
    want = R.pack(_planar_run(interp, dev, rgb, 2).cpu().numpy(), "bgra", alpha=a)
    want[4 * (CUT - 1) + 1:4 * CUT] = want[4 * (CUT - 1)]                  # the hold, alpha included
    n, got = _run(interp, tmp_path, "in.bgra", "f4.bgra", factor=4, scene_cut=10, **raw)
    assert n == 4 * (N - 1) + 1
    got = got.reshape(n, -1)
    assert np.array_equal(got[0::4], src)
    assert np.array_equal(got[:, 3::4], want[:, 3::4])                     # the alpha bytes
    assert np.array_equal(got, want)
    n3, got3 = _run(interp, tmp_path, "in.bgra", "f4_c3.bgra", factor=4, scene_cut=10, chunk_frames=3, **raw)
    assert n3 == n and np.array_equal(got3.reshape(n, -1), got)


# ---- 10. scene cuts -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["rgb24", "bgr24"])
def test_scene_cut_scores_are_the_planar_stacks(interp, dev, clip, fmt):
    rgb, _ = clip
    planar = torch.from_numpy(rgb).to(dev)
    frames = torch.from_numpy(R.pack(rgb, fmt)).to(dev)
    s_planar, f_planar = scene.detect_cuts([planar], 10, 8)
    s_packed, f_packed = scene.detect_cuts([frames], 10, 8)
    assert torch.equal(s_packed, s_planar) and torch.equal(f_packed, f_planar) and int(f_planar.sum()) == 1
    got = P.interpolate_sequence_rgb_packed(interp.model, frames, H, W, fmt, 2, scene_cut=10)
    want = P.interpolate_sequence(interp.model, planar, 2, scene_cut=10)
    assert got.shape == (2 * N - 1, frames.shape[1])
    assert np.array_equal(got.cpu().numpy(), R.pack(want.cpu().numpy(), fmt))
    assert torch.equal(got[2 * CUT - 1], frames[CUT - 1])
