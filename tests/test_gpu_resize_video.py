"""GPU (MI355X): `resize=` on the video routes and on hold-out scoring (stream.py, holdout.py).

The contract is byte identity with the route that has no resize: `interpolate_video(resize=)` writes what "resize every
frame with tests/resize_ref.py on the host, write that clip, run `interpolate_video` on it" writes - for every format, for
chunk_frames 1 and 3 and the whole-clip call, with factor 4 + scene_cut and with fps + dedup - and `score_video(resize=)`
gives the per-frame arrays of `score_video` on the pre-resized clip.  Frames are 52x70 -> 40x48."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import holdout  # noqa: E402
from ai_based_frame_interpolation_amd import imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
RS = P.resize
SRC, DST = (52, 70), (40, 48)        # (h, w): even widths for uyvy422, chroma planes of 26x35 -> 20x24
SIZE = (DST[1], DST[0])              # (width, height), as resize= takes it
THR = 10.0

#: name -> (frame kind of resize.frame_planes, bits, network channels, file extension)
FORMATS = {"y4m-gray": (("y4m", "420jpeg"), 8, 1, ".y4m"), "y4m-mono": (("y4m", "mono"), 8, 1, ".y4m"),
           "y4m-rgb": (("y4m", "420jpeg"), 8, 3, ".y4m"), "y4m-p10": (("y4m", "420p10"), 10, 3, ".y4m"),
           "npy": ("npy", 8, 1, ".npy"), "npy-rgb": (("npy", 3), 8, 3, ".npy"), "nv12": ("nv12", 8, 3, ".raw"),
           "rgb24": ("rgb24", 8, 3, ".raw"), "bgra": ("bgra", 8, 3, ".raw"), "yuv422p10le": ("yuv422p10le", 10, 3, ".raw"),
           "uyvy422": ("uyvy422", 8, 3, ".raw")}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    cache = {}

    def get(fc):
        if fc not in cache:
            m = P.FrameInterpolationUNet(bilinear=True, frame_channels=fc, precision="bf16")
            m.load_state_dict(O.make_seeded_state_dict(1234) if fc == 1 else
                              O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
            cache[fc] = m.to(dev).eval()
        return cache[fc]
    return get


def _pictures(pattern, samples, bits, seed, noise=3):
    """One row of `samples` samples per letter: a random picture per scene ("|" starts a new one), each letter its own
    small noise on it; equal letters are equal frames."""
    rng = np.random.default_rng(seed)
    hi, dt = (256, np.uint8) if bits == 8 else (1024, np.uint16)
    base, made, out = rng.integers(0, hi, samples), {}, []
    for ch in pattern:
        if ch == "|":
            base = rng.integers(0, hi, samples)
            continue
        if ch not in made:
            made[ch] = np.clip(base + rng.integers(-noise, noise + 1, samples), 0, hi - 1).astype(dt)
        out.append(made[ch])
    return np.stack(out)


def _write(path, name, rows, hw):
    """rows [N, frame samples] of `name` frames of hw = (h, w) -> the file at `path`; returns interpolate_video's keywords."""
    kind, bits, _, _ = FORMATS[name]
    h, w = hw
    if name.startswith("y4m"):
        with IO.Y4MWriter(path, w, h, (24, 1), kind[1], None, bits=bits) as wr:
            wr.write(rows)
        return {}
    if name.startswith("npy"):
        np.save(path, rows.reshape((-1, h, w) if kind == "npy" else (-1, h, w, kind[1])))
        return dict(src_fps=Fraction(24))
    rows.tofile(path)
    return dict(raw=kind, width=w, height=h, src_fps=Fraction(24))


def _clips(tmp_path, name, pattern, seed=1):
    """The source clip and the clip resized on the host -> (source path, its keywords, resized path, its keywords)."""
    kind, bits, _, ext = FORMATS[name]
    sp, dp = RS.frame_planes(kind, *SRC), RS.frame_planes(kind, *DST)
    rows = _pictures(pattern, RS.frame_samples(sp), bits, seed)
    small = R.resize_rows(rows, sp, dp, RS.frame_samples(dp), bits)
    src, pre = str(tmp_path / ("src" + ext)), str(tmp_path / ("pre" + ext))
    return src, _write(src, name, rows, SRC), pre, _write(pre, name, small, DST)


def _same_file(a, b, what):
    x, y = open(a, "rb").read(), open(b, "rb").read()
    assert len(x) == len(y), (what, len(x), len(y))
    assert x == y, (what, "first difference at byte", next(i for i, (p, q) in enumerate(zip(x, y)) if p != q))


@pytest.mark.parametrize("name", list(FORMATS))
def test_resize_equals_the_pre_resized_route(dev, models, tmp_path, name):
    _, _, fc, ext = FORMATS[name]
    src, kw, pre, kw_pre = _clips(tmp_path, name, "ABCDE")
    fi = P.FrameInterpolator(model=models(fc), device=dev)
    ref = str(tmp_path / ("ref" + ext))
    n_ref = fi.interpolate_video(pre, ref, 2, **kw_pre)
    assert n_ref == 9
    for cf in (None, 1, 3):
        got = str(tmp_path / (f"got{cf}" + ext))
        assert fi.interpolate_video(src, got, 2, chunk_frames=cf, resize=SIZE, **kw) == n_ref
        _same_file(got, ref, (name, cf))
    if ext == ".y4m":
        with IO.Y4MReader(ref) as rd:
            assert (rd.header["width"], rd.header["height"]) == SIZE


@pytest.mark.parametrize("name", ["y4m-gray", "nv12"])
def test_resize_with_factor_4_and_scene_cut(dev, models, tmp_path, name):
    _, _, fc, ext = FORMATS[name]
    src, kw, pre, kw_pre = _clips(tmp_path, name, "ABC|DEF", seed=2)
    fi = P.FrameInterpolator(model=models(fc), device=dev)
    ref, log = str(tmp_path / ("ref" + ext)), []
    n_ref = fi.interpolate_video(pre, ref, 4, scene_cut=THR, scene_log=log, **kw_pre)
    assert n_ref == 21 and np.concatenate([f for _, f in log]).astype(bool).tolist() == [False, False, True, False, False]
    for cf in (None, 1, 3):
        got, log = str(tmp_path / (f"got{cf}" + ext)), []
        assert fi.interpolate_video(src, got, 4, chunk_frames=cf, scene_cut=THR, scene_log=log, resize=SIZE, **kw) == n_ref
        _same_file(got, ref, (name, cf))
        assert np.concatenate([f for _, f in log]).astype(bool).tolist() == [False, False, True, False, False]


@pytest.mark.parametrize("name", ["npy", "rgb24"])
def test_resize_with_fps_and_dedup(dev, models, tmp_path, name):
    _, _, fc, ext = FORMATS[name]
    src, kw, pre, kw_pre = _clips(tmp_path, name, "AABCCCDE", seed=3)
    fi = P.FrameInterpolator(model=models(fc), device=dev)
    ref, log = str(tmp_path / ("ref" + ext)), []
    n_ref = fi.interpolate_video(pre, ref, fps=60, dedup=0, dedup_log=log, **kw_pre)
    dead = np.concatenate([d for _, d in log]).tolist()
    assert dead == [True, False, False, True, True, False, False]   # equal frames stay equal through the resize
    for cf in (None, 1, 3):
        got, log = str(tmp_path / (f"got{cf}" + ext)), []
        assert fi.interpolate_video(src, got, chunk_frames=cf, fps=60, dedup=0, dedup_log=log, resize=SIZE, **kw) == n_ref
        _same_file(got, ref, (name, cf))
        assert np.concatenate([d for _, d in log]).tolist() == dead


@pytest.mark.parametrize("name", ["y4m-gray", "y4m-p10", "npy-rgb", "bgra", "uyvy422"])
def test_resize_to_the_source_size_changes_nothing(dev, models, tmp_path, name):
    _, _, fc, ext = FORMATS[name]
    src, kw, _, _ = _clips(tmp_path, name, "ABCD", seed=4)
    fi = P.FrameInterpolator(model=models(fc), device=dev)
    ref = str(tmp_path / ("ref" + ext))
    n_ref = fi.interpolate_video(src, ref, 2, **kw)
    for cf in (None, 2):
        got = str(tmp_path / (f"got{cf}" + ext))
        assert fi.interpolate_video(src, got, 2, chunk_frames=cf, resize=(SRC[1], SRC[0]), **kw) == n_ref
        _same_file(got, ref, (name, cf))


@pytest.mark.parametrize("name", ["y4m-gray", "y4m-p10", "npy-rgb", "nv12", "uyvy422"])
def test_score_video_resize_equals_the_pre_resized_clip(dev, models, tmp_path, name):
    kind, bits, fc, _ = FORMATS[name]
    src, kw, pre, kw_pre = _clips(tmp_path, name, "ABC|DEFG", seed=5)
    for k in (kw, kw_pre):
        k.pop("src_fps", None)
    model = models(fc)
    want = holdout.score_video(model, pre, chunk_frames=2, scene_cut=THR, **kw_pre)
    assert "resize" not in want and want["frames"] == 7
    for cf in (1, 2, 32):
        got = holdout.score_video(model, src, chunk_frames=cf, scene_cut=THR, resize=SIZE, **kw)
        assert got["resize"] == list(SIZE) and got["source_size"] == [SRC[1], SRC[0]]
        assert got["planes"] == want["planes"] and got["scored_frames"].tolist() == want["scored_frames"].tolist()
        for m in want["methods"]:
            for p in want["planes"]:
                for key in ("psnr", "ssim", "sse"):
                    a, b = got["per_frame"][m][p][key], want["per_frame"][m][p][key]
                    assert np.array_equal(a, b, equal_nan=True), (cf, m, p, key)
                assert got["summary"][m][p] == want["summary"][m][p] or all(
                    np.array_equal(got["summary"][m][p][k], want["summary"][m][p][k], equal_nan=True) for k in holdout.STATS)
        assert np.array_equal(got["scene_scores"], want["scene_scores"]) and got["excluded"].tolist() == want["excluded"].tolist()
    assert "scored at 48x40" in holdout.summary_table(got)
