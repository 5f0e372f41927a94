"""GPU (MI355X): streamed video (stream.py) against the resident whole-clip path.

  1. byte identity of the output file of `interpolate_video(..., chunk_frames=k)` and the resident run (the same route
     with the whole clip as one chunk): every Y4M and .npy route, factor 2 / 4 / 8, scene_cut None / 10, chunk_frames
     1 / 3 / 8 / > N, odd sizes, N = 1 and 2; the output naming of the two calls
  2. scene cuts at a chunk's first interval, its last interval and its lookahead interval: streamed scores and flags
     equal scene.detect_cuts on the whole clip, and the held frames sit where the resident run holds them
  3. device memory bounded by the chunk: equal streamed peaks at N = 9 and N = 41, resident peaks far apart
  4. the streamed path never reads a whole clip (the whole-file readers and non-mmap np.load raise)
  5. the CLI in a child process over pipes: stdout is the interpolate_video output file, stderr the loading lines
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import imageio_lite as IO, stream
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 10.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _model(dev, fc, precision):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=fc, precision=precision)
    sd = O.make_seeded_state_dict(1234) if fc == 1 else O.make_seeded_state_dict(77, n_channels=6, n_classes=3)
    m.load_state_dict(sd)
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def models(dev):
    cache = {}

    def get(fc, precision):
        if (fc, precision) not in cache:
            cache[(fc, precision)] = _model(dev, fc, precision)
        return cache[(fc, precision)]
    return get


def _clip(n, row_shape, bits, cuts=(), seed=0):
    """n frames of `row_shape` samples: a random picture with small frame-to-frame noise, a new picture after each
    interval in `cuts` (a hard cut)."""
    rng = np.random.default_rng(seed)
    hi, dt = (256, np.uint8) if bits == 8 else (1024, np.uint16)
    base = rng.integers(0, hi, row_shape)
    out = []
    for i in range(n):
        if i - 1 in cuts:
            base = rng.integers(0, hi, row_shape)
        out.append(np.clip(base + rng.integers(-3, 4, row_shape), 0, hi - 1).astype(dt))
    return np.stack(out)


def _y4m(path, n, h, w, tag, bits, cuts=(), seed=0, rng=None):
    hdr = IO._y4m_stream_header(IO._y4m_header_line(w, h, (24, 1), tag, rng, bits), bits)
    frames = _clip(n, (hdr["frame_samples"],), bits, cuts, seed)
    with IO.Y4MWriter(path, w, h, (24, 1), tag, rng, bits=bits) as wr:
        wr.write(frames)
    return frames


def _both(fi, tmp_path, src, ext, factor, scene_cut, chunk_frames, **kw):
    ref, got = str(tmp_path / f"ref{ext}"), str(tmp_path / f"got{ext}")
    n_ref = fi.interpolate_video(src, ref, factor, scene_cut=scene_cut, **kw)
    n_got = fi.interpolate_video(src, got, factor, scene_cut=scene_cut, chunk_frames=chunk_frames, **kw)
    assert n_got == n_ref
    assert not os.path.exists(got + ".part")
    return open(ref, "rb").read(), open(got, "rb").read()


# ---- 1. byte identity ---------------------------------------------------------------------------------------------
# (network, tag, bits, h, w, n, factor, scene_cut, chunk_frames, precision)
Y4M_CASES = [
    (1, "420jpeg", 8, 37, 53, 11, 2, None, 3, "bf16"),
    (1, "420", 8, 37, 53, 1, 2, None, 3, "bf16"),
    (1, "422", 8, 37, 53, 9, 4, THR, 1, "bf16"),
    (1, "444", 8, 37, 53, 10, 2, THR, 8, "bf16"),
    (1, "mono", 8, 37, 53, 7, 2, None, 20, "bf16"),
    (1, "420p10", 10, 37, 53, 10, 2, THR, 3, "fp16"),
    (1, "422p10", 10, 37, 53, 6, 4, None, 3, "fp16"),
    (1, "444p10", 10, 37, 53, 2, 2, None, 8, "fp16"),
    (1, "mono10", 10, 37, 53, 6, 8, THR, 3, "fp16"),
    (3, "420jpeg", 8, 33, 47, 11, 2, THR, 3, "bf16"),
    (3, "420mpeg2", 8, 33, 47, 9, 4, None, 8, "bf16"),
    (3, "420", 8, 33, 47, 2, 2, THR, 1, "bf16"),
    (3, "420p10", 10, 33, 47, 10, 2, THR, 3, "fp16"),
    (3, "420p10", 10, 33, 47, 5, 4, None, 1, "fp16"),
]


@pytest.mark.parametrize("fc,tag,bits,h,w,n,factor,sc,cf,prec", Y4M_CASES)
def test_y4m_stream_is_byte_identical(dev, models, tmp_path, fc, tag, bits, h, w, n, factor, sc, cf, prec):
    src = str(tmp_path / "in.y4m")
    _y4m(src, n, h, w, tag, bits, cuts=(n // 2,), seed=n + factor, rng="FULL" if n % 2 else None)
    fi = P.FrameInterpolator(model=models(fc, prec), device=dev)
    ref, got = _both(fi, tmp_path, src, ".y4m", factor, sc, cf)
    assert got == ref


@pytest.mark.parametrize("tag,bits,prec,cf", [("420jpeg", 8, "bf16", 3), ("mono10", 10, "fp16", 1),
                                              ("422p10", 10, "fp16", 20)])
def test_y4m_to_npy_stream_is_byte_identical(dev, models, tmp_path, tag, bits, prec, cf):
    src = str(tmp_path / "in.y4m")
    _y4m(src, 9, 37, 53, tag, bits, cuts=(4,), seed=bits)
    fi = P.FrameInterpolator(model=models(1, prec), device=dev)
    ref, got = _both(fi, tmp_path, src, ".npy", 2, THR, cf)
    assert got == ref


# (network, frame shape, n, factor, scene_cut, chunk_frames)
NPY_CASES = [
    (1, (37, 53), 11, 2, None, 3),
    (1, (37, 53), 7, 4, THR, 1),
    (1, (33, 47, 3), 9, 2, THR, 8),     # per-channel through the grayscale network
    (3, (33, 47, 3), 10, 2, THR, 3),
    (3, (33, 47, 3), 2, 4, None, 20),
]


@pytest.mark.parametrize("fc,shape,n,factor,sc,cf", NPY_CASES)
def test_npy_stream_is_byte_identical(dev, models, tmp_path, fc, shape, n, factor, sc, cf):
    src = str(tmp_path / "in.npy")
    np.save(src, _clip(n, shape, 8, cuts=(n // 2,), seed=n))
    fi = P.FrameInterpolator(model=models(fc, "bf16"), device=dev)
    ref, got = _both(fi, tmp_path, src, ".npy", factor, sc, cf)
    assert got == ref


def test_resident_output_naming(dev, models, tmp_path):
    """A whole-clip Y4M call writes a `.npy` stack of the luma frames to any name that does not end in `.y4m`, named as
    np.save names it; a streamed call writes Y4M to every name but `.npy`."""
    n, h, w = 3, 37, 53
    src = str(tmp_path / "in.y4m")
    frames = _y4m(src, n, h, w, "420jpeg", 8, seed=12)
    fi = P.FrameInterpolator(model=models(1, "bf16"), device=dev)
    assert fi.interpolate_video(src, str(tmp_path / "out.npy"), 2) == 2 * n - 1
    assert fi.interpolate_video(src, str(tmp_path / "out.bin"), 2) == 2 * n - 1
    assert sorted(p.name for p in tmp_path.iterdir() if p.name.startswith("out")) == ["out.bin.npy", "out.npy"]
    assert (tmp_path / "out.bin.npy").read_bytes() == (tmp_path / "out.npy").read_bytes()
    stack = np.load(tmp_path / "out.npy")
    assert stack.dtype == np.uint8 and stack.shape == (2 * n - 1, h, w)
    assert np.array_equal(stack[0::2], frames[:, :h * w].reshape(n, h, w))
    assert fi.interpolate_video(src, str(tmp_path / "out2.bin"), 2, chunk_frames=2) == 2 * n - 1
    assert not (tmp_path / "out2.bin.npy").exists()
    out, hdr = IO.read_y4m_packed(str(tmp_path / "out2.bin"))
    assert out.shape == (2 * n - 1, frames.shape[1]) and (hdr["height"], hdr["width"]) == (h, w)
    assert np.array_equal(out[:, :h * w].reshape(-1, h, w), stack)


# ---- 2. scene cuts across chunk edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("fc,tag,bits,prec", [(3, "420jpeg", 8, "bf16"), (1, "420p10", 10, "fp16")])
def test_scene_cut_windows_across_chunks(dev, models, tmp_path, fc, tag, bits, prec):
    # chunk_frames 4: chunks hold intervals 0-3, 4-7, 8-11, 12-15, 16-18.  Cut 4: the first interval of a chunk (and
    # the lookahead of the one before); 11: the last of a chunk; 16: the lookahead interval of chunk 12-15
    n, h, w, cuts = 20, 33, 47, (4, 11, 16)
    src = str(tmp_path / "in.y4m")
    frames = _y4m(src, n, h, w, tag, bits, cuts=cuts, seed=5)
    model = models(fc, prec)
    t = torch.from_numpy(frames.view(np.int16) if bits == 10 else frames).to(dev)
    scores, flags = P.scene.detect_cuts(t, THR, bits)
    assert np.flatnonzero(flags.cpu().numpy()).tolist() == list(cuts)
    log = []
    got = str(tmp_path / "got.y4m")
    stream.interpolate_y4m_stream(model, src, got, 2, chunk_frames=4, scene_cut=THR, scene_log=log)
    assert [len(s) for s, _ in log] == [4, 4, 4, 4, 3]
    assert np.array_equal(np.concatenate([s for s, _ in log]), scores.cpu().numpy())
    assert np.array_equal(np.concatenate([f for _, f in log]), flags.cpu().numpy())
    ref = str(tmp_path / "ref.y4m")
    P.FrameInterpolator(model=model, device=dev).interpolate_video(src, ref, 2, scene_cut=THR)
    assert open(got, "rb").read() == open(ref, "rb").read()
    out, _ = (IO.read_y4m_packed if bits == 8 else IO.read_y4m_packed_p10)(got)
    for c in cuts:   # the inserted frame of a cut interval is the frame before the cut
        assert np.array_equal(out[2 * c + 1], out[2 * c])


# ---- 3. bounded device memory -------------------------------------------------------------------------------------
def _peak(dev, fn):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def test_device_memory_is_bounded_by_the_chunk(dev, models, tmp_path):
    # chunk_frames 4: two chunks at N = 9, ten at N = 41 (a chunk after the first also holds its predecessor's result)
    h, w = 270, 480
    fb = P.i420_frame_bytes(h, w)
    fi = P.FrameInterpolator(model=models(3, "bf16"), device=dev)
    peaks = {}
    for n in (9, 41):
        src = str(tmp_path / f"in{n}.y4m")
        _y4m(src, n, h, w, "420jpeg", 8, cuts=(3,), seed=n)
        fi.interpolate_video(src, str(tmp_path / "warm.y4m"), 2, chunk_frames=4, scene_cut=THR)   # warm-up
        peaks[("stream", n)] = _peak(dev, lambda: fi.interpolate_video(src, str(tmp_path / "s.y4m"), 2,
                                                                       chunk_frames=4, scene_cut=THR))
        peaks[("resident", n)] = _peak(dev, lambda: fi.interpolate_video(src, str(tmp_path / "r.y4m"), 2,
                                                                         scene_cut=THR))
    print("peaks (bytes):", peaks, "frame bytes:", fb)
    assert abs(peaks[("stream", 41)] - peaks[("stream", 9)]) <= fb
    assert peaks[("resident", 41)] - peaks[("resident", 9)] > 32 * fb


# ---- 4. no whole-clip reads ---------------------------------------------------------------------------------------
def test_streaming_never_reads_the_whole_clip(dev, models, tmp_path, monkeypatch):
    y4m_src, npy_src = str(tmp_path / "in.y4m"), str(tmp_path / "in.npy")
    _y4m(y4m_src, 9, 33, 47, "420jpeg", 8, seed=1)
    np.save(npy_src, _clip(9, (33, 47, 3), 8, seed=2))
    fi = P.FrameInterpolator(model=models(3, "bf16"), device=dev)
    fi1 = P.FrameInterpolator(model=models(1, "bf16"), device=dev)
    fi.interpolate_video(y4m_src, str(tmp_path / "ref.y4m"), 2)
    fi.interpolate_video(npy_src, str(tmp_path / "ref.npy"), 2)
    fi1.interpolate_video(y4m_src, str(tmp_path / "ref1.y4m"), 2)

    def whole(*a, **k):
        raise AssertionError("a whole-clip read")
    for name in ("read_y4m", "read_y4m_p10", "read_y4m_packed", "read_y4m_packed_p10"):
        monkeypatch.setattr(IO, name, whole)
    real_load = np.load

    def load(*a, **k):
        if k.get("mmap_mode") is None:
            raise AssertionError("np.load without mmap_mode")
        return real_load(*a, **k)
    monkeypatch.setattr(np, "load", load)
    fi.interpolate_video(y4m_src, str(tmp_path / "got.y4m"), 2, chunk_frames=3)
    fi.interpolate_video(npy_src, str(tmp_path / "got.npy"), 2, chunk_frames=3)
    fi1.interpolate_video(y4m_src, str(tmp_path / "got1.y4m"), 2, chunk_frames=3, scene_cut=THR)
    for a, b in (("ref.y4m", "got.y4m"), ("ref.npy", "got.npy"), ("ref1.y4m", "got1.y4m")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes()


# ---- 5. the CLI over pipes ----------------------------------------------------------------------------------------
def test_cli_over_pipes(dev, tmp_path):
    ck = str(tmp_path / "rgb.pth")
    torch.save(O.make_seeded_state_dict(77, n_channels=6, n_classes=3), ck)
    src = str(tmp_path / "in.y4m")
    _y4m(src, 10, 33, 47, "420mpeg2", 8, cuts=(6,), seed=3, rng="FULL")
    ref = str(tmp_path / "ref.y4m")
    model = P.load_model(ck, dev, "bf16", frame_channels=3)
    P.FrameInterpolator(model=model, device=dev, batch=4).interpolate_video(src, ref, 4, scene_cut=THR)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "ai_based_frame_interpolation_amd.cli", "video", "--input", "-",
                          "--output", "-", "--model", ck, "--precision", "bf16", "--factor", "4", "--batch", "4",
                          "--scene-cut", "10", "--chunk-frames", "3"],
                         input=open(src, "rb").read(), capture_output=True, cwd=ROOT, env=env, timeout=300)
    assert res.returncode == 0, res.stderr.decode(errors="replace")
    assert res.stdout == open(ref, "rb").read()
    assert b"Model state dict loaded from" in res.stderr
