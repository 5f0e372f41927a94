"""CPU: the incremental Y4M reader / writer, the streamed path's argument checks and the CLI (stream.py, cli.py,
DESIGN.md 3.3g).  No GPU is touched: every refusal here happens before anything is pinned or launched."""
import io
import os
import threading
import tracemalloc

import numpy as np
import pytest
import torch

import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import cli, imageio_lite as IO, stream

TAGS8 = ["420jpeg", "420", "420mpeg2", "422", "444", "mono"]
TAGS10 = list(IO.Y4M_P10_TAGS)


def _planes(tag, n, h, w, bits, seed):
    rng = np.random.default_rng(seed)
    hi, dt = (256, np.uint8) if bits == 8 else (1024, np.uint16)
    y = rng.integers(0, hi, (n, h, w), dtype=dt)
    if tag.startswith("mono"):
        return y, None
    ch = (h + 1) // 2 if tag.startswith("420") else h
    cw = w if tag.startswith("444") else (w + 1) // 2
    return y, (rng.integers(0, hi, (n, ch, cw), dtype=dt), rng.integers(0, hi, (n, ch, cw), dtype=dt))


def _write_whole(path, tag, y, chroma, bits, rng=None, fps=(24, 1)):
    cs = None if tag == "420" else tag   # "C420" as ffmpeg writes it
    if bits == 8:
        IO.write_y4m(path, y, chroma, fps, cs or "420", colour_range=rng)
    else:
        IO.write_y4m_p10(path, y, chroma, fps, tag, colour_range=rng)


def _read_all(reader, step, dtype):
    buf = np.zeros((step, reader.frame_samples), dtype=dtype)
    out = []
    while True:
        n = reader.read_into(buf, step)
        if not n:
            return np.concatenate(out) if out else None
        out.append(buf[:n].copy())


@pytest.mark.parametrize("rng", [None, "FULL", "LIMITED"])
@pytest.mark.parametrize("tag,bits", [(t, 8) for t in TAGS8] + [(t, 10) for t in TAGS10])
def test_reader_writer_match_whole_file_io(tmp_path, tag, bits, rng):
    n, h, w = 7, 9, 13   # odd sizes
    y, chroma = _planes(tag, n, h, w, bits, seed=len(tag) + bits)
    path = str(tmp_path / "in.y4m")
    _write_whole(path, tag, y, chroma, bits, rng)
    whole, hdr = (IO.read_y4m_packed if bits == 8 else IO.read_y4m_packed_p10)(path)
    dt = np.uint8 if bits == 8 else np.uint16
    for step in (1, 3, n + 5):
        with IO.Y4MReader(path) as r:
            for k, v in hdr.items():
                assert r.header[k] == v, k
            assert r.bits == bits
            assert np.array_equal(_read_all(r, step, dt), whole)
    b = io.BytesIO()
    wr = IO.Y4MWriter(b, w, h, hdr["fps"], hdr["colourspace"], hdr["colour_range"], bits=bits)
    for s in range(0, n, 3):
        wr.write(whole[s:s + 3])
    wr.close()
    assert b.getvalue() == open(path, "rb").read()


def test_writer_defaults_match_whole_file_writers(tmp_path):
    y, chroma = _planes("420jpeg", 3, 6, 8, 8, 1)
    IO.write_y4m(str(tmp_path / "a.y4m"), y, chroma)
    b = io.BytesIO()
    IO.Y4MWriter(b, 8, 6).write(IO.read_y4m_packed(str(tmp_path / "a.y4m"))[0])
    assert b.getvalue() == open(tmp_path / "a.y4m", "rb").read()
    y, chroma = _planes("420p10", 3, 6, 8, 10, 2)
    IO.write_y4m_p10(str(tmp_path / "b.y4m"), y, chroma)
    b = io.BytesIO()
    IO.Y4MWriter(b, 8, 6, bits=10).write(IO.read_y4m_packed_p10(str(tmp_path / "b.y4m"))[0])
    assert b.getvalue() == open(tmp_path / "b.y4m", "rb").read()


def test_frame_lines_with_parameters(tmp_path):
    h, w = 5, 7
    fb = h * w + 2 * 3 * 4
    rng = np.random.default_rng(3)
    fr = rng.integers(0, 256, (4, fb), dtype=np.uint8)
    data = b"YUV4MPEG2 W7 H5 F30:1 Ip A1:1 C420jpeg\n" + b"".join(
        (b"FRAME Ixyz\n" if i % 2 else b"FRAME\n") + fr[i].tobytes() for i in range(4))
    path = tmp_path / "p.y4m"
    path.write_bytes(data)
    assert np.array_equal(IO.read_y4m_packed(str(path))[0], fr)
    with IO.Y4MReader(str(path)) as r:
        assert np.array_equal(_read_all(r, 3, np.uint8), fr)
    assert IO.y4m_frame_count(str(path)) == 4


def test_reader_from_a_pipe(tmp_path):
    y, chroma = _planes("420p10", 40, 17, 23, 10, 4)
    path = str(tmp_path / "in.y4m")
    IO.write_y4m_p10(path, y, chroma, colour_range="FULL")
    data = open(path, "rb").read()
    whole, _ = IO.read_y4m_packed_p10(path)
    rfd, wfd = os.pipe()

    def feed():
        with os.fdopen(wfd, "wb") as f:
            for s in range(0, len(data), 1000):   # dribbled in pieces smaller than a frame
                f.write(data[s:s + 1000])
                f.flush()
    t = threading.Thread(target=feed)
    t.start()
    with os.fdopen(rfd, "rb") as f:
        r = IO.Y4MReader(f)
        got = _read_all(r, 3, np.uint16)
    t.join()
    assert np.array_equal(got, whole)


def _expect_same_error(path, whole_reader, bits=None):
    with pytest.raises(ValueError) as e_whole:
        whole_reader(path)
    with pytest.raises(ValueError) as e_stream:
        with IO.Y4MReader(path, bits=bits) as r:
            _read_all(r, 4, np.uint8 if r.bits == 8 else np.uint16)
    assert str(e_stream.value) == str(e_whole.value)
    return str(e_whole.value)


def test_errors_match_whole_file_readers(tmp_path):
    y, chroma = _planes("420jpeg", 3, 6, 8, 8, 5)
    path = str(tmp_path / "t.y4m")
    IO.write_y4m(path, y, chroma)
    data = open(path, "rb").read()
    (tmp_path / "trunc.y4m").write_bytes(data[:-5])
    assert _expect_same_error(str(tmp_path / "trunc.y4m"), IO.read_y4m_packed) == "Y4M: truncated frame"
    (tmp_path / "empty.y4m").write_bytes(data[:data.index(b"\n") + 1])
    assert _expect_same_error(str(tmp_path / "empty.y4m"), IO.read_y4m_packed) == "Y4M: no frames"
    (tmp_path / "p12.y4m").write_bytes(b"YUV4MPEG2 W8 H6 F30:1 C420p12\nFRAME\n" + bytes(2 * 72))
    assert "bit depth" in _expect_same_error(str(tmp_path / "p12.y4m"), IO.read_y4m_packed)
    assert "bit depth" in _expect_same_error(str(tmp_path / "p12.y4m"), IO.read_y4m_packed_p10, bits=10)
    # an 8-bit stream where the 10-bit reader is asked for, and the reverse
    _expect_same_error(path, IO.read_y4m_packed_p10, bits=10)
    y10, c10 = _planes("420p10", 2, 6, 8, 10, 6)
    IO.write_y4m_p10(str(tmp_path / "ten.y4m"), y10, c10)
    _expect_same_error(str(tmp_path / "ten.y4m"), IO.read_y4m_packed, bits=8)
    with pytest.raises(ValueError, match="truncated frame"):
        IO.y4m_frame_count(str(tmp_path / "trunc.y4m"))


def test_streaming_memory_is_bounded_by_the_chunk(tmp_path):
    n, h, w = 64, 96, 128
    y, chroma = _planes("420jpeg", n, h, w, 8, 7)
    src, dst = str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m")
    IO.write_y4m(src, y, chroma)
    del y, chroma
    fb = IO.Y4MReader(src).frame_bytes
    tracemalloc.start()
    try:
        with IO.Y4MReader(src) as r, IO.Y4MWriter(dst, w, h, r.fps, r.colourspace) as wr:
            buf = np.empty((4, fb), np.uint8)
            while True:
                k = r.read_into(buf, 4)
                if not k:
                    break
                wr.write(buf[:k])
        _, peak = tracemalloc.get_traced_memory()
    finally:
        tracemalloc.stop()
    assert open(dst, "rb").read() == open(src, "rb").read()
    assert peak < 8 * fb, (peak, fb)          # the buffer of 4 frames and some change, not the 64-frame file
    assert os.path.getsize(src) > 50 * fb


# ---- streamed interpolate_video: refusals before any GPU work -------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    """Anything that would pin memory or start the engine fails the test."""
    def boom(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(torch.Tensor, "pin_memory", boom)
    monkeypatch.setattr(stream, "_run", boom)


def _fi(frame_channels):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=frame_channels)
    return P.FrameInterpolator(model=m, device="cpu")


def _no_output(tmp_path):
    return [p.name for p in tmp_path.iterdir() if p.name.startswith("out")] == []


@pytest.mark.parametrize("bad", [0, -1, True, 2.5])
def test_bad_chunk_frames(tmp_path, no_gpu, bad):
    y, chroma = _planes("420jpeg", 3, 6, 8, 8, 8)
    IO.write_y4m(str(tmp_path / "in.y4m"), y, chroma)
    with pytest.raises(ValueError, match="chunk_frames"):
        _fi(1).interpolate_video(str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), chunk_frames=bad)
    assert _no_output(tmp_path)


@pytest.mark.parametrize("tag,bits,msg", [("422", 8, "C422 is not supported by the RGB network"),
                                          ("422p10", 10, "C422p10 is not supported by the RGB network")])
def test_rgb_network_refuses_422(tmp_path, no_gpu, tag, bits, msg):
    y, chroma = _planes(tag, 3, 6, 8, bits, 9)
    _write_whole(str(tmp_path / "in.y4m"), tag, y, chroma, bits)
    with pytest.raises(ValueError, match=msg):
        _fi(3).interpolate_video(str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), chunk_frames=4)
    assert _no_output(tmp_path)


@pytest.mark.parametrize("kw,match", [(dict(matrix="bt2021"), "matrix"), (dict(siting="centre"), "siting"),
                                      (dict(scene_cut=0), "scene_cut"), (dict(factor=3), "factor")])
def test_bad_colour_and_scene_arguments(tmp_path, no_gpu, kw, match):
    y, chroma = _planes("420jpeg", 3, 6, 8, 8, 10)
    IO.write_y4m(str(tmp_path / "in.y4m"), y, chroma)
    with pytest.raises(ValueError, match=match):
        _fi(3).interpolate_video(str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), chunk_frames=4, **kw)
    assert _no_output(tmp_path)


@pytest.fixture
def no_gpu_resident(no_gpu, monkeypatch):
    """`no_gpu` for the whole-clip call: its engine, `stream._run_whole`, fails the test too."""
    def boom(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(stream, "_run_whole", boom)


@pytest.mark.parametrize("tag,out,kw,match", [
    ("422", "out.y4m", {}, "C422 is not supported by the RGB network"),
    ("420jpeg", "out.npy", {}, r"written as \.y4m \(no \.npy output\)"),
    ("420jpeg", "out.y4m", dict(matrix="bt2021"), "matrix"),
    ("420jpeg", "out.y4m", dict(scene_cut=0), "scene_cut"),
    ("420jpeg", "out.y4m", dict(factor=3), "factor"),
])
def test_resident_refusals_before_gpu_work(tmp_path, no_gpu_resident, tag, out, kw, match):
    y, chroma = _planes(tag, 3, 6, 8, 8, 12)
    _write_whole(str(tmp_path / "in.y4m"), tag, y, chroma, 8)
    with pytest.raises(ValueError, match=match):
        _fi(3).interpolate_video(str(tmp_path / "in.y4m"), str(tmp_path / out), **kw)
    assert _no_output(tmp_path)


def test_y4m_from_a_pipe_to_npy_is_refused(tmp_path, no_gpu):
    rfd, wfd = os.pipe()
    os.close(wfd)
    with os.fdopen(rfd, "rb") as f:
        with pytest.raises(ValueError, match="pipe"):
            _fi(1).interpolate_video(f, str(tmp_path / "out.npy"), chunk_frames=4)
    assert _no_output(tmp_path)


def test_npy_writer_header_is_np_save(tmp_path):
    a = np.random.default_rng(11).integers(0, 256, (5, 7, 9, 3), dtype=np.uint8)
    np.save(tmp_path / "ref.npy", a)
    w = stream._NpyWriter(str(tmp_path / "s.npy"), np.uint8, a.shape)
    w.write(a[:2].reshape(2, -1))
    w.write(a[2:].reshape(3, -1))
    w.close(True)
    assert (tmp_path / "s.npy").read_bytes() == (tmp_path / "ref.npy").read_bytes()
    assert not (tmp_path / "s.npy.part").exists()


# ---- the CLI ----------------------------------------------------------------------------------------------------
def test_cli_arguments():
    a = cli.parse_args(["video", "--input", "-", "--output", "-"])
    assert (a.factor, a.model, a.device, a.batch, a.chunk_frames) == (2, "best_model.pth", "auto", 8, 32)
    assert a.scene_cut is None and a.siting is None and a.matrix == "bt709" and a.precision is None
    a = cli.parse_args(["video", "--input", "in.y4m", "--output", "out.y4m", "--factor", "4", "--batch", "4",
                        "--scene-cut", "10", "--siting", "mpeg2", "--precision", "fp16", "--matrix", "bt2020"])
    assert (a.factor, a.batch, a.chunk_frames, a.scene_cut, a.siting, a.precision, a.matrix) == \
        (4, 4, 16, 10.0, "mpeg2", "fp16", "bt2020")
    assert cli.parse_args(["video", "--input", "-", "--output", "-", "--chunk-frames", "5"]).chunk_frames == 5
    with pytest.raises(SystemExit):
        cli.parse_args(["video", "--input", "-"])


def test_cli_frame_channels_from_the_checkpoint():
    gray = P.FrameInterpolationUNet(bilinear=True, frame_channels=1).state_dict()
    rgb = P.FrameInterpolationUNet(bilinear=True, frame_channels=3).state_dict()
    assert cli.frame_channels_of(gray) == 1 and cli.frame_channels_of(rgb) == 3
    assert cli.frame_channels_of({"model_state_dict": rgb, "epoch": 3}) == 3
    with pytest.raises(ValueError):
        cli.frame_channels_of({"x": torch.zeros(1)})
