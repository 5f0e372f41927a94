"""CPU: the definition of the device resize (tests/resize_ref.py), the plane tables, the argument checks and the refusals
of `resize=` - nothing here needs a GPU."""
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as C  # noqa: E402
import resize_ref as R  # noqa: E402
import resize_stream_rows  # noqa: E402  (importing it adds the new entry points' rows to the stream contract's table)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, holdout, imageio_lite, resize, stream  # noqa: E402


# ---- 1. the definition ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", C.SIZES + [(7, 9, 7, 20), (7, 9, 15, 9)])
def test_ref_u8_is_resize_linear_u8(size):
    h, w, H, W = size
    rng = np.random.default_rng(h * 1000 + w)
    yy, xx = np.mgrid[:h, :w]
    for plane in (rng.integers(0, 256, (h, w), dtype=np.uint8), (((yy + xx) & 1) * 255).astype(np.uint8),
                  (((yy // 2 + xx // 3) & 1) * 255).astype(np.uint8)):
        assert np.array_equal(R.resize_plane(plane, (W, H), 8), imageio_lite.resize_linear_u8(plane, (W, H)))


def test_ref_taps_stay_in_range():
    for src_n in range(1, 40):
        for dst_n in range(1, 40):
            i0, i1, c0, c1 = R.axis(dst_n, src_n)
            assert i0.min() >= 0 and i1.max() <= src_n - 1 and (i1 - i0).max() <= 1 and (i1 >= i0).all()
            assert (c0 >= 0).all() and (c1 >= 0).all() and (np.abs(c0 + c1 - 2048) <= 1).all()


def test_ref_p10():
    for v in (0, 1, 512, 1023):
        plane = np.full((9, 14), v, np.uint16)
        for size in ((5, 4), (31, 20), (14, 20), (3, 9)):
            assert (R.resize_plane(plane, size, 10) == v).all(), (v, size)
    over = np.full((9, 14), 60000, np.uint16)   # words above 1023 read as 1023 ...
    assert (R.resize_plane(over, (5, 4), 10) == 1023).all()
    assert (R.resize_plane(over, (14, 9), 10) == 60000).all()   # ... except in the copy, which is sample for sample
    rng = np.random.default_rng(5)
    a = rng.integers(0, 1024, (64, 96)).astype(np.uint16)
    s = a.astype(np.int64)
    want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
    assert np.array_equal(R.resize_plane(a, (48, 32), 10), want)
    b = R.resize_plane(a, (48, 32), 10)
    assert b is not a and R.resize_plane(a, (96, 64), 10) is not a
    # the sum of the definition needs more than 32 unsigned bits only where c0 + c1 = 2049 on both axes
    assert 1023 * (1 << 22) + (1 << 21) < 1 << 32 < 1023 * 2049 * 2049 + (1 << 21)


def test_ref_equal_size_is_a_copy():
    rng = np.random.default_rng(6)
    for bits, dtype in ((8, np.uint8), (10, np.uint16)):
        a = rng.integers(0, 1 << (8 if bits == 8 else 16), (11, 17)).astype(dtype)
        assert np.array_equal(R.resize_plane(a, (17, 11), bits), a)


# ---- 2. the plane tables ------------------------------------------------------------------------------------------------
def _kinds():
    kinds = list(stream.RAW_FORMATS) + ["npy", ("npy", 1), ("npy", 3), ("npy", 4)]
    return kinds + [("y4m", t) for t in ("mono", "420jpeg", "420mpeg2", "422", "444", "mono10", "420p10", "422p10")]


@pytest.mark.parametrize("kind", _kinds(), ids=str)
@pytest.mark.parametrize("hw", [(6, 8), (7, 10), (5, 9)], ids=str)
def test_frame_planes_cover_every_sample_once(kind, hw):
    h, w = hw
    if kind in ("uyvy422", "yuyv422") and w % 2:
        with pytest.raises(ValueError, match="even width"):
            resize.frame_planes(kind, h, w)
        return
    planes = resize.frame_planes(kind, h, w)
    n = resize.frame_samples(planes)
    hits = np.zeros(n, np.int64)
    for p in planes:
        np.add.at(hits, np.lib.stride_tricks.as_strided(np.arange(n)[p[1]:], (p[2], p[3]), (p[4] * 8, p[5] * 8)).ravel(), 1)
    assert (hits == 1).all()
    # ... and the frame is the one the routes read
    if isinstance(kind, str) and kind in stream.RAW_FORMATS:
        assert planes == [tuple(p) for p in holdout.raw_planes(kind, h, w)[0]]
        if kind in P.YUV_FORMATS:
            assert n == P.yuv_frame_samples(kind, h, w)
    elif kind[0] == "y4m":
        bits = 10 if "10" in kind[1] else 8
        hdr = imageio_lite._y4m_stream_header(imageio_lite._y4m_header_line(w, h, (25, 1), kind[1], None, bits), bits)
        assert n == hdr["frame_samples"]
    else:
        assert n == h * w * (1 if kind == "npy" else kind[1])


def test_frame_planes_refuses():
    for bad in ("yuv420p", ("y4m", "411"), ("npy", 0), 3, None):
        with pytest.raises(ValueError):
            resize.frame_planes(bad, 4, 4)
    with pytest.raises(ValueError, match="positive"):
        resize.frame_planes("nv12", 0, 4)


def test_y4m_header_at():
    hdr = imageio_lite._y4m_stream_header(imageio_lite._y4m_header_line(9, 7, (24, 1), "420p10", "LIMITED", 10), 10)
    new = resize.y4m_header_at(hdr, (6, 5))
    assert (new["width"], new["height"], new["chroma"], new["frame_samples"]) == (6, 5, (3, 3), 30 + 18)
    assert all(new[k] == hdr[k] for k in ("fps", "colourspace", "colour_range", "bits"))


# ---- 3. sizes on the command line and in calls ------------------------------------------------------------------------------
def test_check_size():
    assert resize.check_size((256, 144)) == (256, 144) and resize.check_size([np.int64(3), 4]) == (3, 4)
    assert resize.check_size("256x144") == (256, 144) and resize.check_size(" 8 X 6 ") == (8, 6)
    for bad in ((0, 4), (4, -1), (4,), (4, 5, 6), (4.0, 5), (True, 5), "4", "4x", "x4", "4x5x6", "-4x5", "4.5x6", "0x6",
                4, None, ("4", "5"), {}):
        with pytest.raises(ValueError, match="size must be"):
            resize.check_size(bad)


def test_cli_resize():
    a = cli.parse_args(["video", "--input", "a.y4m", "--output", "b.y4m", "--resize", "640x360"])
    assert a.resize == (640, 360) and a.size is None
    a = cli.parse_args(["evaluate", "--input", "-", "--raw", "nv12", "--size", "1920x1080", "--resize", "256x256"])
    assert a.resize == (256, 256) and a.size == (1920, 1080)
    assert cli.parse_args(["evaluate", "--input", "a.y4m"]).resize is None
    for bad in ("256", "256x", "0x5", "axb", "25.6x3"):
        with pytest.raises(SystemExit):
            cli.parse_args(["video", "--input", "a.y4m", "--output", "b.y4m", "--resize", bad])


def test_summary_table_says_where_it_was_scored():
    per = {"psnr": np.array([30.0]), "ssim": np.array([0.9]), "sse": np.array([7], np.uint64)}
    res = {"frames": 3, "triplets": "sliding", "bits": 8, "peak": 255, "planes": ["y"], "methods": ["linear"],
           "fps": None, "scored_frames": np.array([1]), "per_frame": {"linear": {"y": per}},
           "summary": {"linear": {"y": holdout._stats(per["psnr"], per["ssim"], per["sse"], 64, 255)}}}
    assert "scored at" not in holdout.summary_table(res)
    res.update({"resize": [256, 144], "source_size": [1920, 1080]})
    table = holdout.summary_table(res)
    assert "scored at 256x144" in table and "1920x1080" in table
    assert holdout.to_jsonable(res)["resize"] == [256, 144]


# ---- 4. refusals come before any device use -----------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device was used before the refusal")
    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(torch.Tensor, "pin_memory", boom)
    monkeypatch.setattr(stream, "_run", boom)
    monkeypatch.setattr(stream, "_run_whole", boom)
    monkeypatch.setattr(holdout, "_score_chunk", boom)


def test_resize_refusals_come_before_any_device_use(tmp_path, no_gpu):
    rgb, gray = (P.FrameInterpolationUNet(bilinear=True, frame_channels=c) for c in (3, 1))
    h, w = 6, 8
    raw = tmp_path / "clip.raw"
    raw.write_bytes(bytes(3 * h * w * 2))
    y4m = tmp_path / "clip.y4m"
    imageio_lite.write_y4m(str(y4m), np.zeros((3, h, w), np.uint8))
    np.save(tmp_path / "clip.npy", np.zeros((3, h, w), np.uint8))
    out = str(tmp_path / "out")
    fi = P.FrameInterpolator(model=rgb, device="cpu")
    fg = P.FrameInterpolator(model=gray, device="cpu")
    for bad in ((0, 4), "4", (4, 5, 6), 7, (2.5, 4)):
        with pytest.raises(ValueError, match="size must be"):
            fi.interpolate_video(str(raw), out + ".raw", raw="uyvy422", width=w, height=h, src_fps=24, resize=bad)
        with pytest.raises(ValueError, match="size must be"):
            fg.interpolate_video(str(y4m), out + ".y4m", resize=bad)
        with pytest.raises(ValueError, match="size must be"):
            fg.interpolate_video(str(tmp_path / "clip.npy"), out + ".npy", resize=bad)
        with pytest.raises(ValueError, match="size must be"):
            holdout.score_video(gray, str(y4m), resize=bad)
    # the route of the destination size raises its own errors: an odd destination width of uyvy422 / yuyv422 ...
    for chunk in (None, 2):
        with pytest.raises(ValueError, match="even width"):
            fi.interpolate_video(str(raw), out + ".raw", raw="uyvy422", width=w, height=h, src_fps=24, resize=(5, 4),
                                 chunk_frames=chunk)
    with pytest.raises(ValueError, match="even width"):
        holdout.score_video(rgb, str(raw), raw="yuyv422", width=w, height=h, resize="5x4")
    # ... and the source's own refusals stay (the size of the source is still needed and still checked)
    with pytest.raises(ValueError, match="even width"):
        fi.interpolate_video(io.BytesIO(b""), out + ".raw", raw="uyvy422", width=7, height=h, src_fps=24, resize=(4, 4))
    with pytest.raises(ValueError, match="missing: width"):
        fi.interpolate_video(str(raw), out + ".raw", raw="uyvy422", height=h, src_fps=24, resize=(4, 4))
    with pytest.raises(ValueError, match="whole number"):
        holdout.score_video(rgb, str(raw), raw="rgb24", width=w, height=h - 1, resize=(4, 4))
    with pytest.raises(ValueError, match="grayscale"):
        holdout.score_video(gray, str(raw), raw="nv12", width=w, height=h, resize=(4, 4))
    assert not [n for n in os.listdir(tmp_path) if n.startswith("out")]


def test_binding_refuses_planes_past_the_buffer():
    src, dst = torch.zeros(100, dtype=torch.uint8), torch.zeros(50, dtype=torch.uint8)
    with pytest.raises(ValueError, match="reach sample"):
        _native.resize_planes(src, [(0, 10, 10, 10, 1, 101)], dst, [(0, 5, 5, 5, 1, 25)], 2, 8, stream=0)
    with pytest.raises(ValueError, match="reach sample"):
        _native.resize_planes(src, [(0, 10, 10, 10, 1, 100)], dst, [(2, 5, 5, 10, 2, 51)], 1, 8, stream=0)
    with pytest.raises(ValueError, match="source planes for"):
        _native.resize_planes(src, [(0, 10, 10, 10, 1, 100)], dst, [], 1, 8, stream=0)


def test_c_abi_refusals_without_gpu(hip_lib_built):
    """Every check of fiunet_resize_planes_* is made on the host before a device pointer is used."""
    import ctypes
    L = _native.lib()
    ok = [(0, 8, 8, 8, 1, 64)]

    def call(sp, dp, n_planes=1, n_frames=1, src=4096, dst=65536, fn=L.fiunet_resize_planes_u8):
        return fn(src, None if sp is None else _native.resize_plane_array(sp), dst,
                  None if dp is None else _native.resize_plane_array(dp), n_planes, n_frames, None)
    assert call(ok, ok, n_frames=0) == 0                      # nothing to do: nothing launched
    assert call(ok, ok, src=0) == 1 and call(ok, ok, dst=0) == 1 and call(None, ok) == 1 and call(ok, None) == 1
    assert call(ok, ok, n_planes=0) == 1 and call(ok * 5, ok * 5, n_planes=5) == 1 and call(ok, ok, n_frames=-1) == 1
    for bad in ((0, 0, 8, 8, 1, 64), (0, 8, -1, 8, 1, 64), (0, 8, 8, 8, 0, 64), (0, 8, 8, 8, 5, 640), (0, 8, 8, 7, 1, 64),
                (0, 8, 8, 14, 2, 640), (1, 8, 8, 8, 1, 64), (0, 8, 8, 8, 1, 63), (65, 8, 8, 8, 1, 64),
                (0, 8, (1 << 24) + 1, 1 << 25, 1, 1 << 30)):
        assert call([bad], ok) == 1, bad
        assert call(ok, [bad]) == 1, bad
        assert b"plane" in L.fiunet_last_error_string()
    assert call(ok, ok, src=4096, dst=4096 + 63) == 1 and b"overlap" in L.fiunet_last_error_string()
    assert call(ok, ok, n_frames=3, src=4096, dst=4096 + 3 * 64 - 1) == 1
    assert call(ok, ok, src=4097, dst=65536, fn=L.fiunet_resize_planes_p10) == 1
    assert b"misaligned" in L.fiunet_last_error_string()
    assert ctypes.sizeof(_native.ResizePlane) == 40


def test_stream_rows_are_in_the_table():
    import stream_contract as SC
    for r in resize_stream_rows.ROWS:
        assert sum(1 for x in SC.ROWS if x.entry == r.entry) == 1
    n = len(SC.ROWS)
    resize_stream_rows.register()          # idempotent
    assert len(SC.ROWS) == n
