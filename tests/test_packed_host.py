"""CPU: packed RGB frames - the format table, the layout rules in Python and in the library, the raw-video
route's refusals (before any GPU work, leaving no output), the command line, the tests' own numpy restatement, and the
header against the binding.  No GPU is touched."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import packed_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, packed, stream  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fiunet_packed_to_rgb_u8", "fiunet_rgb_to_packed_u8", "fiunet_workspace_bytes_rgb_packed",
       "fiunet_forward_rgb_packed"]
H, W = 37, 53


# ---- formats and layouts ------------------------------------------------------------------------------------------
def test_format_table():
    assert list(packed.FORMATS) == ["rgb24", "bgr24", "rgba", "bgra"]
    assert {k: v[1] for k, v in packed.FORMATS.items()} == R.BPP
    assert [v[0] for v in packed.FORMATS.values()] == [0, 1, 2, 3]
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    for name, (code, _) in packed.FORMATS.items():
        assert re.search(rf"FIUNET_PACKED_{name.upper()} = {code}\b", src), name
    assert set(packed.FORMATS) < set(stream.RAW_FORMATS) and "nv12" in stream.RAW_FORMATS
    assert P.packed is packed and P.PackedLayout is packed.PackedLayout


@pytest.mark.parametrize("fmt", list(R.BPP))
def test_frame_bytes_and_tight_layout(fmt):
    bpp = R.BPP[fmt]
    assert packed.frame_bytes(fmt, H, W) == H * W * bpp == R.tight(fmt, H, W)[1]
    assert packed.frame_bytes(fmt, 1, 1) == bpp
    want = packed.PackedLayout(W * bpp, H * W * bpp)
    assert packed.resolve_layout(None, fmt, H, W) == want == packed.resolve_layout(packed.PackedLayout(), fmt, H, W)
    # a pitch alone: the stride follows it; the smallest legal stride stops at the last pixel
    assert packed.resolve_layout(packed.PackedLayout(W * bpp + 5), fmt, H, W) == (W * bpp + 5, H * (W * bpp + 5))
    edge = (W * bpp + 5, (H - 1) * (W * bpp + 5) + W * bpp)
    assert packed.resolve_layout(packed.PackedLayout(*edge), fmt, H, W) == edge
    with pytest.raises(ValueError, match="row_pitch"):
        packed.resolve_layout(packed.PackedLayout(W * bpp - 1), fmt, H, W)
    with pytest.raises(ValueError, match="frame_stride"):
        packed.resolve_layout(packed.PackedLayout(edge[0], edge[1] - 1), fmt, H, W)


@pytest.mark.parametrize("bad", [(-1, 0), (0, -4), (0, 1.5), (True, 0), (0, False), (1 << 41, 0), (0, 0, 0), (0,)])
def test_layout_values(bad):
    with pytest.raises(ValueError, match="layout"):
        packed.resolve_layout(bad, "rgb24", H, W)


def test_unknown_format_and_size():
    for fn in (lambda: packed.frame_bytes("rgb48", H, W), lambda: packed.resolve_layout(None, "gbrp", H, W),
               lambda: packed.frame_bytes(None, H, W)):
        with pytest.raises(ValueError, match="format"):
            fn()
    with pytest.raises(ValueError, match="frame size"):
        packed.frame_bytes("rgb24", 0, W)


def test_cpu_tensors_are_refused():
    x = torch.zeros((1, H * W * 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        packed.packed_to_rgb(x, H, W, "rgb24")
    with pytest.raises(RuntimeError, match="GPU"):
        packed.rgb_to_packed(torch.zeros((1, 3, H, W), dtype=torch.uint8), "bgra")
    with pytest.raises(ValueError, match="uint8"):
        packed.packed_to_rgb(x.to(torch.int16), H, W, "rgb24")
    with pytest.raises(ValueError, match="frames of 37x53"):
        packed.packed_to_rgb(x[:, :-1], H, W, "rgb24")
    with pytest.raises(ValueError, match="alpha"):
        packed.packed_to_rgb(x, H, W, "rgb24", return_alpha=True)


# ---- the library's host-side checks -------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(R.BPP))
def test_layout_refusals_library(hip_lib_built, fmt):
    """Both conversions refuse a layout on the host, before any launch (no device here: a launch would fail with
    another status)."""
    lib = _native.lib()
    code, bpp = packed.FORMATS[fmt]
    buf = ctypes.create_string_buffer(64)   # never dereferenced: the layout is refused first
    p = ctypes.addressof(buf)
    for layout, word in (((W * bpp - 1, 0), "row_pitch"), ((W * bpp + 3, (H - 1) * (W * bpp + 3) + W * bpp - 1), "frame_stride")):
        lay = ctypes.byref(_native.PackedLayout(*layout))
        assert lib.fiunet_packed_to_rgb_u8(p, lay, p, None, 1, H, W, code, None) == 1   # FIUNET_ERR_INVALID_ARG
        msg = lib.fiunet_last_error_string().decode()
        assert "packed layout" in msg and word in msg, msg
        assert lib.fiunet_rgb_to_packed_u8(p, p, lay, None, None, None, 1, H, W, code, None) == 1
        assert word in lib.fiunet_last_error_string().decode()
        if bpp == 4:   # the alpha sources' own layout
            assert lib.fiunet_rgb_to_packed_u8(p, p, None, p, None, lay, 1, H, W, code, None) == 1
            assert word in lib.fiunet_last_error_string().decode()


def test_library_argument_checks(hip_lib_built):
    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.fiunet_packed_to_rgb_u8(None, None, None, None, 1, H, W, 0, None) == 1
    assert lib.fiunet_packed_to_rgb_u8(p, None, p, None, 1, H, W, 4, None) == 1          # no such format
    assert lib.fiunet_packed_to_rgb_u8(p, None, p, None, 1, H, W, -1, None) == 1
    assert lib.fiunet_packed_to_rgb_u8(p, None, p, None, 0, H, W, 0, None) == 2          # FIUNET_ERR_BAD_SHAPE
    assert lib.fiunet_packed_to_rgb_u8(p, None, p, p, 1, H, W, 0, None) == 1             # rgb24 has no alpha plane
    assert lib.fiunet_rgb_to_packed_u8(p, p, None, p, None, None, 1, H, W, 1, None) == 1  # bgr24 takes no alpha source
    assert lib.fiunet_rgb_to_packed_u8(p, p, None, None, p, None, 1, H, W, 2, None) == 1  # alpha2 without alpha1
    assert lib.fiunet_workspace_bytes_rgb_packed(None, 1, 64, 64, 0) == 0
    assert lib.fiunet_forward_rgb_packed(None, p, p, None, p, None, 1, 64, 64, 0, 0, p, 64, None) == 1


def test_bad_shape_status_is_the_headers():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    assert re.search(r"FIUNET_ERR_INVALID_ARG = 1\b", src) and re.search(r"FIUNET_ERR_BAD_SHAPE = 2\b", src)


# ---- the tests' numpy restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", list(R.BPP))
@pytest.mark.parametrize("h,w", [(3, 5), (1, 1), (4, 8)])
def test_reference_round_trip(fmt, h, w):
    bpp = R.BPP[fmt]
    rng = np.random.default_rng(h * 100 + w)
    fr = rng.integers(0, 256, (2, h * w * bpp)).astype(np.uint8)
    rgb, alpha = R.unpack(fr, fmt, h, w)
    assert rgb.shape == (2, 3, h, w) and (alpha is None) == (bpp == 3)
    first = fr.reshape(2, h, w, bpp)[:, 0, 0]
    r_at = 2 if fmt.startswith("bgr") else 0
    assert np.array_equal(rgb[:, 0, 0, 0], first[:, r_at]) and np.array_equal(rgb[:, 1, 0, 0], first[:, 1])
    assert np.array_equal(R.pack(rgb, fmt, alpha=alpha), fr)
    if bpp == 4:
        assert (R.pack(rgb, fmt)[:, 3::4] == 255).all()
    lay = (w * bpp + 3, h * (w * bpp + 3) + 7)
    pitched = R.pack(rgb, fmt, lay, alpha, fill=0xA5)
    assert pitched.shape == (2, lay[1]) and R.used_mask(fmt, h, w, lay).sum() == h * w * bpp
    assert (pitched[:, ~R.used_mask(fmt, h, w, lay)] == 0xA5).all()
    back, aback = R.unpack(pitched, fmt, h, w, lay)
    assert np.array_equal(back, rgb) and (alpha is None or np.array_equal(aback, alpha))
    a, b = np.array([0, 1, 255, 254], np.uint8), np.array([1, 1, 255, 255], np.uint8)
    assert R.alpha_average(a, b).tolist() == [1, 1, 255, 255]


# ---- the raw route: refusals before any GPU work ------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(torch.Tensor, "pin_memory", boom)
    monkeypatch.setattr(stream, "_run", boom)
    monkeypatch.setattr(stream, "_run_whole", boom)


def _fi(frame_channels):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=frame_channels)
    return P.FrameInterpolator(model=m, device="cpu")


def _no_output(tmp_path):
    return [p.name for p in tmp_path.iterdir() if p.name.startswith("out")] == []


GOOD = dict(raw="rgb24", width=8, height=6, src_fps=24)


@pytest.mark.parametrize("cf,out,kw,match", [
    (1, "out.rgb", {}, "grayscale"),
    (1, "out.rgb", dict(raw="bgra"), "grayscale"),
    (3, "out.npy", {}, "no .npy output"),
    (3, "out.rgb", dict(width=None), "width"),
    (3, "out.rgb", dict(height=None), "height"),
    (3, "out.rgb", dict(src_fps=None), "src_fps"),
    (3, "out.rgb", dict(raw="rgb48le"), "raw must be one of"),
    (3, "out.rgb", dict(raw="nv21"), "raw must be one of"),
    (3, "out.rgb", dict(raw="rgba"), "whole number"),     # 3 rgb24 frames are 2.25 rgba frames
    (3, "out.rgb", dict(chunk_frames=0), "chunk_frames"),
], ids=["gray", "gray-bgra", "npy", "no-width", "no-height", "no-src-fps", "format", "nv21", "file-size", "chunk"])
def test_raw_route_refusals(tmp_path, no_gpu, cf, out, kw, match):
    src = tmp_path / "in.rgb"
    src.write_bytes(bytes(3 * packed.frame_bytes("rgb24", 6, 8)))
    with pytest.raises(ValueError, match=match):
        _fi(cf).interpolate_video(str(src), str(tmp_path / out), **dict(GOOD, **kw))
    assert _no_output(tmp_path)


@pytest.mark.parametrize("fmt", list(R.BPP))
def test_raw_route_rows(fmt):
    """The route of every packed format: rows of H*W*bpp bytes in and out, 8 bits; the colour options are not looked at."""
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    r = stream._raw_route(m, fmt, 6, 8, False, 2, "no-such-matrix", "no-such-siting")
    assert (r.bits, r.row, r.out_row) == (8, 6 * 8 * R.BPP[fmt], 6 * 8 * R.BPP[fmt])


def test_truncated_stream_is_an_error_at_that_point(tmp_path, monkeypatch):
    """interpolate_video(raw="rgb24") on a pipe that ends inside a frame: the reader raises where the data stops (the
    run is replaced by one that only reads, so no GPU is needed)."""
    def read_only(model, route, reader, write, *a, **k):
        buf = np.zeros((4, route.row), np.uint8)
        while reader.read_into(buf, 4):
            pass
        return 0
    monkeypatch.setattr(stream, "_run_whole", read_only)
    row = packed.frame_bytes("rgb24", 6, 8)
    with pytest.raises(ValueError, match="ends inside a frame"):
        _fi(3).interpolate_video(io.BytesIO(bytes(2 * row + 7)), str(tmp_path / "out.rgb"), **GOOD)
    assert not (tmp_path / "out.rgb").exists()


# ---- the CLI ----------------------------------------------------------------------------------------------------
def test_cli_raw_arguments():
    base = ["video", "--input", "-", "--output", "-"]
    a = cli.parse_args(base + ["--raw", "bgra", "--size", "64x48", "--src-fps", "24"])
    assert a.raw == "bgra" and a.size == (64, 48) and (a.src_fps.numerator, a.src_fps.denominator) == (24, 1)
    for fmt in R.BPP:
        a = cli.parse_args(base + ["--raw", fmt, "--size", "64x48", "--src-fps", "30000/1001", "--fps", "60", "--scene-cut",
                                   "10", "--chunk-frames", "16", "--factor", "2"])
        assert a.raw == fmt and a.chunk_frames == 16 and a.scene_cut == 10
    for bad in (["--raw", "rgb24", "--size", "64x48"],                # no --src-fps
                ["--raw", "rgba", "--src-fps", "24"],                 # no --size
                ["--raw", "nv21", "--size", "64x48", "--src-fps", "24"],
                ["--raw", "rgb48le", "--size", "64x48", "--src-fps", "24"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)


# ---- header and binding -----------------------------------------------------------------------------------------
def test_new_header_names_are_in_the_binding():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"\b(fiunet_[a-z0-9_]*packed[a-z0-9_]*)\s*\(", src)
    assert sorted(declared) == sorted(NEW) and set(NEW) <= set(_native.SYMBOLS)
    assert re.search(r"#define FIUNET_ABI_VERSION 8\b", src) and _native.ABI_VERSION == 8
    assert "typedef struct fiunet_packed_layout" in src
    assert [f for f, _ in _native.PackedLayout._fields_] == list(packed.PackedLayout._fields) == \
        re.search(r"fiunet_packed_layout \{\s*size_t ([^;]+);", src).group(1).replace(" ", "").split(",")
