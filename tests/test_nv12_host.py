"""CPU: NV12 / P010 decoder surfaces - the layout rules in Python and in the library, the raw-video
route's refusals (before any GPU work, leaving no output), the command line, the tests' own repack helper, and the
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
import nv12_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, colour, stream  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fiunet_nv12_to_rgb_u8", "fiunet_rgb_to_nv12_u8", "fiunet_workspace_bytes_nv12", "fiunet_forward_nv12",
       "fiunet_p010_to_rgb_p10", "fiunet_rgb_p10_to_p010", "fiunet_workspace_bytes_p010", "fiunet_forward_p010"]
H, W = 49, 67   # Hc 25, Wc 34: tight (67, 3283, 68, 4983)

# one case per refusal: (layout, the word its message carries)
BAD = [((66, 0, 0, 0), "luma_pitch"),
       ((0, 0, 67, 0), "chroma_pitch"),
       ((71, 48 * 71 + 66, 0, 9000), "chroma_offset"),
       ((71, 49 * 71, 69, 49 * 71 + 24 * 69 + 67), "frame_stride")]


# ---- the layout ---------------------------------------------------------------------------------------------------
def test_tight_layout():
    want = colour.SurfaceLayout(W, H * W, 68, colour.i420_frame_bytes(H, W))
    assert colour.resolve_layout(None, H, W) == want == colour.resolve_layout(colour.SurfaceLayout(), H, W)
    assert tuple(want) == R.tight(H, W)
    # a surface as a decoder pads it: every field given; the smallest legal values pass
    assert colour.resolve_layout(colour.SurfaceLayout(96, 96 * 56, 96, 96 * 84), 48, 64) == (96, 96 * 56, 96, 96 * 84)
    edge = (71, 48 * 71 + 67, 69, 48 * 71 + 67 + 24 * 69 + 68)
    assert colour.resolve_layout(colour.SurfaceLayout(*edge), H, W) == edge


@pytest.mark.parametrize("layout,word", BAD, ids=[w for _, w in BAD])
def test_layout_refusals_python(layout, word):
    with pytest.raises(ValueError, match=word):
        colour.resolve_layout(colour.SurfaceLayout(*layout), H, W)


@pytest.mark.parametrize("bad", [(-1, 0, 0, 0), (0, 0, 0, 1.5), (True, 0, 0, 0), (1 << 41, 0, 0, 0), (0, 0, 0)])
def test_layout_values_python(bad):
    with pytest.raises(ValueError, match="layout"):
        colour.resolve_layout(bad, H, W)


@pytest.mark.parametrize("layout,word", BAD, ids=[w for _, w in BAD])
def test_layout_refusals_library(hip_lib_built, layout, word):
    """The four conversions refuse the layout on the host, before any launch (no device here: a launch would fail
    with another status)."""
    lib = _native.lib()
    buf = ctypes.create_string_buffer(64)   # never dereferenced: the layout is refused first
    p = ctypes.addressof(buf)
    lay = ctypes.byref(_native.SurfaceLayout(*layout))
    for fn, args in ((lib.fiunet_nv12_to_rgb_u8, (p, lay, p)), (lib.fiunet_rgb_to_nv12_u8, (p, p, lay)),
                     (lib.fiunet_p010_to_rgb_p10, (p, lay, p)), (lib.fiunet_rgb_p10_to_p010, (p, p, lay))):
        assert fn(*args, 1, H, W, 0, None) == 1   # FIUNET_ERR_INVALID_ARG
        msg = lib.fiunet_last_error_string().decode()
        assert "surface layout" in msg and word in msg, msg


def test_library_argument_checks(hip_lib_built):
    lib = _native.lib()
    assert lib.fiunet_nv12_to_rgb_u8(None, None, None, 1, H, W, 0, None) == 1
    assert lib.fiunet_workspace_bytes_nv12(None, 1, 64, 64, 0) == 0
    assert lib.fiunet_workspace_bytes_p010(None, 1, 64, 64, 0) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.fiunet_nv12_to_rgb_u8(p, None, p, 1, H, W, _native.YUV_BT2020, None) == 1   # BT.2020: 10 bits only
    assert lib.fiunet_forward_nv12(None, p, p, None, p, None, 1, 64, 64, 0, 0, p, 64, None) == 1


# ---- the tests' repack helper ---------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(49, 67), (48, 64), (1, 1), (5, 2), (2, 5)])
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_repack_round_trip(h, w, dtype):
    hc, wc, ny, nc = R.dims(h, w)
    rng = np.random.default_rng(h * 100 + w)
    fr = rng.integers(0, 256 if dtype == np.uint8 else 1024, (3, ny + 2 * nc)).astype(dtype)
    nv = R.i420_to_nv12(fr, h, w)
    assert nv.shape == fr.shape and nv.dtype == dtype
    assert np.array_equal(nv[:, :ny], fr[:, :ny])
    assert np.array_equal(nv[:, ny::2], fr[:, ny:ny + nc]) and np.array_equal(nv[:, ny + 1::2], fr[:, ny + nc:])
    assert np.array_equal(R.nv12_to_i420(nv, h, w), fr)
    assert np.array_equal(np.sort(nv, axis=1), np.sort(fr, axis=1))   # the same multiset of samples
    lay = (w + 5, (h + 3) * (w + 5) + 1, 2 * wc + 3, (h + 3) * (w + 5) + 1 + hc * (2 * wc + 3) + 7)
    surf = R.to_surface(nv, h, w, lay, 0xA5)
    assert surf.shape == (3, lay[3]) and R.used_mask(h, w, lay).sum() == ny + 2 * nc
    assert np.array_equal(R.from_surface(surf, h, w, lay), nv)
    assert (surf[:, ~R.used_mask(h, w, lay)] == 0xA5).all()
    assert surf[0, (h - 1) * lay[0] + w - 1] == nv[0, ny - 1] and surf[0, lay[1] + 1] == nv[0, ny + 1]
    assert np.array_equal(R.to_surface(nv, h, w, R.tight(h, w), 0), nv)


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


GOOD = dict(raw="nv12", width=8, height=6, src_fps=24)


@pytest.mark.parametrize("cf,out,kw,match", [
    (1, "out.nv12", {}, "grayscale"),
    (3, "out.npy", {}, "no .npy output"),
    (3, "out.nv12", dict(width=None), "width"),
    (3, "out.nv12", dict(height=None), "height"),
    (3, "out.nv12", dict(src_fps=None), "src_fps"),
    (3, "out.nv12", dict(raw="nv21"), "raw"),
    (3, "out.nv12", dict(width=9), "whole number"),
    (3, "out.nv12", dict(matrix="bt2021"), "matrix"),
    (3, "out.nv12", dict(chunk_frames=0), "chunk_frames"),
], ids=["gray", "npy", "no-width", "no-height", "no-src-fps", "format", "file-size", "matrix", "chunk"])
def test_raw_route_refusals(tmp_path, no_gpu, cf, out, kw, match):
    src = tmp_path / "in.nv12"
    src.write_bytes(bytes(3 * colour.i420_frame_bytes(6, 8)))
    with pytest.raises(ValueError, match=match):
        _fi(cf).interpolate_video(str(src), str(tmp_path / out), **dict(GOOD, **kw))
    assert _no_output(tmp_path)


def test_size_without_raw_is_refused(tmp_path, no_gpu):
    with pytest.raises(ValueError, match="raw"):
        _fi(3).interpolate_video(str(tmp_path / "in.y4m"), str(tmp_path / "out.y4m"), width=8, height=6)
    assert _no_output(tmp_path)


def test_raw_reader_whole_frames_and_a_truncated_pipe():
    row = 10
    data = bytes(range(35))
    r = stream._RawReader(io.BytesIO(data[:30]), row)
    buf = np.zeros((2, row), np.uint8)
    assert r.read_into(buf, 2) == 2 and bytes(buf) == data[:20]
    assert r.read_into(buf, 2) == 1 and bytes(buf[0]) == data[20:30]
    assert r.read_into(buf, 2) == 0
    r = stream._RawReader(io.BytesIO(data), row)
    big = np.zeros((4, row), np.uint8)
    with pytest.raises(ValueError, match="ends inside a frame"):
        r.read_into(big, 4)


# ---- the CLI ----------------------------------------------------------------------------------------------------
def test_cli_raw_arguments():
    a = cli.parse_args(["video", "--input", "-", "--output", "-", "--raw", "nv12", "--size", "1920x1080", "--src-fps",
                        "24000/1001"])
    assert a.raw == "nv12" and a.size == (1920, 1080) and (a.src_fps.numerator, a.src_fps.denominator) == (24000, 1001)
    a = cli.parse_args(["video", "--input", "-", "--output", "-"])
    assert a.raw is None and a.size is None
    base = ["video", "--input", "-", "--output", "-"]
    for bad in (["--raw", "nv12", "--size", "1920x1080"],            # no --src-fps
                ["--raw", "nv12", "--src-fps", "24"],                # no --size
                ["--size", "64x48"],                                 # --size without --raw
                ["--raw", "nv21", "--size", "64x48", "--src-fps", "24"],
                ["--raw", "nv12", "--size", "64", "--src-fps", "24"],
                ["--raw", "nv12", "--size", "64x0", "--src-fps", "24"]):
        with pytest.raises(SystemExit):
            cli.parse_args(base + bad)


# ---- header and binding -----------------------------------------------------------------------------------------
def test_new_header_names_are_the_bindings_additions():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"\b(fiunet_[a-z0-9_]*(?:nv12|p010)[a-z0-9_]*)\s*\(", src)
    assert sorted(declared) == sorted(NEW)
    assert list(_native.SYMBOLS[-len(NEW):]) == NEW
    assert re.search(r"#define FIUNET_ABI_VERSION 8\b", src) and _native.ABI_VERSION == 8
    assert "typedef struct fiunet_surface_layout" in src
    assert [f for f, _ in _native.SurfaceLayout._fields_] == list(colour.SurfaceLayout._fields) == \
        re.search(r"fiunet_surface_layout \{\s*size_t ([^;]+);", src).group(1).replace(" ", "").split(",")
