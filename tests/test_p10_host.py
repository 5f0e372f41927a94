"""CPU: 10-bit video.  The integer YUV 4:2:0 <-> RGB definition at 10 bits (tests/colour10_ref.py, restating
csrc/colour.hip.h on uint16 samples) against the float64 textbook formulas for BT.601, BT.709 and BT.2020, the 10-bit
Y4M reader and writer, the colour flags, and the argument checks of the 10-bit entry points that come before any GPU
work."""
import ctypes
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour10_ref as C  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO  # noqa: E402

CONFIGS = [(m, r) for m in ("bt601", "bt709", "bt2020") for r in ("limited", "full")]


def _grid(lo, hi, step=8):
    """lo .. hi in steps of `step`, both extremes included."""
    return np.unique(np.r_[np.arange(lo, hi + 1, step), hi]).astype(np.int64)


@pytest.mark.parametrize("matrix,colour_range", CONFIGS)
def test_decode_every_y_code_within_one_code_of_textbook(matrix, colour_range):
    k = C.coef(matrix, colour_range)
    ylo, yhi, clo, chi = (64, 940, 64, 960) if colour_range == "limited" else (0, 1023, 0, 1023)
    cs = _grid(clo, chi)
    assert len(cs) >= 113 and cs[0] == clo and cs[-1] == chi
    cb, cr = (a.ravel() for a in np.meshgrid(cs, cs, indexing="ij"))
    for y in range(ylo, yhi + 1):
        yy = np.full_like(cb, y)
        got = C.decode(yy, 16 * cb, 16 * cr, k)   # flat chroma: the x16 up-sampled value is 16 * the sample
        want = C.textbook_decode(yy, cb, cr, matrix, colour_range)
        for gch, wch in zip(got, want):
            assert np.abs(gch.astype(np.int64) - np.clip(wch, 0, 1023)).max() <= 1, y


@pytest.mark.parametrize("matrix,colour_range", CONFIGS)
def test_encode_rgb_grid_within_one_code_of_textbook(matrix, colour_range):
    k = C.coef(matrix, colour_range)
    g = _grid(0, 1023)
    r, gg, b = (a.ravel() for a in np.meshgrid(g, g, g, indexing="ij"))
    ty, tcb, tcr = C.textbook_encode(r, gg, b, matrix, colour_range)
    y = C.encode_y(r, gg, b, k).astype(np.int64)
    assert np.abs(y - np.clip(ty, 0, 1023)).max() <= 1
    for n in (4, 8):   # a flat jpeg 2x2 block / a flat mpeg2 [1,2,1] x [1,1] footprint
        cb, cr = (c.astype(np.int64) for c in C.encode_c(n * r, n * gg, n * b, n, k))
        assert np.abs(cb - np.clip(tcb, 0, 1023)).max() <= 1
        assert np.abs(cr - np.clip(tcr, 0, 1023)).max() <= 1


@pytest.mark.parametrize("matrix,colour_range", CONFIGS)
def test_grey_encodes_to_centre_chroma_exactly(matrix, colour_range):
    k = C.coef(matrix, colour_range)
    assert k["yr"] + k["yg"] + k["yb"] == C._rnd(1.0 if colour_range == "full" else 876 / 1023)
    assert k["cbr"] + k["cbg"] + k["cbb"] == 0 and k["crr"] + k["crg"] + k["crb"] == 0
    v = np.arange(1024, dtype=np.int64)
    for n in (4, 8):
        cb, cr = C.encode_c(n * v, n * v, n * v, n, k)
        assert (cb == 512).all() and (cr == 512).all()
    y = C.encode_y(v, v, v, k).astype(np.int64)
    r, g, b = C.decode(y, np.full_like(y, 16 * 512), np.full_like(y, 16 * 512), k)
    assert (r == g).all() and (g == b).all()
    if colour_range == "full":
        assert (r == v).all()   # full range: grey round-trips exactly


@pytest.mark.parametrize("matrix,colour_range", CONFIGS)
def test_int32_bounds_of_the_kernels(matrix, colour_range):
    """The worst-case intermediates over every input (the corners of the sample cube; every term is linear in one
    input) stay below the bounds colour.hip.h states: 6.0e8 for the decode, 2.1e8 for the encode."""
    k = C.coef(matrix, colour_range)
    top = 16 * 1023
    dec = max(abs(int(t)) for y, u, v in itertools.product((0, 1023), (0, top), (0, top))
              for t in C.decode_terms(np.int64(y), np.int64(u), np.int64(v), k))
    assert dec <= 6.0e8 < 2 ** 31
    enc = 0
    for n, sh in ((4, 16), (8, 17)):
        bias = (512 << sh) + (1 << (sh - 1))
        for row in (("cbr", "cbg", "cbb"), ("crr", "crg", "crb")):
            enc = max(enc, sum(abs(k[c]) for c in row) * n * 1023 + bias)
    enc = max(enc, (k["yr"] + abs(k["yg"]) + k["yb"]) * 1023 + k["yoff"] * C.S + C.S // 2)
    assert enc <= 2.1e8


@pytest.mark.parametrize("siting", ["jpeg", "mpeg2"])
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (5, 7), (49, 67)])
def test_flat_colour_frames_round_trip(siting, h, w):
    rng = np.random.default_rng(h * 100 + w)
    for matrix, colour_range in CONFIGS:
        col = rng.integers(0, 1024, size=(3, 3, 1, 1))
        rgb = np.broadcast_to(col, (3, 3, h, w)).astype(np.uint16)
        f = C.rgb_to_yuv420p10(rgb, siting, matrix, colour_range)
        assert f.dtype == np.uint16 and f.shape == (3, P.yuv420p10_frame_samples(h, w))
        back = C.yuv420p10_to_rgb(f, h, w, siting, matrix, colour_range)
        assert np.abs(back.astype(int) - rgb.astype(int)).max() <= 3


def test_samples_above_1023_read_as_1023():
    k = C.coef("bt2020", "full")
    f = np.full((1, C.frame_samples(4, 4)), 0xFFFF, np.uint16)
    want = C.yuv420p10_to_rgb(np.full_like(f, 1023), 4, 4, "jpeg", "bt2020", "full")
    assert np.array_equal(C.yuv420p10_to_rgb(f, 4, 4, "jpeg", "bt2020", "full"), want)
    assert C.pre10(np.array([1023, 1024, 65535])).tolist() == [1.0, 1.0, 1.0]
    assert k["yoff"] == 0


def test_pre10_post10_reference_values():
    codes = np.arange(1024)
    x = C.pre10(codes)
    assert x[0] == -1.0 and x[1023] == 1.0 and x.dtype == np.float32
    assert (np.diff(x) > 0).all()
    want = (codes.astype(np.float32) / np.float32(1023)) * np.float32(2) - np.float32(1)
    assert np.array_equal(x, want)
    assert C.post10(np.array([-1.0, 1.0, 0.0, 5.0, -5.0, np.nan], np.float32)).tolist() == [0, 1023, 511, 1023, 0, 0]


# ---- the Y4M container at 10 bits -----------------------------------------------------------------------------
def _planes(rng, n, h, w, tag):
    y = rng.integers(0, 1024, (n, h, w), dtype=np.uint16)
    if tag == "mono10":
        return y, None
    ch = {"420p10": ((h + 1) // 2, (w + 1) // 2), "422p10": (h, (w + 1) // 2), "444p10": (h, w)}[tag]
    return y, (rng.integers(0, 1024, (n,) + ch, dtype=np.uint16), rng.integers(0, 1024, (n,) + ch, dtype=np.uint16))


@pytest.mark.parametrize("tag", ["420p10", "422p10", "444p10", "mono10"])
@pytest.mark.parametrize("h,w", [(3, 5), (49, 67), (16, 17)])
def test_y4m_p10_round_trips_odd_sizes(tmp_path, tag, h, w):
    rng = np.random.default_rng(h * w)
    n = 3
    y, ch = _planes(rng, n, h, w, tag)
    p = tmp_path / "o.y4m"
    IO.write_y4m_p10(str(p), y, ch, fps=(30000, 1001), colourspace=tag, colour_range="LIMITED")
    y2, ch2, fps, cs = IO.read_y4m_p10(str(p))
    assert y2.dtype == np.uint16 and np.array_equal(y2, y)
    assert (ch2 is None) == (ch is None) and (ch is None or all(np.array_equal(a, b) for a, b in zip(ch, ch2)))
    assert fps == (30000, 1001) and cs == tag
    frames, hdr = IO.read_y4m_packed_p10(str(p))
    want = [y.reshape(n, -1)] + ([] if ch is None else [c.reshape(n, -1) for c in ch])
    assert frames.dtype == np.uint16 and np.array_equal(frames, np.concatenate(want, axis=1))
    assert hdr["colour_range"] == "LIMITED" and hdr["bits"] == 10 and hdr["frame_bytes"] == 2 * frames.shape[1]
    if tag == "420p10":
        assert frames.shape[1] == P.yuv420p10_frame_samples(h, w)
    # the samples are little-endian 16-bit words after each FRAME line
    raw = p.read_bytes()
    first = raw.index(b"FRAME\n") + 6
    assert raw[first:first + 2] == int(y[0, 0, 0]).to_bytes(2, "little")


def test_y4m_p10_reads_the_ffmpeg_header(tmp_path):
    h, w = 4, 6
    y = np.arange(h * w, dtype="<u2") * 40
    u = np.full(6, 300, "<u2")
    v = np.full(6, 700, "<u2")
    p = tmp_path / "ff.y4m"
    p.write_bytes(b"YUV4MPEG2 W6 H4 F25:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=LIMITED\nFRAME\n"
                  + y.tobytes() + u.tobytes() + v.tobytes())
    frames, hdr = IO.read_y4m_packed_p10(str(p))
    assert hdr["colourspace"] == "420p10" and hdr["colour_range"] == "LIMITED" and hdr["fps"] == (25, 1)
    assert frames.shape == (1, 36) and frames[0, :24].tolist() == y.tolist() and frames[0, 24:30].tolist() == [300] * 6
    # what write_y4m_p10 writes is that header
    IO.write_y4m_p10(str(tmp_path / "w.y4m"), y.reshape(1, h, w), (u.reshape(1, 2, 3), v.reshape(1, 2, 3)),
                     fps=(25, 1), colour_range="LIMITED")
    assert (tmp_path / "w.y4m").read_bytes() == p.read_bytes()
    IO.write_y4m_p10(str(tmp_path / "m.y4m"), y.reshape(1, h, w))
    assert (tmp_path / "m.y4m").read_bytes().startswith(b"YUV4MPEG2 W6 H4 F30:1 Ip A1:1 Cmono10\nFRAME\n")


def test_y4m_p10_rejects_bad_streams(tmp_path):
    bad = tmp_path / "bad.y4m"
    bad.write_bytes(b"YUV4MPEG2 W4 H4 F25:1 C420p10\nFRAME\n" + bytes(47))   # one byte short of 24 samples
    with pytest.raises(ValueError, match="truncated"):
        IO.read_y4m_p10(str(bad))
    for tag in ("420p12", "422p14", "444p16", "mono12", "mono16"):
        bad.write_bytes(f"YUV4MPEG2 W4 H4 F25:1 C{tag}\nFRAME\n".encode() + bytes(96))
        with pytest.raises(ValueError, match="bit depth"):
            IO.read_y4m_packed_p10(str(bad))
    bad.write_bytes(b"YUV4MPEG2 W4 H4 F25:1 C420jpeg\nFRAME\n" + bytes(24))
    with pytest.raises(ValueError, match="10-bit"):
        IO.read_y4m_p10(str(bad))
    with pytest.raises(ValueError):
        IO.write_y4m_p10(str(bad), np.zeros((1, 4, 4), np.uint16), colourspace="420p12")
    # the 8-bit reader keeps refusing 10-bit streams
    bad.write_bytes(b"YUV4MPEG2 W4 H4 F25:1 C420p10\nFRAME\n" + bytes(48))
    with pytest.raises(ValueError, match="bit depth"):
        IO.read_y4m(str(bad))
    assert IO.y4m_colourspace(str(bad)) == "420p10"


# ---- flags and the entry points' checks before any GPU work ---------------------------------------------------
def test_colour_flags_bits():
    assert P.colour.colour_flags() == _native.YUV_BT709
    assert P.colour.colour_flags(bits=10) == _native.YUV_BT709
    assert P.colour.colour_flags("mpeg2", "bt2020", "full", bits=10) == (
        _native.YUV_MPEG2 | _native.YUV_BT2020 | _native.YUV_FULL_RANGE)
    assert P.colour.colour_flags("jpeg", "bt601", "limited", bits=10) == 0
    with pytest.raises(ValueError, match="bt2020|matrix"):
        P.colour.colour_flags(matrix="bt2020")
    with pytest.raises(ValueError, match="matrix"):
        P.colour.colour_flags(matrix="bt2020", bits=8)
    for bits in (9, 12, 16):
        with pytest.raises(ValueError, match="bits"):
            P.colour.colour_flags(bits=bits)
    assert P.yuv420p10_frame_samples(1080, 1920) == P.i420_frame_bytes(1080, 1920)


def test_c_abi_rejects_bad_p10_arguments_without_gpu(hip_lib_built):
    """Host-side checks that return before any launch (status 1: invalid argument, 2: bad shape)."""
    lib = _native.lib()
    fake = ctypes.c_void_p(256)
    big = 1 << 30
    # conversions: unknown bits, BT.709 with BT.2020, NULL pointers, bad shape, short strides
    for fn in (lambda c: lib.fiunet_yuv420p10_to_rgb_p10(fake, 0, fake, 1, 16, 16, c, None),
               lambda c: lib.fiunet_rgb_p10_to_yuv420p10(fake, fake, 0, 1, 16, 16, c, None)):
        assert fn(16) == 1 and fn(1 << 31) == 1
        assert fn(_native.YUV_BT709 | _native.YUV_BT2020) == 1
    assert lib.fiunet_yuv420p10_to_rgb_p10(None, 0, fake, 1, 16, 16, 0, None) == 1
    assert lib.fiunet_rgb_p10_to_yuv420p10(fake, None, 0, 1, 16, 16, 0, None) == 1
    assert lib.fiunet_yuv420p10_to_rgb_p10(fake, 0, fake, 0, 16, 16, 0, None) == 2
    assert lib.fiunet_yuv420p10_to_rgb_p10(fake, 383, fake, 1, 16, 16, 0, None) == 1   # 384 samples per frame
    assert lib.fiunet_rgb_p10_to_yuv420p10(fake, fake, 100, 1, 16, 16, 0, None) == 1
    # the 8-bit conversions keep rejecting the BT.2020 bit
    assert lib.fiunet_yuv420_to_rgb_u8(fake, 0, fake, 1, 16, 16, _native.YUV_BT2020, None) == 1
    assert lib.fiunet_rgb_to_yuv420_u8(fake, fake, 0, 1, 16, 16, _native.YUV_BT2020, None) == 1
    # forwards: NULL pointers, H or W < 16, short frame stride, colour bits (before the context is looked at)
    assert lib.fiunet_forward_p10(None, None, fake, fake, 0, 1, 64, 64, 0, fake, big, None) == 1
    assert lib.fiunet_forward_p10(None, fake, fake, fake, 0, 1, 64, 64, 0, fake, big, None) == 1   # NULL ctx
    assert lib.fiunet_forward_p10(None, fake, fake, fake, 0, 1, 15, 64, 0, fake, big, None) == 2
    assert lib.fiunet_forward_p10(None, fake, fake, fake, 0, 1, 64, 8, 0, fake, big, None) == 2
    yuv = lambda *a: lib.fiunet_forward_yuv420p10(*a)  # noqa: E731
    assert yuv(None, fake, None, fake, 0, 1, 64, 64, 0, 0, fake, big, None) == 1
    assert yuv(None, fake, fake, fake, 0, 1, 8, 64, 0, 0, fake, big, None) == 2
    assert yuv(None, fake, fake, fake, 0, 1, 64, 15, 0, 0, fake, big, None) == 2
    assert yuv(None, fake, fake, fake, 100, 1, 64, 64, 0, 0, fake, big, None) == 1   # < 6144 samples per frame
    assert yuv(None, fake, fake, fake, 0, 1, 64, 64, 32, 0, fake, big, None) == 1
    assert yuv(None, fake, fake, fake, 0, 1, 64, 64, _native.YUV_BT709 | _native.YUV_BT2020, 0, fake, big, None) == 1
    assert lib.fiunet_workspace_bytes_p10(None, 1, 64, 64, 0) == 0
    assert lib.fiunet_workspace_bytes_yuv420p10(None, 1, 64, 64, 0) == 0
    assert lib.fiunet_preprocess_p10(None, fake, 4, None) == 1
    assert lib.fiunet_postprocess_p10(fake, None, 4, None) == 1


def _interpolator(frame_channels):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=frame_channels).eval()   # stays on the CPU
    return P.FrameInterpolator(model=m, device="cuda")


@pytest.mark.parametrize("tag", ["422p10", "444p10", "mono10"])
def test_rgb_model_rejects_non_420_p10_tags(tmp_path, tag):
    y, ch = _planes(np.random.default_rng(0), 2, 16, 16, tag)
    p = tmp_path / "in.y4m"
    IO.write_y4m_p10(str(p), y, ch, colourspace=tag)
    with pytest.raises(ValueError, match=f"C{tag}"):
        _interpolator(3).interpolate_video(str(p), str(tmp_path / "out.y4m"), 2)


def test_video_options_checked_before_gpu(tmp_path):
    y, ch = _planes(np.random.default_rng(1), 2, 16, 16, "420p10")
    p = tmp_path / "in.y4m"
    IO.write_y4m_p10(str(p), y, ch)
    with pytest.raises(ValueError, match="matrix"):
        _interpolator(3).interpolate_video(str(p), str(tmp_path / "out.y4m"), 2, matrix="bt2100")
    with pytest.raises(ValueError, match="siting"):
        _interpolator(3).interpolate_video(str(p), str(tmp_path / "out.y4m"), 2, siting="left")
    with pytest.raises(ValueError, match=r"\.y4m"):
        _interpolator(3).interpolate_video(str(p), str(tmp_path / "out.npy"), 2)
    # 8-bit video: bt2020 is refused (BT.2020 defines 10- and 12-bit coding only)
    q = tmp_path / "in8.y4m"
    IO.write_y4m(str(q), np.zeros((2, 16, 16), np.uint8), (np.zeros((2, 8, 8), np.uint8),) * 2)
    with pytest.raises(ValueError, match="matrix"):
        _interpolator(3).interpolate_video(str(q), str(tmp_path / "out.y4m"), 2, matrix="bt2020")


def test_p10_forwards_reject_bad_inputs_before_gpu():
    rgb = P.FrameInterpolationUNet(bilinear=True, frame_channels=3).eval()
    gray = P.FrameInterpolationUNet(bilinear=True, frame_channels=1).eval()
    f = torch.zeros(1, P.yuv420p10_frame_samples(16, 16), dtype=torch.uint16)
    with pytest.raises(RuntimeError, match="RGB"):
        gray.forward_yuv420p10(f, f, 16, 16)
    with pytest.raises(ValueError, match="matrix"):
        rgb.forward_yuv420p10(f, f, 16, 16, matrix="bt2100")
    with pytest.raises(RuntimeError, match="GPU|HIP device"):
        rgb.forward_yuv420p10(f, f, 16, 16, matrix="bt2020")
    with pytest.raises(RuntimeError, match="HIP device"):
        gray.forward_p10(torch.zeros(1, 1, 16, 16, dtype=torch.uint16), torch.zeros(1, 1, 16, 16, dtype=torch.uint16))
    with pytest.raises(RuntimeError, match="channel"):
        rgb.forward_p10(torch.zeros(1, 1, 16, 16, dtype=torch.uint16), torch.zeros(1, 1, 16, 16, dtype=torch.uint16))
