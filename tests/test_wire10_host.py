"""CPU: the 10-bit 4:2:2 wire packings - the layout pinned by literals that no code here produced, the
numpy restatement's round trips, the sizes, the ABI names, and every host refusal of the `packing` keyword."""
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wire10_ref as R  # noqa: E402
import wire10_stream_rows  # noqa: E402,F401  (adds the two entry points to the stream-contract table)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, holdout, stream, wire10  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = {"v210": (2, 4, 6, 8, 46, 48, 50), "y210le": (2, 4, 6, 8, 46, 48, 50), "p210le": (1, 2, 4, 6, 7, 8, 46, 48, 50)}
CASES = [(p, w) for p in R.PACKINGS for w in WIDTHS[p]]


def _planar(seed, b, h, w, top=1024):
    return np.random.default_rng(seed).integers(0, top, (b, R.planar_samples(h, w))).astype(np.uint16)


# ---- 1. the layout, pinned independently of any code ----------------------------------------------------------------------
def test_the_literal_v210_group():
    y, u, v = np.arange(64, 70), np.array([512, 513, 514]), np.array([768, 769, 770])
    planar = np.concatenate([y, u, v]).astype(np.uint16)[None]
    wire = R.pack(planar, 1, 6, "v210")
    assert wire.shape == (1, 128) and not wire[0, 16:].any()
    assert [hex(x) for x in wire[0, :16].view("<u4")] == ["0x30010200", "0x4280441", "0x20210f01", "0x45c0844"]
    assert wire[0, :16].view("<u4").tolist() == [0x30010200, 0x04280441, 0x20210F01, 0x045C0844]
    assert np.array_equal(R.unpack(wire, 1, 6, "v210"), planar)


def test_the_literal_frame_sizes():
    for fb in (R.frame_bytes, wire10.frame_bytes):
        assert fb("v210", 1080, 1920) == 5120 * 1080 == 5_529_600
        assert fb("v210", 720, 1280) == 3456 * 720
        assert fb("y210le", 1080, 1920) == 4 * 1920 * 1080
        assert fb("p210le", 1080, 1920) == 2 * 2 * 1920 * 1080
        assert fb("p210le", 3, 7) == 2 * (21 + 2 * 3 * 4)
    assert R.row_bytes("v210", 1920) == wire10.row_bytes("v210", 1920) == 5120
    assert R.row_bytes("v210", 1280) == wire10.row_bytes("v210", 1280) == 3456
    for p, w in CASES:
        assert wire10.frame_bytes(p, 3, w) == R.frame_bytes(p, 3, w) and wire10.frame_bytes(p, 3, w) % 2 == 0
    assert wire10.planar_samples(3, 7) == R.planar_samples(3, 7) == P.colour.yuv_frame_samples("yuv422p10le", 3, 7)


def test_y210_and_p210_words_by_hand():
    planar = np.array([[100, 101, 102, 103, 200, 201, 300, 301]], dtype=np.uint16)   # 1 x 4: Y, U, V
    assert R.pack(planar, 1, 4, "y210le").view("<u2").tolist() == [[100 << 6, 200 << 6, 101 << 6, 300 << 6,
                                                                    102 << 6, 201 << 6, 103 << 6, 301 << 6]]
    assert R.pack(planar, 1, 4, "p210le").view("<u2").tolist() == [[100 << 6, 101 << 6, 102 << 6, 103 << 6,
                                                                    200 << 6, 300 << 6, 201 << 6, 301 << 6]]


# ---- 2. round trips of the restatement --------------------------------------------------------------------------------
@pytest.mark.parametrize("packing,w", CASES)
def test_unpack_of_pack_is_the_identity(packing, w):
    x = _planar(w, 2, 3, w)
    wire = R.pack(x, 3, w, packing)
    assert wire.shape == (2, R.frame_bytes(packing, 3, w))
    assert np.array_equal(R.unpack(wire, 3, w, packing), x)


@pytest.mark.parametrize("packing,w", CASES)
def test_pack_of_unpack_is_the_identity_on_canonical_frames(packing, w):
    """A canonical frame: ignored bits, fields past W and row padding zero - what `pack` writes.  Any frame becomes
    canonical through one round trip, and the ignored bits do not change what is read."""
    rng = np.random.default_rng(100 + w)
    noisy = rng.integers(0, 256, (2, R.frame_bytes(packing, 3, w)), dtype=np.uint8)
    x = R.unpack(noisy, 3, w, packing)
    assert x.max() <= 1023
    f = R.pack(x, 3, w, packing)
    assert np.array_equal(R.pack(R.unpack(f, 3, w, packing), 3, w, packing), f)
    if packing == "v210":
        words = f.view("<u4")
        assert not (words >> 30).any()
    else:
        assert not (f.view("<u2") & 63).any()
    if (packing, w) == ("v210", 50):   # 9 groups = 144 bytes of 256; the last group holds pixels 48, 49: 5 fields of 12
        rows = f.reshape(2, 3, 256)
        assert not rows[:, :, 144:].any()
        last = rows[:, :, 128:144].copy().view("<u4")
        assert not (last[..., 1] >> 10).any() and not last[..., 2:].any()


def test_words_above_1023_pack_as_1023():
    x = _planar(5, 1, 2, 12, top=65536)
    for p in R.PACKINGS:
        assert np.array_equal(R.unpack(R.pack(x, 2, 12, p), 2, 12, p), np.minimum(x, 1023))


def test_pitched_rows_of_the_restatement():
    x = _planar(6, 2, 3, 10)
    for p, pitch in (("v210", 192), ("y210le", 48)):
        wire = R.pack(x, 3, 10, p, pitch=pitch)
        assert wire.shape == (2, 3 * pitch) and np.array_equal(R.unpack(wire, 3, 10, p, pitch=pitch), x)
        tight = R.pack(x, 3, 10, p)
        rb = R.row_bytes(p, 10)
        assert np.array_equal(wire.reshape(2, 3, pitch)[:, :, :rb], tight.reshape(2, 3, rb))


# ---- 3. the ABI -----------------------------------------------------------------------------------------------------
NEW = ["fiunet_unpack_422p10", "fiunet_pack_422p10"]


def test_header_enum_and_binding():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"enum fiunet_packing10 \{([^}]*)\}", code)
    values = {k: int(v) for k, v in re.findall(r"FIUNET_PACK10_([A-Z0-9]+) = (\d+)", m.group(1))}
    assert values == {"V210": 0, "Y210": 1, "P210": 2}
    assert wire10.PACKINGS == {"v210": 0, "y210le": 1, "p210le": 2} == R.CODES
    assert (_native.PACK10_V210, _native.PACK10_Y210, _native.PACK10_P210) == (0, 1, 2)
    declared = re.findall(r"\b(fiunet_[a-z0-9_]+)\s*\(", code)
    assert set(NEW) <= set(declared) and set(NEW) <= set(_native.SYMBOLS)
    # added without a version bump, before the packed RGB / surface block that older tests read off the tail
    assert re.search(r"#define FIUNET_ABI_VERSION 8\b", src) and _native.ABI_VERSION == 8
    sym = list(_native.SYMBOLS)
    assert max(sym.index(n) for n in NEW) < sym.index("fiunet_packed_to_rgb_u8") and sym[-1] == "fiunet_forward_p010"
    for name in NEW:
        args = re.search(rf"int\s+{name}\s*\(([^)]*)\)", code).group(1)
        assert "const fiunet_packed_layout*" in args and "const fiunet_surface_layout*" in args
        assert args.strip().endswith("void* stream")


def test_library_exports_the_entry_points_and_kernels(hip_lib_built):
    import ctypes
    lib = ctypes.CDLL(hip_lib_built)
    for name in NEW:
        assert hasattr(lib, name)
    blob = open(hip_lib_built, "rb").read()
    assert b"unpack_422p10_kernel" in blob and b"pack_422p10_kernel" in blob


def test_one_translation_unit_holds_the_kernels():
    csrc = os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc")
    units = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    assert len(units) == 9
    assert '#include "wire10.hip.h"' in open(os.path.join(csrc, "formats.hip")).read()
    assert not re.search(r"\basm\b", open(os.path.join(csrc, "wire10.hip.h")).read())


def test_exports():
    assert P.wire10 is wire10 and "wire10" in P.__all__
    for name in ("PACKINGS", "frame_bytes", "unpack", "pack", "forward"):
        assert name in wire10.__all__ and hasattr(wire10, name)
    assert list(wire10.PACKINGS) == list(R.PACKINGS) == list(cli.PACKING_CHOICES)
    # the names stay out of the raw formats: they arrive through the keyword beside `raw`
    assert not set(wire10.PACKINGS) & set(stream.RAW_FORMATS) and not set(wire10.PACKINGS) & set(P.colour.YUV_FORMATS)


def test_layout_rules():
    PL, SL = P.PackedLayout, P.SurfaceLayout
    assert wire10.resolve_layout(None, "v210", 3, 50) == PL(256, 768)
    assert wire10.resolve_layout(PL(384, 0), "v210", 3, 50) == PL(384, 1152)
    assert wire10.resolve_layout(None, "y210le", 3, 50) == PL(200, 600)
    assert wire10.resolve_layout(None, "p210le", 3, 7) == SL(7, 21, 8, 45)
    assert wire10.resolve_layout(SL(16, 64, 16, 104), "p210le", 3, 7) == SL(16, 64, 16, 104)
    for bad, packing, h, w, match in ((PL(255, 0), "v210", 3, 50, "row_pitch"), (PL(0, 767), "v210", 3, 50, "frame_stride"),
                                      (PL(258, 0), "v210", 3, 50, None), (PL(257, 0), "v210", 3, 50, "even"),
                                      (PL(0, 0), "v210", 3, 7, "even width"), (PL(0, 0), "y210le", 3, 7, "even width"),
                                      (SL(0, 0, 0, 0), "v210", 3, 8, "PackedLayout"), (PL(0, 0), "p210le", 3, 8, "SurfaceLayout"),
                                      (SL(6, 0, 0, 0), "p210le", 3, 7, "luma_pitch"), (SL(0, 20, 0, 0), "p210le", 3, 7, "chroma_offset"),
                                      (SL(0, 0, 7, 0), "p210le", 3, 7, "chroma_pitch"), (SL(0, 0, 0, 44), "p210le", 3, 7, "frame_stride"),
                                      (None, "v410", 3, 8, "packing must be one of")):
        if match is None:
            wire10.resolve_layout(bad, packing, h, w)
            continue
        with pytest.raises(ValueError, match=match):
            wire10.resolve_layout(bad, packing, h, w)
    with pytest.raises(ValueError, match="frame_stride"):
        wire10.resolve_layout(SL(16, 64, 16, 64 + 2 * 16 + 7), "p210le", 3, 7)
    with pytest.raises(RuntimeError, match="no CPU path"):
        wire10.unpack(torch.zeros((1, 768), dtype=torch.uint8), 3, 50, "v210")
    with pytest.raises(RuntimeError, match="no CPU path"):
        wire10.pack(torch.zeros((1, R.planar_samples(3, 50)), dtype=torch.int16), 3, 50, "v210")
    with pytest.raises(ValueError, match="uint8"):
        wire10.unpack(torch.zeros((1, 767), dtype=torch.uint8), 3, 50, "v210")


# ---- 4. the video routes: refusals before any GPU work ------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(torch.Tensor, "pin_memory", boom)
    monkeypatch.setattr(stream, "_run", boom)
    monkeypatch.setattr(stream, "_run_whole", boom)
    monkeypatch.setattr(holdout, "_score_chunk", boom)
    monkeypatch.setattr(holdout.scene, "pair_sad", boom)
    monkeypatch.setattr(wire10, "unpack", boom)
    monkeypatch.setattr(wire10, "pack", boom)


def _model(frame_channels=3):
    return P.FrameInterpolationUNet(bilinear=True, frame_channels=frame_channels)


def _fi(frame_channels=3):
    return P.FrameInterpolator(model=_model(frame_channels), device="cpu")


def _no_output(tmp_path):
    return [p.name for p in tmp_path.iterdir() if p.name.startswith("out")] == []


GOOD = dict(raw="yuv422p10le", packing="v210", width=8, height=6, src_fps=24)
REFUSALS = [
    (dict(raw="yuv422p"), "yuv422p10le"),
    (dict(raw="nv12"), "yuv422p10le"),
    (dict(raw="uyvy422"), "yuv422p10le"),
    (dict(raw="yuv444p10le"), "yuv422p10le"),
    (dict(packing="v410"), r"packing must be one of \['v210', 'y210le', 'p210le'\]"),
    (dict(packing="V210"), "packing must be one of"),
    (dict(packing=0), "packing must be one of"),
    (dict(width=7), "even width"),
    (dict(packing="y210le", width=7), "even width"),
    (dict(resize=(7, 6)), "even width"),
    (dict(raw="v210", packing=None), "raw must be one of"),
    (dict(raw="v210"), "raw must be one of"),
    (dict(packing="y210le"), "whole number"),      # (the file gets 2 more bytes)
    (dict(packing="p210le"), "whole number"),
]


@pytest.mark.parametrize("kw,match", REFUSALS, ids=[f"{i}-{'-'.join(str(v) for v in kw.values())}" for i, (kw, _) in enumerate(REFUSALS)])
def test_video_refusals(tmp_path, no_gpu, kw, match):
    src = tmp_path / "in.v210"
    size = 3 * wire10.frame_bytes("v210", 6, 8)
    src.write_bytes(bytes(size + (2 if "whole number" in match else 0)))
    with pytest.raises(ValueError, match=match):
        _fi().interpolate_video(str(src), str(tmp_path / "out.v210"), **dict(GOOD, **kw))
    assert _no_output(tmp_path)
    with pytest.raises(ValueError, match=match):   # (the same opener: the packing's rules hold at both sizes here too)
        holdout.score_video(_model(), str(src), **dict(GOOD, **kw))


def _raw_file(frames):
    return lambda tmp_path, kw: _write(tmp_path / "in.raw", bytes(int(frames * (
        wire10.frame_bytes(kw["packing"], 6, 8) if kw.get("packing") else 2 * wire10.planar_samples(6, 8)))))


def _write(path, data):
    path.write_bytes(data)
    return path


def _npy_u16(tmp_path, kw):
    np.save(tmp_path / "in.npy", np.zeros((5, 6, 8), np.uint16))
    return tmp_path / "in.npy"


PLAIN = dict(GOOD, packing=None)
SOURCE_FAULTS = [   # (what makes the source, the keywords of both calls, the exception, a piece of its message)
    (_raw_file(1.5), PLAIN, ValueError, "288 bytes is not a whole number of 8x6 yuv422p10le frames of 192 bytes"),
    (_raw_file(1.5), GOOD, ValueError, "1152 bytes is not a whole number of 8x6 v210 frames of 768 bytes"),
    (lambda tmp_path, kw: tmp_path / "none.raw", GOOD, FileNotFoundError, "Video file not found"),
    (_raw_file(3), dict(GOOD, raw="nv12"), ValueError, "pass raw=\"yuv422p10le\" with it"),
    (_raw_file(3), dict(GOOD, width=7), ValueError, "even width"),
    (_raw_file(3), dict(GOOD, resize=(7, 6)), ValueError, "even width"),
    (_npy_u16, {}, ValueError, "expected a uint8 .npy stack"),
    (_raw_file(3), dict(GOOD, resize=(16, 6), resize_filter="area"), ValueError, "area"),
]


@pytest.mark.parametrize("make,kw,exc,piece", SOURCE_FAULTS,
                         ids=["part-frame-plain", "part-frame-v210", "missing", "packing-nv12", "odd-source", "odd-resize",
                              "npy-uint16", "area-grows"])
def test_a_source_fault_is_the_same_refusal_from_both_entry_points(tmp_path, no_gpu, make, kw, exc, piece):
    """The video routes and hold-out scoring open a source through the same opener (stream.py): the same exception type
    with the same text, before any GPU work, and no output file (`.part` included)."""
    src = make(tmp_path, kw)
    with pytest.raises(exc) as video:
        _fi(1 if src.suffix == ".npy" else 3).interpolate_video(str(src), str(tmp_path / ("out" + src.suffix)), **kw)
    with pytest.raises(exc) as scoring:
        holdout.score_video(_model(1 if src.suffix == ".npy" else 3), str(src), **kw)
    assert type(video.value) is type(scoring.value) is exc
    assert str(video.value) == str(scoring.value) and piece in str(video.value)
    assert _no_output(tmp_path)


def test_whole_wire_frames_are_counted_not_working_frames(tmp_path, no_gpu):
    """3 v210 frames of 8 x 6 are 3 x 768 bytes; as yuv422p10le (192 bytes a frame) the same file would pass as 12 frames."""
    src = tmp_path / "in.v210"
    src.write_bytes(bytes(3 * 768 - 192))
    with pytest.raises(ValueError, match="whole number of 8x6 v210 frames of 768 bytes"):
        _fi().interpolate_video(str(src), str(tmp_path / "out.v210"), **GOOD)
    with pytest.raises(ValueError, match="whole number of 8x6 v210 frames of 768 bytes"):
        holdout.score_video(_model(), str(src), **GOOD)
    assert _no_output(tmp_path)


def test_y4m_and_npy_take_no_packing(tmp_path, no_gpu):
    np.save(tmp_path / "clip.npy", np.zeros((5, 16, 16, 3), np.uint8))
    y4m = tmp_path / "clip.y4m"
    y4m.write_bytes(b"YUV4MPEG2 W16 H16 F24:1 C420jpeg\n" + (b"FRAME\n" + bytes(16 * 16 * 3 // 2)) * 3)
    for src in (tmp_path / "clip.npy", y4m):
        with pytest.raises(ValueError, match="take no packing"):
            _fi().interpolate_video(str(src), str(tmp_path / ("out" + src.suffix)), packing="v210")
        with pytest.raises(ValueError, match="take no packing"):
            holdout.score_video(_model(), str(src), packing="v210")
    with pytest.raises(ValueError, match="take no packing"):
        _fi().interpolate_video(io.BytesIO(y4m.read_bytes()), io.BytesIO(), packing="p210le", chunk_frames=2)
    assert _no_output(tmp_path)


def test_grayscale_model_is_refused_as_on_the_working_route(tmp_path, no_gpu):
    src = tmp_path / "in.v210"
    src.write_bytes(bytes(3 * 768))
    with pytest.raises(ValueError, match="grayscale"):
        _fi(1).interpolate_video(str(src), str(tmp_path / "out.v210"), **GOOD)


def test_the_wire_sizes_of_a_run():
    w = stream.check_packing("v210", "yuv422p10le", 6, 8, (50, 4))
    assert (w.in_row, w.out_row, w.src, w.dst) == (768 // 2, 4 * 256 // 2, (6, 8), (4, 50))
    assert stream.check_packing(None, "nv12") is None
    w = stream.check_packing("p210le", "yuv422p10le", 3, 7)
    assert w.in_row == w.out_row == 45


# ---- 5. the command line ------------------------------------------------------------------------------------------------
def test_cli_accepts_the_three_names_and_rejects_others(capsys):
    base = ["--input", "-", "--raw", "yuv422p10le", "--size", "1920x1080", "--model", "m.pth"]
    for name in wire10.PACKINGS:
        a = cli.parse_args(["video", "--output", "-", "--src-fps", "30"] + base + ["--packing", name])
        assert a.packing == name and a.raw == "yuv422p10le"
        assert cli.parse_args(["evaluate"] + base + ["--packing", name]).packing == name
    assert cli.parse_args(["video", "--output", "-", "--src-fps", "30"] + base).packing is None
    for bad in ("v410", "V210", "y210", "p210", "yuv422p10le"):
        with pytest.raises(SystemExit):
            cli.parse_args(["evaluate"] + base + ["--packing", bad])
    for cmd in (["video", "--output", "-", "--src-fps", "30"], ["evaluate"]):
        with pytest.raises(SystemExit):   # the packing of another raw format, or of none
            cli.parse_args(cmd + ["--input", "-", "--raw", "nv12", "--size", "8x6", "--model", "m.pth", "--packing", "v210"])
        with pytest.raises(SystemExit):
            cli.parse_args(cmd + ["--input", "-", "--model", "m.pth", "--packing", "v210"])
        with pytest.raises(SystemExit):   # v210 is no --raw name
            cli.parse_args(cmd + ["--input", "-", "--raw", "v210", "--size", "8x6", "--model", "m.pth"])
    capsys.readouterr()
    assert "--packing v210" in cli.__doc__ and "-c:v v210 -f rawvideo" in cli.__doc__
    assert "-f rawvideo -c:v v210 -s 1920x1080" in cli.__doc__


def test_raw_v210_keeps_its_refusal():
    with pytest.raises(ValueError, match="raw must be one of"):
        stream._raw_route(_model(), "v210", 6, 8, False, 2, "bt709", None)
    assert "v210" not in stream.RAW_FORMATS and "v210" not in cli.RAW_CHOICES


def test_documents_name_the_section():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "3.3s" in design and "unpinned against ffmpeg" in readme.lower().replace("\n", " ")
    for word in ("--raw v210", "P216", "12 bits"):
        assert word in design
