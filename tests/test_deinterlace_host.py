"""CPU: the deinterlacer's definition (tests/deinterlace_ref.py), the host side of `fi.deinterlace`, the
`I` token of a Y4M header, the refusals of `deinterlace_video` and of the C entry points (which return before any launch,
so they need no GPU), and the warning of the commands that take interlaced frames as they are."""
import io
import os
import sys
import warnings
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deinterlace_ref as R  # noqa: E402
import deinterlace_stream_rows  # noqa: E402,F401  (registers the stream-contract rows of the two entry points)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, deinterlace as D, holdout, imageio_lite as IO, stream  # noqa: E402
from ai_based_frame_interpolation_amd.layout import frame_layout  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H, W = 24, 40


# ---- 1. a static clip -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", R.ORDERS)
def test_a_static_clip_passes_through_without_the_spatial_check_and_not_with_it(order):
    still = np.random.default_rng(1).integers(0, 256, (H, W)).astype(np.uint8)
    clip = R.interlace(np.repeat(still[None], 8, axis=0), order)
    assert np.array_equal(clip, np.repeat(still[None], 4, axis=0))
    for rate in R.RATES:
        out = R.deinterlace(clip, order, rate, "adaptive", spatial_check=False)
        assert out.shape[0] == (8 if rate == "field" else 4)
        assert all(np.array_equal(f, still) for f in out)
        checked = R.deinterlace(clip, order, rate, "adaptive", spatial_check=True)
        assert not np.array_equal(checked, out)   # (uniform noise looks combed to the check: the flag is wired this way)
        kept = 1 if order == "bff" else 0
        assert np.array_equal(checked[0][kept::2], still[kept::2])


# ---- 2. what it is for ------------------------------------------------------------------------------------------------------
SQUARE = 192   # mid-gray + 64; see test_adaptive_beats_bob_against_the_progressive_truth


def _moving_square(speed, n_fields=10, seed=2):
    """A 5x5-box-blurred random background (mean 127, sigma 15) with an 8x8 square of value SQUARE moving `speed` px per
    field from column 2 on; it stays inside the frame (2 + 3 * 9 + 8 <= 40) -> [n_fields, H, W] uint8."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 256, (H + 4, W + 4)).astype(np.int64)
    bg = sum(noise[dy:dy + H, dx:dx + W] for dy in range(5) for dx in range(5)) // 25
    clip = np.repeat(bg[None], n_fields, axis=0)
    for f in range(n_fields):
        x = 2 + speed * f
        assert x + 8 <= W
        clip[f, 8:16, x:x + 8] = SQUARE
    return clip.astype(np.uint8)


def _psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2, axis=(1, 2))
    return float(np.mean(10 * np.log10(255.0 ** 2 / np.maximum(mse, 1e-12))))


@pytest.mark.parametrize("speed", [0, 1, 3])
def test_adaptive_beats_bob_against_the_progressive_truth(speed):
    """Mean PSNR over the frames, adaptive minus bob, measured with tests/deinterlace_ref.py on the clips above:
    0 px per field +9.59 dB, 1 px +4.93 dB, 3 px +1.71 dB.  The bound is 1 dB in each row.

    The square's value is this test's choice: 192, a quarter of the range above the mid-gray background.  What the two
    methods differ in is the background and the square's interior; the square's moving top and bottom edge is rebuilt
    by neither (no row of the field holds it), and that shared error grows with the square of its contrast.  At video
    white it drowns the difference: 235 measures +11.86 / +3.87 / +0.10 dB on this seed, and seeds 0..3 agree (the 3 px
    row crosses 1 dB near 200).  A square of the contrast of an object in a scene keeps the comparison about the
    deinterlacers."""
    truth = _moving_square(speed)
    clip = R.interlace(truth, "tff")
    gain = _psnr(R.deinterlace(clip, "tff", "field", "adaptive"), truth) - _psnr(R.deinterlace(clip, "tff", "field", "bob"), truth)
    print(f"speed {speed}: adaptive - bob = {gain:+.2f} dB")
    assert gain >= 1.0, gain


# ---- 3. one sample on each branch, by hand ---------------------------------------------------------------------------------
def _three_rows(c, e, prev_mid, cur_mid, x):
    """Three-row frames (tff, field 0: row 1 is missing, ym = 0, yp = 2, no spatial check at this height): rows 0 and 2 are
    c and e in prev, cur and next (t1 = t2 = 0); row 1 differs at x between prev and cur -> out[1][x] of frame 1."""
    cur = np.zeros((3, len(c)), np.uint8)
    cur[0], cur[2] = c, e
    prev = cur.copy()
    prev[1, x], cur[1, x] = prev_mid, cur_mid
    out = R.deinterlace(np.stack([prev, cur, cur]), "tff", "frame", "adaptive", first=1, count=1)
    return int(out[0, 1, x])


def test_direction_minus_two_is_taken():
    # x = 4: S(0) = 160 + 150 + 40 = 350, score 349; S(-1) = 170 + 20 + 16 = 206, taken; S(-2) = 0 + 4 + 0 = 4, taken:
    # pred = (c[2] + e[6]) >> 1 = (30 + 34) >> 1 = 32; S(+1) = 150 + 140 + 130 = 420 fails.  d = (0 + 64) >> 1 = 32,
    # diff = t0 >> 1 = 32: the band [0, 64] leaves 32 alone.  (Direction -1 alone would give (40 + 20) >> 1 = 30.)
    c = [10, 20, 30, 40, 50, 60, 70, 80, 90]
    e = [200, 200, 200, 200, 200, 20, 34, 40, 200]
    assert _three_rows(c, e, 0, 64, 4) == 32


def test_direction_plus_one_is_taken_after_minus_one_failed():
    # x = 4: S(0) = 140 + 24 + 30 = 194, score 193; S(-1) = 126 + 110 + 50 = 286 fails; S(+1) = 0 + 0 + 4 = 4, taken:
    # pred = (c[5] + e[3]) >> 1 = 60; S(+2) = 40 + 20 + 140 = 200 fails.  d = (20 + 100) >> 1 = 60, diff = 40.
    # (Without a direction pred would be (50 + 74) >> 1 = 62.)
    c = [200, 200, 200, 200, 50, 60, 70, 200, 200]
    e = [10, 20, 50, 60, 74, 90, 100, 110, 120]
    assert _three_rows(c, e, 20, 100, 4) == 60


def test_the_clamp_on_both_sides():
    # two columns (no direction search): pred = (100 + 120) >> 1 = 110 and (10 + 30) >> 1 = 20; d = (50 + 54) >> 1 = 52
    # and (80 + 90) >> 1 = 85, diff = 4 >> 1 = 2 and 10 >> 1 = 5: 110 comes down to 54, 20 comes up to 80
    cur = np.array([[100, 10], [54, 90], [120, 30]], np.uint8)
    prev = cur.copy()
    prev[1] = [50, 80]
    out = R.deinterlace(np.stack([prev, cur, cur]), "tff", "frame", "adaptive", first=1, count=1)
    assert out[0, 1].tolist() == [54, 80]
    assert R.deinterlace(np.stack([prev, cur, cur]), "tff", "frame", "bob", first=1, count=1)[0, 1].tolist() == [110, 20]


def test_a_mirrored_row():
    # bff, field 0 keeps the odd rows: row 0 of a two-row frame is missing, ym = yp = 1, so pred = cur[1] = 77, 33;
    # d = (70 + 90) >> 1 = 80 and (40 + 20) >> 1 = 30, diff = 20 >> 1 = 10: both inside their bands
    cur = np.array([[90, 20], [77, 33]], np.uint8)
    prev = np.array([[70, 40], [77, 33]], np.uint8)
    out = R.deinterlace(np.stack([prev, cur, cur]), "bff", "frame", "adaptive", first=1, count=1)
    assert out[0].tolist() == [[77, 33], [77, 33]]
    # tff: row 1 = H - 1 is missing, ym = yp = 0
    assert R.deinterlace(cur[None], "tff", "frame", "bob")[0].tolist() == [[90, 20], [90, 20]]


def test_no_direction_search_left_of_column_three():
    # x = 2: S(0) = 180 + 20 + 16 = 216 and S(-1) = 0 + 4 + 0 = 4 would take pred = (c[1] + e[3]) >> 1 = 22, but x < 3:
    # pred = (c[2] + e[2]) >> 1 = (30 + 10) >> 1 = 20; d = 30, diff = 30
    c = [10, 20, 30, 40, 50, 60, 70, 80, 90]
    e = [200, 200, 10, 24, 30, 40, 50, 60, 70]
    assert _three_rows(c, e, 0, 60, 2) == 20
    # the same rows one column further in, where the search runs: x = 3, S(0) = 20 + 16 + 20 = 56, S(-1) = 4 + 0 + 0 = 4
    # taken, pred = (c[2] + e[4]) >> 1 = 30, S(-2) = |c[0] - e[4]| + |c[1] - e[5]| + |c[2] - e[6]| = 20 + 20 + 20 fails,
    # S(+1) = |c[3] - e[1]| + ... fails; d = 30, diff = 30
    assert _three_rows(c, e, 0, 60, 3) == 30


# ---- 4., 5. fields and rates ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("order", R.ORDERS)
def test_interlace_then_deinterlace_keeps_the_kept_rows_and_frame_rate_is_the_even_outputs(order, bits):
    rng = np.random.default_rng(3)
    prog = rng.integers(0, 1 << bits, (10, 9, 13)).astype(np.uint8 if bits == 8 else np.uint16)
    clip = R.interlace(prog, order)
    out = R.deinterlace(clip, order, "field")
    p = 1 if order == "bff" else 0
    for k in range(10):
        par = p ^ (k & 1)
        assert np.array_equal(out[k, par::2], prog[k, par::2]), k
    assert np.array_equal(R.deinterlace(clip, order, "frame"), out[0::2])
    assert out.min() >= prog.min() and out.max() <= prog.max()
    # the package's torch `interlace` is the reference's, plane by plane
    lay = frame_layout(("y4m", "420jpeg" if bits == 8 else "420p10"), 9, 13)
    rows = rng.integers(0, 1 << bits, (6, lay.samples)).astype(np.int16 if bits == 10 else np.uint8)
    woven = D.interlace(torch.from_numpy(rows), lay, order).numpy()
    for _, off, h, w, pitch, step in lay.planes:
        idx = off + np.arange(h)[:, None] * pitch + np.arange(w)[None, :] * step
        assert np.array_equal(woven[:, idx], R.interlace(rows[:, idx], order))


def test_a_window_with_context_equals_the_whole_clip():
    clip = np.random.default_rng(4).integers(0, 256, (6, 7, 11)).astype(np.uint8)
    whole = R.deinterlace(clip, "bff", "field")
    for first in range(6):
        lo, hi = max(first - 1, 0), min(first + 2, 6)
        part = R.deinterlace(clip[lo:hi], "bff", "field", first=first - lo, count=1)
        assert np.array_equal(part, whole[2 * first:2 * first + 2]), first


# ---- 6. the `I` token -------------------------------------------------------------------------------------------------------
def _y4m_bytes(token, n=3, h=6, w=8, seed=5, fps=(25, 1)):
    head = b"YUV4MPEG2 W%d H%d F%d:%d" % (w, h, fps[0], fps[1]) + (b" " + token if token else b"") + b" A1:1 C420jpeg\n"
    rng = np.random.default_rng(seed)
    body = b"".join(b"FRAME\n" + rng.integers(0, 256, w * h * 3 // 2).astype(np.uint8).tobytes() for _ in range(n))
    return head + body


@pytest.mark.parametrize("token,mode", [(b"It", "t"), (b"Ib", "b"), (b"Ip", "p"), (b"Im", "m"), (None, None)])
def test_the_interlace_token_is_read_and_the_header_dict_is_what_it_was(token, mode):
    data = _y4m_bytes(token)
    line = data[:data.index(b"\n") + 1]
    assert IO.y4m_interlace(line) == mode
    with IO.Y4MReader(io.BytesIO(data)) as r, IO.Y4MReader(io.BytesIO(_y4m_bytes(None))) as plain:
        assert r.interlace == mode
        assert r.header == plain.header and "interlace" not in r.header


# ---- 7. the refusals of deinterlace_video -----------------------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(D, "deinterlace", boom)
    monkeypatch.setattr(torch.Tensor, "to", boom)


def test_deinterlace_video_refusals(tmp_path, no_gpu):
    out = str(tmp_path / "out.y4m")

    def src(token):
        return io.BytesIO(_y4m_bytes(token))
    for token, match in ((b"Ip", r'Ip \(progressive\).*order="tff"'), (None, r'no field order.*order="tff"'),
                         (b"Im", "Im")):
        with pytest.raises(ValueError, match=match):
            D.deinterlace_video(src(token), out)
    raw = tmp_path / "clip.raw"
    raw.write_bytes(bytes(3 * 6 * 8 * 3))
    with pytest.raises(ValueError, match="raw video has none"):
        D.deinterlace_video(str(raw), out, raw="rgb24", width=8, height=6)
    with pytest.raises(ValueError, match="order must be one of"):
        D.deinterlace_video(src(b"It"), out, order="top")
    with pytest.raises(ValueError, match="rate must be one of"):
        D.deinterlace_video(src(b"It"), out, rate="double")
    with pytest.raises(ValueError, match="method must be one of"):
        D.deinterlace_video(src(b"It"), out, method="yadif")
    for bad in (0, -1, True, 2.5):
        with pytest.raises(ValueError, match="chunk_frames"):
            D.deinterlace_video(src(b"It"), out, chunk_frames=bad)
    with pytest.raises(ValueError, match="describe raw= video"):
        D.deinterlace_video(src(b"It"), out, width=8, height=6)
    with pytest.raises(ValueError, match="describe raw= video"):
        D.deinterlace_video(src(b"It"), out, packing="v210")
    with pytest.raises(ValueError, match="raw must be one of"):
        D.deinterlace_video(str(raw), out, order="tff", raw="yuv420p", width=8, height=6)
    with pytest.raises(ValueError, match="pass width and height"):
        D.deinterlace_video(str(raw), out, order="tff", raw="rgb24", width=8)
    with pytest.raises(ValueError, match="even width"):
        D.deinterlace_video(str(raw), out, order="tff", raw="uyvy422", width=7, height=6)
    with pytest.raises(ValueError, match="packing"):
        D.deinterlace_video(str(raw), out, order="tff", raw="rgb24", width=8, height=6, packing="v210")
    with pytest.raises(ValueError, match="packing must be one of"):
        D.deinterlace_video(str(raw), out, order="tff", raw="yuv422p10le", width=8, height=6, packing="v211")
    with pytest.raises(ValueError, match="h >= 2"):   # the chroma of a two-row 4:2:0 frame has one row
        D.deinterlace_video(io.BytesIO(_y4m_bytes(b"It", h=2)), out)
    with pytest.raises(ValueError, match="h >= 2"):
        D.deinterlace_video(str(raw), out, order="tff", raw="rgb24", width=8, height=1)
    with pytest.raises(FileNotFoundError):
        D.deinterlace_video(str(tmp_path / "none.raw"), out, order="tff", raw="rgb24", width=8, height=6)
    with pytest.raises(ValueError, match="not a YUV4MPEG2 stream"):
        D.deinterlace_video(io.BytesIO(b"RIFF....\n"), out)
    assert not os.path.exists(out)


def test_device_rows_are_checked_before_the_library_is_called():
    lay = frame_layout("nv12", 6, 8)
    rows = torch.zeros((3, lay.samples), dtype=torch.uint8)
    for kw, match in ((dict(order="auto"), "order"), (dict(rate="frames"), "rate"), (dict(method="weave"), "method"),
                      (dict(first=3, count=1), "window"), (dict(first=-1), "window"), (dict(count=4), "window"),
                      (dict(out=torch.zeros((3, lay.samples), dtype=torch.uint8)), "out must be")):
        with pytest.raises(ValueError, match=match):
            D.deinterlace(rows, lay, 8, **kw)
    with pytest.raises(ValueError, match="bits"):
        D.deinterlace(rows, lay, 10)
    with pytest.raises(ValueError, match="the rows have"):
        D.deinterlace(rows[:, :-1].contiguous(), lay, 8)
    with pytest.raises(ValueError, match="h >= 2"):
        D.deinterlace(rows, [(0, 1, 8, 8, 1)], 8)
    assert D.double_rate((25, 1)) == (50, 1) and D.double_rate((30000, 1001)) == (60000, 1001)
    assert D.double_rate((25, 2)) == (25, 1)


def test_cli_deinterlace_flags():
    a = cli.parse_args(["deinterlace", "--input", "-", "--output", "-"])
    assert (a.order, a.rate, a.method, a.no_spatial_check, a.chunk_frames, a.raw) == ("auto", "field", "adaptive", False, 32, None)
    a = cli.parse_args(["deinterlace", "--input", "a", "--output", "b", "--order", "bff", "--rate", "frame", "--method", "bob",
                        "--no-spatial-check", "--raw", "yuv422p10le", "--size", "24x18", "--packing", "v210", "--src-fps",
                        "30000/1001", "--chunk-frames", "3"])
    assert (a.order, a.rate, a.method, a.no_spatial_check, a.chunk_frames) == ("bff", "frame", "bob", True, 3)
    assert (a.raw, a.size, a.packing, a.src_fps) == ("yuv422p10le", (24, 18), "v210", Fraction(30000, 1001))
    for bad in (["--raw", "nv12"], ["--size", "8x6"], ["--packing", "v210"], ["--raw", "nv12", "--size", "8x6"],
                ["--order", "top"], ["--model", "x.pth"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["deinterlace", "--input", "-", "--output", "-"] + bad)
    # the other commands parse as they did
    assert cli.parse_args(["video", "--input", "-", "--output", "-"]).chunk_frames == 32


# ---- 8. the warning ------------------------------------------------------------------------------------------------------------
class _Reached(Exception):
    """The engine was reached: everything before it, the warning included, has happened."""


@pytest.fixture
def engines_stop(monkeypatch):
    def stop(*a, **k):
        raise _Reached()
    for mod, name in ((stream, "_run"), (stream, "_run_whole"), (holdout, "_score_chunk"), (holdout.scene, "pair_sad")):
        monkeypatch.setattr(mod, name, stop)
    monkeypatch.setattr(torch.Tensor, "pin_memory", stop)


def _warnings_of(call):
    with warnings.catch_warnings(record=True) as got:
        warnings.simplefilter("always")
        try:
            call()
        except _Reached:
            pass
    return [w for w in got if issubclass(w.category, UserWarning) and "cli deinterlace" in str(w.message)]


@pytest.mark.parametrize("token,count", [(b"It", 1), (b"Ib", 1), (b"Im", 1), (b"Ip", 0), (None, 0)])
def test_the_four_commands_warn_once_about_interlaced_input(tmp_path, monkeypatch, engines_stop, token, count):
    from ai_based_frame_interpolation_amd import inference
    path = str(tmp_path / "in.y4m")
    with open(path, "wb") as f:
        f.write(_y4m_bytes(token, n=5, h=16, w=16))
    model = P.FrameInterpolationUNet(bilinear=True, frame_channels=1)
    ckpt = str(tmp_path / "model.pth")
    torch.save(model.state_dict(), ckpt)
    monkeypatch.setattr(inference, "load_model", lambda *a, **k: model)
    fi = P.FrameInterpolator(model=model, device="cpu")
    out = str(tmp_path / "out.y4m")
    calls = {
        "interpolate_video": lambda: fi.interpolate_video(path, out, chunk_frames=4),
        "score_video": lambda: holdout.score_video(model, path),
        "cli video": lambda: cli.main(["video", "--input", path, "--output", out, "--model", ckpt, "--device", "cpu"]),
        "cli evaluate": lambda: cli.main(["evaluate", "--input", path, "--model", ckpt, "--device", "cpu"]),
    }
    for name, call in calls.items():
        got = _warnings_of(call)
        assert len(got) == count, (name, [str(w.message) for w in got])
        if count:
            assert "I" + token[1:].decode() in str(got[0].message)


# ---- 9., 10. the C ABI -----------------------------------------------------------------------------------------------------
def test_header_and_binding_name_the_entry_points(hip_lib_built):
    new = ["fiunet_deinterlace_u8", "fiunet_deinterlace_p10"]
    hdr = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    for name in new:
        assert name in _native.SYMBOLS and name + "(" in hdr
    assert "#define FIUNET_ABI_VERSION 8" in hdr and _native.ABI_VERSION == 8
    L = _native.lib()
    assert L.fiunet_abi_version() == 8
    assert len(L.fiunet_deinterlace_u8.argtypes) == len(L.fiunet_deinterlace_p10.argtypes) == 12
    for c_name, value in (("FIUNET_DEINT_TFF = 0", _native.DEINT_TFF), ("FIUNET_DEINT_BFF = 1", _native.DEINT_BFF),
                          ("FIUNET_DEINT_FIELD_RATE = 0", _native.DEINT_FIELD_RATE),
                          ("FIUNET_DEINT_FRAME_RATE = 1", _native.DEINT_FRAME_RATE),
                          ("FIUNET_DEINT_ADAPTIVE = 0", _native.DEINT_ADAPTIVE), ("FIUNET_DEINT_BOB = 1", _native.DEINT_BOB),
                          ("FIUNET_DEINT_NO_SPATIAL_CHECK = 256", _native.DEINT_NO_SPATIAL_CHECK)):
        assert c_name in hdr and int(c_name.split("= ")[1]) == value
    assert {"fiunet_deinterlace_u8", "fiunet_deinterlace_p10"} <= {r.entry for r in deinterlace_stream_rows.SC.ROWS}
    # the kernels live in a header of their own, and the library stays nine translation units
    csrc = os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc")
    assert os.path.exists(os.path.join(csrc, "deinterlace.hip.h"))
    assert len([f for f in os.listdir(csrc) if f.endswith(".hip")]) == 9


SRC, DST = 1 << 24, 1 << 28     # addresses that are never dereferenced: every refusal comes before a launch


def _plane(off=0, h=6, w=8, pitch=8, step=1, fs=48):
    return (off, h, w, pitch, step, fs)


def _call(L, name="fiunet_deinterlace_u8", src=SRC, n_src=3, sp=None, dst=DST, dp=None, n_planes=None, first=0, n_frames=3,
          order=0, rate=0, flags=0):
    sp = [_plane()] if sp is None else sp
    dp = sp if dp is None else dp
    arr = _native.resize_plane_array
    return getattr(L, name)(src, n_src, arr(sp) if sp != "null" else None, dst, arr(dp) if dp != "null" else None,
                            len(sp) if n_planes is None else n_planes, first, n_frames, order, rate, flags, None)


@pytest.mark.parametrize("name", ["fiunet_deinterlace_u8", "fiunet_deinterlace_p10"])
def test_c_abi_refusals_come_before_any_launch(hip_lib_built, name):
    L = _native.lib()
    item = 2 if name.endswith("p10") else 1
    bad = [
        dict(src=None), dict(dst=None), dict(sp="null", dp=[_plane()], n_planes=1), dict(dp="null", n_planes=1),
        dict(n_planes=0), dict(sp=[_plane()] * 5),
        dict(order=2), dict(order=-1), dict(rate=2), dict(rate=-1), dict(flags=2), dict(flags=512), dict(flags=-1),
        dict(flags=_native.DEINT_NO_SPATIAL_CHECK | 2),
        dict(first=-1), dict(n_frames=-1), dict(first=3, n_frames=1), dict(first=1, n_frames=3), dict(n_src=-1, n_frames=0),
        dict(first=2 ** 31 - 1, n_frames=2 ** 31 - 1), dict(n_src=40000, n_frames=32768),   # 65536 output frames
        dict(sp=[_plane(h=1, fs=8)]), dict(sp=[_plane(h=0)]), dict(sp=[_plane(w=0)]), dict(sp=[_plane(step=5)]),
        dict(sp=[_plane(step=0)]), dict(sp=[_plane(pitch=7)]), dict(sp=[_plane(fs=47)]), dict(sp=[_plane(off=1)]),
        dict(sp=[_plane(h=(1 << 24) + 1, fs=8 * ((1 << 24) + 1))]),
        dict(sp=[_plane()], dp=[_plane(h=5)]), dict(sp=[_plane()], dp=[_plane(w=7)]),
        dict(dst=SRC), dict(dst=SRC + (3 * 48 - 1) * item), dict(dst=SRC - (6 * 48 - 1) * item),   # dst overlaps src
        dict(sp=[_plane(fs=1 << 63)]),                                                          # leaves the address space
    ]
    if item == 2:
        bad += [dict(src=SRC + 1), dict(dst=DST + 1)]
    for kw in bad:
        assert _call(L, name, **kw) == 1, kw
        assert L.fiunet_last_error_string()
    for kw in (dict(dst=SRC), dict(dst=SRC + (3 * 48 - 1) * item)):
        assert _call(L, name, **kw) == 1 and b"overlap" in L.fiunet_last_error_string()
    # a filter other than 0 in either plane
    for which in ("sp", "dp"):
        arrs = {"sp": _native.resize_plane_array([_plane()]), "dp": _native.resize_plane_array([_plane()])}
        arrs[which] = _native.resize_plane_array([_plane()], 1)
        assert getattr(L, name)(SRC, 3, arrs["sp"], DST, arrs["dp"], 1, 0, 3, 0, 0, 0, None) == 1
        assert b"filter" in L.fiunet_last_error_string()
    # nothing to do is no error, and launches nothing: adjacent buffers, no frames
    assert _call(L, name, n_frames=0) == 0
    assert _call(L, name, first=3, n_frames=0) == 0
    assert _call(L, name, n_src=0, n_frames=0) == 0
