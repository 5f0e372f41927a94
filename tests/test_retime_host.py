"""CPU: the frame-rate conversion's plan (retime.py) against brute-force Fraction arithmetic (tests/retime_ref.py), the
argument checks of `fps` / `src_fps` / `time_depth` / `retime` and of the two C entry points, which come before any GPU
work, and the command line's new flags."""
import ctypes
import os
import sys
from fractions import Fraction
from math import floor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retime_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, imageio_lite as IO  # noqa: E402

RT = P.retime

# (source, target, p / q expected)
RATES = [
    ("24", "60", (2, 5)),
    ("24000/1001", "60000/1001", (2, 5)),
    ("24", "60000/1001", (1001, 2500)),      # 24 -> 59.94
    ("25", "60", (5, 12)),
    ("30", "60", (1, 2)),
    ("50", "60", (5, 6)),
    ("24", "120", (1, 5)),
    ("24", "240", (1, 10)),
]
N = 50


@pytest.mark.parametrize("depth", [1, 2, 3, 4])
@pytest.mark.parametrize("src,dst,pq", RATES)
def test_plan_against_fraction_arithmetic(src, dst, pq, depth):
    pl = RT.plan(src, dst, depth)
    p, q, G = pl
    assert (p, q) == pq and G == 2 ** depth and pl.depth == depth
    fi, fo = Fraction(src), Fraction(dst)
    # J by counting the times that lie in the clip
    J = sum(1 for j in range(N * q // p + 2) if j * fi / fo <= N - 1)
    assert pl.n_out(N) == J == R.n_out(N, fi, fo)
    assert pl.n_out(1) == 1 and pl.n_out(2) == floor(fo / fi) + 1
    for j in range(J):
        t = j * fi / fo
        i, r, lo, wn = pl.frame(j)
        assert i == floor(t) and Fraction(r, q) == t - i
        assert 0 <= i <= N - 1 and (i < N - 1 or (j == J - 1 and r == 0))
        g = (t - i) * G
        assert lo == floor(g) and Fraction(wn, q) == g - lo and 0 <= wn < q and 0 <= lo < G
        assert (wn == 0) == ((t * G).denominator == 1)          # exactly the times k / G
        ri, on_input, rlo, rw = R.place(j, fi, fo, depth)
        assert (ri, on_input, rlo, rw) == (i, r == 0, lo, Fraction(wn, q))


@pytest.mark.parametrize("src,dst,pq", RATES)
@pytest.mark.parametrize("chunk", [1, 3, 32])
@pytest.mark.parametrize("n", [1, 2, 12, N])
def test_chunk_spans_partition_the_output(src, dst, pq, chunk, n):
    pl = RT.plan(src, dst)
    J, nxt, s = pl.n_out(n), 0, 0
    fi, fo = Fraction(src), Fraction(dst)
    while True:   # the chunks stream._run makes: `chunk` intervals each, the last one what is left (possibly none)
        c = min(chunk, n - 1 - s)
        last = s + c == n - 1
        j0, k = pl.span(s, c, last)
        assert j0 == nxt and k >= 0 and k <= -(-chunk * pl.q // pl.p) + 1
        for j in range(j0, j0 + k):
            t = j * fi / fo
            assert s <= t < s + c or (last and t == s + c)
        nxt = j0 + k
        s += c
        if last:
            break
    assert nxt == J


def test_parse_fps():
    f = RT.parse_fps
    assert f(60) == 60 and f("60") == 60 and f(" 60000/1001 ") == Fraction(60000, 1001)
    assert f((24000, 1001)) == Fraction(24000, 1001) and f([30, 1]) == 30
    assert f(Fraction(25, 2)) == Fraction(25, 2) and f(np.int64(24)) == 24
    assert isinstance(f(60), Fraction)
    with pytest.raises(ValueError, match="60000/1001"):
        f(59.94)
    with pytest.raises(ValueError, match="60000/1001"):
        f(60.0)
    for bad in ("59.94", "", "a/b", "1/0", "1/2/3", "-24", 0, -1, (24,), (24, 0), (24.0, 1), None, True, b"24",
                Fraction(0), "0/5"):
        with pytest.raises(ValueError):
            f(bad)


def test_plan_refusals():
    for src, dst in (("60", "60"), ("60", "24"), ("60000/1001", "59")):
        with pytest.raises(ValueError, match="above the source rate"):
            RT.plan(src, dst)
    with pytest.raises(ValueError, match=r"2\*\*20"):
        RT.plan("24", "1048577/1000")          # q = 1048577 * ... > 2**20
    assert RT.plan(1, 1 << 20).q == 1 << 20    # the limit itself is accepted
    for depth in (0, 5, -1, 2.0, True, "2"):
        with pytest.raises(ValueError, match="time_depth"):
            RT.plan(24, 60, depth)
    with pytest.raises(ValueError, match="retime"):
        RT.check_mode("linear")


# ---- interpolate_video refuses before any GPU work and leaves no output behind ------------------------------------
def _cpu_model(channels=1):
    return P.FrameInterpolationUNet(bilinear=True, frame_channels=channels).eval()   # stays on the CPU


@pytest.fixture()
def sources(tmp_path):
    npy = tmp_path / "in.npy"
    np.save(npy, np.zeros((2, 16, 16), np.uint8))
    y4m = tmp_path / "in.y4m"
    IO.write_y4m(str(y4m), np.zeros((2, 16, 16), np.uint8), (np.zeros((2, 8, 8), np.uint8),) * 2, fps=(24, 1))
    return str(npy), str(y4m)


REFUSALS = [
    (dict(fps=59.94), "60000/1001"),
    (dict(fps=24), "above the source rate"),
    (dict(fps="20"), "above the source rate"),
    (dict(fps="1048577/1000"), r"2\*\*20"),
    (dict(fps=60, factor=4), "factor"),
    (dict(fps=60, time_depth=0), "time_depth"),
    (dict(fps=60, time_depth=5), "time_depth"),
    (dict(fps=60, retime="linear"), "retime"),
]


@pytest.mark.parametrize("chunk_frames", [None, 3])
@pytest.mark.parametrize("kw,match", REFUSALS)
def test_interpolate_video_refuses_before_gpu_work(tmp_path, sources, kw, match, chunk_frames):
    npy, y4m = sources
    kw = dict(kw)
    factor = kw.pop("factor", 2)
    for ch in (1, 3):
        fi = P.FrameInterpolator(model=_cpu_model(ch), device="cuda")
        for src, dst, extra in ((npy, "out.npy", dict(src_fps=24)), (y4m, "out.y4m", {})):
            out = tmp_path / dst
            with pytest.raises(ValueError, match=match) as e:
                fi.interpolate_video(src, str(out), factor, chunk_frames=chunk_frames, **extra, **kw)
            if "fps" in kw and factor == 4:
                assert "fps" in str(e.value) and "factor" in str(e.value)    # names both
            assert sorted(os.listdir(tmp_path)) == ["in.npy", "in.y4m"]    # no output, no .part


@pytest.mark.parametrize("chunk_frames", [None, 3])
def test_npy_input_needs_src_fps(tmp_path, sources, chunk_frames):
    npy, _ = sources
    fi = P.FrameInterpolator(model=_cpu_model(1), device="cuda")
    out = tmp_path / "out.npy"
    with pytest.raises(ValueError, match="src_fps"):
        fi.interpolate_video(npy, str(out), fps=60, chunk_frames=chunk_frames)
    assert not out.exists() and not (tmp_path / "out.npy.part").exists()


def test_src_fps_overrides_the_header(tmp_path, sources):
    _, y4m = sources   # the header says 24: with src_fps=60, fps=60 is no longer above the source
    fi = P.FrameInterpolator(model=_cpu_model(1), device="cuda")
    with pytest.raises(ValueError, match="above the source rate"):
        fi.interpolate_video(y4m, str(tmp_path / "out.y4m"), fps=60, src_fps="60")


def test_factor_keeps_its_check_and_text(tmp_path, sources):
    npy, _ = sources
    fi = P.FrameInterpolator(model=_cpu_model(1), device="cuda")
    with pytest.raises(ValueError, match="factor must be a power of two"):
        fi.interpolate_video(npy, str(tmp_path / "out.npy"), 3)
    with pytest.raises(ValueError, match="factor must be a power of two"):
        fi.interpolate_video(npy, str(tmp_path / "out.npy"), 3, fps=60, src_fps=24)


# ---- the C entry points' host-side checks -------------------------------------------------------------------------
def test_c_abi_rejects_bad_retime_arguments_without_gpu(hip_lib_built):
    """Host-side checks that return before any launch."""
    lib = _native.lib()
    fake = ctypes.c_void_p(256)
    # a grid of 3 intervals at depth 2 covering clip intervals 4..7; 24 -> 60: frames 10 (t = 4) .. 17 (t = 6.8)
    good = dict(grid=fake, n_int=3, fs=16, depth=2, first=4, j0=10, n_out=8, p=2, q=5, mode=0, flags=fake, out=fake)

    def call(fn, **kw):
        a = dict(good, **kw)
        return fn(a["grid"], a["n_int"], a["fs"], a["depth"], a["first"], a["j0"], a["n_out"], a["p"], a["q"],
                  a["mode"], a["flags"], a["out"], None)

    for fn in (lib.fiunet_retime_u8, lib.fiunet_retime_p10):
        for bad in (dict(grid=None), dict(out=None), dict(depth=0), dict(depth=5), dict(depth=-1), dict(p=0),
                    dict(p=5), dict(p=6), dict(q=(1 << 20) + 1, p=1), dict(mode=2), dict(mode=-1), dict(n_int=-1),
                    dict(n_out=-1),
                    dict(j0=9),             # t = 3.6: before the grid
                    dict(n_out=9),          # frame 18, t = 7.2: behind the grid
                    dict(j0=17, n_out=2),   # the same
                    dict(n_int=0),          # frame 11, t = 4.4, needs an interval
                    dict(j0=(1 << 64) - 1, n_out=2)):
            assert call(fn, **bad) == 1, bad
            assert lib.fiunet_last_error_string()
        # no launch: n_out == 0, whatever the frame range; and an empty frame
        assert call(fn, n_out=0) == 0 and call(fn, n_out=0, j0=0) == 0 and call(fn, n_out=0, flags=None) == 0
        assert call(fn, fs=0) == 0
        assert call(fn, fs=0, j0=15, n_out=1, first=4, n_int=2) == 0     # t = 6 = the grid's last row, r == 0
        assert call(fn, fs=0, j0=16, n_out=1, first=4, n_int=2) == 1     # t = 6.4
        assert call(fn, fs=0, q=1 << 20, p=1, first=0, j0=0, n_out=1) == 0


# ---- the command line ---------------------------------------------------------------------------------------------
def test_cli_flags():
    base = ["video", "--input", "a.y4m", "--output", "b.y4m"]
    a = cli.parse_args(base)
    assert a.fps is None and a.src_fps is None and a.time_depth == 2 and a.retime == "blend"
    assert a.factor == 2 and a.chunk_frames == 32 and a.batch == 8 and a.scene_cut is None
    a = cli.parse_args(base + ["--fps", "60000/1001", "--time-depth", "3", "--retime", "nearest", "--src-fps",
                               "24000/1001"])
    assert (a.fps, a.time_depth, a.retime, a.src_fps) == (Fraction(60000, 1001), 3, "nearest", Fraction(24000, 1001))
    assert cli.parse_args(base + ["--fps", "60"]).fps == 60
    for bad in (["--fps", "59.94"], ["--src-fps", "0"], ["--retime", "linear"], ["--time-depth", "5"]):
        with pytest.raises(SystemExit):       # argparse refuses them: nothing is loaded first
            cli.parse_args(base + bad)
