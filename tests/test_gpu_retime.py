"""GPU (MI355X): frame-rate conversion (retime.py, csrc/retime.hip.h).  Every comparison is exact.

  1. the kernel against tests/retime_ref.py (Fractions and Python / int64 integers): 8 and 10 bit, aligned and
     unaligned bases, every path, with flags, as a streamed chunk passes its arguments
  2. dyadic identity: fps = 2 x and 4 x the source rate writes the bytes of factor = 2 / 4, on every route
  3. general rates by composition: the fps output equals retime_ref applied to the frames of the factor = G output
     file, on every route; no frame blends across a cut
  4. streaming: chunk_frames 1 / 3 / 32 against the resident run, and the command line over two pipes
  5. device memory of a streamed fps run is bounded by the chunk
"""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retime_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THR = 10.0
RT = P.retime


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    cache = {}

    def get(fc, precision):
        if (fc, precision) not in cache:
            m = P.FrameInterpolationUNet(bilinear=True, frame_channels=fc, precision=precision)
            m.load_state_dict(O.make_seeded_state_dict(1234) if fc == 1 else
                              O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
            cache[(fc, precision)] = m.to(dev).eval()
        return cache[(fc, precision)]
    return get


# ---- 1. the kernel ------------------------------------------------------------------------------------------------
# 2/5, 1001/2500, 5/6 and 1/10 are the issue's; 2/3 and (2^20 - 1) / 2^20 are the smallest and the largest divisor
RATIOS = [(2, 5), (1001, 2500), (5, 6), (1, 10), (2, 3), ((1 << 20) - 1, 1 << 20)]
SAMPLES = [1, 15, 16, 17, 6144 + 3]


def _stack(rng, rows, fs, bits):
    if bits == 8:
        return rng.integers(0, 256, (rows, fs), dtype=np.uint8)
    a = rng.integers(0, 1024, (rows, fs)).astype(np.uint16)
    over = rng.random((rows, fs)) < 0.1            # some words above 1023, the top bit among them
    a[over] = rng.choice(np.array([1024, 2000, 32768, 65535], np.uint16), int(over.sum()))
    return a.view(np.int16)


def _on_device(dev, a, offset):
    """`a` on the device in a buffer whose base is `offset` samples past an allocation's (16-byte aligned) start."""
    flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a[:0]).dtype, device=dev)
    t = flat[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == (offset * a.itemsize) % 16
    return t


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("p,q", RATIOS)
def test_kernel_matches_the_reference(dev, bits, p, q):
    rng = np.random.default_rng(1000 * bits + p)
    src, fps = Fraction(p), Fraction(q)        # any pair of rates whose ratio is p / q
    checked = blended = 0
    for depth in (1, 2, 3, 4):
        pl = RT.plan(src, fps, depth)
        assert (pl.p, pl.q, pl.G) == (p, q, 1 << depth)
        for fs in SAMPLES:
            for first, n_int, last in ((0, 3, False), (7, 3, True), (5, 1, False)):
                rows = n_int * pl.G + 1
                grid = _stack(rng, rows, fs, bits)
                j0, n_out = pl.span(first, n_int, last)
                for offset in (0, 1):
                    d = _on_device(dev, grid, offset)
                    for flags in (None, np.ones(n_int, np.uint8), (np.arange(n_int) % 2).astype(np.uint8)):
                        dflags = None if flags is None else torch.from_numpy(flags).to(dev)
                        for mode in RT.MODES:
                            out = _on_device(dev, np.zeros((n_out, fs), grid.dtype), offset)
                            got = RT.resample(d, pl, first, j0, n_out, bits=bits, flags=dflags, mode=mode, out=out)
                            assert got is out
                            got = got.cpu().numpy()
                            for k in range(n_out):
                                want = R.frame(grid, j0 + k, src, fps, depth, bits, mode, flags, first)
                                assert np.array_equal(got[k], want), (depth, fs, first, offset, mode, j0 + k)
                                checked += 1
                                blended += int(pl.frame(j0 + k)[3] != 0 and mode == "blend" and flags is None)
    assert checked and blended   # the blend path ran


def test_kernel_exhausts_the_sample_pairs(dev):
    """Every (A, B) pair of 10-bit codes at the weights where a truncated estimate of the quotient is most at risk:
    the largest divisor and its neighbours, weights at both ends and in the middle.  One interval at depth 1 has the
    rows 0, 1, 2: a frame in its first half (lo = 0) blends rows 0 and 1, one in its second half rows 1 and 2, so the
    grid is A, B, B or A, A, B: the two rows blended are always A and B."""
    a, b = np.meshgrid(np.arange(1024, dtype=np.int16), np.arange(1024, dtype=np.int16), indexing="ij")
    a, b = a.reshape(-1), b.reshape(-1)
    grids = [np.stack([a, b, b]), np.stack([a, a, b])]        # by lo
    dgrids = [torch.from_numpy(g).to(dev) for g in grids]
    weights = set()
    for q in (1 << 20, (1 << 20) - 1, (1 << 20) - 3, 3, 5, 1001, 2500):
        for p in sorted({1, 2, q // 3, q // 2 - 1, q - 2, q - 1}):
            if not 0 < p < q or Fraction(p, q).denominator != q:
                continue
            pl = RT.plan(Fraction(p), Fraction(q), 1)
            j = 1                                             # time p / q, in interval 0
            i, r, lo, wn = pl.frame(j)
            assert i == 0 and wn != 0
            grid = grids[lo]
            got = RT.resample(dgrids[lo], pl, 0, j, 1, bits=10).cpu().numpy()[0]
            want = R.frame(grid, j, Fraction(p), Fraction(q), 1, 10)
            assert np.array_equal(got, want), (p, q, lo, wn)
            direct = (a.astype(np.int64) * (q - wn) + b.astype(np.int64) * wn + q // 2) // q   # A and B it is
            assert np.array_equal(got, direct.astype(np.int16)), (p, q, lo, wn)
            weights.add((q, wn))
    assert len(weights) >= 24 and {(1 << 20, 2), (1 << 20, (1 << 20) - 2), (3, 2), (5, 4)} <= weights


# ---- clips and routes ---------------------------------------------------------------------------------------------
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


def _y4m(path, n, h, w, tag, bits, fps, cuts=(), seed=0, rng=None):
    hdr = IO._y4m_stream_header(IO._y4m_header_line(w, h, fps, tag, rng, bits), bits)
    frames = _clip(n, (hdr["frame_samples"],), bits, cuts, seed)
    with IO.Y4MWriter(path, w, h, fps, tag, rng, bits=bits) as wr:
        wr.write(frames)
    return frames


# (name, network, precision, Y4M tag or None, bits, frame shape of a .npy clip)
H, W = 33, 47
ROUTES = [
    ("gray-420jpeg", 1, "bf16", "420jpeg", 8, None),
    ("gray-420p10", 1, "fp16", "420p10", 10, None),
    ("rgb-420mpeg2", 3, "bf16", "420mpeg2", 8, None),
    ("rgb-420p10", 3, "fp16", "420p10", 10, None),
    ("npy-gray", 1, "bf16", None, 8, (H, W)),
    ("npy-rgb-gray-net", 1, "bf16", None, 8, (H, W, 3)),
    ("npy-rgb", 3, "bf16", None, 8, (H, W, 3)),
]
# Y4M in, a .npy stack of the luma frames out (grayscale network): the cuts are still detected on all three planes
LUMA_ROUTES = [
    ("gray-420jpeg-to-npy", 1, "bf16", "420jpeg", 8, None),
    ("gray-422p10-to-npy", 1, "fp16", "422p10", 10, None),
]
ROUTE_IDS = [r[0] for r in ROUTES]


def _source(tmp_path, route, n, fps, cuts, seed):
    """Writes the clip; -> (path, extension, input frames as stored, src_fps keyword)."""
    _, _, _, tag, bits, shape = route
    if tag is None:
        src = str(tmp_path / "in.npy")
        frames = _clip(n, shape, 8, cuts, seed)
        np.save(src, frames)
        return src, ".npy", frames, dict(src_fps=fps)
    src = str(tmp_path / "in.y4m")
    return src, ".y4m", _y4m(src, n, H, W, tag, bits, fps, cuts, seed, rng="FULL" if seed % 2 else None), {}


def _read(path, bits):
    """-> (frames as stored [N, ...], header rate or None, the bytes after the stream header)."""
    if path.endswith(".npy"):
        return np.load(path), None, open(path, "rb").read()
    frames, hdr = (IO.read_y4m_packed if bits == 8 else IO.read_y4m_packed_p10)(path)
    blob = open(path, "rb").read()
    return frames, tuple(hdr["fps"]), blob[blob.index(b"\n") + 1:]


def _flags(dev, frames, bits, cuts, n):
    t = torch.from_numpy(frames.view(np.int16) if bits == 10 else frames).to(dev)
    flags = P.scene.detect_cuts(t, THR, bits)[1].cpu().numpy()
    assert np.flatnonzero(flags).tolist() == list(cuts)
    return flags


# ---- 2. dyadic identity -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
def test_dyadic_rates_write_the_bytes_of_factor(dev, models, tmp_path, route):
    _, fc, prec, tag, bits, _ = route
    n, cuts = 6, (2,)
    src, ext, _, kw = _source(tmp_path, route, n, (48000, 2002), cuts, seed=3)   # an unreduced header rate
    fi = P.FrameInterpolator(model=models(fc, prec), device=dev)
    for sc in (None, THR):
        for mult in (2, 4):
            ref = str(tmp_path / f"ref{ext}")
            n_ref = fi.interpolate_video(src, ref, mult, scene_cut=sc)
            assert n_ref == (n - 1) * mult + 1
            _, rate, want = _read(ref, bits)
            if rate is not None:
                assert rate == (48000 * mult, 2002)
            for depth in (2, 3):
                for fps in (Fraction(24000 * mult, 1001), (48000 * mult, 2002), f"{48000 * mult}/2002"):
                    got = str(tmp_path / f"got{ext}")
                    n_got = fi.interpolate_video(src, got, fps=fps, time_depth=depth, scene_cut=sc, **kw)
                    assert n_got == n_ref
                    _, rate, have = _read(got, bits)
                    assert have == want, (sc, mult, depth)
                    if rate is not None:   # the same rate, reduced
                        assert rate == (Fraction(24000 * mult, 1001).numerator, 1001)
                    if depth == 3:
                        break              # the three spellings of fps once per factor


# ---- 3. general rates by composition --------------------------------------------------------------------------------
@pytest.mark.parametrize("src_rate,dst_rate", [((24, 1), "60"), ((24000, 1001), "60000/1001")])
@pytest.mark.parametrize("route", ROUTES + LUMA_ROUTES, ids=ROUTE_IDS + [r[0] for r in LUMA_ROUTES])
def test_general_rates_equal_the_reference_on_the_factor_output(dev, models, tmp_path, route, src_rate, dst_rate):
    _, fc, prec, tag, bits, _ = route
    n, cuts, depth = 7, (3,), 2
    src, ext, frames, kw = _source(tmp_path, route, n, src_rate, cuts, seed=5)
    before_cut = frames[cuts[0]]
    if route in LUMA_ROUTES:
        ext, before_cut = ".npy", frames[cuts[0]][:H * W].reshape(H, W)
    fi = P.FrameInterpolator(model=models(fc, prec), device=dev)
    flags = _flags(dev, frames, bits, cuts, n)
    fi_, fo_ = Fraction(*src_rate), Fraction(dst_rate)
    J = R.n_out(n, fi_, fo_)
    assert J == 16                                                        # 6 intervals x 5 / 2 + 1
    for sc in (None, THR):
        ref = str(tmp_path / f"ref{ext}")
        fi.interpolate_video(src, ref, 1 << depth, scene_cut=sc)
        grid, _, _ = _read(ref, bits)
        assert grid.shape[0] == (n - 1) * 4 + 1
        for mode in ("blend", "nearest"):
            got = str(tmp_path / f"got{ext}")
            n_got = fi.interpolate_video(src, got, fps=dst_rate, scene_cut=sc, retime=mode, **kw)
            out, rate, _ = _read(got, bits)
            assert n_got == J == out.shape[0]
            if rate is not None:
                assert rate == (fo_.numerator, fo_.denominator)
            want = R.resample(grid, n, fi_, fo_, depth, bits, mode, flags if sc is not None else None)
            assert out.dtype == want.dtype and np.array_equal(out, want), (sc, mode)
            if sc is not None:   # nothing blends across the cut: every frame strictly inside it is the frame before it
                inside = [j for j in range(J) if cuts[0] < j * fi_ / fo_ < cuts[0] + 1]
                assert len(inside) >= 2
                for j in inside:
                    assert np.array_equal(out[j], before_cut), j


# ---- 4. streaming -------------------------------------------------------------------------------------------------
STREAMED = [ROUTES[0], ROUTES[2], ROUTES[6]]


@pytest.mark.parametrize("n,sc", [(12, None), (12, THR), (11, None), (11, THR), (2, None), (2, THR), (1, None)])
@pytest.mark.parametrize("route", STREAMED, ids=[r[0] for r in STREAMED])
def test_streamed_fps_run_is_byte_identical(dev, models, tmp_path, route, n, sc):
    # 24 -> 60: the last frame of an 11-frame clip (time 10 = 25 x 2 / 5) sits on a chunk's edge at chunk_frames 1,
    # that of a 12-frame clip does not exist (time 11 is no multiple of 2 / 5)
    _, fc, prec, tag, bits, _ = route
    src, ext, _, kw = _source(tmp_path, route, n, (24, 1), (n // 2,) if n > 3 else (), seed=n)
    fi = P.FrameInterpolator(model=models(fc, prec), device=dev)
    ref = str(tmp_path / f"ref{ext}")
    n_ref = fi.interpolate_video(src, ref, fps=60, scene_cut=sc, **kw)
    assert n_ref == (n - 1) * 5 // 2 + 1
    want = open(ref, "rb").read()
    for cf in (1, 3, 32):
        got = str(tmp_path / f"got{ext}")
        assert fi.interpolate_video(src, got, fps=60, scene_cut=sc, chunk_frames=cf, **kw) == n_ref
        assert open(got, "rb").read() == want, cf
        assert not os.path.exists(got + ".part")


@pytest.mark.parametrize("tag,bits,prec", [("420jpeg", 8, "bf16"), ("422p10", 10, "fp16")])
@pytest.mark.parametrize("n", [12, 2, 1])
def test_streamed_y4m_to_npy_is_byte_identical(dev, models, tmp_path, tag, bits, prec, n):
    src = str(tmp_path / "in.y4m")
    _y4m(src, n, 37, 53, tag, bits, (24000, 1001), cuts=(n // 2,) if n > 3 else (), seed=bits + n)
    fi = P.FrameInterpolator(model=models(1, prec), device=dev)
    ref = str(tmp_path / "ref.npy")
    n_ref = fi.interpolate_video(src, ref, fps="60000/1001", scene_cut=THR, time_depth=3)
    assert np.load(ref).shape == (n_ref, 37, 53) and n_ref == (n - 1) * 5 // 2 + 1
    for cf in (1, 3, 32):
        got = str(tmp_path / "got.npy")
        assert fi.interpolate_video(src, got, fps="60000/1001", scene_cut=THR, time_depth=3, chunk_frames=cf) == n_ref
        assert open(got, "rb").read() == open(ref, "rb").read(), cf


def test_cli_over_pipes_with_fps(dev, tmp_path):
    ck = str(tmp_path / "rgb.pth")
    torch.save(O.make_seeded_state_dict(77, n_channels=6, n_classes=3), ck)
    src = str(tmp_path / "in.y4m")
    _y4m(src, 10, 33, 47, "420mpeg2", 8, (24000, 1001), cuts=(6,), seed=3, rng="FULL")
    ref = str(tmp_path / "ref.y4m")
    model = P.load_model(ck, dev, "bf16", frame_channels=3)
    n_ref = P.FrameInterpolator(model=model, device=dev, batch=4).interpolate_video(
        src, ref, fps="60000/1001", scene_cut=THR, time_depth=3, retime="nearest")
    assert n_ref == 23 and IO.read_y4m_packed(ref)[1]["fps"] == (60000, 1001)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "ai_based_frame_interpolation_amd.cli", "video", "--input", "-",
                          "--output", "-", "--model", ck, "--precision", "bf16", "--batch", "4", "--scene-cut", "10",
                          "--chunk-frames", "3", "--fps", "60000/1001", "--time-depth", "3", "--retime", "nearest"],
                         input=open(src, "rb").read(), capture_output=True, cwd=ROOT, env=env, timeout=300)
    assert res.returncode == 0, res.stderr.decode(errors="replace")
    assert res.stdout == open(ref, "rb").read()
    assert b"wrote 23 frames" in res.stderr


# ---- 5. bounded device memory -------------------------------------------------------------------------------------
def _peak(dev, fn):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize(dev)
    return torch.cuda.max_memory_allocated(dev) - base


def test_device_memory_of_an_fps_run_is_bounded_by_the_chunk(dev, models, tmp_path):
    # chunk_frames 4: two chunks at N = 9, eight at N = 33 (a clip four times as long)
    h, w = 270, 480
    fb = P.i420_frame_bytes(h, w)
    fi = P.FrameInterpolator(model=models(3, "bf16"), device=dev)
    peaks = {}
    for n in (9, 33):
        src = str(tmp_path / f"in{n}.y4m")
        _y4m(src, n, h, w, "420jpeg", 8, (24, 1), cuts=(3,), seed=n)
        run = lambda dst, **kw: fi.interpolate_video(src, str(tmp_path / dst), fps=60, scene_cut=THR, **kw)  # noqa: E731
        run("warm.y4m", chunk_frames=4)
        peaks[("stream", n)] = _peak(dev, lambda: run("s.y4m", chunk_frames=4))
        peaks[("resident", n)] = _peak(dev, lambda: run("r.y4m"))
    print("peaks (bytes):", peaks, "frame bytes:", fb)
    assert abs(peaks[("stream", 33)] - peaks[("stream", 9)]) <= fb
    assert peaks[("resident", 33)] - peaks[("resident", 9)] > 24 * fb
