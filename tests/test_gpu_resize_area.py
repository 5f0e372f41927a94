"""GPU (MI355X): the area filter of the resize (csrc/resize.hip.h resize_area_kernel) against the brute-force
restatement tests/resize_area_ref.py.  Every comparison is exact, at 8 and 10 bits, over the whole destination buffer:
what lies between and around the destination planes keeps its sentinel.

  1. the kernel on pitched planes, odd offsets and three frames a frame stride apart: ratios that are no whole number,
     one axis equal, a single row at the ratio limit, widths with head, body and tail from an odd base, stepped sources
     and destinations, four planes of different sizes in one launch, a plane of equal size beside ones that shrink
  2. tensors and the formats' plane tables through resize.py; the linear filter through the new binding
  3. refusals leave the destination untouched
  4. a side stream, a captured graph replayed twice, and a frame behind byte 2^32
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import large_extent as L  # noqa: E402
import resize_area_ref as A  # noqa: E402
import resize_cases as C  # noqa: E402
import resize_ref as R  # noqa: E402
import stream_contract as SC  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
RS = P.resize
AREA = _native.RESIZE_AREA


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _up(a: np.ndarray, dev):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _down(t: torch.Tensor, dtype):
    return t.cpu().numpy().view(dtype)


def _run_case(dev, bits, src, sp, dst, dp, n, stream=None):
    d_src, d_dst = _up(src, dev), _up(dst, dev)
    _native.resize_planes(d_src, sp, d_dst, dp, n, bits, stream=stream, filter=AREA)
    torch.cuda.synchronize(dev)
    got, want = _down(d_dst, dst.dtype), A.resize_planes(src, sp, dst, dp, n, bits)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]}, "
                           f"want {want[bad[0]]} (sentinel {C.SENTINEL[bits]})")
    assert np.array_equal(_down(d_src, src.dtype), src)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------
# (h, w, H, W): ratios that are no whole number; one axis equal; a single row at the limit, 64; whole ratios; one sample
SIZES = [(23, 35, 7, 9), (16, 16, 16, 5), (1, 128, 1, 2), (48, 64, 12, 8), (37, 53, 18, 26), (9, 40, 1, 1), (65, 3, 2, 3)]


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_kernel_on_pitched_planes(dev, bits, size):
    for k, (sbase, dbase) in enumerate(((3, 7), (0, 0), (16, 5))):   # odd offsets; aligned ones; a head of every length
        _run_case(dev, bits, *C.case(100 * k + bits, bits, size, 1, 1, 2, 3, sbase=sbase, dbase=dbase))


@pytest.mark.parametrize("bits", [8, 10])
def test_kernel_widths_with_head_body_and_tail(dev, bits):
    # rows that start at each of the 16 byte phases in turn (pitch 16 k + 1, an odd base): a head, whole 16-byte stores and
    # a tail at 37; one whole store at most at 16; a row inside one store at 15; one sample
    for W in (37, 16, 15, 1):
        src, sp, dst, dp, n = C.case(W, bits, (29, 2 * W + 5, 11, W), 1, 1, 1, 2, dpad=(17 - W % 16) % 16 or 16)
        _run_case(dev, bits, src, sp, dst, dp, n)


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("dstep", [1, 2, 3, 4])
@pytest.mark.parametrize("sstep", [1, 2, 3, 4])
def test_kernel_steps(dev, bits, sstep, dstep):
    # as many planes as the wider interleave has components: nv12's U V (2), rgb24 (3), rgba and uyvy's U (4)
    for size in ((37, 53, 18, 26), (13, 40, 13, 7)):
        _run_case(dev, bits, *C.case(sstep * 10 + dstep, bits, size, sstep, dstep, max(sstep, dstep, 2), 3))


@pytest.mark.parametrize("bits", [8, 10])
def test_four_planes_of_different_sizes_in_one_launch(dev, bits):
    """Four plane pairs, each with its own sizes, pitches and steps - one of them of equal size, the copy (at 10 bits
    with its words above 1023) - three frames, frame strides larger than the frames; the guard samples between, before
    and behind the destination planes keep their sentinel."""
    rng = np.random.default_rng(40 + bits)
    dtype = np.uint8 if bits == 8 else np.uint16
    shapes = [((23, 35), (7, 9), 1, 1), ((20, 31), (20, 31), 1, 1), ((19, 50), (6, 17), 2, 1), ((30, 21), (30, 4), 1, 3)]
    sp, dp, s_at, d_at = [], [], 5, 9
    for (h, w), (H, W), ss, ds in shapes:
        sp.append([s_at, h, w, w * ss + 3, ss, 0])
        dp.append([d_at, H, W, W * ds + 2, ds, 0])
        s_at += h * (w * ss + 3) + 7
        d_at += H * (W * ds + 2) + 11
    sfs, dfs = s_at + 13, d_at + 17
    sp, dp = [tuple(p[:5]) + (sfs,) for p in sp], [tuple(p[:5]) + (dfs,) for p in dp]
    src = C.content(rng, 3 * sfs, bits)
    dst = np.full(3 * dfs, C.SENTINEL[bits], dtype)
    _run_case(dev, bits, src, sp, dst, dp, 3)
    want = A.resize_planes(src, sp, dst, dp, 3, bits)
    touched = want != dst
    assert touched.sum() <= 3 * sum(p[1] * p[2] for p in dp) and not touched[:9].any() and not touched[-17:].any()


@pytest.mark.parametrize("bits", [8, 10])
def test_kernel_extremes(dev, bits):
    rng = np.random.default_rng(9)
    top, dtype = (255, np.uint8) if bits == 8 else (1023, np.uint16)
    h, w, H, W = 41, 67, 3, 19
    yy, xx = np.mgrid[:h, :w]
    for plane in (np.full((h, w), top), ((yy + xx) & 1) * top, np.zeros((h, w)), rng.integers(0, 2, (h, w)) * top,
                  np.full((h, w), 65535 if bits == 10 else 255)):
        src = plane.astype(dtype).ravel()
        dst = np.full(H * W, C.SENTINEL[bits], dtype)
        _run_case(dev, bits, src, [(0, h, w, w, 1, h * w)], dst, [(0, H, W, W, 1, H * W)], 1)


def test_alias_probe_on_the_device(dev):
    plane = np.zeros((8, 64), np.uint8)
    plane[:, [c for c in range(64) if c % 8 in (3, 4)]] = 255
    t = _up(plane, dev)[None]
    assert (RS.resize_planes(t, (8, 8)) == 255).all() and (RS.resize_planes(t, (8, 8), filter="area") == 64).all()


def test_no_frames_is_a_no_op(dev):
    src, sp, dst, dp, _ = C.case(1, 8, (23, 35, 7, 9))
    _run_case(dev, 8, src, sp, dst, dp, 0)


# ---- 2. resize.py, and the linear filter through the new binding ------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
def test_resize_planes_of_tensors(dev, bits):
    rng = np.random.default_rng(4)
    dtype = np.uint8 if bits == 8 else np.uint16
    n, c, h, w = 3, 2, 30, 41
    a = C.content(rng, n * c * h * (w + 7), bits).reshape(n, c, h, w + 7)
    t = _up(a, dev)
    for size in ((26, 18), (41, 7), (41, 30), "5x30"):
        W, H = RS.check_size(size)
        want = np.stack([np.stack([A.resize_plane(a[i, j, :, :w], (W, H), bits) for j in range(c)]) for i in range(n)])
        got = RS.resize_planes(t[..., :w], size, filter="area")                 # a pitched source: rows w + 7 apart
        assert got.shape == (n, c, H, W) and got.is_contiguous() and np.array_equal(_down(got, dtype), want)
        got = RS.resize_planes(t[:, 1, :, :w], size, filter="area")             # [N, H, W], frames two planes apart
        assert got.shape == (n, H, W) and np.array_equal(_down(got, dtype), want[:, 1])
        assert np.array_equal(want, np.stack([np.stack([P.imageio_lite.resize_area(a[i, j, :, :w], (W, H), bits)
                                                        for j in range(c)]) for i in range(n)]))
    with pytest.raises(ValueError, match="linear"):
        RS.resize_planes(t[..., :w], (42, 30), filter="area")
    with pytest.raises(ValueError, match="resize filter must be"):
        RS.resize_planes(t[..., :w], (20, 20), filter="cubic")


FORMATS = [("nv12", 8), ("rgb24", 8), ("rgba", 8), ("uyvy422", 8), ("yuv422p10le", 10), (("y4m", "420jpeg"), 8),
           (("y4m", "420p10"), 10), ("npy", 8), (("npy", 3), 8)]


@pytest.mark.parametrize("kind,bits", FORMATS, ids=lambda v: str(v))
def test_resize_frames_of_every_format(dev, kind, bits):
    rng = np.random.default_rng(3)
    for (h, w), (H, W) in (((37, 54), (18, 26)), ((24, 32), (24, 32)), ((46, 68), (9, 14))):
        sp, dp = RS.frame_planes(kind, h, w), RS.frame_planes(kind, H, W)
        row_s, row_d = RS.frame_samples(sp), RS.frame_samples(dp)
        rows = C.content(rng, 3 * row_s, bits).reshape(3, row_s)
        got = RS.resize_frames(_up(rows, dev), sp, dp, bits, filter="area")
        want = A.resize_rows(rows, sp, dp, row_d, bits)
        assert got.shape == (3, row_d) and np.array_equal(_down(got, rows.dtype), want)
        if (h, w) == (H, W):
            assert np.array_equal(want, rows)   # the copy, words above 1023 included
        out = torch.empty((3, row_d), dtype=got.dtype, device=dev)
        assert RS.FrameResize(sp, dp, bits, (W, H), (w, h), filter="area")(_up(rows, dev), out=out) is out
        assert torch.equal(out, got)


@pytest.mark.parametrize("bits", [8, 10])
def test_linear_through_the_new_binding_is_the_old_call(dev, bits):
    """filter=RESIZE_LINEAR, the default and `filter="linear"` give the bytes of the call that names no filter - the
    reference of tests/resize_ref.py, which the linear kernel's own tests hold it to."""
    L_ = _native.lib()
    for size in ((37, 53, 18, 26), (18, 26, 37, 53), (64, 96, 32, 48)):
        src, sp, dst, dp, n = C.case(bits, bits, size, 2, 1, 2, 3)
        want = R.resize_planes(src, sp, dst, dp, n, bits)
        d_src = _up(src, dev)
        outs = []
        for kw in ({}, {"filter": _native.RESIZE_LINEAR}):
            d_dst = _up(dst, dev)
            _native.resize_planes(d_src, sp, d_dst, dp, n, bits, **kw)
            outs.append(_down(d_dst, dst.dtype))
        d_dst = _up(dst, dev)   # the raw call, the planes built as before this field had a name: zero
        fn = L_.fiunet_resize_planes_p10 if bits == 10 else L_.fiunet_resize_planes_u8
        assert fn(d_src.data_ptr(), _native.resize_plane_array(sp), d_dst.data_ptr(), _native.resize_plane_array(dp), len(sp),
                  n, torch.cuda.current_stream(dev).cuda_stream) == 0
        outs.append(_down(d_dst, dst.dtype))
        for o in outs:
            assert np.array_equal(o, want)
    a = C.content(np.random.default_rng(1), 2 * 30 * 41, bits).reshape(2, 30, 41)
    assert torch.equal(RS.resize_planes(_up(a, dev), (26, 18)), RS.resize_planes(_up(a, dev), (26, 18), filter="linear"))


# ---- 3. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_destination_untouched(dev):
    L_ = _native.lib()
    buf = torch.full((16384,), 0xA5, dtype=torch.uint8, device=dev)
    src, dst = buf[:8192], buf[8192:]
    big, small = (0, 8, 130, 130, 1, 2048), (0, 8, 64, 64, 1, 512)

    def call(sp, dp, d_filter, s_filter=0, n_frames=2):
        d_arr = _native.resize_plane_array(dp, d_filter if isinstance(d_filter, int) else 0)
        if not isinstance(d_filter, int):
            for p, f in zip(d_arr, d_filter):
                p.filter = f
        return L_.fiunet_resize_planes_u8(src.data_ptr(), _native.resize_plane_array(sp, s_filter), dst.data_ptr(), d_arr,
                                          len(sp), n_frames, torch.cuda.current_stream(dev).cuda_stream)
    assert call([big], [small], 2) == 1 and call([big], [small], -1) == 1
    assert call([big], [small], 1, s_filter=1) == 1
    assert call([big, big], [small, small], (1, 0)) == 1 and call([big, big], [small, small], (0, 1)) == 1   # mixed
    assert call([small], [big], 1) == 1 and b"linear" in L_.fiunet_last_error_string()                        # grows
    assert call([(0, 8, 64, 64, 1, 512)], [(0, 9, 32, 32, 1, 512)], 1) == 1
    assert call([big], [(0, 8, 2, 2, 1, 16)], 1) == 7 and b"64" in L_.fiunet_last_error_string()              # ratio 65
    assert call([big, big], [small, (0, 8, 2, 2, 1, 512)], 1) == 7     # a later plane is checked before the first launch
    with pytest.raises(ValueError, match="ratios up to 64"):
        RS.resize_planes(src[:1040].view(1, 8, 130), (2, 8), filter="area")
    torch.cuda.synchronize(dev)
    assert (buf == 0xA5).all()
    assert call([(0, 8, 128, 128, 1, 2048)], [(0, 8, 2, 2, 1, 16)], 1) == 0                                   # 64 itself
    torch.cuda.synchronize(dev)
    assert (dst[:32] == 0xA5).all() and (dst[32:] == 0xA5).all() and (src == 0xA5).all()   # (the mean of 0xA5 is 0xA5)


# ---- 4. streams, graphs, far offsets --------------------------------------------------------------------------------------------
def _row(bits, size, sstep, dstep, n_planes):
    def build(env):
        lib = _native.lib()
        a, sp, dst, dp, n = C.case(1, bits, size, sstep, dstep, n_planes)
        b = C.case(2, bits, size, sstep, dstep, n_planes)[0]
        inp = SC._inp(_up(a, env.dev), _up(b, env.dev))
        out = _up(dst, env.dev)
        fn = lib.fiunet_resize_planes_p10 if bits == 10 else lib.fiunet_resize_planes_u8
        s_arr, d_arr = _native.resize_plane_array(sp), _native.resize_plane_array(dp, AREA)
        views = [out.as_strided((n, h, w), (fs, pitch, step), off) for off, h, w, pitch, step, fs in dp]
        return SC.Buffers(lambda s: fn(inp[0].data_ptr(), s_arr, out.data_ptr(), d_arr, len(sp), n, s), [inp], views, [out])
    return build


ROWS = [SC.Row("fiunet_resize_planes_u8", "area-37x53-18x26-nv12-like", None, None, None, _row(8, (37, 53, 18, 26), 2, 1, 2)),
        SC.Row("fiunet_resize_planes_p10", "area-23x35-7x9-four-planes", None, None, None, _row(10, (23, 35, 7, 9), 1, 4, 4))]


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"{r.entry}-{r.ident}")
def test_side_stream_and_graph_capture(dev, row):
    """The instrument of tests/stream_contract.py: the call on a side stream and captured into a graph, replayed twice
    with the inputs replaced and the outputs poisoned, equals the eager call bit for bit."""
    env = SC.Env(dev)
    try:
        SC.check_row(row, env)
    finally:
        env.close()


def test_eager_on_a_side_stream_equals_the_restatement(dev):
    src, sp, dst, dp, n = C.case(3, 8, (67, 131, 23, 67), 3, 1, 3)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    d_src, d_dst = _up(src, dev), _up(dst, dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    _native.resize_planes(d_src, sp, d_dst, dp, n, 8, stream=side.cuda_stream, filter=AREA)
    side.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), A.resize_planes(src, sp, dst, dp, n, 8))


@pytest.mark.parametrize("bits", [8, 10])
def test_frame_1_past_byte_2_32(dev, bits):
    """A small plane in each of two frames a large frame stride apart, on both sides of the call: frame 1's plane lies
    behind byte 2^32 of both buffers.  Skipped, with both numbers, where the card lacks the memory (the rule of
    tests/large_extent.py)."""
    past = 32
    item = 1 if bits == 8 else 2
    dtype, tdtype = (np.uint8, torch.uint8) if bits == 8 else (np.uint16, torch.int16)
    h, w, H, W = 37, 53, 18, 26
    fs = ((1 << past) // item) + 4099
    off = (1 << 20) + 3
    sp, dp = [(off, h, w, w + 3, 1, fs)], [(off + 8, H, W, W + 2, 1, fs)]
    n_src, n_dst = fs + off + h * (w + 3) + 64, fs + off + 8 + H * (W + 2) + 64   # (64: the window behind the plane)
    need = (n_src + n_dst) * item
    free, _ = torch.cuda.mem_get_info()
    if free < need + L.HEADROOM:
        pytest.skip(f"far planes: plans {need / L.GIB:.1f} GiB + {L.HEADROOM / L.GIB:.0f} GiB headroom, the card has "
                    f"{free / L.GIB:.1f} GiB free")
    assert (fs + off) * item > 1 << past
    rng = np.random.default_rng(past + bits)
    d_src = torch.empty(n_src, dtype=tdtype, device=dev)      # (not filled: only the windows below are read)
    d_dst = torch.empty(n_dst, dtype=tdtype, device=dev)
    s_len, d_len = h * (w + 3) + 128, H * (W + 2) + 128
    s_win = [C.content(rng, s_len, bits) for _ in range(2)]
    d_win = [np.full(d_len, C.SENTINEL[bits], dtype) for _ in range(2)]
    for f in range(2):
        d_src[f * fs + off - 64:f * fs + off - 64 + s_len] = _up(s_win[f], dev)
        d_dst[f * fs + off + 8 - 64:f * fs + off + 8 - 64 + d_len] = _up(d_win[f], dev)
    _native.resize_planes(d_src, sp, d_dst, dp, 2, bits, filter=AREA)
    torch.cuda.synchronize(dev)
    for f in range(2):
        got = d_dst[f * fs + off + 8 - 64:f * fs + off + 8 - 64 + d_len].cpu().numpy().view(dtype)
        want = A.resize_planes(s_win[f], [(64, h, w, w + 3, 1, s_len)], d_win[f], [(64, H, W, W + 2, 1, d_len)], 1, bits)
        assert np.array_equal(got, want), (f, int((got != want).sum()))
    del d_src, d_dst
    torch.cuda.empty_cache()
