"""GPU (MI355X): the resize kernel (csrc/resize.hip.h, resize.py) against tests/resize_ref.py.  Every
comparison is exact, over the whole destination buffer: what lies between and around the destination planes keeps its
sentinel.

  1. fiunet_resize_planes_u8 / _p10 on pitched rows, odd offsets, three frames a frame stride apart, two to four planes a
     launch: every size of resize_cases.SIZES, every pair of source and destination steps 1..4
  2. the formats' own plane tables through `resize.resize_frames` (nv12's U V, rgb24, bgra, uyvy's Y at step 2 and U at
     step 4, planar 10-bit 4:2:2, Y4M 4:2:0) and tensors through `resize.resize_planes`
  3. every refusal of the C ABI leaves the destination untouched

The kernel computes its taps itself (there is no table to read back): the first part holds them to the host's through
every axis pair of the sizes above, on content whose every tap shows in the result.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as C  # noqa: E402
import resize_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native  # noqa: E402

pytestmark = pytest.mark.gpu
RS = P.resize


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _up(a: np.ndarray, dev):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _down(t: torch.Tensor, dtype):
    return t.cpu().numpy().view(dtype)


def _run_case(dev, bits, src, sp, dst, dp, n):
    d_src, d_dst = _up(src, dev), _up(dst, dev)
    _native.resize_planes(d_src, sp, d_dst, dp, n, bits)
    torch.cuda.synchronize(dev)
    got, want = _down(d_dst, dst.dtype), R.resize_planes(src, sp, dst, dp, n, bits)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]}, "
                           f"want {want[bad[0]]} (sentinel {C.SENTINEL[bits]})")
    assert np.array_equal(_down(d_src, src.dtype), src)


# ---- 1. the kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("size", C.SIZES, ids=lambda s: "%dx%d-%dx%d" % s)
def test_kernel_on_pitched_planes(dev, bits, size):
    for k, (sbase, dbase) in enumerate(((3, 7), (0, 0), (16, 5))):   # odd offsets; aligned ones; a head of every length
        _run_case(dev, bits, *C.case(100 * k + bits, bits, size, 1, 1, 2, 3, sbase=sbase, dbase=dbase))


@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("dstep", [1, 2, 3, 4])
@pytest.mark.parametrize("sstep", [1, 2, 3, 4])
def test_kernel_steps(dev, bits, sstep, dstep):
    # as many planes as the wider interleave has components: nv12's U V (2), rgb24 (3), bgra and uyvy's U (4)
    for size in ((37, 53, 18, 26), (18, 26, 37, 53), (13, 3, 11, 19), (9, 40, 9, 40)):
        _run_case(dev, bits, *C.case(sstep * 10 + dstep, bits, size, sstep, dstep, max(sstep, dstep, 2), 3))


def test_kernel_destination_rows_at_every_alignment(dev):
    # one plane whose rows start at each of the 16 byte phases in turn (pitch 16 k + 1), widths around the vector width
    for bits in (8, 10):
        for W in (1, 7, 15, 16, 17, 31, 33, 48):
            src, sp, dst, dp, n = C.case(W, bits, (11, 23, 17, W), 1, 1, 1, 2, dpad=(17 - W % 16) % 16 or 16)
            _run_case(dev, bits, src, sp, dst, dp, n)


def test_kernel_extremes(dev):
    rng = np.random.default_rng(9)
    for bits, top in ((8, 255), (10, 1023)):
        dtype = np.uint8 if bits == 8 else np.uint16
        h, w, H, W = 21, 34, 50, 19
        yy, xx = np.mgrid[:h, :w]
        for plane in (np.full((h, w), top), ((yy + xx) & 1) * top, np.zeros((h, w)), rng.integers(0, 2, (h, w)) * top):
            src = plane.astype(dtype).ravel()
            dst = np.full(H * W, C.SENTINEL[bits], dtype)
            _run_case(dev, bits, src, [(0, h, w, w, 1, h * w)], dst, [(0, H, W, W, 1, H * W)], 1)


def test_no_frames_is_a_no_op(dev):
    src, sp, dst, dp, _ = C.case(1, 8, (13, 3, 11, 19))
    _run_case(dev, 8, src, sp, dst, dp, 0)


# ---- 2. the formats and the tensor entry ------------------------------------------------------------------------------------
FORMATS = [("nv12", 8), ("rgb24", 8), ("bgra", 8), ("uyvy422", 8), ("yuyv422", 8), ("yuv422p10le", 10), ("yuv444p", 8),
           (("y4m", "420jpeg"), 8), (("y4m", "420p10"), 10), (("y4m", "mono"), 8), ("npy", 8), (("npy", 3), 8)]


@pytest.mark.parametrize("kind,bits", FORMATS, ids=lambda v: str(v))
def test_resize_frames_of_every_format(dev, kind, bits):
    rng = np.random.default_rng(3)
    for (h, w), (H, W) in (((37, 54), (18, 26)), ((18, 26), (37, 54)), ((24, 32), (24, 32))):
        sp, dp = RS.frame_planes(kind, h, w), RS.frame_planes(kind, H, W)
        row_s, row_d = RS.frame_samples(sp), RS.frame_samples(dp)
        rows = C.content(rng, 3 * row_s, bits).reshape(3, row_s)
        got = RS.resize_frames(_up(rows, dev), sp, dp, bits)
        assert got.shape == (3, row_d)
        want = R.resize_rows(rows, sp, dp, row_d, bits)
        assert np.array_equal(_down(got, rows.dtype), want)
        if (h, w) == (H, W):
            assert np.array_equal(want, rows)   # the copy, words above 1023 included
        out = torch.empty((3, row_d), dtype=got.dtype, device=dev)
        assert RS.resize_frames(_up(rows, dev), sp, dp, bits, out=out) is out and torch.equal(out, got)


def test_resize_frames_refuses(dev):
    sp, dp = RS.frame_planes("nv12", 8, 8), RS.frame_planes("nv12", 4, 4)
    rows = torch.zeros((2, 96), dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError, match="contiguous"):
        RS.resize_frames(rows[:, ::2], sp, dp, 8)
    with pytest.raises(ValueError, match="does not match"):
        RS.resize_frames(rows, sp, dp, 10)
    with pytest.raises(ValueError, match="the rows have"):
        RS.resize_frames(rows[:, :95].contiguous(), sp, dp, 8)
    with pytest.raises(ValueError, match="out must be"):
        RS.resize_frames(rows, sp, dp, 8, out=torch.empty((2, 23), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match="destination planes"):
        RS.resize_frames(rows, sp, dp[:2], 8)


@pytest.mark.parametrize("bits", [8, 10])
def test_resize_planes_of_tensors(dev, bits):
    rng = np.random.default_rng(4)
    dtype = np.uint8 if bits == 8 else np.uint16
    n, c, h, w = 3, 2, 30, 41
    a = C.content(rng, n * c * h * (w + 7), bits).reshape(n, c, h, w + 7)
    t = _up(a, dev)
    for size in ((26, 18), (53, 37), (41, 30), "256x256"):
        W, H = RS.check_size(size)
        want = np.stack([np.stack([R.resize_plane(a[i, j, :, :w], (W, H), bits) for j in range(c)]) for i in range(n)])
        got = RS.resize_planes(t[..., :w], size)                          # rows a pitch apart
        assert got.shape == (n, c, H, W) and got.is_contiguous() and np.array_equal(_down(got, dtype), want)
        got = RS.resize_planes(t[..., :w].contiguous(), size)             # contiguous
        assert np.array_equal(_down(got, dtype), want)
        got = RS.resize_planes(t[:, 1, :, :w], size)                      # [N, H, W], frames two planes apart
        assert got.shape == (n, H, W) and np.array_equal(_down(got, dtype), want[:, 1])
        got = RS.resize_planes(t[..., :w].permute(1, 0, 2, 3), size)      # planes outside the frame stride: a copy first
        assert np.array_equal(_down(got, dtype), want.transpose(1, 0, 2, 3))
    if bits == 8:   # the serving test's shape, against the host function preprocess_image calls
        img = rng.integers(0, 256, (300, 280), dtype=np.uint8)
        got = RS.resize_planes(_up(img, dev)[None], (256, 256))[0]
        assert np.array_equal(_down(got, np.uint8), P.imageio_lite.resize_linear_u8(img, (256, 256)))
    with pytest.raises(ValueError, match="expected uint8"):
        RS.resize_planes(torch.zeros((1, 4, 4), device=dev), (2, 2))
    with pytest.raises(ValueError, match=r"\[N, C, H, W\]"):
        RS.resize_planes(torch.zeros((4, 4), dtype=torch.uint8, device=dev), (2, 2))


# ---- 3. the refusals of the C ABI -------------------------------------------------------------------------------------------
def test_c_abi_refusals_leave_the_destination_untouched(dev):
    L = _native.lib()
    buf = torch.full((8192,), 0xA5, dtype=torch.uint8, device=dev)
    src, dst = buf[:4096], buf[4096:]
    ok = (0, 8, 8, 8, 1, 64)

    def call(sp, dp, n_planes=1, n_frames=2, s=src, d=dst, fn=L.fiunet_resize_planes_u8):
        return fn(None if s is None else s.data_ptr(), None if sp is None else _native.resize_plane_array(sp),
                  None if d is None else d.data_ptr(), None if dp is None else _native.resize_plane_array(dp), n_planes,
                  n_frames, torch.cuda.current_stream(dev).cuda_stream)
    assert call([ok], [ok], s=None) == 1 and call([ok], [ok], d=None) == 1
    assert call(None, [ok]) == 1 and call([ok], None) == 1
    assert call([ok], [ok], n_planes=0) == 1 and call([ok] * 5, [ok] * 5, n_planes=5) == 1
    assert call([ok], [ok], n_frames=-1) == 1
    bad = [(0, 0, 8, 8, 1, 64), (0, 8, 0, 8, 1, 64), (0, -3, 8, 8, 1, 64),            # sizes
           (0, 8, 8, 8, 0, 64), (0, 8, 8, 40, 5, 640), (0, 8, 8, 8, -1, 64),           # step 1..4
           (0, 8, 8, 7, 1, 64), (0, 8, 8, 14, 2, 256), (0, 8, 8, 28, 4, 512),          # pitch >= (w - 1) * step + 1
           (1, 8, 8, 8, 1, 64), (0, 8, 8, 8, 1, 63), (65, 8, 8, 8, 1, 64), (0, 8, 8, 9, 1, 70)]   # inside the frame stride
    for p in bad:
        assert call([p], [ok]) == 1, p
        assert call([ok], [p]) == 1, p
        assert call([ok, p], [ok, ok], n_planes=2) == 1, p        # a later plane is checked before the first launch too
    # overlap of the ranges given: the same buffer, the last source sample, a destination below the source
    assert call([ok], [ok], d=src) == 1 and b"overlap" in L.fiunet_last_error_string()
    assert call([ok], [ok], d=buf[127:]) == 1 and call([ok], [ok], s=buf[127:], d=buf) == 1
    assert call([ok], [ok], d=buf[128:]) == 0                     # ... and right behind it is fine
    assert call([ok], [ok], s=src[1:], fn=L.fiunet_resize_planes_p10) == 1 and b"misaligned" in L.fiunet_last_error_string()
    torch.cuda.synchronize(dev)
    got = buf.cpu().numpy()
    assert (got[:128] == 0xA5).all() and (got[256:] == 0xA5).all()   # (the one call that ran copied 128 sentinels)
    assert (got[128:256] == 0xA5).all()
