"""The host restatement of the device resize (csrc/resize.hip.h), in numpy.  Not imported by the package.

8 bits: `imageio_lite.resize_linear_u8` to the last bit (tests/test_resize_host.py holds the two together).  10 bits: the
project's own integer definition on the same taps.  Equal size: a copy of the plane, sample for sample."""
import numpy as np


def axis(dst_n: int, src_n: int):
    """-> (i0, i1, c0, c1) int64 arrays over the destination indices of one axis: half-pixel centres, the coordinate in
    fp64 (product and subtraction rounded separately) then fp32, index clamp with weight 0 outside, 11-bit coefficients
    rounded half to even, `1.f - frac` in fp32."""
    scale = np.float64(src_n) / np.float64(dst_n)
    f = ((np.arange(dst_n, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    fl = np.floor(f)
    i0 = fl.astype(np.int64)
    frac = (f - fl).astype(np.float32)
    lo = i0 < 0
    frac[lo], i0[lo] = 0.0, 0
    hi = i0 >= src_n - 1
    frac[hi], i0[hi] = 0.0, src_n - 1
    i1 = np.minimum(i0 + 1, src_n - 1)
    inv = (np.float32(1.0) - frac).astype(np.float32)
    c1 = np.rint(frac.astype(np.float64) * 2048.0).astype(np.int64)
    c0 = np.rint(inv.astype(np.float64) * 2048.0).astype(np.int64)
    return i0, i1, c0, c1


def resize_plane(plane: np.ndarray, size, bits: int = 8) -> np.ndarray:
    """plane [h, w] (uint8 at 8 bits, uint16 at 10) -> [H, W] for size = (W, H), a new array."""
    tw, th = int(size[0]), int(size[1])
    sh, sw = plane.shape
    if bits not in (8, 10):
        raise ValueError("bits must be 8 or 10")
    if (sh, sw) == (th, tw):
        return plane.copy()
    x0, x1, a0, a1 = axis(tw, sw)
    y0, y1, b0, b1 = axis(th, sh)
    src = plane.astype(np.int64)
    if bits == 10:
        src = np.minimum(src, 1023)
    rows = src[:, x0] * a0 + src[:, x1] * a1
    r0, r1 = rows[y0], rows[y1]
    if bits == 8:
        out = (((b0[:, None] * (r0 >> 4)) >> 16) + ((b1[:, None] * (r1 >> 4)) >> 16) + 2) >> 2
        return np.clip(out, 0, 255).astype(np.uint8)
    out = (b0[:, None] * r0 + b1[:, None] * r1 + (1 << 21)) >> 22
    return np.minimum(out, 1023).astype(np.uint16)


def plane_view(buf: np.ndarray, plane, frame: int = 0) -> np.ndarray:
    """The [h, w] view of plane (offset, h, w, pitch, step, frame_stride) of frame `frame` in the flat array `buf`."""
    off, h, w, pitch, step, fs = plane
    item = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[off + frame * fs:], (h, w), (pitch * item, step * item))


def resize_planes(src: np.ndarray, src_planes, dst: np.ndarray, dst_planes, n_frames: int, bits: int) -> np.ndarray:
    """What fiunet_resize_planes_* leaves in a copy of the flat buffer `dst`."""
    out = dst.copy()
    for sp, dp in zip(src_planes, dst_planes):
        for f in range(n_frames):
            plane_view(out, dp, f)[...] = resize_plane(np.ascontiguousarray(plane_view(src, sp, f)), (dp[2], dp[1]), bits)
    return out


def resize_rows(rows: np.ndarray, src_planes, dst_planes, row_dst: int, bits: int) -> np.ndarray:
    """Tight frames rows [k, row_src] with planes (name, offset, h, w, pitch, step) -> [k, row_dst]."""
    k = rows.shape[0]
    out = np.zeros((k, row_dst), dtype=rows.dtype)
    flat_in, flat_out = np.ascontiguousarray(rows).reshape(-1), out.reshape(-1)
    row_src = rows.shape[1]
    sp = [tuple(p[-5:]) + (row_src,) for p in src_planes]
    dp = [tuple(p[-5:]) + (row_dst,) for p in dst_planes]
    return resize_planes(flat_in, sp, flat_out, dp, k, bits).reshape(k, row_dst)
