"""The area filter of the device resize (csrc/resize.hip.h resize_area_kernel), restated by brute force
with Python ints straight from its definition - independent of `imageio_lite.resize_area`, which states it as two matrix
products.  Pure numpy; small planes only (every destination sample walks its whole span in Python).

  axis    n_src -> n_dst, n_dst <= n_src, in units of 1 / n_dst of a source sample: destination d covers
          [d * n_src, (d + 1) * n_src), source j covers [j * n_dst, (j + 1) * n_dst),
          w(d, j) = max(0, min((d + 1) * n_src, (j + 1) * n_dst) - max(d * n_src, j * n_dst))
  plane   N = sum_y wy(r, y) * sum_x wx(c, x) * v(y, x), D = sw * sh, out = (N + D // 2) // D; samples above 1023 read
          as 1023 at 10 bits; a destination of the source's size is the plane itself, words above 1023 included
"""
import numpy as np


def weight(d: int, j: int, n_src: int, n_dst: int) -> int:
    return max(0, min((d + 1) * n_src, (j + 1) * n_dst) - max(d * n_src, j * n_dst))


def span(d: int, n_src: int, n_dst: int):
    """[(j, w(d, j))] of the non-zero weights of destination index d."""
    first = (d * n_src) // n_dst
    last = -((-(d + 1) * n_src) // n_dst) - 1
    return [(j, weight(d, j, n_src, n_dst)) for j in range(first, last + 1)]


def resize_plane(plane: np.ndarray, size, bits: int) -> np.ndarray:
    """[h, w] uint8 (bits 8) or uint16 (bits 10) -> [H, W] for size = (W, H), H <= h and W <= w."""
    W, H = size
    h, w = plane.shape
    assert H <= h and W <= w, "the area filter only down-scales"
    if (h, w) == (H, W):
        return plane.copy()
    v = [[min(int(s), 1023) if bits == 10 else int(s) for s in row] for row in plane]
    xs = [span(c, w, W) for c in range(W)]
    D = w * h
    out = np.empty((H, W), plane.dtype)
    for r in range(H):
        ys = span(r, h, H)
        for c in range(W):
            N = sum(wy * sum(wx * v[y][x] for x, wx in xs[c]) for y, wy in ys)
            out[r, c] = (N + D // 2) // D
    return out


def plane_view(buf: np.ndarray, plane, frame: int = 0) -> np.ndarray:
    """The [h, w] view of plane (offset, h, w, pitch, step, frame_stride) of frame `frame` in the flat array `buf`."""
    off, h, w, pitch, step, fs = plane
    item = buf.itemsize
    return np.lib.stride_tricks.as_strided(buf[off + frame * fs:], (h, w), (pitch * item, step * item))


def resize_planes(src: np.ndarray, src_planes, dst: np.ndarray, dst_planes, n_frames: int, bits: int) -> np.ndarray:
    """What fiunet_resize_planes_* leaves in a copy of the flat buffer `dst` under FIUNET_RESIZE_AREA."""
    out = dst.copy()
    for sp, dp in zip(src_planes, dst_planes):
        for f in range(n_frames):
            plane_view(out, dp, f)[...] = resize_plane(np.ascontiguousarray(plane_view(src, sp, f)), (dp[2], dp[1]), bits)
    return out


def resize_rows(rows: np.ndarray, src_planes, dst_planes, row_dst: int, bits: int) -> np.ndarray:
    """Tight frames rows [k, row_src] with planes (name, offset, h, w, pitch, step) -> [k, row_dst]."""
    k, row_src = rows.shape
    out = np.zeros((k, row_dst), dtype=rows.dtype)
    sp = [tuple(p[-5:]) + (row_src,) for p in src_planes]
    dp = [tuple(p[-5:]) + (row_dst,) for p in dst_planes]
    return resize_planes(np.ascontiguousarray(rows).reshape(-1), sp, out.reshape(-1), dp, k, bits).reshape(k, row_dst)
