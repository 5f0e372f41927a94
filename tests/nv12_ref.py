"""Plain numpy repacks between packed I420 / C420p10 frames and NV12 / P010 surfaces, for the NV12 tests.

The yardstick of the semi-planar entry points is the I420 path (tests/colour_ref.py, tests/colour10_ref.py and the
4:2:0 entry points) plus these repacks; nothing here touches the library.  Layouts are (luma_pitch, chroma_offset,
chroma_pitch, frame_stride) in samples, every field set (`tight(h, w)` gives the tight one)."""
import numpy as np


def dims(h, w):
    hc, wc = (h + 1) // 2, (w + 1) // 2
    return hc, wc, h * w, hc * wc


def tight(h, w):
    hc, wc, ny, nc = dims(h, w)
    return (w, ny, 2 * wc, ny + 2 * nc)


def i420_to_nv12(frames, h, w):
    """[N, F] packed I420 (Y, U, V planes) -> [N, F] tight NV12 (Y plane, then U,V pairs); any dtype."""
    _, _, ny, nc = dims(h, w)
    n = frames.shape[0]
    uv = np.stack([frames[:, ny:ny + nc], frames[:, ny + nc:ny + 2 * nc]], axis=-1).reshape(n, 2 * nc)
    return np.concatenate([frames[:, :ny], uv], axis=1)


def nv12_to_i420(frames, h, w):
    _, _, ny, nc = dims(h, w)
    n = frames.shape[0]
    uv = frames[:, ny:ny + 2 * nc].reshape(n, nc, 2)
    return np.concatenate([frames[:, :ny], uv[:, :, 0], uv[:, :, 1]], axis=1)


def used_mask(h, w, layout):
    """bool [frame_stride]: the samples of a surface that belong to the frame."""
    lp, co, cp, fs = layout
    hc, wc, _, _ = dims(h, w)
    m = np.zeros(fs, bool)
    for y in range(h):
        m[y * lp:y * lp + w] = True
    for i in range(hc):
        m[co + i * cp:co + i * cp + 2 * wc] = True
    return m


def to_surface(frames, h, w, layout, fill):
    """[N, F] tight NV12 -> [N, frame_stride] in `layout`, every other sample `fill`."""
    out = np.full((frames.shape[0], layout[3]), fill, dtype=frames.dtype)
    out[:, used_mask(h, w, layout)] = frames   # (the used samples of a surface are in the tight frame's order)
    return out


def from_surface(surf, h, w, layout):
    return surf[:, used_mask(h, w, layout)]
