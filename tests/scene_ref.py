"""numpy restatement of the scene-cut definition (csrc/scene.hip.h, ai_based_frame_interpolation_amd/scene.py,
DESIGN.md 3.3f): exact int64 sad, the float64 score in the stated order, the flags, and the sample-and-hold."""
import numpy as np


def _frames(stack, bits):
    a = np.asarray(stack)
    if bits == 10:
        a = np.minimum(a.view(np.uint16) if a.dtype == np.int16 else a, 1023)
    return a.reshape(a.shape[0], -1).astype(np.int64)


def pair_sad(stacks, bits=8):
    """int64 [N-1]: sum over every sample of every stack of |F[i+1] - F[i]| (10 bits: samples above 1023 read as 1023)."""
    if not isinstance(stacks, (list, tuple)):
        stacks = [stacks]
    n = np.asarray(stacks[0]).shape[0]
    sad = np.zeros(max(n - 1, 0), np.int64)
    for s in stacks:
        f = _frames(s, bits)
        sad += np.abs(f[1:] - f[:-1]).sum(axis=1, dtype=np.int64)
    return sad


def mafd(sad, count, bits=8):
    """sad * 100.0 / count / 2**bits in float64, in exactly that order."""
    return np.asarray(sad, np.int64) * 100.0 / count / 2 ** bits


def scores(sad, count, bits=8):
    m = mafd(sad, count, bits)
    s = m.copy()
    if m.size > 1:
        s[1:] = np.minimum(s[1:], np.abs(m[1:] - m[:-1]))
        s[:-1] = np.minimum(s[:-1], np.abs(m[:-1] - m[1:]))
    return s


def detect(stacks, threshold, bits=8):
    """-> (scores float64 [N-1], flags uint8 [N-1])."""
    if not isinstance(stacks, (list, tuple)):
        stacks = [stacks]
    count = sum(int(np.prod(np.asarray(s).shape[1:])) for s in stacks)
    sc = scores(pair_sad(stacks, bits), count, bits)
    return sc, (sc >= threshold).astype(np.uint8)


def hold(video, flags, factor):
    """Copy of `video` [(N-1)*factor + 1, ...] with frames i*factor+1 .. i*factor+factor-1 replaced by frame i*factor
    for every flagged interval i."""
    out = np.array(video, copy=True)
    for i in np.flatnonzero(np.asarray(flags)):
        out[i * factor + 1:i * factor + factor] = out[i * factor]
    return out


def cut_clip(h, w, n_a=5, n_b=5):
    """uint8 [n_a + n_b, h, w]: one seeded scene, then a hard cut to the inverted frames of another (interval n_a - 1
    is the cut)."""
    from ai_based_frame_interpolation_amd import synthetic
    a = synthetic.moving_frames(0, n_a, h, w, seed=1).numpy()
    b = 255 - synthetic.moving_frames(n_a, n_b, h, w, seed=2).numpy()
    return np.concatenate([a, b])
