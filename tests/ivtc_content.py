"""The film content of the inverse-telecine tests (tests/test_ivtc_host.py, tests/test_gpu_ivtc_video.py): frames cut from
one large uniform-noise image, box-blurred 13 x 13 and stretched to 0..255, which moves (dx, dy) pixels per film frame,
with an 8 x 8 inverted square moving on top.  Smooth enough that a film frame has few combed samples, moving enough that
the fields of two different film frames comb: the separation the tests check on the reference's own scores."""
import numpy as np

FILM_FRAMES = 16
SIZES = ((24, 40), (34, 70), (48, 136))
MOTIONS = ((3, 1), (5, 3), (4, 0))
BLUR = 13
PASSES = 2   # (one pass leaves curvature that reads as comb: a film frame then scores above `combed`)


def _background(h, w, n, dx, dy, seed):
    rng = np.random.default_rng(seed)
    big_h, big_w = h + n * abs(dy) + BLUR, w + n * abs(dx) + BLUR
    box = rng.integers(0, 256, (big_h + PASSES * BLUR, big_w + PASSES * BLUR)).astype(np.float64)
    for _ in range(PASSES):
        c = np.cumsum(np.cumsum(np.pad(box, ((1, 0), (1, 0))), axis=0), axis=1)
        box = c[BLUR:, BLUR:] - c[:-BLUR, BLUR:] - c[BLUR:, :-BLUR] + c[:-BLUR, :-BLUR]
    box = box[:big_h, :big_w]
    return np.rint((box - box.min()) * (255.0 / (box.max() - box.min()))).astype(np.int64)


def film(h, w, motion=(3, 1), n=FILM_FRAMES, seed=7, bits=8):
    """[n, h, w] film frames: uint8, or uint16 10-bit codes (the 8-bit picture times four)."""
    dx, dy = motion
    bg = _background(h, w, n, dx, dy, seed)
    out = np.empty((n, h, w), np.int64)
    for f in range(n):
        out[f] = bg[f * dy:f * dy + h, f * dx:f * dx + w]
        y0, x0 = (2 + 3 * f) % max(h - 8, 1), (1 + 5 * f) % max(w - 8, 1)
        out[f, y0:y0 + 8, x0:x0 + 8] = 255 - out[f, y0:y0 + 8, x0:x0 + 8]
    return (out * 4).astype(np.uint16) if bits == 10 else out.astype(np.uint8)
