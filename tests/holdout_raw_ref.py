"""TEST INFRASTRUCTURE ONLY: a numpy restatement of hold-out scoring of raw video - where the planes
of every raw format lie in a tight frame, as index arrays into the frame's samples; the exact sse and float64 PSNR and
the brute-force SSIM (tests/holdout_ref.py's); the rule that leaves targets next to a scene cut out; and the synthetic
clips the tests score."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from holdout_ref import peak_of, predict, psnr, psnr_of_sse, samples, sse, ssim, ssim_bruteforce  # noqa: E402,F401

#: format -> (bits, plane names); the formats of stream.RAW_FORMATS, written out
FORMATS = {"nv12": (8, "yuv"), "rgb24": (8, "rgb"), "bgr24": (8, "rgb"), "rgba": (8, "rgba"), "bgra": (8, "rgba"),
           "yuv422p": (8, "yuv"), "yuv444p": (8, "yuv"), "yuv422p10le": (10, "yuv"), "yuv444p10le": (10, "yuv"),
           "uyvy422": (8, "yuv"), "yuyv422": (8, "yuv")}
CAPTURE = ("uyvy422", "yuyv422")
BYTE_ORDER = {"rgb24": "rgb", "bgr24": "bgr", "rgba": "rgba", "bgra": "bgra", "uyvy422": "uyvy", "yuyv422": "yuyv"}


def frame_samples(fmt: str, h: int, w: int) -> int:
    hc, wc = (h + 1) // 2, (w + 1) // 2
    if fmt == "nv12":
        return h * w + 2 * hc * wc
    if fmt in ("rgb24", "bgr24"):
        return 3 * h * w
    if fmt in ("rgba", "bgra"):
        return 4 * h * w
    if fmt.startswith("yuv422p"):
        return h * w + 2 * h * wc
    if fmt.startswith("yuv444p"):
        return 3 * h * w
    assert fmt in CAPTURE and w % 2 == 0
    return 2 * h * w


def plane_indices(fmt: str, h: int, w: int) -> dict:
    """{plane name: int64 [ph, pw] indices into the samples of one tight frame}, in the order the result names them."""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    idx = np.arange(frame_samples(fmt, h, w), dtype=np.int64)
    if fmt == "nv12":
        uv = idx[h * w:].reshape(hc, wc, 2)
        return {"y": idx[:h * w].reshape(h, w), "u": uv[:, :, 0], "v": uv[:, :, 1]}
    if fmt in ("rgb24", "bgr24", "rgba", "bgra"):
        order = BYTE_ORDER[fmt]
        px = idx.reshape(h, w, len(order))
        return {c: px[:, :, order.index(c)] for c in FORMATS[fmt][1]}
    if fmt.startswith("yuv4"):
        cw = w if "444" in fmt else wc
        return {"y": idx[:h * w].reshape(h, w), "u": idx[h * w:h * w + h * cw].reshape(h, cw),
                "v": idx[h * w + h * cw:].reshape(h, cw)}
    quad = idx.reshape(h, w // 2, 4)   # two pixels: U Y0 V Y1 (uyvy422) or Y0 U Y1 V (yuyv422)
    order = BYTE_ORDER[fmt]
    y0, y1 = (i for i, c in enumerate(order) if c == "y")
    return {"y": np.stack([quad[:, :, y0], quad[:, :, y1]], axis=-1).reshape(h, w), "u": quad[:, :, order.index("u")],
            "v": quad[:, :, order.index("v")]}


def planes_of(fmt: str, frame: np.ndarray, h: int, w: int) -> dict:
    return {name: frame[ix] for name, ix in plane_indices(fmt, h, w).items()}


# ---- scene cuts -------------------------------------------------------------------------------------------------------
def excluded(cut_flags, targets) -> np.ndarray:
    """Held-out frame t is excluded when interval t-1 (frames t-1, t) or interval t (frames t, t+1) is a cut."""
    cut = [bool(c) for c in cut_flags]
    return np.array([cut[t - 1] or cut[t] for t in targets], dtype=bool)


# ---- clips ------------------------------------------------------------------------------------------------------------
def _texture(hh, ww, t, k, peak, rng, speed=1.5):
    yy, xx = np.mgrid[0:hh, 0:ww].astype(np.float64)
    x = xx - speed * t / (1 + (k > 0))
    v = 0.5 + 0.33 * np.sin(x / (4.0 + k)) * np.cos(yy / (6.0 - 0.5 * k)) + 0.1 * np.cos((x + yy) / 3.0 + k)
    return v * peak + rng.normal(0, peak / 200, v.shape)


def clip(fmt: str, n: int, h: int, w: int, seed: int = 0) -> np.ndarray:
    """[n, frame_samples] tight frames of `fmt` (uint8, or uint16 words of 10-bit codes): every plane a moving texture
    with a little noise."""
    bits = FORMATS[fmt][0]
    peak = peak_of(bits)
    rng = np.random.default_rng(2000 + seed)
    ix = plane_indices(fmt, h, w)
    out = np.zeros((n, frame_samples(fmt, h, w)), np.uint8 if bits == 8 else np.uint16)
    for t in range(n):
        for k, (name, i) in enumerate(ix.items()):
            out[t, i] = np.clip(np.rint(_texture(i.shape[0], i.shape[1], t, k, peak, rng)), 0, peak)
    return out


def cut_planes(h: int, w: int, n: int = 12, cut: int = 6):
    """R, G, B planes uint8 [n, h, w] x 3 of a clip with ONE hard cut between frames cut-1 and cut: a slowly moving bright
    texture, then a dark, differently shaped one."""
    rng = np.random.default_rng(77)
    planes = []
    for k in range(3):
        a = [0.55 * _texture(h, w, t, k, 255, rng, speed=0.5) + 110 for t in range(cut)]
        b = [0.25 * _texture(w, h, t, k + 1, 255, rng, speed=0.5).T[::-1] for t in range(cut, n)]
        planes.append(np.clip(np.rint(np.stack(a + b)), 0, 255).astype(np.uint8))
    return planes


def cut_clip(kind: str, h: int, w: int, n: int = 12, cut: int = 6) -> np.ndarray:
    """The cut clip as "npy" ([n, h, w, 3]), "i420" / "nv12" rows (Y = G, U and V = every second sample of R and B: the
    same samples in two orders) or "rgb24" rows."""
    r, g, b = cut_planes(h, w, n, cut)
    if kind == "npy":
        return np.stack([r, g, b], axis=-1)
    if kind == "rgb24":
        return np.stack([r, g, b], axis=-1).reshape(n, -1)
    u, v = r[:, ::2, ::2], b[:, ::2, ::2]
    if kind == "i420":
        return np.concatenate([g.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1)
    assert kind == "nv12"
    return np.concatenate([g.reshape(n, -1), np.stack([u, v], axis=-1).reshape(n, -1)], axis=1)
