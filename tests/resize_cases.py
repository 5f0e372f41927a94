"""Plane layouts and contents for the resize tests (tests/test_gpu_resize.py and its relatives).  Pure numpy."""
import numpy as np

# (h, w, H, W): 13x3 -> 11x19 and 3x13 -> 19x11 hold the two axes on which a scale computed in fp32 changes a tap
# (13 -> 11 at d = 5, 3 -> 19 at d = 9); 64x96 -> 32x48 is an exact 2x; 67x131 -> 131x67 has no vector multiple;
# 300x280 -> 256x256 is the serving test's shape; 256x256 -> 256x256 the copy
SIZES = [(13, 3, 11, 19), (3, 13, 19, 11), (1, 5, 5, 1), (5, 1, 1, 5), (37, 53, 18, 26), (18, 26, 37, 53),
         (64, 96, 32, 48), (67, 131, 131, 67), (300, 280, 256, 256), (256, 256, 256, 256)]
SENTINEL = {8: 0xA5, 10: 0x5A5A}


def layout(h: int, w: int, step: int, n_planes: int, base: int, pad: int):
    """n_planes planes of h x w at sample step `step`: `step` of them interleaved per group (nv12's U V, the bytes of
    rgb24 / bgra, uyvy's U at step 4), groups one after the other; rows `pad` samples longer than they need to be, the
    first plane at the offset `base`, the frame stride 5 samples more than the frame.  -> (planes [(offset, h, w, pitch,
    step, frame_stride)], frame_stride)."""
    pitch = w * step + pad   # (the interleaved planes of a group share the rows)
    group = h * pitch + 2
    offs = [base + (j % step) + (j // step) * group for j in range(n_planes)]
    fs = max(offs) + (h - 1) * pitch + (w - 1) * step + 1 + 5
    return [(o, h, w, pitch, step, fs) for o in offs], fs


def content(rng, n: int, bits: int) -> np.ndarray:
    """n samples: random codes with runs of the extremes; at 10 bits 1023 and words above 1023 among them."""
    if bits == 8:
        a = rng.integers(0, 256, n, dtype=np.uint8)
        a[rng.random(n) < 0.1] = 255
        a[rng.random(n) < 0.1] = 0
        return a
    a = rng.integers(0, 1024, n).astype(np.uint16)
    a[rng.random(n) < 0.1] = 1023
    a[rng.random(n) < 0.05] = 0
    over = rng.random(n) < 0.05
    a[over] = rng.integers(1024, 65536, int(over.sum())).astype(np.uint16)
    return a


def case(seed: int, bits: int, size, sstep: int = 1, dstep: int = 1, n_planes: int = 2, n_frames: int = 3,
         sbase: int = 3, dbase: int = 7, spad: int = 3, dpad: int = 2):
    """-> (src flat array, src planes, dst flat array full of the sentinel, dst planes, n_frames)."""
    h, w, H, W = size
    rng = np.random.default_rng(seed)
    sp, sfs = layout(h, w, sstep, n_planes, sbase, spad)
    dp, dfs = layout(H, W, dstep, n_planes, dbase, dpad)
    dtype = np.uint8 if bits == 8 else np.uint16
    src = content(rng, sfs * n_frames, bits)
    dst = np.full(dfs * n_frames, SENTINEL[bits], dtype=dtype)
    return src, sp, dst, dp, n_frames
