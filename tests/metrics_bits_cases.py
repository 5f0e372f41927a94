"""The cases of tests/golden/metrics_u8_bits.npz: shared by tools/record_metrics_bits.py, which records what
`metrics.psnr_u8` / `ssim_u8` return for them, and tests/test_gpu_metrics_bits.py, which holds every route to those bits.

All are contiguous uint8, pred against target, the smallest shapes at which each path of the squared-error and SSIM
kernels runs.  kind "noise": target uniform in 0..255, pred = target + uniform noise in -25..25, clipped (the `_pair(...,
noise=25)` of tests/test_gpu_holdout.py); "same": pred == target; "extremes": pred all 0, target all 255.  offset: pred
is a flat slice starting that many bytes into a larger device buffer."""
import hashlib

import numpy as np

#        shape          seed  kind        offset   what it reaches
CASES = (
    ((1, 7, 7),         701, "noise",     0),   # one SSIM window; a row shorter than one 16-byte vector
    ((2, 16, 64),       702, "noise",     0),   # aligned bases, vector body only, one SSIM tile
    ((2, 16, 64),       703, "noise",     5),   # the two sides at different offsets in a 16-byte line: all scalar
    ((3, 37, 83),       704, "noise",     0),   # images 1, 2 at odd addresses: scalar head, vector body, scalar tail;
                                                # partial SSIM tiles both ways
    ((1, 33, 4099),     705, "noise",     0),   # more than one 4096-sample piece, a ragged last piece
    ((2, 1, 8200),      706, "noise",     0),   # the [b, 1, n] planes the evaluator scores; PSNR only (SSIM refuses H < 7)
    ((2, 3, 9, 11),     707, "noise",     0),   # leading dimensions
    ((1, 16, 64),       708, "same",      0),   # +inf; SSIM 1
    ((1, 16, 64),       709, "extremes",  0),   # 0 dB; the largest window sums
)


def has_ssim(shape) -> bool:
    return shape[-2] >= 7 and shape[-1] >= 7


def make_inputs(shape, seed, kind):
    """-> (pred, target), contiguous uint8 host arrays"""
    rng = np.random.default_rng(seed)
    if kind == "extremes":
        return np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    target = rng.integers(0, 256, shape)
    if kind == "same":
        return target.astype(np.uint8), target.astype(np.uint8)
    assert kind == "noise", kind
    pred = np.clip(target + rng.integers(-25, 26, shape), 0, 255)
    return pred.astype(np.uint8), target.astype(np.uint8)


def checksum(pred, target) -> str:
    return hashlib.sha256(pred.tobytes() + target.tobytes()).hexdigest()


def to_device(pred, target, offset, dev):
    """-> (pred, target) device tensors; pred starts `offset` bytes into its buffer and stays contiguous"""
    import torch
    t = torch.from_numpy(target).to(dev)
    if not offset:
        return torch.from_numpy(pred).to(dev), t
    buf = torch.zeros(pred.size + offset + 16, dtype=torch.uint8, device=dev)
    p = buf[offset:offset + pred.size].view(pred.shape)
    p.copy_(torch.from_numpy(pred).to(dev))
    assert p.is_contiguous() and p.data_ptr() == buf.data_ptr() + offset
    return p, t


def bits(t) -> np.ndarray:
    """a float64 device tensor -> its int64 bit patterns, flat"""
    return t.detach().cpu().numpy().reshape(-1).view(np.int64).copy()
