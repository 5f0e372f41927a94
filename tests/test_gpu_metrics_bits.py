"""GPU (MI355X): every metric route returns the bits the separate uint8 kernels returned.

Until the metric kernels were unified, `psnr_u8` / `ssim_u8` ran kernels with arithmetic of their own (a uint8 squared
error, a second copy of the 7x7 SSIM) and `psnr_planes` / `ssim_planes` the strided ones.  tests/golden/metrics_u8_bits.npz holds what the
uint8 kernels of the last commit that had them returned (tools/record_metrics_bits.py, with that commit's library) on
the cases of tests/metrics_bits_cases.py.  Here the inputs are regenerated (and their checksum compared, so that a
drifting generator is a fixture error), and all four routes must return exactly the recorded bits: no tolerance.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import metrics_bits_cases as C  # noqa: E402

from ai_based_frame_interpolation_amd import metrics  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "metrics_u8_bits.npz")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fixture_lists_the_cases(golden):
    assert int(golden["cases"]) == len(C.CASES)
    assert str(golden["commit"]) and str(golden["library"])
    for k, (shape, seed, kind, offset) in enumerate(C.CASES):
        assert tuple(golden[f"c{k}_shape"]) == shape and int(golden[f"c{k}_seed"]) == seed
        assert str(golden[f"c{k}_kind"]) == kind and int(golden[f"c{k}_offset"]) == offset


@pytest.mark.parametrize("k", range(len(C.CASES)), ids=[f"{'x'.join(map(str, c[0]))}-{c[2]}+{c[3]}" for c in C.CASES])
def test_recorded_bits(dev, golden, k):
    shape, seed, kind, offset = C.CASES[k]
    pred, target = C.make_inputs(shape, seed, kind)
    assert C.checksum(pred, target) == str(golden[f"c{k}_sha256"]), "the input generator drifted: fixture error"
    p, t = C.to_device(pred, target, offset, dev)
    want_psnr, want_ssim = golden[f"c{k}_psnr"], golden[f"c{k}_ssim"]
    assert want_psnr.dtype == np.int64 and want_psnr.shape == (int(np.prod(shape[:-2])),)
    for name, fn in (("psnr_u8", lambda: metrics.psnr_u8(p, t)), ("psnr_planes", lambda: metrics.psnr_planes(p, t, 8))):
        got = C.bits(fn())
        print(f"{name}: {got.view(np.float64)!r} recorded {want_psnr.view(np.float64)!r}")
        assert np.array_equal(got, want_psnr), name
    if not C.has_ssim(shape):   # both routes refuse, each with its own exception type
        assert want_ssim.size == 0
        with pytest.raises(RuntimeError, match="7x7 window"):
            metrics.ssim_u8(p, t)
        with pytest.raises(ValueError, match="7x7 window"):
            metrics.ssim_planes(p, t, 8)
        return
    assert want_ssim.dtype == np.int64 and want_ssim.shape == want_psnr.shape
    for name, fn in (("ssim_u8", lambda: metrics.ssim_u8(p, t)), ("ssim_planes", lambda: metrics.ssim_planes(p, t, 8))):
        got = C.bits(fn())
        print(f"{name}: {got.view(np.float64)!r} recorded {want_ssim.view(np.float64)!r}")
        assert np.array_equal(got, want_ssim), name
    if kind == "same":
        assert np.all(want_psnr.view(np.float64) == np.inf) and np.all(want_ssim.view(np.float64) == 1.0)
    if kind == "extremes":
        assert np.all(want_psnr.view(np.float64) == 0.0)
