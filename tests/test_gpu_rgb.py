"""GPU (MI355X): the RGB 6->3 network (the reference's UNet(n_channels=6, n_classes=3), unet.py:66,72) at the sizes
where its stems loop, and at bench.py's RGB shape (batch 8 of 1080p), against the oracle and the reference's own 1080p
sample (tests/golden/out_rgb_b1_1080x1920_sample.npz).

The bf16 and bf16x2 RGB networks start with stem_rgb_split_kernel (csrc/pointwise.hip.h), a persistent kernel over
16x32 tiles on min(ntiles, 512) workgroups: from its second tile on, a workgroup prefetches the next tile's patch into
registers, stages it in the other of two LDS buffers and carries the image index and edge mask across tiles.  The
fp32 network's stem, conv3x3_first_kernel<float, 3>, is a grid-stride loop capped at 16 384 workgroups.  The shapes:

  1x425x600    27 x 19 = 513 tiles: workgroup 0 alone runs a second tile, the partial bottom-right corner
  2x530x950    34 x 30 x 2 = 2 040 tiles: workgroups 0-503 run 4, 504-511 run 3; image 0 -> 1 inside a sequence;
               partial bottom (2 rows) and right (22 columns) tiles
  1x1080x1920  4 080 tiles, ~8 per workgroup: the reference sample
  8x1080x1920  32 640 tiles, ~64 per workgroup: the benchmark shape (fp32: 129 600 row runs, past the 16 384 cap)

Tolerances are the suite's own contracts (test_gpu_parity.py, test_gpu_configs.py).
"""
import os

import numpy as np
import pytest
import torch

import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3
RGB_WEIGHT_SEED = 77
PRECISIONS = ["bf16", "bf16x2", "fp32", "fp16"]
REL_L2 = {"bf16": 2e-2, "fp16": 5e-3}   # the whole network against the oracle / the reference's sample
STEM_GRID = 512          # 256 CUs x FIUNET_RGB_STEM_OCC: workgroups of the persistent RGB stem
STEM_TH, STEM_TW = 16, 32
K0 = "unet.inc.double_conv.0"
MULTI_TILE = [(1, 425, 600), (2, 530, 950)]
FRAME_SEED = {(1, 425, 600): 61, (2, 530, 950): 62}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rgb_sd():
    return O.make_seeded_state_dict(RGB_WEIGHT_SEED, n_channels=6, n_classes=3)


@pytest.fixture(scope="module")
def models(dev, rgb_sd):
    ms = {}
    for prec in PRECISIONS:
        m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision=prec)
        m.load_state_dict(rgb_sd)
        ms[prec] = m.to(dev).eval()
    yield ms
    ms.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def oracle(rgb_sd):
    """(frame1, frame2, oracle output, oracle stem output) per shape; each CPU forward runs once per module."""
    cache = {}

    def get(shape):
        if shape not in cache:
            b, h, w = shape
            f1, f2 = O.make_frames(FRAME_SEED[shape], b, h, w, c=3)
            taps = {}
            ref = O.unet_forward(rgb_sd, f1, f2, taps)
            cache[shape] = (f1, f2, ref, taps[K0])
        return cache[shape]

    return get


@pytest.fixture(scope="module")
def sample(golden_dir):
    g = np.load(os.path.join(golden_dir, "out_rgb_b1_1080x1920_sample.npz"))
    assert int(g["weight_seed"]) == RGB_WEIGHT_SEED
    f1, f2 = O.make_frames(int(g["seed"]), 1, 1080, 1920, c=3)
    return g, f1, f2


def _stem_tiles(h, w):
    return -(-h // STEM_TH), -(-w // STEM_TW)


def _where(bad, excess, h, w):
    """Where a stem comparison failed, in the persistent stem's terms: the worst element's (b, c, y, x), its 16x32 tile t
    and the loop pass t // 512 that ran it, and the failing pixels counted per pass."""
    tiles_y, tiles_x = _stem_tiles(h, w)
    b, c, y, x = np.unravel_index(int(excess.reshape(-1).argmax()), tuple(excess.shape))
    t = (b * tiles_y + y // STEM_TH) * tiles_x + x // STEM_TW
    bb, yy, xx = torch.nonzero(bad.any(dim=1), as_tuple=True)
    passes = ((bb * tiles_y + yy // STEM_TH) * tiles_x + xx // STEM_TW) // STEM_GRID
    per_pass = {int(p): int(n) for p, n in zip(*torch.unique(passes, return_counts=True))}
    return (f"worst at (b={b}, c={c}, y={y}, x={x}): stem tile t={t}, pass t // {STEM_GRID} = {t // STEM_GRID}; "
            f"failing pixels per pass: {per_pass}")


def _check_bf16_whole(out, ref, what):
    assert out.shape == ref.shape and torch.isfinite(out).all(), what
    rel = ((out - ref).norm() / ref.norm()).item()
    d = (out - ref).abs().max().item()
    rng = (ref.max() - ref.min()).item()
    assert rel <= 2e-2 and d <= 0.04 * rng, (what, rel, d, rng)


def _check_fp16_whole(out, ref, what):
    """fp16's contract against the oracle (tests/test_gpu_fp16.py): rel-L2 <= 5e-3."""
    assert out.shape == ref.shape and torch.isfinite(out).all(), what
    rel = ((out - ref).norm() / ref.norm()).item()
    assert rel <= REL_L2["fp16"], (what, rel)


def _check_fp32_contract(out, ref, rel_tol, what):
    assert out.shape == ref.shape, what
    d = (out - ref).abs().max().item()
    assert d <= FP32_TOL and d <= rel_tol * max(1.0, ref.abs().max().item()), (what, d)


@pytest.mark.parametrize("shape", MULTI_TILE, ids=["513tiles", "2040tiles"])
@pytest.mark.parametrize("prec", PRECISIONS)
def test_rgb_stem_tap0_multi_tile(models, dev, oracle, prec, shape):
    """The stem's own output (tap 0, dither off: it perturbs the input by +-2^-9) over the whole tensor against the
    oracle's relu(bn(conv(cat(f1, f2)))), at tile counts where the persistent stem's workgroups run more than one tile.
    bf16: one bf16 rounding plus the split arithmetic (test_gpu_configs.py, RGB bf16 stem); bf16x2: the per-layer
    bound, 2e-4 of the layer's range; fp32: 1e-4 relative; fp16 (stem_rgb_split_kernel<false, _Float16>): bf16's line with
    one fp16 rounding, 2^-11 relative."""
    b, h, w = shape
    f1, f2, _, want = oracle(shape)
    m = models[prec]
    m.set_options(no_dither=True)
    try:
        acts, _ = m.debug_activations(f1.to(dev), f2.to(dev), taps=[0])
    finally:
        m.set_options()
    got = acts[K0].cpu().float()
    assert got.shape == want.shape == (b, 64, h, w)
    err = (got - want).abs()
    bound = {"bf16": (2.0 ** -8 + 2.0 ** -13) * want.abs() + 5e-4,
             "fp16": (2.0 ** -11 + 2.0 ** -13) * want.abs() + 5e-4,
             "bf16x2": torch.full_like(want, 2e-4 * want.abs().max().item()),
             "fp32": torch.full_like(want, 1e-4 * max(1.0, want.abs().max().item()))}[prec]
    bad = err > bound
    if bad.any():
        pytest.fail(f"{prec} {shape}: {int(bad.sum())} stem outputs out of bound, max err {err.max().item():.3e}; "
                    + _where(bad, err - bound, h, w))


@pytest.mark.parametrize("prec", PRECISIONS)
def test_rgb_whole_net_multi_tile_vs_oracle(models, dev, oracle, prec):
    """The whole RGB network at 2x530x950 (2 040 stem tiles, the large-frame launch choices of inc.3 and the 3-class
    head), fused and unfused, against the oracle.  bf16: RGB has no fused stem, so the 18 stage outputs are bit-identical
    fused vs unfused."""
    shape = (2, 530, 950)
    f1, f2, ref, _ = oracle(shape)
    m = models[prec]
    acts = {}
    try:
        for unfused in (False, True):
            m.set_options(unfused=unfused)
            if prec == "bf16":
                acts[unfused], out = m.debug_activations(f1.to(dev), f2.to(dev))
            else:
                out = m(f1.to(dev), f2.to(dev))
            out = out.cpu()
            what = f"{prec} unfused={unfused}"
            if prec == "bf16":
                _check_bf16_whole(out, ref, what)
            elif prec == "fp16":
                _check_fp16_whole(out, ref, what)
            else:
                _check_fp32_contract(out, ref, 1e-4 if prec == "fp32" else 2e-4, what)
    finally:
        m.set_options()
    if prec == "bf16":
        assert len(acts[False]) == 18
        for k in acts[False]:
            assert torch.equal(acts[False][k], acts[True][k]), k


@pytest.mark.parametrize("prec", PRECISIONS)
def test_rgb_1080p_against_reference_sample(models, dev, rgb_sd, sample, prec):
    """B=1 1080p RGB (4 080 stem tiles) against the reference's own 4 096-point sample, float64 sum and uint8 histogram;
    fp32 also against the oracle over the whole tensor."""
    g, f1, f2 = sample
    m = models[prec]
    out = m(f1.to(dev), f2.to(dev)).cpu()
    assert out.shape == (1, 3, 1080, 1920) and torch.isfinite(out).all()
    got = out.reshape(-1)[torch.from_numpy(g["idx"])].numpy()
    if prec in ("bf16", "fp16"):
        rel = np.linalg.norm(got - g["val"]) / np.linalg.norm(g["val"])
        assert rel <= REL_L2[prec], rel
        return
    assert np.abs(got - g["val"]).max() <= FP32_TOL, np.abs(got - g["val"]).max()
    if prec == "fp32":
        _check_fp32_contract(out, O.unet_forward(rgb_sd, f1, f2), 1e-4, "fp32 1080p vs oracle")
    sum_tol, ramp_frac = {"fp32": (1e-5, 1e-3), "bf16x2": (1e-4, 5e-3)}[prec]
    assert abs(out.double().sum().item() - float(g["sum"])) <= sum_tol * float(g["abssum"])
    # Values straddling a truncation boundary move between neighbouring bins; only values on the unclamped ramp
    # (bins 1..254) can.  The gray sample has 28 159 of those (its 200 / 2 000 allowances), this one 1 965 159, so the
    # allowance is a fraction of the ramp: 1 965 / 9 826 (measured 510 / 1 376; gray at the same rates: 28 / 141,
    # measured 16 / 96).
    hist = np.bincount(O.postprocess_tensor(out).reshape(-1), minlength=256)
    ramp = int(g["u8_hist"][1:255].sum())
    assert np.abs(hist - g["u8_hist"]).sum() <= ramp_frac * ramp, (np.abs(hist - g["u8_hist"]).sum(), ramp)


@pytest.fixture(scope="module")
def batch8(dev, sample):
    """bench.py's RGB shape: 8 seeded uniform [-1, 1] 1080p RGB pairs, the fixture's pair at position 5."""
    _, f1, f2 = sample
    gen = torch.Generator(device="cpu").manual_seed(3)
    b1 = torch.rand(8, 3, 1080, 1920, generator=gen) * 2 - 1
    b2 = torch.rand(8, 3, 1080, 1920, generator=gen) * 2 - 1
    b1[5], b2[5] = f1[0], f2[0]
    return b1.to(dev), b2.to(dev)


@pytest.mark.parametrize("prec", PRECISIONS)
def test_rgb_1080p_batch8_properties(models, dev, sample, batch8, prec):
    """At the benchmark shape (~64 tiles per workgroup of the persistent stem; fp32's stem past its workgroup cap): the
    pair at position 5 of the batch equals the pair run alone bit for bit (no layer cuts K by batch from 1080p up),
    and in bf16 and fp16 two forwards agree bit for bit, every output is finite and the lone pair meets the sample's
    bound."""
    g, f1, f2 = sample
    b1, b2 = batch8
    m = models[prec]
    assert m.batch_invariant_from(1080, 1920) == 1, (prec, m.batch_invariant_from(1080, 1920))
    out_a = m(b1, b2)
    single = m(f1.to(dev), f2.to(dev))
    assert torch.equal(single[0], out_a[5])               # batch / position invariant
    if prec in ("bf16", "fp16"):
        out_b = m(b1, b2)
        assert torch.equal(out_a, out_b)                  # deterministic
        assert torch.isfinite(out_a).all()
        got = single.cpu().reshape(-1)[torch.from_numpy(g["idx"])].numpy()
        rel = np.linalg.norm(got - g["val"]) / np.linalg.norm(g["val"])
        assert rel <= REL_L2[prec], rel


def test_rgb_1080p_batch8_forward_u8_bitwise(models, dev, rgb_sd):
    """forward_u8 at the benchmark shape in bf16 (the stem reads the uint8 frames itself, through its long loop) ==
    preprocess_u8 -> forward -> postprocess_u8 bit for bit.  Both sides run the same stem, so pair 5 is also held to the
    oracle on the reference's pre/post-processing (inference.py:31-35, :54-61) within the bf16 uint8 contract."""
    m = models["bf16"]
    gen = torch.Generator().manual_seed(8)
    a = torch.randint(0, 256, (8, 3, 1080, 1920), dtype=torch.uint8, generator=gen).to(dev)
    b = torch.randint(0, 256, (8, 3, 1080, 1920), dtype=torch.uint8, generator=gen).to(dev)
    got = m.forward_u8(a, b)
    want = _native.postprocess_u8(m(_native.preprocess_u8(a), _native.preprocess_u8(b)))
    assert got.dtype == torch.uint8 and got.shape == a.shape
    assert torch.equal(got, want)
    pa, pb = O.preprocess_array(a[5].cpu().numpy())[0], O.preprocess_array(b[5].cpu().numpy())[0]
    ref = O.postprocess_tensor(O.unet_forward(rgb_sd, pa, pb))
    psnr = O.psnr_u8(ref, got[5].cpu().numpy())
    assert psnr >= 35.0, psnr
