"""GPU (MI355X): the BatchNorm fold on trained-like statistics, stage by stage.

The checkpoints (oracle.make_trained_like_state_dict, statistics in tests/golden/bn_trained_like_*.npz) have negative,
zero, tiny and large gammas, running variances from 1e-7 to 1e7 and folded scales over six decades with both signs, so
the fold (scale into the weights, shift into the accumulators or the stems' bias k-slot), the bf16 rounding of the
folded weights and the K cuts are exercised where they can go wrong.

Every stage is checked on the device's OWN read-back inputs against a float64 restatement (oracle.stage_reference):
the error of one kernel, not what earlier layers passed on.  Bounds per element, in units of M = sum of |terms|:
  fp32    |y - y_ref| <= 2^-16 M                      exact-fp32 MFMA; fp32 folded weights are 2^-24 off
  bf16x2  |y - y_ref| <= 2^-14 M + 2^-16 |y_ref|      two bf16 pieces: the dropped wl*xl term and the pieces' own
                                                      representation are ~2^-17 of each term; output stored in two pieces
  bf16    |y - y_ref| <= 2^-8 |y_ref| + 2^-14 M + E   y_ref from the device's exact bf16 weights (the host's fold and
                                                      error-feedback rounding restated bit for bit), so only fp32
                                                      accumulation and the bf16 output rounding (2^-9) remain.  E covers
                                                      the inputs the kernel rounds itself (lerped upsample half, fused
                                                      stem): one bf16 ulp of every input value that lies within the
                                                      kernel's own error of a rounding midpoint, times |W*sc|.  The
                                                      lerp's error grows with the image: its fp32 source coordinate
                                                      y * (h - 1) / (2h - 1) carries ~2^-23 * h into the lerp weights
                                                      (a 2^-21 band alone let 154 of 2.1 M elements of up4.0 through
                                                      at 135x240, none at 50x70).
  fp16    |y - y_ref| <= 2^-11 |y_ref| + 2^-25        y_ref from the device's exact fp16 weights (the fp32 fold through
                         + 2^-14 M + E                pack_f16x2's clamp and RNE, subnormals kept, restated bit for bit) and
                                                      clamped at 65504 as the store is: one RNE rounding to 11 significant
                                                      bits, half the subnormal spacing 2^-24 for outputs below 2^-14, bf16's
                                                      accumulation term (the same fp32 accumulators and summation orders)
                                                      and E with fp16 ulps (never below 2^-24).
The bf16 head reads the last conv's fp32 accumulators, the read-back tap holds them rounded to bf16: 2^-8 M; fp16: 2^-11 M.
The bound itself is oracle.stage_oracle.stage_bound; tests/test_stage_oracle_fp16_host.py shows on the CPU that the fp16
line rejects flushed subnormal weights and a wrong column at a tile seam.
"""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native
from oracle import stage_oracle as S
from oracle import unet_oracle as O

pytestmark = pytest.mark.gpu

VARIANTS = {"gray": (2, 1, True), "rgb": (6, 3, True), "convt": (2, 1, False)}
WEIGHTS = {"fp32": "exact", "bf16x2": "exact", "bf16": "bf16_feedback", "fp16": "fp16_rne"}
_REPORT = {}   # (precision, stage family) -> worst error / bound and error / M seen


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    yield torch.device("cuda:0")
    path = os.environ.get("FIUNET_BN_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({f"{k[0]} {k[1]}": v for k, v in sorted(_REPORT.items())}, f, indent=1)


@pytest.fixture(scope="module")
def sds():
    return {v: O.make_trained_like_state_dict(*a) for v, a in VARIANTS.items()}


@pytest.fixture(scope="module")
def caches():
    """Per-variant stage-weight caches (the bf16 error-feedback rounding of every filter is computed once)."""
    return {v: {} for v in VARIANTS}


@pytest.fixture(scope="module")
def models(dev, sds):
    out = {}
    for v, (nc, ncl, bil) in VARIANTS.items():
        m = P.FrameInterpolationUNet(bilinear=bil, frame_channels=ncl)
        m.load_state_dict(sds[v])
        out[v] = m.to(dev).eval()
    return out


def _stage1_fused(prec, cf, bilinear, flags, b, h, w):
    """Does conv 1 evaluate the stem inside its gather (form STEM) in this configuration (fiunet_debug_stage_cfg)?"""
    fn = _native.lib().fiunet_debug_stage_cfg
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]
    out = (ctypes.c_int * 6)()
    code = {"fp32": _native.FP32, "bf16": _native.BF16, "bf16x2": _native.BF16X2, "fp16": _native.FP16}[prec]
    assert fn(cf, int(bilinear), flags, code, b, h, w, 1, out) == 0
    return out[4] == 6


def check_stage(sd, stage, acts, prec, weights, stem="tap", label="", cache=None):
    """oracle.stage_oracle.check_stage with this module's report of the worst ratios."""
    S.check_stage(sd, stage, acts, prec, weights, stem, label, cache, report=_REPORT)


def run_layer_local(model, sd, variant, prec, b, h, w, unfused=False, rne=False, seed=71, stages=None, frames=None,
                    cache=None, image=None):
    """Forward with every stage kept, then check `stages` (default: all, the head, the ConvTranspose2d halves).  image:
    check only that image of the batch (the launches still see all B; the float64 reference costs 1/B)."""
    nc, cf, bil = VARIANTS[variant]
    model.precision = prec
    model.set_options(unfused=unfused, no_dither=True, rne_weights=rne)
    try:
        f1, f2 = frames if frames is not None else O.make_frames(seed, b, h, w, c=cf)
        taps = None if stages is None else sorted({t for st in stages for t in (st, st - 1, S.SKIP_OF_CONCAT.get(st, 0),
                                                                             S.POOL_OF.get(st, 0))} - {-1})
        acts, out = model.debug_activations(f1.to(dev_of(model)), f2.to(dev_of(model)), taps=taps, with_up=not bil)
    finally:
        model.set_options()
    sl = slice(None) if image is None else slice(image, image + 1)
    acts = {k: v[sl].cpu() for k, v in acts.items()}
    acts.update(frame1=f1[sl], frame2=f2[sl])
    acts[S.HEAD] = out[sl].cpu()
    flags = _native.OPT_KEEP_ALL | _native.OPT_NO_DITHER | (_native.OPT_UNFUSED if unfused else 0)
    stem = "fused" if _stage1_fused(prec, cf, bil, flags, b, h, w) else "tap"
    weights = "bf16_rne" if (prec == "bf16" and rne) else WEIGHTS[prec]
    label = f"{variant} {b}x{h}x{w}{' unfused' if unfused else ''}{' rne' if rne else ''}"
    todo = stages if stages is not None else list(range(18)) + [S.HEAD] + ([] if bil else S.UP)
    for st in todo:
        if isinstance(st, str) and st != S.HEAD and st not in acts:
            continue
        check_stage(sd, st, acts, prec, weights, stem if st == 1 else "tap", label, cache)
    return acts, out


def dev_of(model):
    return next(model.parameters()).device


# fused and unfused in fp32 and bf16; bf16x2 has no ablation path (plan_stages ignores FIUNET_OPT_UNFUSED for it), so
# its unfused run would repeat the fused one
_FU = {"fp32": (False, True), "bf16": (False, True), "bf16x2": (False,), "fp16": (False, True)}
_PRECS = ("fp32", "bf16x2", "bf16", "fp16")
LAYER_CASES = (
    [("gray", p, 1, 32, 48, u) for p in _PRECS for u in _FU[p]]
    + [("gray", p, 1, 135, 240, False) for p in _PRECS]
    + [("gray", p, 2, 50, 70, u) for p in _PRECS for u in _FU[p]]
    + [("rgb", p, 2, 45, 71, u) for p in _PRECS for u in _FU[p]]
    + [("convt", p, 1, 34, 52, u) for p in _PRECS for u in _FU[p]]
)


@pytest.mark.parametrize("variant,prec,b,h,w,unfused", LAYER_CASES)
def test_every_stage_within_its_precision_bound(models, sds, caches, variant, prec, b, h, w, unfused):
    """All 18 stages, the head and (bilinear=False) the four ConvTranspose2d halves, each on the device's own inputs."""
    run_layer_local(models[variant], sds[variant], variant, prec, b, h, w, unfused, cache=caches[variant])


@pytest.mark.parametrize("prec,variant", [(p, v) for p in ("fp32", "bf16x2", "bf16") for v in ("gray", "rgb")]
                         + [("fp16", "gray")])
def test_multi_tile_size_stem_and_deep_stages(models, sds, caches, variant, prec):
    """B=2 540x960, where the launches are the production ones (tuned tiles, whole K loops, the persistent RGB stem's
    multi-tile loop, the in-gather upsample of a deep concat conv in bf16): the stem, inc.3 and the deep stages
    down4.0, down4.3 and up1.0, checked on the second image (all of the batch is launched).  fp16: gray only, where
    its fused stem and the tuned-tile instantiations run."""
    run_layer_local(models[variant], sds[variant], variant, prec, 2, 540, 960, stages=[0, 1, 8, 9, 10], seed=73,
                    cache=caches[variant], image=1)


def test_bf16_round_to_nearest_weights_stage_by_stage(models, sds):
    """The rne_weights option: the reference restates that rounding instead of the error feedback."""
    run_layer_local(models["gray"], sds["gray"], "gray", "bf16", 1, 32, 48, rne=True)


@pytest.mark.parametrize("variant", ["gray", "rgb"])
@pytest.mark.parametrize("prec", ["fp32", "bf16", "bf16x2", "fp16"])
def test_forced_tile_families_and_k_cuts(models, sds, caches, variant, prec):
    """Every tile family and K cut the configuration tests force (tests/test_gpu_configs.py): a cut K sum must add the
    shift exactly once, and the large shifts of this checkpoint make a mistake there visible.  On the uncut K loop the
    two tile families stay bit-identical on every stage, as tests/test_gpu_configs.py asserts on the seeded checkpoint."""
    m, sd = models[variant], sds[variant]
    f1, f2 = O.make_frames(43, 2, 48, 80, c=VARIANTS[variant][1])
    m.precision = prec
    m(f1.to(dev_of(m)), f2.to(dev_of(m)))   # (creates the context)
    try:
        for k in (1, 2, 4, 16):
            outs = []
            for tile in (1, 2):
                for layer in range(1, 18):
                    m._ctx.force_cfg(layer, tile, k)
                acts, out = run_layer_local(m, sd, variant, prec, 2, 48, 80, frames=(f1, f2), cache=caches[variant])
                outs.append((acts, out))
            if k == 1:
                for name in outs[0][0]:
                    assert torch.equal(outs[0][0][name], outs[1][0][name]), (prec, name)
                assert torch.equal(outs[0][1], outs[1][1])
        for layer in range(1, 18):
            m._ctx.force_cfg(layer, 3, 0)    # conv3x3_kwave_kernel: the K loop cut over the waves of a workgroup
        run_layer_local(m, sd, variant, prec, 2, 48, 80, frames=(f1, f2), cache=caches[variant])
    finally:
        m._ctx.force_cfg(-1)
        m.precision = "fp32"


def test_fp32_fused_equals_unfused_bitwise(models):
    """fp32: the fused pool epilogue and the fused upsample gather give the stage outputs of the ablation path bit for
    bit on this checkpoint too (tests/test_gpu_parity.py::test_fused_equals_unfused_bitwise)."""
    m = models["gray"]
    f1, f2 = O.make_frames(21, 2, 50, 70)
    m.precision = "fp32"
    m.set_options(unfused=False)
    a, _ = m.debug_activations(f1.to(dev_of(m)), f2.to(dev_of(m)))
    m.set_options(unfused=True)
    b, _ = m.debug_activations(f1.to(dev_of(m)), f2.to(dev_of(m)))
    m.set_options()
    for k in a:
        assert torch.equal(a[k], b[k]), k


WHOLE = [("gray", "tl_gray_b1_32x48"), ("gray", "tl_gray_b1_135x240"), ("rgb", "tl_rgb_b2_40x56"),
         ("convt", "tl_convt_b1_34x52")]


def _fixture(golden_dir, name, cf):
    g = np.load(os.path.join(golden_dir, f"out_{name}.npz"))
    if "frame1" in g.files:
        return torch.from_numpy(g["frame1"]), torch.from_numpy(g["frame2"]), g
    b, h, w = (int(x) for x in re.search(r"_b(\d+)_(\d+)x(\d+)$", name).groups())
    f1, f2 = O.make_frames(int(g["seed"]), b, h, w, c=cf)
    return f1, f2, g


@pytest.mark.parametrize("variant,name", WHOLE)
def test_whole_network_fp32_against_float64_reference(models, golden_dir, variant, name):
    """fp32 end to end: the device's error against the reference's float64 output is at most 4x the reference's own
    fp32 error (max and rel-L2), plus 1e-6 of the output's range."""
    m = models[variant]
    f1, f2, g = _fixture(golden_dir, name, VARIANTS[variant][1])
    m.precision = "fp32"
    m.set_options()
    out = m(f1.to(dev_of(m)), f2.to(dev_of(m))).cpu().double()
    if "idx" in g.files:
        got, r64, r32 = out.reshape(-1)[torch.from_numpy(g["idx"])].numpy(), g["val64"], g["val32"].astype(np.float64)
    else:
        got, r64, r32 = out.numpy(), g["out64"], g["out32"].astype(np.float64)
    floor = 1e-6 * np.abs(r64).max()
    assert np.abs(got - r64).max() <= 4 * np.abs(r32 - r64).max() + floor, (np.abs(got - r64).max(), np.abs(r32 - r64).max())
    rel = np.linalg.norm(got - r64) / np.linalg.norm(r64)
    rel_ref = np.linalg.norm(r32 - r64) / np.linalg.norm(r64)
    assert rel <= 4 * rel_ref + 1e-6, (rel, rel_ref)


@pytest.mark.parametrize("variant,name", [w for w in WHOLE if "135x240" not in w[1]])
@pytest.mark.parametrize("prec", ["bf16x2", "bf16", "fp16"])
def test_whole_network_reduced_precision_against_its_emulation(models, sds, golden_dir, variant, name, prec):
    """bf16 / bf16x2 / fp16 end to end with the default options (bf16: dither on): the device's rel-L2 against the float64
    reference is at most 2x that of a CPU emulation of the precision's storage points on the same checkpoint
    (oracle.stage_oracle.emulate_forward), plus the reference's own fp32 rel-L2 (the arithmetic the emulation does not
    model: fp32 accumulation, which dominates bf16x2's storage rounding only where both are ~1e-6)."""
    m, sd = models[variant], sds[variant]
    f1, f2, g = _fixture(golden_dir, name, VARIANTS[variant][1])
    r64 = torch.from_numpy(g["out64"])
    emu = S.emulate_forward(sd, f1, f2, prec)
    rel_emu = ((emu - r64).norm() / r64.norm()).item()
    rel_ref = np.linalg.norm(g["out32"] - g["out64"]) / np.linalg.norm(g["out64"])
    m.precision = prec
    m.set_options()
    out = m(f1.to(dev_of(m)), f2.to(dev_of(m))).cpu().double()
    rel = ((out - r64).norm() / r64.norm()).item()
    assert rel <= 2 * rel_emu + rel_ref, (prec, variant, rel, rel_emu, rel_ref)
    m.precision = "fp32"


@pytest.mark.parametrize("prec", ["fp32", "bf16x2", "bf16", "fp16"])
def test_u8_path_bitwise_on_trained_like_checkpoint(models, prec):
    """forward_u8 == preprocess -> forward -> postprocess bit for bit (gray, where bf16 fuses the uint8 read into the
    stem, and RGB)."""
    for v in ("gray", "rgb"):
        m = models[v]
        cf = VARIANTS[v][1]
        m.precision = prec
        m.set_options()
        gen = torch.Generator().manual_seed(5)
        a = torch.randint(0, 256, (2, cf, 64, 96), dtype=torch.uint8, generator=gen).to(dev_of(m))
        b = torch.randint(0, 256, (2, cf, 64, 96), dtype=torch.uint8, generator=gen).to(dev_of(m))
        got = m.forward_u8(a, b)
        want = _native.postprocess_u8(m(_native.preprocess_u8(a), _native.preprocess_u8(b)))
        assert torch.equal(got, want), (v, prec)
        m.precision = "fp32"
