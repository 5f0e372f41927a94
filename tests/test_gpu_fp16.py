"""GPU (MI355X): precision "fp16" (include/fiunet.h FIUNET_FP16) - bf16's kernels with IEEE half values.

  1. every out_*.npz golden (gray, RGB, ConvTranspose2d, odd sizes, trained-like): finite, rel-L2 <= 5e-3 and <= 0.3x
     the bf16 path's on the same input
  2. the per-layer read-back (KEEP_ALL) against the layers_*.npz fixtures: every tap within rel-L2 3e-3
  3. PSNR against the truth on two interpolating checkpoints: within 0.01 dB of the fp32 GPU path
  4. 10-bit: forward_p10 (gray, RGB) and forward_yuv420p10 within 1 code of the CPU oracle through pre10 / post10
  5. the same bits through every entry point (u8, strided u8, yuv420, p10, yuv420p10 against their public chains, fused
     and unfused; row bands; a captured graph; the in-gather upsample); fused against unfused stage by stage
  6. batch invariance from fiunet_min_unsplit_batch on, which equals bf16's
  7. saturation: activations beyond fp16's range give a finite output
  8. FrameInterpolator.interpolate_video on a C420p10 file, RGB network, within 1 code of the fp32 run
"""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour10_ref as C  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO, tiling  # noqa: E402
from ai_based_frame_interpolation_amd import synthetic as S  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _model(dev, sd, cf=1, bilinear=True, precision="fp16"):
    m = P.FrameInterpolationUNet(bilinear=bilinear, frame_channels=cf, precision=precision)
    m.load_state_dict(sd)
    return m.to(dev).eval()


def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return ((a - b).norm() / b.norm()).item()


# ---- 1. goldens --------------------------------------------------------------------------------------------------
def _golden_cases():
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    return sorted(f[4:-4] for f in os.listdir(d) if f.startswith("out_") and f.endswith(".npz") and "1080x1920" not in f)


def _golden_setup(name, golden_dir):
    """(state dict, frame channels, bilinear, frame1, frame2, reference, flat indices of a sampled reference or None)"""
    g = np.load(os.path.join(golden_dir, f"out_{name}.npz"))
    if name.startswith("tl_"):
        _, nc, ncl, bil, _ = O.TRAINED_LIKE[name.split("_")[1]]
        sd = O.make_trained_like_state_dict(nc, ncl, bil)
        if "frame1" in g.files:
            return sd, ncl, bil, torch.from_numpy(g["frame1"]), torch.from_numpy(g["frame2"]), torch.from_numpy(g["out32"]), None
        b, h, w = (int(x) for x in re.search(r"_b(\d+)_(\d+)x(\d+)$", name).groups())
        f1, f2 = O.make_frames(int(g["seed"]), b, h, w, c=ncl)
        return sd, ncl, bil, f1, f2, torch.from_numpy(g["val32"]), torch.from_numpy(g["idx"])
    f1, f2, ref = torch.from_numpy(g["frame1"]), torch.from_numpy(g["frame2"]), torch.from_numpy(g["out"])
    cf, bil = f1.shape[1], not name.startswith("convt_")
    sd = O.make_seeded_state_dict(int(g["weight_seed"]) if "weight_seed" in g.files else 1234, n_channels=2 * cf, n_classes=cf,
                                  bilinear=bil)
    return sd, cf, bil, f1, f2, ref, None


@pytest.mark.parametrize("name", _golden_cases())
def test_goldens_fp16_well_inside_bf16(dev, golden_dir, name):
    sd, cf, bil, f1, f2, ref, idx = _golden_setup(name, golden_dir)
    m = _model(dev, sd, cf, bil)
    out = m(f1.to(dev), f2.to(dev)).cpu()
    m.precision = "bf16"
    o16 = m(f1.to(dev), f2.to(dev)).cpu()
    assert out.shape == f1.shape and torch.isfinite(out).all()
    if idx is not None:
        out, o16 = out.reshape(-1)[idx], o16.reshape(-1)[idx]
    e, e_bf = _rel(out, ref), _rel(o16, ref)
    print(f"{name}: fp16 rel-L2 {e:.3e}  bf16 {e_bf:.3e}  ratio {e / e_bf:.3f}")
    assert e <= 5e-3 and e <= 0.3 * e_bf, (e, e_bf)


# ---- 2. per-layer read-back --------------------------------------------------------------------------------------
@pytest.mark.parametrize("fixture,bil,tl", [("layers_b1_32x48", True, False), ("layers_convt_b1_34x52", False, False),
                                            ("layers_tl_gray_b1_32x48", True, True)])
def test_per_layer_read_back(dev, golden_dir, fixture, bil, tl):
    g = np.load(os.path.join(golden_dir, f"{fixture}.npz"))
    sd = O.make_trained_like_state_dict(2, 1, True) if tl else O.make_seeded_state_dict(1234, bilinear=bil)
    m = _model(dev, sd, 1, bil)
    acts, _ = m.debug_activations(torch.from_numpy(g["frame1"]).to(dev), torch.from_numpy(g["frame2"]).to(dev),
                                  with_up=not bil)
    suffix = "|val32" if tl else "|val"
    n = 0
    for name, a in acts.items():
        if f"{name}|idx" not in g.files:
            continue
        a = a.cpu()
        if name.endswith(".up"):   # stored after F.pad: cut the fixture's window out of it
            shape = tuple(g[f"{name}|shape"])
            dy, dx = a.shape[2] - shape[2], a.shape[3] - shape[3]
            a = a[:, :, dy // 2:dy // 2 + shape[2], dx // 2:dx // 2 + shape[3]].contiguous()
        got = a.reshape(-1)[torch.from_numpy(g[f"{name}|idx"])].numpy()
        want = g[f"{name}{suffix}"]
        rel = np.linalg.norm(got - want) / max(np.linalg.norm(want), 1e-30)
        assert np.isfinite(got).all() and rel <= 3e-3, (name, rel)
        n += 1
    assert n >= 18


# ---- 3. PSNR -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(256, 256), (540, 960)])
@pytest.mark.parametrize("ckpt", [4321, 5321])
def test_psnr_within_0p01_db_of_fp32(dev, h, w, ckpt):
    m = _model(dev, O.make_interpolating_state_dict(seed=ckpt))
    for scene in (1, 2):
        a, truth, c = S.triplet(h, w, device="cpu", seed=scene)
        ps = {}
        for prec in ("fp32", "fp16"):
            m.precision = prec
            u8 = m.forward_u8(a[None, None].to(dev), c[None, None].to(dev))[0, 0].cpu().numpy()
            ps[prec] = O.psnr_u8(truth.numpy(), u8)
        print(f"PSNR {h}x{w} ckpt {ckpt} scene {scene}: fp32 {ps['fp32']:.4f} fp16 {ps['fp16']:.4f} "
              f"delta {ps['fp16'] - ps['fp32']:+.5f} dB")
        assert ps["fp32"] >= 27.0 and abs(ps["fp16"] - ps["fp32"]) <= 0.01, ps


# ---- 4. 10-bit against the CPU oracle ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def interp_models(dev):
    out = {}
    for cf in (1, 3):
        sd = O.make_interpolating_state_dict(n_channels=2 * cf, n_classes=cf)
        out[cf] = (_model(dev, sd, cf), sd)
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _smooth10(rng, b, cf, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    imgs = []
    for i in range(b * cf):
        ph = rng.uniform(0, 6.28, 3)
        v = 512 + 300 * np.sin(xx / 9.0 + ph[0]) * np.cos(yy / 11.0 + ph[1]) + 150 * np.sin((xx + yy) / 5.0 + ph[2])
        imgs.append(v + rng.normal(0, 8, v.shape))
    return np.clip(np.rint(np.stack(imgs)), 0, 1023).astype(np.uint16).reshape(b, cf, h, w)


@pytest.mark.parametrize("cf", [1, 3])
def test_p10_within_one_code_of_oracle(dev, interp_models, cf):
    b, h, w = 1, 64, 96
    rng = np.random.default_rng(4096 + cf)
    a = _smooth10(rng, b, cf, h, w)
    c = np.roll(a, 2, axis=-1)
    m, sd = interp_models[cf]
    ref = O.unet_forward(sd, torch.from_numpy(C.pre10(a)), torch.from_numpy(C.pre10(c))).numpy()
    want = C.post10(ref).astype(int)
    got = _np(m.forward_p10(_dev(a, dev), _dev(c, dev))).astype(int)
    d = np.abs(got - want)
    print(f"p10 cf={cf}: max {d.max()} codes, {int((d != 0).sum())} of {d.size} off")
    assert d.max() <= 1
    if cf == 3:
        opts = dict(siting="mpeg2", matrix="bt2020", colour_range="limited")
        ya, yc = C.rgb_to_yuv420p10(a, **opts), C.rgb_to_yuv420p10(c, **opts)
        ra, rc = C.yuv420p10_to_rgb(ya, h, w, **opts), C.yuv420p10_to_rgb(yc, h, w, **opts)
        r = O.unet_forward(sd, torch.from_numpy(C.pre10(ra)), torch.from_numpy(C.pre10(rc))).numpy()
        want_y = C.rgb_to_yuv420p10(C.post10(r), **opts).astype(int)
        got_y = _np(m.forward_yuv420p10(_dev(ya, dev), _dev(yc, dev), h, w, **opts)).astype(int)
        dy = np.abs(got_y - want_y)
        print(f"yuv420p10: max {dy.max()} codes, {int((dy != 0).sum())} of {dy.size} off")
        assert dy.max() <= 1


# ---- 5. the same bits through every entry point -----------------------------------------------------------------
@pytest.fixture(scope="module")
def seeded(dev):
    out = {1: _model(dev, O.make_seeded_state_dict(1234)),
           3: _model(dev, O.make_seeded_state_dict(77, n_channels=6, n_classes=3), 3)}
    yield out
    out.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("cf,h,w,unfused", [(1, 64, 96, False), (1, 33, 47, False), (1, 48, 80, True),
                                            (3, 40, 56, False), (3, 40, 56, True), (3, 530, 950, False)])
def test_u8_and_p10_equal_their_public_chains(dev, seeded, cf, h, w, unfused):
    m = seeded[cf]
    m.set_options(unfused=unfused)
    try:
        gen = torch.Generator().manual_seed(h * 131 + w)
        a = torch.randint(0, 256, (2, cf, h, w), dtype=torch.uint8, generator=gen).to(dev)
        b = torch.randint(0, 256, (2, cf, h, w), dtype=torch.uint8, generator=gen).to(dev)
        want = _native.postprocess_u8(m(_native.preprocess_u8(a), _native.preprocess_u8(b)))
        assert torch.equal(m.forward_u8(a, b), want)
        inter = torch.full((4, cf, h, w), 0xA5, dtype=torch.uint8, device=dev)
        m.forward_u8(a, b, out=inter[1::2])
        assert torch.equal(inter[1::2], want) and (inter[0::2] == 0xA5).all()
        rng = np.random.default_rng(h + w)
        p, q = (_dev(rng.integers(0, 1024, (2, cf, h, w), dtype=np.uint16), dev) for _ in range(2))
        want10 = _np(_native.postprocess_p10(m(_native.preprocess_p10(p), _native.preprocess_p10(q))))
        assert np.array_equal(_np(m.forward_p10(p, q)), want10)
        if cf == 3 and h < 100:
            fr = [_dev(np.random.default_rng(s).integers(0, 256, (2, h * w + 2 * ((h + 1) // 2) * ((w + 1) // 2)),
                                                         dtype=np.uint8), dev) for s in (1, 2)]
            ra, rb = P.yuv420_to_rgb(fr[0], h, w), P.yuv420_to_rgb(fr[1], h, w)
            assert torch.equal(m.forward_yuv420(fr[0], fr[1], h, w), P.rgb_to_yuv420(m.forward_u8(ra, rb)))
            fr10 = [_dev(C.rgb_to_yuv420p10(rng.integers(0, 1024, (2, 3, h, w), dtype=np.uint16)), dev) for _ in range(2)]
            r10a, r10b = P.yuv420p10_to_rgb(fr10[0], h, w), P.yuv420p10_to_rgb(fr10[1], h, w)
            assert np.array_equal(_np(m.forward_yuv420p10(fr10[0], fr10[1], h, w)),
                                  _np(P.rgb_to_yuv420p10(m.forward_p10(r10a, r10b))))
    finally:
        m.set_options()


def test_row_bands_equal_the_whole_frame(dev, seeded):
    m = seeded[1]
    f1, f2 = O.make_frames(51, 1, 512, 160)
    f1, f2 = f1.to(dev), f2.to(dev)
    assert torch.equal(tiling.forward_tiled(m.forward_strip, f1, f2, 2), m(f1, f2))


def test_graph_replay_and_gather_upsample_bits(dev, seeded):
    m = seeded[1]
    f1, f2 = (t.to(dev) for t in O.make_frames(41, 1, 64, 96))
    ref = m(f1, f2).clone()
    g = P.GraphedForward(m, 1, 64, 96)
    for _ in range(2):
        assert torch.equal(g(f1, f2), ref)
    svc = P.InterpolationService(model=m, device="cuda")
    t1 = torch.rand(1, 1, 64, 96, generator=torch.Generator().manual_seed(3)).to(dev) * 2 - 1
    t2 = torch.rand(1, 1, 64, 96, generator=torch.Generator().manual_seed(4)).to(dev) * 2 - 1
    eager = m(t1, t2)
    assert torch.equal(svc._forward(t1, t2), eager) and torch.equal(svc._forward(t1, t2), eager)
    # the in-gather upsample against the materialised one, where the launch plan materialises it (1080p level 1)
    a, b = (t.to(dev) for t in O.make_frames(43, 1, 1080, 1920))
    base = m(a, b)
    m.set_options(gather_upsample=True)
    try:
        assert torch.equal(m(a, b), base)
    finally:
        m.set_options()


def test_fused_against_unfused_stage_by_stage(dev, seeded):
    m = seeded[1]
    f1, f2 = (t.to(dev) for t in O.make_frames(21, 2, 50, 70))
    acts_a, a = m.debug_activations(f1, f2)
    m.set_options(unfused=True)
    try:
        acts_b, b = m.debug_activations(f1, f2)
    finally:
        m.set_options()
    for k in acts_a:
        rel = (acts_a[k] - acts_b[k]).norm().item() / acts_b[k].norm().item()
        assert rel <= 2e-3, (k, rel)
    assert _rel(a, b) <= 2e-3


# ---- 6. batch invariance -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(256, 256), (720, 1280), (1080, 1920)])
def test_min_unsplit_batch_and_batch_invariance(dev, seeded, h, w):
    m = seeded[1]
    ctx = m._context(dev)
    n16 = ctx.min_unsplit_batch(h, w, _native.FP16)
    assert n16 == ctx.min_unsplit_batch(h, w, _native.BF16)
    if n16 > 8 or h > 720:
        return   # (1080p: checked at B = 1 against B = 2 below only where it is cheap)
    f1, f2 = (t.to(dev) for t in O.make_frames(7, n16 + 1, h, w))
    big = m(f1, f2)
    small = m(f1[:n16].contiguous(), f2[:n16].contiguous())
    assert torch.equal(big[:n16], small)


# ---- 7. saturation -----------------------------------------------------------------------------------------------
def test_saturation_gives_a_finite_output(dev):
    sd = O.make_seeded_state_dict(1234)
    for k in list(sd):
        if k.endswith(".bias") and "down3.maxpool_conv.1.double_conv" in k:
            sd[k] = torch.full_like(sd[k], 2e5)   # BatchNorm shift: every down3 activation beyond 65504
    m = _model(dev, sd)
    f1, f2 = (t.to(dev) for t in O.make_frames(5, 1, 64, 64))
    acts, out = m.debug_activations(f1, f2)
    assert max(a.abs().max().item() for a in acts.values()) >= 65504.0   # the test reaches the clamp
    assert torch.isfinite(out).all() and all(torch.isfinite(a).all() for a in acts.values())
    assert torch.isfinite(m(f1, f2)).all()


# ---- 8. video ----------------------------------------------------------------------------------------------------
def _moving_texture10(n, h, w):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    out = []
    for t in range(n):
        x = xx - 2 * t
        out.append(np.stack([512 + 400 * np.sin(x / 5.0) * np.cos(yy / 7.0), 512 + 360 * np.cos((x + yy) / 6.0),
                             512 + 320 * np.sin((x - 0.5 * yy) / 4.0)]))
    return np.clip(np.rint(np.stack(out)), 0, 1023).astype(np.uint16)


def test_interpolate_video_c420p10_rgb_fp16(tmp_path, dev, interp_models):
    m = interp_models[3][0]
    h, w, n = 49, 67, 5
    packed = C.rgb_to_yuv420p10(_moving_texture10(n, h, w), "mpeg2", "bt2020")
    ny, nc = h * w, ((h + 1) // 2) * ((w + 1) // 2)
    y = packed[:, :ny].reshape(n, h, w)
    ch = (packed[:, ny:ny + nc].reshape(n, (h + 1) // 2, (w + 1) // 2),
          packed[:, ny + nc:].reshape(n, (h + 1) // 2, (w + 1) // 2))
    src = tmp_path / "in.y4m"
    IO.write_y4m_p10(str(src), y, ch, fps=(50, 1))
    outs = {}
    for prec in ("fp32", "fp16"):
        m.precision = prec
        dst = tmp_path / f"out_{prec}.y4m"
        cnt = P.FrameInterpolator(model=m, device="cuda").interpolate_video(str(src), str(dst), 2, matrix="bt2020")
        assert cnt == 2 * (n - 1) + 1
        outs[prec], hdr = IO.read_y4m_packed_p10(str(dst))
    m.precision = "fp16"
    assert outs["fp16"].shape == outs["fp32"].shape and outs["fp16"].max() <= 1023
    assert np.array_equal(outs["fp16"][0::2], outs["fp32"][0::2])
    d = np.abs(outs["fp16"].astype(int) - outs["fp32"].astype(int))
    print(f"video fp16 vs fp32: max {d.max()} codes")
    assert d.max() <= 1
