"""GPU (MI355X): every kernel's addressing where byte offsets pass 2^31 and 2^32.

make_plan accepts any frame below 2^26 pixels; the conv kernels then address a 64-B pixel record inside one plane with a
32-bit offset (the LDS-DMA gathers take a wave-uniform 64-bit base and a 32-bit lane offset, the per-tile walk wraps its
offsets mod 2^32 on purpose).  The rest of the suite stops at 2160x3840, below 2^29.  Here (shapes and the zone - level-0
pixels from index 2^25 on, byte offset 2^31 on - in tests/large_extent.py; the host-side conditions in
tests/test_large_extent_host.py):

  1. whole frame == its row bands, bit for bit (torch.equal on the device): tiling.forward_tiled computes the same output
     from bands of fewer than 2^25 pixels, whose offsets stay below 2^31, through launches that are the whole frame's stage
     by stage (the host test), and each band path is pinned to the float64 and reference oracles at sizes up to 4K by the
     rest of the suite.  Every precision, the ablation path (upcat_kernel, maxpool2_kernel, head1x1_kernel and the concat
     scratch past 4 GiB), the RGB network (the persistent stem loop, EPI_HEAD3), the ConvTranspose2d network
     (convt2x2_kernel), either tile family forced on the level-0 convs (the hoisted-offset gather and the three-register
     walk both run in the zone), and forward_u8, whose fused head writes uint8 at b*stride + (c*H + y)*W + x in the zone.
  2. the level-0 stages per element against the float64 windowed reference under the unchanged stage_bound
     (test_gpu_stage_windows.run_windows), on tiles around the pixel where byte 2^31 falls and at the far corners; the
     read-back then writes 9.7 GB fp32 taps, past 2^31 elements.
  3. frames more than 2^32 bytes from their base: every video-side kernel that takes a frame or image stride, on a view of
     one large buffer against the same call on a tight copy, guard bytes untouched; and the three kernels on contiguous
     stacks (pair_sad_u8, retime_u8, hold_cut_frames) with frames of 2^30 + 3 samples against int64 torch.

Every test first compares the free device memory with its planned need plus 4 GiB and skips with both numbers if the card
lacks the room.  Each prints one line `large-extent <case>: peak <GiB> GiB, <seconds> s`.

Measured on an MI355X (peak torch allocation, seconds inside the case; none skipped on a 288 GB card):
  part 1   gray bf16 A 14.1 GiB 0.6 s, B 24.8 GiB 0.7 s, C 14.9 GiB 0.4 s; gray fp16 A 14.1 GiB 0.1 s; fp32 A 28.1 GiB 0.7 s;
           bf16x2 A 36.0 GiB 0.2 s; bf16 unfused A 23.6 GiB 2.3 s; rgb bf16 A 16.4 GiB 1.1 s; ConvTranspose2d bf16 A 16.9 GiB
           0.3 s; forced families 13.9 GiB 0.1 s; forward_u8 13.8 GiB 0.2 s - all bit for bit
  part 2   56.8 GiB, 0.3 s; worst error / bound (error / M) per stage family at 1 x 4603 x 8201, bf16, dither off:
           stem 0.973 (3.6e-03), inc.3 0.945 (3.5e-03), pool-fed 0.980 (3.7e-03), concat 0.940 (3.2e-03), direct 0.945
           (3.1e-03), head 0.679 (2.7e-03) - the figures of 8 x 552 x 1000 (test_gpu_stage_windows.py), as they must be
  part 3   every family bit for bit, guards intact; the stacks 16.3 GiB, 0.4 s
"""
import gc
import time

import pytest
import torch

import large_extent as L
import test_gpu_stage_windows as W
from ai_based_frame_interpolation_amd import _native, tiling
from oracle import stage_oracle as S
from oracle import unet_oracle as O
from test_gpu_bn_stats import _REPORT, caches, dev, models, sds  # noqa: F401

pytestmark = pytest.mark.gpu
_FRAMES = {}


def frames_for(name, cf):
    """The frame pair of a shape, made once per channel count and left unchanged (host tensors)."""
    if (name, cf) not in _FRAMES:
        _FRAMES[name, cf] = O.make_frames(97, *L.SHAPES[name], c=cf)
    return _FRAMES[name, cf]


def release(model):
    """Drop the model's cached workspace and give the allocator's blocks back, so that the next case starts empty."""
    model._ws = None
    gc.collect()
    torch.cuda.empty_cache()


class Case:
    """Skip unless the card has room for `need` bytes plus the headroom; on exit print peak allocation and duration."""

    def __init__(self, label, need, model):
        self.label, self.need, self.model = label, need, model

    def __enter__(self):
        release(self.model)
        free, total = torch.cuda.mem_get_info()
        if free < self.need + L.HEADROOM:
            pytest.skip(f"{self.label}: plans {self.need / L.GIB:.1f} GiB + {L.HEADROOM / L.GIB:.0f} GiB headroom, the card "
                        f"has {free / L.GIB:.1f} GiB free of {total / L.GIB:.1f}")
        torch.cuda.reset_peak_memory_stats()
        self.base = torch.cuda.memory_allocated()      # (what earlier modules of the same process still hold)
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - self.base
        print(f"\nlarge-extent {self.label}: peak {peak / L.GIB:.2f} GiB, {time.perf_counter() - self.t0:.1f} s")
        self.model.set_options()
        self.model.precision = "fp32"
        release(self.model)
        if exc[0] is None:
            assert peak <= self.need, (self.label, peak, self.need)      # the plan the skip rule rests on held
        return False


def assert_same(got, want, width, what):
    """torch.equal on the device; a mismatch names the first differing element and whether it lies in the zone."""
    if torch.equal(got, want):
        return
    ne = (got != want).flatten()
    n = int(ne.sum())
    first = int(ne.nonzero()[0])
    x, y = first % width, first // width % got.shape[-2]
    c = first // (width * got.shape[-2]) % got.shape[1]
    raise AssertionError(f"{what}: {n} element(s) differ, the first at (c={c}, y={y}, x={x}), "
                         f"{'in' if L.in_zone(y, x, width) else 'below'} the zone (from row {L.zone_start(width)[0]}, "
                         f"column {L.zone_start(width)[1]} on): {got.flatten()[first].item()!r} != "
                         f"{want.flatten()[first].item()!r}")


# ---- 1. whole frame == its row bands -------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,variant,prec,name,unfused", L.WHOLE_VS_BANDS, ids=[c[0] for c in L.WHOLE_VS_BANDS])
def test_whole_frame_equals_its_row_bands_bit_for_bit(models, dev, label, variant, prec, name, unfused):
    model = models[variant]
    with Case(label, L.whole_vs_bands_need(variant, prec, name, unfused), model):
        f1, f2 = (t.to(dev) for t in frames_for(name, L.VARIANTS[variant][0]))
        model.precision = prec
        model.set_options(unfused=unfused)
        whole = model(f1, f2)
        tiled = tiling.forward_tiled(model.forward_strip, f1, f2, L.N_BANDS[name])
        assert_same(whole, tiled, L.SHAPES[name][2], f"{label}: whole against {L.N_BANDS[name]} bands")
        assert bool(whole.isfinite().all()) and whole[..., L.zone_start(L.SHAPES[name][2])[0] + 1:, :].std().item() > 0


def test_either_tile_family_on_the_level_0_convs_at_far_offsets(models, dev):
    """The families are bit-identical on an uncut K loop (test_forced_tile_families_and_k_cuts): stages 1, 16 and 17 forced
    to the tuned and to the small tile must give the unforced whole."""
    model = models["gray"]
    with Case("gray-bf16-A forced families", L.whole_vs_bands_need("gray", "bf16", "A", False), model):
        f1, f2 = (t.to(dev) for t in frames_for("A", 1))
        model.precision = "bf16"
        model.set_options()
        whole = model(f1, f2)
        ctx = model._context(dev)
        try:
            for tile in (1, 2):
                for layer in L.FORCED_STAGES:
                    ctx.force_cfg(layer, tile, 1)
                assert_same(model(f1, f2), whole, L.SHAPES["A"][2], f"stages {L.FORCED_STAGES} forced to tile family {tile}")
        finally:
            ctx.force_cfg(-1)


def test_forward_u8_equals_the_three_step_route_in_the_zone(models, dev):
    model = models["gray"]
    with Case("gray-bf16-A forward_u8", L.u8_need("A"), model):
        b, h, w = L.SHAPES["A"]
        g = torch.Generator().manual_seed(101)
        u1, u2 = (torch.randint(0, 256, (b, 1, h, w), dtype=torch.uint8, generator=g).to(dev) for _ in range(2))
        model.precision = "bf16"
        model.set_options()
        fused = model.forward_u8(u1, u2)
        steps = _native.postprocess_u8(model(_native.preprocess_u8(u1), _native.preprocess_u8(u2)))
        assert_same(fused, steps, w, "forward_u8 against postprocess_u8(forward(preprocess_u8))")
        assert fused[..., L.zone_start(w)[0] + 1:, :].float().std().item() > 0


# ---- 2. the level-0 stages per element in the zone ------------------------------------------------------------------------
def test_level_0_stages_per_element_in_the_zone(models, sds, caches, dev, monkeypatch):
    """gray bf16 at A, no dither, every stage kept: stages 0, 1, 2 (which reads the pooled level-0 tensor), 16, 17 and the
    head on large_extent.zone_windows, through run_windows and check_stage_windows as they are."""
    model = models["gray"]
    full_w = L.SHAPES["A"][2]
    monkeypatch.setattr(W, "stage_windows", lambda st, th, tw, b, h, w: L.zone_windows(st, th, tw, b, h, w, full_w))
    with Case("gray-bf16-A windows", L.window_need("A"), model):
        W.run_windows(model, sds["gray"], "gray", "bf16", frames_for("A", 1), caches["gray"], L.WINDOW_STAGES,
                      label=" zone")
    for (prec, family), r in sorted(_REPORT.items()):
        if family.endswith("@%dx%dx%d" % L.SHAPES["A"]):
            print(f"large-extent windows {prec} {family}: worst error / bound {r['max_err_over_bound']:.3f}, "
                  f"error / M {r['max_err_over_M']:.1e}")


# ---- 3. frames more than 2^32 bytes from their base -----------------------------------------------------------------------
FAR_BYTES = (1 << 32) + 4099        # from frame 0 to frame 1 of a far view, in bytes (16-bit samples: the next even number)
SLOT = 1 << 20                      # a far view may start at a multiple of this (several stacks in one buffer)
GUARD = 0xA5
SIZES = [(66, 130), (64, 128)]      # odd tails; and whole vectors, for the kernels that have a vector path


class Far:
    """One large guarded buffer and views of two frames FAR_BYTES apart inside it."""

    def __init__(self, device):
        self.buf = torch.empty(FAR_BYTES + 8 * SLOT + 1, dtype=torch.uint8, device=device)      # (an even size)
        self.buf.fill_(GUARD)
        self.used = []

    def frames(self, dtype, n, slot=0, shape=None):
        """[2, n] (or [2, *shape]) of `dtype` starting `slot` slots into the buffer, frame 1 FAR_BYTES after frame 0."""
        es = torch.empty(0, dtype=dtype).element_size()
        stride = -(-FAR_BYTES // es)
        assert stride * es >= 1 << 32 and n * es <= SLOT
        self.used += [(slot * SLOT, n * es), (slot * SLOT + stride * es, n * es)]
        flat = self.buf[slot * SLOT:].view(torch.int16 if es == 2 else torch.uint8)
        inner = (n,) if shape is None else tuple(shape)
        strides, acc = [], 1
        for d in reversed(inner):
            strides.insert(0, acc)
            acc *= d
        v = torch.as_strided(flat, (2,) + inner, (stride,) + tuple(strides))
        return v.view(dtype) if v.dtype != dtype else v

    def put(self, tight, slot=0):
        """The far view holding a copy of the contiguous `tight` [2, ...]."""
        v = self.frames(tight.dtype, tight[0].numel(), slot, tight.shape[1:])
        raw = torch.int16 if tight.element_size() == 2 else torch.uint8
        v.view(raw).copy_(tight.view(raw))
        return v

    def check(self):
        """Every byte outside the views handed out still holds the guard; the views are then refilled."""
        edges, self.used = sorted(set(self.used)), []
        pos = 0
        for start, size in edges + [(self.buf.numel(), 0)]:
            assert start >= pos, "far views overlap"
            gap = self.buf[pos:start]
            assert bool((gap == GUARD).all()), f"guard bytes {pos}..{start} were written"
            pos = start + size
        for start, size in edges:
            self.buf[start:start + size].fill_(GUARD)


@pytest.fixture(scope="module")
def far(dev, models):
    release(models["gray"])
    need = 2 * (FAR_BYTES + 8 * SLOT + 1)    # the buffer, and the compare's boolean temporary over the gap
    free, total = torch.cuda.mem_get_info()
    if free < need + L.HEADROOM:
        pytest.skip(f"far frames: plans {need / L.GIB:.1f} GiB + {L.HEADROOM / L.GIB:.0f} GiB headroom, the card has "
                    f"{free / L.GIB:.1f} GiB free of {total / L.GIB:.1f}")
    f = Far(dev)
    yield f
    del f.buf
    torch.cuda.empty_cache()


def same(a, b):
    raw = torch.int16 if a.element_size() == 2 else a.dtype
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(raw).contiguous(), b.view(raw).contiguous())


def codes(seed, shape, bits, dev, shift=0):
    """Random samples: uint8, or uint16 words of 10-bit codes (shift 6: P010 words)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    if bits == 8:
        return torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8)).to(dev)
    return torch.from_numpy((rng.integers(0, 1024, shape, dtype=np.uint16) << shift).astype(np.uint16)).to(dev)


def _conversions():
    from ai_based_frame_interpolation_amd import colour as C
    from ai_based_frame_interpolation_amd import packed as PK
    i420 = C.i420_frame_bytes
    table = {
        "yuv420": (8, 0, i420, C.yuv420_to_rgb, lambda rgb, out: C.rgb_to_yuv420(rgb, out=out)),
        "yuv420p10": (10, 0, i420, C.yuv420p10_to_rgb, lambda rgb, out: C.rgb_to_yuv420p10(rgb, out=out)),
        "nv12": (8, 0, i420, C.nv12_to_rgb, lambda rgb, out: C.rgb_to_nv12(rgb, out=out)),
        "p010": (10, 6, i420, C.p010_to_rgb, lambda rgb, out: C.rgb_to_p010(rgb, out=out)),
    }
    for fmt in ("uyvy422", "yuv444p10le"):          # one 4:2:2 format, one 4:4:4 format
        table[fmt] = (C.YUV_FORMATS[fmt][1], 0, lambda h, w, fmt=fmt: C.yuv_frame_samples(fmt, h, w),
                      lambda f, h, w, fmt=fmt: C.yuv_to_rgb(f, h, w, fmt),
                      lambda rgb, out, fmt=fmt: C.rgb_to_yuv(rgb, fmt, out=out))
    for fmt in ("rgb24", "bgra"):
        table[fmt] = (8, 0, lambda h, w, fmt=fmt: PK.frame_bytes(fmt, h, w),
                      lambda f, h, w, fmt=fmt: PK.packed_to_rgb(f, h, w, fmt),
                      lambda rgb, out, fmt=fmt: PK.rgb_to_packed(rgb, fmt, out=out))
    return table


FAMILIES = ["yuv420", "yuv420p10", "nv12", "p010", "uyvy422", "yuv444p10le", "rgb24", "bgra"]


@pytest.mark.parametrize("family", FAMILIES)
def test_frame_conversions_on_frames_2_32_bytes_apart(far, dev, family):
    """Both directions of one frame format: reading frames from a far view gives what the tight copy gives, and writing
    them into one gives the tight result in both frames and leaves every byte between and after them alone."""
    bits, shift, samples, to_rgb, from_rgb = _conversions()[family]
    for h, w in SIZES:
        n = samples(h, w)
        tight = codes(11, (2, n), bits, dev, shift)
        assert same(to_rgb(far.put(tight), h, w), to_rgb(tight, h, w)), (family, h, w, "to RGB")
        far.check()
        rgb = codes(12, (2, 3, h, w), bits, dev)
        want = from_rgb(rgb, None)
        out = far.frames(want.dtype, n)
        from_rgb(rgb, out)
        assert same(out, want), (family, h, w, "from RGB")
        far.check()


@pytest.mark.parametrize("h,w", SIZES)
def test_flow_and_warp_on_frames_2_32_bytes_apart(far, dev, h, w):
    from ai_based_frame_interpolation_amd import optical_flow as F
    a, b = codes(21, (2, h, w), 8, dev), codes(22, (2, h, w), 8, dev)
    fa, fb = far.put(a, 0), far.put(b, 1)
    flow = F.farneback_flow(a, b)
    assert torch.equal(F.farneback_flow(fa, fb), flow)
    for mode in F.MODES:
        want = F.warp(a, b, flow, mode)
        out = far.frames(torch.uint8, h * w, 2, (h, w))
        F.warp(fa, fb, flow, mode, out=out)
        assert same(out, want), mode
    far.check()


@pytest.mark.parametrize("h,w", SIZES)
def test_plane_metrics_on_frames_2_32_bytes_apart(far, dev, h, w):
    from ai_based_frame_interpolation_amd import metrics as M
    a, b = codes(31, (2, h, w), 8, dev), codes(32, (2, h, w), 8, dev)
    fa, fb = far.put(a, 0), far.put(b, 1)
    for got, want in zip(M.psnr_planes(fa, fb, 8, return_sse=True), M.psnr_planes(a, b, 8, return_sse=True)):
        assert torch.equal(got, want)
    assert torch.equal(M.ssim_planes(fa, fb, 8), M.ssim_planes(a, b, 8))
    far.check()
    a3, b3 = codes(33, (2, h, w, 3), 8, dev), codes(34, (2, h, w, 3), 8, dev)
    fa, fb = far.put(a3, 0), far.put(b3, 1)
    for got, want in zip(M.psnr_interleaved(fa, fb, 8, return_sse=True), M.psnr_interleaved(a3, b3, 8, return_sse=True)):
        assert torch.equal(got, want)
    far.check()


@pytest.mark.parametrize("bits", [8, 10])
def test_forward_u8_and_p10_into_images_2_32_bytes_apart(far, models, dev, bits):
    model = models["gray"]
    model.precision = "bf16"
    model.set_options()
    try:
        for h, w in SIZES:
            u1, u2 = codes(41, (2, 1, h, w), bits, dev), codes(42, (2, 1, h, w), bits, dev)
            fwd = model.forward_u8 if bits == 8 else model.forward_p10
            want = fwd(u1, u2)
            out = far.frames(want.dtype, h * w, 0, (1, h, w))
            fwd(u1, u2, out=out)
            assert same(out, want), (bits, h, w)
            far.check()
    finally:
        model.precision = "fp32"
        release(model)


def test_contiguous_stacks_whose_frames_pass_2_32_bytes(dev, models):
    """pair_sad_u8, retime_u8 and hold_cut_frames take contiguous stacks only: 5 frames of 2^30 + 3 samples, against torch
    on the device in int64, chunk by chunk."""
    from ai_based_frame_interpolation_amd import retime as RT
    from ai_based_frame_interpolation_amd import scene as SC
    n, chunk = (1 << 30) + 3, 1 << 27
    with Case("stacks of 2^30 + 3 samples", 20 * L.GIB, models["gray"]):
        g = torch.Generator(device=dev).manual_seed(51)
        stack = torch.randint(0, 256, (5, n), dtype=torch.uint8, device=dev, generator=g)
        want = torch.zeros(4, dtype=torch.int64, device=dev)
        for i in range(4):
            for c in range(0, n, chunk):
                d = stack[i + 1, c:c + chunk].to(torch.int16) - stack[i, c:c + chunk].to(torch.int16)
                want[i] += d.abs().sum(dtype=torch.int64)
        assert torch.equal(SC.pair_sad(stack, 8), want)
        # 24 -> 60 fps on one level of bisection (G = 2): the 5 rows are two intervals; output frames 3..5
        plan = RT.plan(24, 60, 1)
        p, q, G = plan
        got = RT.resample(stack, plan, 0, 3, 3, bits=8)
        for k, j in enumerate(range(3, 6)):
            i, r, lo, wn = plan.frame(j)
            for c in range(0, n, chunk):
                A = stack[i * G + lo, c:c + chunk]
                if wn:
                    B = stack[i * G + lo + 1, c:c + chunk].to(torch.int64)
                    A = ((A.to(torch.int64) * (q - wn) + B * wn + q // 2) // q).to(torch.uint8)
                assert torch.equal(got[k, c:c + chunk], A), (j, c)
        del got
        # a factor-2 loop over 3 frames, the second interval flagged: row 3 becomes a copy of row 2, the rest stays
        before = stack.clone()
        SC.hold_cut_frames(stack, torch.tensor([0, 1], dtype=torch.uint8, device=dev), 2)
        for row, src in enumerate((0, 1, 2, 2, 4)):
            assert torch.equal(stack[row], before[src]), row
