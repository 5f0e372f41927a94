"""GPU (MI355X): the workspace contract of every forward entry point, through `_native.Context` with a workspace the test
owns.  tests/test_workspace_plan.py pins the layout on the host; this file pins what the kernels do with it:

  * bounds - the workspace is the middle of one allocation, exactly as many bytes as the matching `*_workspace_bytes`
    query answers, with 1 MiB of guard bytes on either side that must come back untouched;
  * stale contents - the workspace is never cleared, and one block serves every shape, option set and precision in turn,
    so a forward must not depend on a single byte it finds there.  Each case runs three times, the whole allocation and
    the output filled with 0x00, 0x7B (a large finite positive number in bf16, fp16 and fp32: it survives ReLU, max-pool
    and the fp16 clamp) and 0xFF (NaN in all three: it survives a multiplication by zero), and the three results must be
    the same bits - which also says that every output element was written.  Under KEEP_ALL the same holds for every
    stored tensor, padding included;
  * the result equals the module's public call (its own larger, reused workspace), and `fiunet_debug_plan`'s total is
    what the context's query answers;
  * a workspace one byte short or not 256-B aligned is refused before anything is launched.

Shapes are the smallest at which each mechanism is live (the table at CASES).  All comparisons are bitwise, on integer
views (NaN != NaN would hide an all-NaN tensor from torch.equal on floats)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, colour, packed, tiling  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 1 << 20            # bytes on either side of the workspace; a multiple of 256, so the middle view stays aligned
FILLS = (0x00, 0x7B, 0xFF)
PREC = {"fp32": _native.FP32, "bf16": _native.BF16, "bf16x2": _native.BF16X2, "fp16": _native.FP16}
LEVEL = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]
ERR_INVALID_ARG, ERR_WORKSPACE = 1, 5   # include/fiunet.h: enum fiunet_status


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev, seeded_sd):
    """The seeded checkpoints of the other GPU tests: gray (conftest), RGB (seed 77), ConvTranspose2d decoder (1234)."""
    sds = {"gray": (seeded_sd, 1, True), "rgb": (O.make_seeded_state_dict(77, n_channels=6, n_classes=3), 3, True),
           "convt": (O.make_seeded_state_dict(1234, bilinear=False), 1, False)}
    out = {}
    for v, (sd, cf, bil) in sds.items():
        m = P.FrameInterpolationUNet(bilinear=bil, frame_channels=cf)
        m.load_state_dict(sd)
        out[v] = m.to(dev).eval()
    return out


class _Configured:
    """`with _Configured(model, prec, opt) as ctx`: the module at that precision and option, its context; restored after."""

    def __init__(self, m, prec, opt):
        self.m, self.prec, self.opt = m, prec, opt

    def __enter__(self):
        self.m.precision = self.prec
        self.m.set_options(**({} if self.opt == "default" else {self.opt: True}))
        ctx = self.m._context(next(self.m.parameters()).device)
        ctx.prepare(PREC[self.prec])
        return ctx

    def __exit__(self, *exc):
        self.m.set_options()
        self.m.precision = "fp32"
        if self.m._ctx is not None:
            self.m._ctx.force_cfg(-1)


class _Guarded:
    """GUARD + n + GUARD bytes in one tensor; `.ws` is the middle view of exactly n bytes."""

    def __init__(self, dev, n):
        self.n = n
        self.buf = torch.empty(GUARD + n + GUARD, dtype=torch.uint8, device=dev)
        self.ws = self.buf[GUARD:GUARD + n]
        assert self.ws.numel() == n and self.ws.data_ptr() % 256 == 0

    def fill(self, byte):
        self.buf.fill_(byte)

    def check(self, byte, what=""):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.n:]
        bad_lo, bad_hi = int((lo != byte).sum()), int((hi != byte).sum())
        assert bad_lo == 0 and bad_hi == 0, (f"{what}: {bad_lo} guard bytes below and {bad_hi} above the workspace changed "
                                             f"(fill {byte:#04x})")


def _bytes(t):
    return t.view(torch.uint8)


def _bits(t):
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not torch.equal(a, b):
        d = a != b
        raise AssertionError(f"{what}: {int(d.sum())} of {d.numel()} elements differ, first at {d.nonzero()[0].tolist()}")


def _check_fills(dev, nbytes, new_out, run, want, taps=None, what=""):
    """`run(ws, out)` once per fill on a guarded workspace of exactly `nbytes`: guards intact, the outputs (and, with
    `taps(ws)` -> {name: tensor}, every read-back tensor) bit-identical across the fills; the output equals `want`.
    -> {name: tensor} of the read-back (first fill)."""
    g = _Guarded(dev, nbytes)
    first = None
    for fill in FILLS:
        g.fill(fill)
        out = new_out()
        _bytes(out).fill_(fill)
        run(g.ws, out)
        torch.cuda.synchronize(dev)
        g.check(fill, what)
        got_t = taps(g.ws) if taps else {}
        got = (_bits(out).clone(), {k: _bits(v) for k, v in got_t.items()})
        if first is None:
            first, first_t = got, got_t
            continue
        _same(got[0], first[0], f"{what}: output, fill {fill:#04x} against {FILLS[0]:#04x} (stale workspace bytes are read)")
        assert got[1].keys() == first[1].keys()
        for k in got[1]:
            _same(got[1][k], first[1][k], f"{what}: tap {k}, fill {fill:#04x} against {FILLS[0]:#04x}")
    _same(first[0], _bits(want), f"{what}: output against the module's public call")
    return first_t


def _levels(h, w):
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append(hs[-1] // 2); ws.append(ws[-1] // 2)
    return hs, ws


def _read_taps(ctx, b, h, w, prec):
    """Every tensor the read-back offers under KEEP_ALL: taps 0..17, and 18..21 (the upsampled halves) where stored."""
    def read(ws):
        out = {}
        for t in range(22):
            try:
                out[t] = ctx.read_activation(ws, b, h, w, PREC[prec], t)
            except _native.NativeError as e:
                if t < 18 or e.status != _native.ERR_UNSUPPORTED:   # (unsupported: interpolated inside the gather)
                    raise
        return out
    return read


def _forward_case(m, ctx, dev, prec, b, h, w, seed=5, what=""):
    """fiunet_forward at the module's current options under guards and fills; with KEEP_ALL also every read-back tap."""
    cf, bil, flags = m.frame_channels, m.unet.bilinear, m._options
    f1, f2 = (t.to(dev) for t in O.make_frames(seed, b, h, w, c=cf))
    want = m(f1, f2)
    n = ctx.workspace_bytes(b, h, w, PREC[prec])
    assert _native.debug_plan(cf, bil, flags, PREC[prec], b, h, w)[1] == n
    keep = bool(flags & _native.OPT_KEEP_ALL)
    taps = _check_fills(dev, n, lambda: torch.empty_like(f1), lambda ws, out: ctx.forward(f1, f2, out, PREC[prec], ws), want,
                        _read_taps(ctx, b, h, w, prec) if keep else None, what)
    if keep:
        assert set(range(18)) <= set(taps)
        if not bil:   # F.pad of the ConvTranspose2d halves (unet.py:49-53): exactly zero around the 2x upsampled tensor
            hs, ws_ = _levels(h, w)
            for k in range(4):
                lv = LEVEL[10 + 2 * k]
                top, left = (hs[lv] - 2 * hs[lv + 1]) // 2, (ws_[lv] - 2 * ws_[lv + 1]) // 2
                t = _bits(taps[18 + k]).clone()
                assert t.shape[-2:] == (hs[lv], ws_[lv])
                t[..., top:top + 2 * hs[lv + 1], left:left + 2 * ws_[lv + 1]] = 0
                assert int((t != 0).sum()) == 0, (what, "padding of up half", k)


# shape -> what it exercises; (precision, variant, option) so that every precision meets every shape, every option every
# variant (bf16x2 ignores unfused / gather_upsample), and the ConvTranspose2d model runs both 64x96 (no F.pad: its memset
# is skipped) and padded shapes.  No KEEP_ALL at 2x270x480.
CASES = {
    (1, 16, 16): [("fp32", "gray", "default"), ("bf16", "convt", "keep_all"), ("bf16x2", "rgb", "keep_all"),       # deepest level 1x1
                  ("fp16", "gray", "unfused")],
    (3, 17, 31): [("fp32", "convt", "unfused"), ("bf16", "gray", "keep_all"), ("bf16x2", "convt", "default"),      # odd at every level,
                  ("fp16", "rgb", "gather_upsample"), ("fp32", "convt", "keep_all")],                             # F.pad everywhere, K cuts
    (2, 50, 70): [("fp32", "rgb", "keep_all"), ("bf16", "convt", "gather_upsample"), ("bf16x2", "gray", "default"),
                  ("fp16", "convt", "keep_all")],
    (1, 64, 96): [("fp32", "convt", "default"), ("bf16", "rgb", "unfused"), ("bf16x2", "convt", "keep_all"),       # small tiles, no padding
                  ("fp16", "gray", "gather_upsample")],
    (2, 135, 240): [("fp32", "rgb", "gather_upsample"), ("bf16", "gray", "default"), ("bf16", "gray", "gather_upsample"),   # materialised upsample
                    ("bf16x2", "rgb", "default"), ("fp16", "convt", "unfused"), ("bf16", "gray", "keep_all")],             # against gather
    (2, 270, 480): [("fp32", "gray", "unfused"), ("bf16", "gray", "default"), ("bf16x2", "rgb", "default"),         # tuned tiles, whole K loops
                    ("fp16", "rgb", "unfused"), ("bf16", "convt", "default")],
}
_FORWARD = [pytest.param(*shape, *c, id=f"{shape[0]}x{shape[1]}x{shape[2]}-{c[0]}-{c[1]}-{c[2]}")
            for shape, cs in CASES.items() for c in cs]


def test_the_case_table_covers_what_it_claims():
    assert all({c[0] for c in cs} == set(PREC) for cs in CASES.values())
    pairs = {(c[1], c[2]) for cs in CASES.values() for c in cs}
    assert pairs == {(v, o) for v in ("gray", "rgb", "convt") for o in ("default", "unfused", "gather_upsample", "keep_all")}
    assert not any(c[0] == "bf16x2" and c[2] in ("unfused", "gather_upsample") for cs in CASES.values() for c in cs)
    assert not any(c[2] == "keep_all" for c in CASES[2, 270, 480])
    convt = {s for s, cs in CASES.items() for c in cs if c[1] == "convt"}
    assert (1, 64, 96) in convt and {(3, 17, 31), (2, 50, 70), (2, 135, 240)} <= convt


@pytest.mark.parametrize("b,h,w,prec,variant,opt", _FORWARD)
def test_forward_guards_and_fills(models, dev, b, h, w, prec, variant, opt):
    m = models[variant]
    with _Configured(m, prec, opt) as ctx:
        _forward_case(m, ctx, dev, prec, b, h, w, what=f"{variant} {prec} {opt} {b}x{h}x{w}")


@pytest.mark.parametrize("variant,prec", [("convt", "fp32"), ("convt", "bf16"), ("convt", "bf16x2"), ("gray", "fp32"),
                                          ("gray", "bf16"), ("gray", "fp16")])
def test_strips_guards_and_fills(models, dev, variant, prec):
    """A 70x86 frame as the bands [0, 32) and [32, 70) through fiunet_forward_strip: F.pad, the upsample mapping and - with
    the ConvTranspose2d decoder - the cleared band edges are evaluated in whole-image coordinates, on a workspace that is
    one band's.  Each band equals the module's `forward_strip` of it, and `tiling.forward_tiled` through the guarded
    workspace equals `tiling.forward_tiled` on the module (its plan needs 112 halo rows, so at this height both of its
    bands are the whole frame at origin 0: the strip entry point as the un-tiled forward)."""
    m, b, h, w = models[variant], 2, 70, 86
    f1, f2 = (t.to(dev) for t in O.make_frames(9, b, h, w))
    with _Configured(m, prec, "default") as ctx:
        def guarded(a, c, y0, hg, what):
            a, c = a.contiguous(), c.contiguous()
            n = ctx.workspace_bytes(b, a.shape[-2], w, PREC[prec])
            assert _native.debug_plan(1, m.unet.bilinear, 0, PREC[prec], b, a.shape[-2], w)[1] == n
            want, outs = m.forward_strip(a, c, y0, hg), []

            def run(ws, out):
                ctx.forward_strip(a, c, out, y0, hg, PREC[prec], ws)
                outs.append(out)
            _check_fills(dev, n, lambda: torch.empty_like(a), run, want, what=what)
            return outs[-1]
        for y0, y1 in ((0, 32), (32, 70)):
            guarded(f1[:, :, y0:y1], f2[:, :, y0:y1], y0, h, f"{variant} {prec} band [{y0}, {y1})")
        tiled = tiling.forward_tiled(lambda a, c, y0, hg: guarded(a, c, y0, hg, f"{variant} {prec} tiled band at {y0}"), f1, f2, 2)
        _same(_bits(tiled), _bits(tiling.forward_tiled(m.forward_strip, f1, f2, 2)), "forward_tiled")


_FORCED = [(1, 2), (1, 4), (1, 16), (2, 2), (2, 4), (2, 16), (3, 0)]   # (tile family, K cut); 3: the in-workgroup cut


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("b,h,w,opt", [(2, 48, 80, "default"), (3, 33, 47, "keep_all")], ids=["2x48x80", "3x33x47-keep_all"])
def test_forced_configurations_guards_and_fills(models, dev, prec, b, h, w, opt):
    """K cuts 2, 4 and 16 on the tuned and the small tiles, and the cut over the waves of a workgroup: the slab is the only
    buffer that several workgroups write before anyone reads it, and a partial tile's slices lie past the tensor's edge."""
    m = models["gray"]
    with _Configured(m, prec, opt) as ctx:
        for tile, k in _FORCED:
            for layer in range(1, 18):
                ctx.force_cfg(layer, tile, k)
            _forward_case(m, ctx, dev, prec, b, h, w, seed=43, what=f"gray {prec} {opt} {b}x{h}x{w} tile {tile} ksplit {k}")


# ---- the uint8 / 10-bit / colour wrappers, each with exactly its own workspace query ---------------------------------
def _rand_u8(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8))


def _rand_p10(seed, *shape):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 1024, shape).astype(np.uint16))


# name -> (variant, precision, option).  forward_u8's three staging cases: fp32 gray stages the frames in fp32, the
# ablation path stages the logits, bf16 gray at W >= 32 (fused stem, fused head) stages neither.
WRAPPERS = {
    "u8-fp32-gray": ("gray", "fp32", "default"), "u8-unfused": ("gray", "bf16", "unfused"),
    "u8-bf16-gray": ("gray", "bf16", "default"), "u8-rgb": ("rgb", "fp16", "default"),
    "p10": ("gray", "fp16", "default"), "yuv420": ("rgb", "bf16", "default"), "yuv420p10": ("rgb", "fp16", "default"),
    "nv12": ("rgb", "bf16", "default"), "rgb_packed": ("rgb", "bf16x2", "default"), "yuv422p": ("rgb", "fp32", "default"),
    "forward": ("gray", "bf16", "default"), "forward_strip": ("convt", "fp32", "default"),
}


def _wrapper(name, m, ctx, dev, prec, b, h, w):
    """-> (workspace bytes, new_out(), run(ws, out), public() -> tensor) of one entry point on random frames."""
    code, cf, L, hnd = PREC[prec], m.frame_channels, _native.lib(), ctx._h
    if name.startswith("u8"):
        a, c = _rand_u8(1, b, cf, h, w).to(dev), _rand_u8(2, b, cf, h, w).to(dev)
        return (ctx.workspace_bytes(b, h, w, code, u8=True), lambda: torch.empty_like(a),
                lambda ws, out: ctx.forward_u8(a, c, out, code, ws), lambda: m.forward_u8(a, c))
    if name == "p10":
        a, c = _rand_p10(1, b, cf, h, w).to(dev), _rand_p10(2, b, cf, h, w).to(dev)
        return (ctx.workspace_bytes(b, h, w, code, p10=True), lambda: torch.empty_like(a),
                lambda ws, out: ctx.forward_p10(a, c, out, code, ws), lambda: m.forward_p10(a, c))
    if name in ("yuv420", "yuv420p10"):
        bits = 10 if name.endswith("p10") else 8
        fs, rand = colour.i420_frame_bytes(h, w), _rand_p10 if bits == 10 else _rand_u8
        a, c = rand(1, b, fs).to(dev), rand(2, b, fs).to(dev)
        flags = colour.colour_flags("jpeg", "bt709", "limited", bits=bits)
        pub = m.forward_yuv420p10 if bits == 10 else m.forward_yuv420
        return (ctx.workspace_bytes(b, h, w, code, yuv=True, p10=bits == 10), lambda: torch.empty_like(a),
                lambda ws, out: ctx.forward_yuv420(a, c, out, h, w, flags, code, ws, bits), lambda: pub(a, c, h, w))
    if name == "nv12":
        lay = colour.resolve_layout(None, h, w)
        a, c = _rand_u8(1, b, lay.frame_stride).to(dev), _rand_u8(2, b, lay.frame_stride).to(dev)
        flags = colour.colour_flags("mpeg2", "bt709", "limited", bits=8)
        return (L.fiunet_workspace_bytes_nv12(hnd, b, h, w, code), lambda: torch.empty_like(a),
                lambda ws, out: ctx.forward_surface(a, c, lay, out, lay, h, w, flags, code, ws, 8),
                lambda: m.forward_nv12(a, c, h, w))
    if name == "rgb_packed":
        lay = packed.resolve_layout(None, "rgb24", h, w)
        a, c = _rand_u8(1, b, lay.frame_stride).to(dev), _rand_u8(2, b, lay.frame_stride).to(dev)
        return (L.fiunet_workspace_bytes_rgb_packed(hnd, b, h, w, code), lambda: torch.empty_like(a),
                lambda ws, out: ctx.forward_rgb_packed(a, c, lay, out, lay, h, w, packed.FORMATS["rgb24"][0], code, ws),
                lambda: m.forward_rgb_packed(a, c, h, w, format="rgb24"))
    if name == "yuv422p":
        lay = colour.resolve_yuv_layout(None, name, h, w)
        a, c = _rand_u8(1, b, lay.frame_stride).to(dev), _rand_u8(2, b, lay.frame_stride).to(dev)
        flags = colour.yuv_flags(name, None, "bt709", "limited")
        return (L.fiunet_workspace_bytes_yuv(hnd, b, h, w, code, 8), lambda: torch.empty_like(a),
                lambda ws, out: ctx.forward_yuv(a, c, colour.YUV_FORMATS[name][0], lay, out, lay, h, w, flags, code, ws, 8),
                lambda: m.forward_yuv(a, c, h, w, format=name))
    f1, f2 = (t.to(dev) for t in O.make_frames(3, b, h, w, c=cf))
    if name == "forward":
        return (ctx.workspace_bytes(b, h, w, code), lambda: torch.empty_like(f1),
                lambda ws, out: ctx.forward(f1, f2, out, code, ws), lambda: m(f1, f2))
    assert name == "forward_strip"   # rows [16, 16 + h) of an image 16 rows taller
    return (ctx.workspace_bytes(b, h, w, code), lambda: torch.empty_like(f1),
            lambda ws, out: ctx.forward_strip(f1, f2, out, 16, h + 16, code, ws), lambda: m.forward_strip(f1, f2, 16, h + 16))


@pytest.mark.parametrize("b,h,w", [(2, 37, 53), (1, 48, 64)], ids=["2x37x53", "1x48x64"])
@pytest.mark.parametrize("name", [n for n in WRAPPERS if not n.startswith("forward")])
def test_wrappers_guards_and_fills(models, dev, name, b, h, w):
    variant, prec, opt = WRAPPERS[name]
    m = models[variant]
    with _Configured(m, prec, opt) as ctx:
        n, new_out, run, public = _wrapper(name, m, ctx, dev, prec, b, h, w)
        base, image = ctx.workspace_bytes(b, h, w, PREC[prec]), (b * m.frame_channels * h * w * 4 + 255) // 256 * 256
        assert n >= base
        if name == "u8-fp32-gray":
            assert n - base == 2 * image     # the two frames in fp32
        if name == "u8-unfused":
            assert n - base >= image         # (at least) the logits
        if name == "u8-bf16-gray":
            assert n == base                 # fused stem and fused head: nothing staged
        _check_fills(dev, n, new_out, run, public(), what=f"{name} {b}x{h}x{w}")


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_short_or_misaligned_workspace_is_refused_before_any_launch(models, dev, name):
    variant, prec, opt = WRAPPERS[name]
    m, (b, h, w), fill = models[variant], (1, 48, 64), 0x7B
    with _Configured(m, prec, opt) as ctx:
        n, new_out, run, _ = _wrapper(name, m, ctx, dev, prec, b, h, w)
        g = _Guarded(dev, n)
        g.fill(fill)
        out = new_out()
        _bytes(out).fill_(fill)
        with pytest.raises(_native.NativeError) as e:
            run(g.buf[GUARD:GUARD + n - 1], out)                 # one byte short
        assert e.value.status == ERR_WORKSPACE, e.value
        with pytest.raises(_native.NativeError) as e:
            run(g.buf[GUARD + 128:GUARD + 128 + n], out)         # large enough, 128 B off the alignment
        assert e.value.status == ERR_INVALID_ARG, e.value
        torch.cuda.synchronize(dev)
        assert int((g.buf != fill).sum()) == 0 and int((_bytes(out) != fill).sum()) == 0
        run(g.ws, out)                                           # (and the exact one is accepted)
        torch.cuda.synchronize(dev)
        g.check(fill, name)
