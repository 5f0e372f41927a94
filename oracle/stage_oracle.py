"""Layer-local float64 references and precision emulations for the HIP path -- TEST INFRASTRUCTURE.

`stage_reference(sd, stage, inputs, weights)` recomputes ONE stage of the network from the device's own read-back taps of
the stages that feed it, in float64, and returns the exact result `y_ref` together with `M`, the sum of the magnitudes
of the terms that make up each output element.  Checking a stage on its own inputs isolates that kernel's error from
what earlier layers passed on, and a bound in units of M holds whatever the BatchNorm statistics are.

The bf16 path's weights are restated bit for bit (`fold_bn`, `bf16_feedback`: csrc/fiunet.hip fiunet_load_weights,
f32_to_bf16_feedback), so a bf16 stage is compared against its own weights and the bound only covers the accumulation
and the rounding of its output.  The fp16 path's likewise (`f16_rne_sat`: csrc/pointwise.hip.h f16_pack_weights_kernel).
`emulate_forward` runs the whole network with the activations rounded where a precision stores them.

`stage_error` / `check_stage` hold a stage's read-back output to the precision's per-element bound (stated in
tests/test_gpu_bn_stats.py, which checks the device with it; tests/test_stage_oracle_fp16_host.py checks on the CPU that
the fp16 bound rejects what it is there to catch).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import unet_oracle as O

#: the 18 conv stages in state-dict order, as (block prefix, conv index, BatchNorm index)
PREFIXES = ["unet.inc"] + [f"unet.down{k}.maxpool_conv.1" for k in (1, 2, 3, 4)] + [f"unet.up{k}.conv" for k in (1, 2, 3, 4)]
STAGES = [(p, ci, bi) for p in PREFIXES for ci, bi in ((0, 1), (3, 4))]
TAP = [f"{p}.double_conv.{ci}" for p, ci, _ in STAGES]
HEAD = "unet.outc"
UP = [f"unet.up{k}.up" for k in (1, 2, 3, 4)]
SKIP_OF_CONCAT = {10: 7, 12: 5, 14: 3, 16: 1}   # concat stage -> stage whose output is the skip; the low-res input is i-1
POOL_OF = {2: 1, 4: 3, 6: 5, 8: 7}              # down stage -> stage whose output is max-pooled into it


# ---- bf16 rounding, restated from the host code -------------------------------------------------------------------------
def bf16_rne(x):
    """Round-to-nearest-even to bf16 (fp32 in, fp32 out; f32_to_bf16_rne without the NaN branch)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return (u.astype(np.uint32)).view(np.float32)


def bf16_split(x):
    """Two-piece bf16 form of fp32 values: (hi, lo) with hi = rne(x), lo = rne(x - hi)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


def bf16_feedback(w):
    """f32_to_bf16_feedback over the rows of `w` [filters, K] (fp32): each weight goes to the bf16 neighbour (toward or
    away from zero) that keeps the filter's running sum of rounding errors (float64) closest to zero, K in order."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    u = w.view(np.uint32)
    f0 = (u & np.uint32(0xFFFF0000)).view(np.float32)
    f1 = ((u & np.uint32(0xFFFF0000)) + np.uint32(0x10000)).view(np.float32)
    e0 = w.astype(np.float64) - f0
    e1 = w.astype(np.float64) - f1
    out = np.empty_like(w)
    carry = np.zeros(w.shape[0])
    for k in range(w.shape[1]):
        a, b = e0[:, k], e1[:, k]
        pick0 = (a == 0) | (np.abs(carry + a) <= np.abs(carry + b))
        out[:, k] = np.where(pick0, f0[:, k], f1[:, k])
        carry += np.where(pick0, a, b)
    return out


# ---- fp16 rounding, restated from the device code -------------------------------------------------------------------------
F16_MAX = 65504.0


def f16_rne_sat(x):
    """pack_f16x2 (csrc/conv3x3_mfma.hip.h), fp32 in, fp32 out: clamp to +-65504, then round to nearest even to IEEE
    half, subnormals kept (spacing 2^-24 below 2^-14).  `np.clip(x, -65504, 65504).astype(np.float16)` does exactly
    this: numpy's float32 -> float16 conversion rounds to nearest even and keeps subnormals, and after the clamp no
    value reaches the overflow threshold 65520."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return np.clip(x, np.float32(-F16_MAX), np.float32(F16_MAX)).astype(np.float16).astype(np.float32)


def fold_bn(sd, stage, exact=True):
    """(scale, shift) of a stage's BatchNorm: float64 from the statistics when `exact`, else the host's fp32
    arithmetic (inv = 1/sqrt(var + 1e-5f), scale = gamma * inv, shift = beta - mean * scale)."""
    p, _, bi = STAGES[stage]
    g, b, m, v = (sd[f"{p}.double_conv.{bi}.{k}"].double().numpy()
                  for k in ("weight", "bias", "running_mean", "running_var"))
    if exact:
        sc = g / np.sqrt(v + O.BN_EPS)
        return sc, b - m * sc
    f = np.float32
    inv = f(1.0) / np.sqrt(v.astype(f) + f(1e-5))
    sc = g.astype(f) * inv
    return sc.astype(np.float64), (b.astype(f) - m.astype(f) * sc).astype(np.float64)


def stage_weights(sd, stage, weights="exact", cache=None):
    """(W [Cout, Cin, 3, 3], shift [Cout]) float64 of a conv stage as the device's precision holds them.
    exact: W * scale and the shift in float64.  bf16_feedback / bf16_rne: the host's fp32 product W * scale rounded to
    bf16 per filter over (ci, tap) in OIHW order, and its fp32 shift (the stem keeps exact weights in every precision).
    fp16_rne: that fp32 product through f16_rne_sat, each weight on its own (f16_pack_weights_kernel bit for bit).
    cache: a dict the caller owns for one unchanging state dict (the feedback rounding walks every filter in order)."""
    key = (stage, weights)
    if cache is not None and key in cache:
        return cache[key]
    p, ci, _ = STAGES[stage]
    w = sd[f"{p}.double_conv.{ci}.weight"]
    if weights == "exact" or stage == 0:
        sc, sh = fold_bn(sd, stage, exact=True)
        res = (w.double().numpy() * sc[:, None, None, None], sh)
    else:
        sc, sh = fold_bn(sd, stage, exact=False)
        w32 = (w.numpy().astype(np.float32) * sc.astype(np.float32)[:, None, None, None]).reshape(w.shape[0], -1)
        wb = _ROUND_WEIGHTS[weights](w32)
        res = (wb.reshape(w.shape).astype(np.float64), sh)
    if cache is not None:
        cache[key] = res
    return res


_ROUND_WEIGHTS = {"bf16_feedback": bf16_feedback, "bf16_rne": bf16_rne, "fp16_rne": f16_rne_sat}


def convt_weights(sd, k, weights="exact"):
    """ConvTranspose2d of up{k} [Cin, Cout, 2, 2] and bias, float64; bf16 modes round per filter = (cout, tap) over ci,
    fp16_rne every weight on its own."""
    w = sd[f"unet.up{k}.up.weight"].numpy().astype(np.float32)
    b = sd[f"unet.up{k}.up.bias"].double().numpy()
    if weights == "exact":
        return w.astype(np.float64), b
    cin, cout = w.shape[:2]
    rows = w.transpose(1, 2, 3, 0).reshape(cout * 4, cin)       # filter (co, tap), K = ci
    rb = _ROUND_WEIGHTS[weights](rows)
    return rb.reshape(cout, 2, 2, cin).transpose(3, 0, 1, 2).astype(np.float64), b


def _t(x):
    return x if isinstance(x, torch.Tensor) and x.dtype == torch.float64 else torch.as_tensor(np.asarray(x)).double()


def _pad_to(up, skip):
    dy, dx = skip.shape[2] - up.shape[2], skip.shape[3] - up.shape[3]
    return F.pad(up, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])


def _bf16_uncertain(v, err):
    """bf16 rounding of float64 values a kernel forms with an absolute error of up to `err`: (rounded, slack), where slack
    is one bf16 ulp wherever the kernel's value may round to the other neighbour (within err of a rounding midpoint)."""
    a = v.numpy()
    r = bf16_rne(a.astype(np.float32)).astype(np.float64)
    ulp = np.ldexp(1.0, np.frexp(np.abs(a))[1] - 8)               # bf16 ulp in the binade of |v|
    to_mid = ulp / 2 - np.abs(a - r)                                 # distance to the nearest rounding midpoint
    slack = np.where(to_mid <= err.numpy() + np.abs(a) * 2.0 ** -22, ulp, 0.0)
    return torch.from_numpy(r), torch.from_numpy(slack)


def _f16_uncertain(v, err):
    """_bf16_uncertain for fp16 (f16_rne_sat): the ulp of the binade of |v| is 2^(e-11) for 2^(e-1) <= |v| < 2^e, and
    never below 2^-24, the subnormal spacing."""
    a = np.clip(v.numpy(), -F16_MAX, F16_MAX)
    r = f16_rne_sat(a.astype(np.float32)).astype(np.float64)
    ulp = np.ldexp(1.0, np.maximum(np.frexp(np.abs(a))[1] - 11, -24))
    to_mid = ulp / 2 - np.abs(a - r)
    slack = np.where(to_mid <= err.numpy() + np.abs(a) * 2.0 ** -22, ulp, 0.0)
    return torch.from_numpy(r), torch.from_numpy(slack)


def _up_axis(n):
    """Source indices and fp32 weights of a x2 align_corners axis as the kernels form them (conv3x3_mfma.hip.h up_axis):
    scale = fl((n - 1) / (2n - 1)), f = fl(scale * c), l = f - floor(f), h = 1 - l, all in fp32."""
    f32 = np.float32
    scale = f32(n - 1) / f32(2 * n - 1) if 2 * n > 1 else f32(0)
    f = (scale * np.arange(2 * n, dtype=f32)).astype(f32)
    g0 = f.astype(np.int64)
    g1 = np.where(g0 < n - 1, g0 + 1, g0)
    lo = (f - g0.astype(f32)).astype(f32)
    return g0, g1, (f32(1) - lo).astype(f32), lo


def _fma32(a, b, c):
    # fp32 fma: the float64 product of two fp32 numbers is exact; the sum is rounded twice (float64, then fp32), which
    # can differ from a single rounding only when it lands on an fp32 midpoint (covered by the bf16 band below)
    return (a.astype(np.float64) * b + c).astype(np.float32)


def upsample_fp32(x):
    """Bilinear x2 (align_corners=True) of fp32 values with the kernels' arithmetic (chunk_bilerp, x2_upsample_kernel):
    top = fma(lx, b, hx*a), bottom likewise, fma(ly, bottom, hy*top), on the fp32 coordinates of _up_axis."""
    a = x.numpy().astype(np.float32)
    y0, y1, hy, ly = _up_axis(a.shape[2])
    x0, x1, hx, lx = _up_axis(a.shape[3])
    rows = _fma32(lx, a[..., x1], (hx * a[..., x0]).astype(np.float32))
    top, bot = rows[:, :, y0], rows[:, :, y1]
    out = _fma32(ly[:, None], bot, (hy[:, None] * top).astype(np.float32))
    return torch.from_numpy(out.astype(np.float64))


def stage_input(sd, stage, inputs, weights="exact", stem="tap", cache=None):
    """(x, slack) float64 input of conv stage `stage` formed from the device's taps: max-pool, or upsample + F.pad +
    concat.  bf16 modes round the lerped upsample half to bf16 as the kernels do (slack marks values that may round the
    other way); stem="fused" forms inc.3's input as the fused bf16 stem does (split-bf16 evaluation of the stem, ~2^-16
    of its terms, then bf16) instead of reading tap 0.  Weight mode fp16_rne: the same two roundings to fp16."""
    bf16 = weights != "exact"
    uncertain = _f16_uncertain if weights == "fp16_rne" else _bf16_uncertain
    if stage == 0:
        x = torch.cat([_t(inputs["frame1"]), _t(inputs["frame2"])], 1)
        return x, torch.zeros_like(x)
    if stage == 1 and stem == "fused":
        y, m = stage_reference(sd, 0, inputs, "exact")
        return uncertain(y, m * 2.0 ** -14)
    if stage in POOL_OF:
        x = F.max_pool2d(_t(inputs[TAP[POOL_OF[stage]]]), 2)
        return x, torch.zeros_like(x)
    if stage in SKIP_OF_CONCAT:
        skip, low = _t(inputs[TAP[SKIP_OF_CONCAT[stage]]]), _t(inputs[TAP[stage - 1]])
        k = (stage - 10) // 2 + 1
        slack_up = None
        if UP[k - 1] in inputs:      # the upsampled half as given (read back padded, an emulation's copy, an oracle tap)
            up = _pad_to(_t(inputs[UP[k - 1]]), skip)
        elif f"unet.up{k}.up.weight" in sd:
            up = _pad_to(stage_reference(sd, UP[k - 1], inputs, weights, cache=cache)[0], skip)
        else:
            # the kernels' own fp32 lerp, restated (coordinates and association); bf16 then rounds it to bf16, and
            # only a value within one fp32 ulp of a bf16 rounding midpoint (the fma's double rounding here) is uncertain
            up = _pad_to(upsample_fp32(low), skip)
            if bf16:
                up, slack_up = uncertain(up, up.abs() * 2.0 ** -22)
        x = torch.cat([skip, up], 1)
        slack = torch.zeros_like(x)
        if slack_up is not None:
            slack[:, skip.shape[1]:] = slack_up
        return x, slack
    x = _t(inputs[TAP[stage - 1]])
    return x, torch.zeros_like(x)


@torch.no_grad()
def stage_reference(sd, stage, inputs, weights="exact", stem="tap", with_slack=False, cache=None):
    """float64 (y_ref, M) of one stage on the device's own inputs.

    stage: 0..17 (conv + BatchNorm + ReLU: y_ref = relu(conv(x, W*sc) + sh), M = conv(|x|, |W*sc|) + |sh|), "unet.outc"
    (the 1x1 head, no ReLU) or "unet.up{k}.up" (the ConvTranspose2d half of a bilinear=False decoder: before F.pad, as the
    reference's module returns it).  inputs: {"frame1", "frame2", tap name: tensor} - the read-back taps (NCHW) of the
    stages that feed this one.  weights: "exact", "bf16_feedback" (the default bf16 rounding), "bf16_rne" or "fp16_rne"
    (precision fp16, whose stores saturate: y_ref = min(relu(...), 65504), a ConvTranspose2d half clamped on both sides;
    the clamp is monotonic and 1-Lipschitz, so a bound on the unclamped value holds for the clamped one).
    with_slack: also return the bound's extra term for inputs the kernel rounds to bf16 / fp16 itself (lerped upsample
    half, fused stem), conv(slack, |W*sc|): one ulp of each input that may round the other way.
    cache: see stage_weights."""
    if stage == HEAD:
        x = _t(inputs[TAP[17]])
        w = sd["unet.outc.conv.weight"].double()
        b = sd["unet.outc.conv.bias"].double()
        y = F.conv2d(x, w, b)
        m = F.conv2d(x.abs(), w.abs(), b.abs())
        return (y, m, torch.zeros_like(y)) if with_slack else (y, m)
    if isinstance(stage, str):
        k = UP.index(stage) + 1
        x = _t(inputs[TAP[8 + 2 * (k - 1) + 1]])
        w, b = convt_weights(sd, k, weights)
        w, b = torch.from_numpy(w), torch.from_numpy(b)
        y = F.conv_transpose2d(x, w, b, stride=2)
        m = F.conv_transpose2d(x.abs(), w.abs(), b.abs(), stride=2)
        if weights == "fp16_rne":
            y = y.clamp(-F16_MAX, F16_MAX)
        return (y, m, torch.zeros_like(y)) if with_slack else (y, m)
    x, slack = stage_input(sd, stage, inputs, weights, stem, cache)
    w, sh = stage_weights(sd, stage, weights, cache)
    w, sh = torch.from_numpy(w), torch.from_numpy(sh)
    y = F.relu(F.conv2d(x, w, sh, padding=1))
    if weights == "fp16_rne":
        y = y.clamp(max=F16_MAX)
    m = F.conv2d(x.abs(), w.abs(), sh.abs(), padding=1)
    if not with_slack:
        return y, m
    e = F.conv2d(slack, w.abs(), padding=1) if slack.any() else torch.zeros_like(y)
    return y, m, e


# ---- the per-element bound of a stage ------------------------------------------------------------------------------------
def stage_family(stage):
    if stage == HEAD:
        return "head"
    if isinstance(stage, str):
        return "convt"
    return {0: "stem", 1: "inc.3"}.get(stage, "pool-fed" if stage in POOL_OF else
                                        "concat" if stage in SKIP_OF_CONCAT else "direct")


def stage_bound(prec, stage, y, m, e):
    """The largest |y_dev - y| a precision may show on one stage, per element (tests/test_gpu_bn_stats.py derives each
    term).  y, m, e: stage_reference(..., with_slack=True)."""
    if prec == "fp32":
        return 2.0 ** -16 * m
    if prec == "bf16x2":
        return 2.0 ** -14 * m + 2.0 ** -16 * y.abs()
    if prec == "bf16":
        return 2.0 ** -8 * m if stage == HEAD else 2.0 ** -8 * y.abs() + 2.0 ** -14 * m + e
    assert prec == "fp16", prec
    return 2.0 ** -11 * m if stage == HEAD else 2.0 ** -11 * y.abs() + 2.0 ** -25 + 2.0 ** -14 * m + e


def stage_error(sd, stage, acts, prec, weights, stem="tap", cache=None):
    """(y_dev, y_ref, M, error / bound, error / M) of one stage, float64: acts holds the stage's own read-back output
    under its tap name next to its inputs (a ConvTranspose2d half as F.pad leaves it)."""
    name = stage if isinstance(stage, str) else TAP[stage]
    y_dev = acts[name].double().cpu()
    y, m, e = stage_reference(sd, stage, acts, weights, stem, with_slack=True, cache=cache)
    if isinstance(stage, str) and stage != HEAD:
        skip = acts[TAP[SKIP_OF_CONCAT[10 + 2 * UP.index(stage)]]]
        y, m, e = (_pad_to(t, skip) for t in (y, m, e))
    assert y_dev.shape == y.shape, (name, y_dev.shape, y.shape)
    bound = stage_bound(prec, stage, y, m, e)
    err = (y_dev - y).abs()
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
    return y_dev, y, m, ratio, err / m.clamp_min(1e-300)


def check_stage(sd, stage, acts, prec, weights, stem="tap", label="", cache=None, report=None):
    """Assert the per-element bound of one stage; on failure report stage, channel, element, error/M, gamma and var.
    report: a dict that collects the worst error / bound and error / M per (precision, stage family)."""
    name = stage if isinstance(stage, str) else TAP[stage]
    y_dev, y, m, ratio, over_m = stage_error(sd, stage, acts, prec, weights, stem, cache)
    if report is not None:
        r = report.setdefault((prec, stage_family(stage)), {"max_err_over_bound": 0.0, "max_err_over_M": 0.0})
        r["max_err_over_bound"] = max(r["max_err_over_bound"], ratio.max().item())
        r["max_err_over_M"] = max(r["max_err_over_M"], over_m.max().item())
    if ratio.max().item() > 1.0:
        i = int(ratio.argmax())
        b, c, py, px = np.unravel_index(i, tuple(y.shape))
        extra = ""
        if isinstance(stage, int):
            p, _, bi = STAGES[stage]
            g = sd[f"{p}.double_conv.{bi}.weight"][c].item()
            var = sd[f"{p}.double_conv.{bi}.running_var"][c].item()
            extra = f" gamma {g:.4g} running_var {var:.4g}"
        bad = int((ratio > 1).sum())
        raise AssertionError(
            f"{label} {prec} stage {name}: {bad} element(s) over the bound; worst at (b={b}, c={c}, y={py}, x={px}): "
            f"device {y_dev.reshape(-1)[i].item():.9g} ref {y.reshape(-1)[i].item():.9g} err/M {over_m.reshape(-1)[i].item():.3e} "
            f"err/bound {ratio.max().item():.3g}{extra}")


# ---- whole-network emulation of a precision's storage points -------------------------------------------------------------
def stem_dither(h, w, amplitude=2.0 ** -8):
    """The bf16 stem's ordered input dither d(y, x) (conv3x3_mfma.hip.h stem_dither): +d on frame 1, -d on frame 2."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    a, b = (x ^ y) & 7, y & 7
    m = ((a & 1) << 5) | ((b & 1) << 4) | ((a & 2) << 2) | ((b & 2) << 1) | ((a & 4) >> 1) | ((b & 4) >> 2)
    d = ((m.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 64.0) - np.float32(0.5)) * np.float32(amplitude)
    return torch.from_numpy(d.astype(np.float32))


def _split(x):
    hi, lo = bf16_split(x.numpy().astype(np.float32))
    return torch.from_numpy(hi.astype(np.float64)), torch.from_numpy(lo.astype(np.float64))


def _x2_product(op, x, w, *args, **kw):
    """bf16x2's product of two-piece operands: wh*xh + wl*xh + wh*xl (the wl*xl term is dropped), float64 sums."""
    (xh, xl), (wh, wl) = (t.to(x.dtype) for t in _split(x)), (t.to(x.dtype) for t in _split(w))
    return op(xh, wh, *args, **kw) + op(xh, wl, *args, **kw) + op(xl, wh, *args, **kw)


def _store(x, precision):
    if precision == "bf16":
        return torch.from_numpy(bf16_rne(x.numpy().astype(np.float32)).astype(np.float64))
    if precision == "bf16x2":
        hi, lo = bf16_split(x.numpy().astype(np.float32))
        return torch.from_numpy(hi.astype(np.float64) + lo.astype(np.float64))
    if precision == "fp16":
        return torch.from_numpy(f16_rne_sat(x.numpy().astype(np.float32)).astype(np.float64))
    return x


@torch.no_grad()
def emulate_forward(sd, frame1, frame2, precision, dither=True, weights="bf16_feedback", dtype=torch.float64, keep=None):
    """The network in float64 with the activations rounded where `precision` stores them: "bf16" - bf16 weights
    (`weights`), the dithered frames into an fp32-grade stem, every conv output but the last (which feeds the fp32 head
    from registers) and every upsampled half rounded to bf16; "bf16x2" - the same points rounded to two bf16 pieces,
    and every conv's product formed from two-piece operands as the kernels form it (wh*xh + wl*xh + wh*xl); "fp16" -
    bf16's storage points rounded to fp16 (f16_rne_sat), "fp16_rne" weights whatever `weights` says, no dither.  The
    summation order is not the kernels', so this models the rounding, not the bits.  dtype: the arithmetic of the convs
    (float32 also models the kernels' fp32 accumulation, at a fraction of float64's cost).  keep: a dict that receives
    the frames as the stem saw them, every tap and every upsampled half as stored (what debug_activations reads back)."""
    wmode = weights if precision == "bf16" else "fp16_rne" if precision == "fp16" else "exact"
    f1, f2 = frame1.double(), frame2.double()
    if precision == "bf16" and dither:
        d = stem_dither(f1.shape[2], f1.shape[3]).double()
        f1, f2 = (frame1.float() + d.float()).double(), (frame2.float() - d.float()).double()
    taps = {"frame1": f1, "frame2": f2}
    cache = {}

    def conv(i):
        x, _ = stage_input(sd, i, taps, "exact")
        w, sh = stage_weights(sd, i, wmode, cache)
        x, w, sh = x.to(dtype), torch.from_numpy(w).to(dtype), torch.from_numpy(sh).to(dtype).view(1, -1, 1, 1)
        if precision == "bf16x2":
            y = F.relu(_x2_product(F.conv2d, x, w, padding=1) + sh)
        else:
            y = F.relu(F.conv2d(x, w, padding=1) + sh)
        y = y.double()
        taps[TAP[i]] = y if i == 17 else _store(y, precision)

    for i in range(18):
        if i in SKIP_OF_CONCAT:
            k = (i - 10) // 2 + 1
            skip, low = taps[TAP[SKIP_OF_CONCAT[i]]], taps[TAP[i - 1]]
            if f"unet.up{k}.up.weight" in sd:
                w, b = (torch.from_numpy(t).to(dtype) for t in convt_weights(sd, k, wmode))
                if precision == "bf16x2":
                    up = _x2_product(F.conv_transpose2d, low.to(dtype), w, stride=2) + b.view(1, -1, 1, 1)
                else:
                    up = F.conv_transpose2d(low.to(dtype), w, b, stride=2)
                up = up.double()
            else:
                up = upsample_fp32(low)
            taps[UP[k - 1]] = _store(_pad_to(up, skip), precision)
        conv(i)
    if keep is not None:
        keep.update(taps)
    return stage_reference(sd, HEAD, taps)[0]
