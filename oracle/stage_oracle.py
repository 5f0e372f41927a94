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


# ---- the same reference on a window of one image ---------------------------------------------------------------------------
def _crop(t, b, y0, y1, x0, x1):
    """float64 host copy of image b, rows [y0, y1), columns [x0, x1) of an NCHW tensor (cut where the tensor lives: a
    device tap is cropped on the device, and only the crop is copied)."""
    t = t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))
    return t[b:b + 1, :, y0:y1, x0:x1].double().cpu()


def _zero_extend(ts, region, clipped):
    """Tensors that cover `clipped` = (y0, y1, x0, x1), zero-padded out to `region` (which contains it)."""
    (ry0, ry1, rx0, rx1), (cy0, cy1, cx0, cx1) = region, clipped
    pad = [cx0 - rx0, rx1 - cx1, cy0 - ry0, ry1 - cy1]
    return tuple(F.pad(t, pad) if any(pad) else t for t in ts)


def _clip(region, h, w):
    y0, y1, x0, x1 = region
    y0, y1, x0, x1 = max(y0, 0), min(y1, h), max(x0, 0), min(x1, w)
    return y0, max(y1, y0), x0, max(x1, x0)


def _level_shape(inputs, stage):
    """(h, w) of conv stage `stage`'s level, from the shapes of the taps alone."""
    if stage in (0, 1) and "frame1" in inputs:
        return tuple(inputs["frame1"].shape[2:])
    if stage in POOL_OF:
        h, w = inputs[TAP[POOL_OF[stage]]].shape[2:]
        return h // 2, w // 2
    if stage in SKIP_OF_CONCAT:
        return tuple(inputs[TAP[SKIP_OF_CONCAT[stage]]].shape[2:])
    return tuple(inputs[TAP[stage - 1]].shape[2:])


def _up_window(low, b, n_rows, n_cols, clipped):
    """upsample_fp32 of image b of `low`, rows / columns `clipped` of the (2 n_rows) x (2 n_cols) result: the whole-image
    _up_axis indices and weights, and only the low-res rows and columns they name are cut out of the tap."""
    y0, y1, x0, x1 = clipped
    gy0, gy1, hy, ly = (a[y0:y1] for a in _up_axis(n_rows))
    gx0, gx1, hx, lx = (a[x0:x1] for a in _up_axis(n_cols))
    ry, rx = int(gy0.min()), int(gx0.min())
    a = _crop(low, b, ry, int(gy1.max()) + 1, rx, int(gx1.max()) + 1).numpy().astype(np.float32)
    rows = _fma32(lx, a[..., gx1 - rx], (hx * a[..., gx0 - rx]).astype(np.float32))
    top, bot = rows[:, :, gy0 - ry], rows[:, :, gy1 - ry]
    out = _fma32(ly[:, None], bot, (hy[:, None] * top).astype(np.float32))
    return torch.from_numpy(out.astype(np.float64))


def _convt_window(sd, k, inputs, b, region, weights):
    """(y, M) of the ConvTranspose2d half of up{k} on `region` of its F.pad-ded form (the level of the skip): zero in the
    F.pad band and outside the image, the 2x2 transposed conv of the low-res rows and columns it needs elsewhere."""
    low = inputs[TAP[8 + 2 * (k - 1) + 1]]
    hl, wl = low.shape[2:]
    hs, ws = inputs[TAP[SKIP_OF_CONCAT[10 + 2 * (k - 1)]]].shape[2:]
    py, px = (hs - 2 * hl) // 2, (ws - 2 * wl) // 2
    ry0, ry1, rx0, rx1 = region
    u = _clip((ry0 - py, ry1 - py, rx0 - px, rx1 - px), 2 * hl, 2 * wl)     # in the coordinates of the unpadded result
    cout = sd[f"unet.up{k}.up.weight"].shape[1]
    if u[1] == u[0] or u[3] == u[2]:
        z = torch.zeros(1, cout, ry1 - ry0, rx1 - rx0, dtype=torch.float64)
        return z, z.clone()
    ly0, lx0 = u[0] // 2, u[2] // 2
    x = _crop(low, b, ly0, (u[1] - 1) // 2 + 1, lx0, (u[3] - 1) // 2 + 1)
    w, bias = (torch.from_numpy(t) for t in convt_weights(sd, k, weights))
    sl = (..., slice(u[0] - 2 * ly0, u[1] - 2 * ly0), slice(u[2] - 2 * lx0, u[3] - 2 * lx0))
    y = F.conv_transpose2d(x, w, bias, stride=2)[sl]
    m = F.conv_transpose2d(x.abs(), w.abs(), bias.abs(), stride=2)[sl]
    if weights == "fp16_rne":
        y = y.clamp(-F16_MAX, F16_MAX)
    return _zero_extend((y, m), region, (u[0] + py, u[1] + py, u[2] + px, u[3] + px))


def stage_input_window(sd, stage, inputs, b, region, weights="exact", stem="tap", cache=None):
    """stage_input on `region` = (y0, y1, x0, x1) of image b at the stage's level; the region may reach past the image,
    where it reads zero (the conv's padding).  Only the crops the region needs are cut out of the taps."""
    bf16 = weights != "exact"
    uncertain = _f16_uncertain if weights == "fp16_rne" else _bf16_uncertain
    h, w = _level_shape(inputs, stage)
    c = _clip(region, h, w)
    slack = None
    if stage == 0:
        x = torch.cat([_crop(inputs["frame1"], b, *c), _crop(inputs["frame2"], b, *c)], 1)
    elif stage == 1 and stem == "fused":
        y, m, _ = stage_reference_window(sd, 0, inputs, (b,) + c, "exact")
        x, slack = uncertain(y, m * 2.0 ** -14)
    elif stage in POOL_OF:
        x = F.max_pool2d(_crop(inputs[TAP[POOL_OF[stage]]], b, 2 * c[0], 2 * c[1], 2 * c[2], 2 * c[3]), 2)
    elif stage in SKIP_OF_CONCAT:
        skip = _crop(inputs[TAP[SKIP_OF_CONCAT[stage]]], b, *c)
        k = (stage - 10) // 2 + 1
        if UP[k - 1] in inputs:
            up = _crop(inputs[UP[k - 1]], b, *c)
        elif f"unet.up{k}.up.weight" in sd:
            up = _convt_window(sd, k, inputs, b, c, weights)[0]
        else:
            low = inputs[TAP[stage - 1]]
            hl, wl = low.shape[2:]
            py, px = (h - 2 * hl) // 2, (w - 2 * wl) // 2             # F.pad in whole-image coordinates
            u = _clip((c[0] - py, c[1] - py, c[2] - px, c[3] - px), 2 * hl, 2 * wl)
            if u[1] > u[0] and u[3] > u[2]:
                up = _up_window(low, b, hl, wl, u)
            else:
                up = torch.zeros(1, low.shape[1], u[1] - u[0], u[3] - u[2], dtype=torch.float64)
            (up,) = _zero_extend((up,), c, (u[0] + py, u[1] + py, u[2] + px, u[3] + px))
            if bf16:
                up, slack_up = uncertain(up, up.abs() * 2.0 ** -22)
                slack = torch.cat([torch.zeros_like(skip), slack_up], 1)
        x = torch.cat([skip, up], 1)
    else:
        x = _crop(inputs[TAP[stage - 1]], b, *c)
    if slack is None:
        slack = torch.zeros_like(x)
    return _zero_extend((x, slack), region, c)


@torch.no_grad()
def stage_reference_window(sd, stage, inputs, window, weights="exact", stem="tap", with_slack=True, cache=None):
    """(y_ref, M, E) of stage_reference on the output window (b, y0, y1, x0, x1) of ONE image: rows [y0, y1) and columns
    [x0, x1) at the stage's level, each [1, Cout, y1 - y0, x1 - x0].  No whole-tensor float64 input is formed: the taps in
    `inputs` (host or device tensors, whole) are cut to the window plus its 1-pixel conv halo - the 2x region of the
    producer for a pool-fed stage; the skip crop and the upsampled half of the crop alone for a concat stage (whole-image
    lerp indices and fp32 weights, F.pad in whole-image coordinates, the bf16 / fp16 rounding with its slack band); one
    more halo pixel of the frames for the fused stem - and the halo is zero only where it leaves the image.  A
    ConvTranspose2d half ("unet.up{k}.up") takes its window in the coordinates of the read-back tap, i.e. as F.pad leaves
    it at the level of the skip.  with_slack=False returns (y_ref, M)."""
    b, y0, y1, x0, x1 = window
    if stage == HEAD:
        x = _crop(inputs[TAP[17]], b, y0, y1, x0, x1)
        w = sd["unet.outc.conv.weight"].double()
        bias = sd["unet.outc.conv.bias"].double()
        y = F.conv2d(x, w, bias)
        m = F.conv2d(x.abs(), w.abs(), bias.abs())
        return (y, m, torch.zeros_like(y)) if with_slack else (y, m)
    if isinstance(stage, str):
        y, m = _convt_window(sd, UP.index(stage) + 1, inputs, b, (y0, y1, x0, x1), weights)
        return (y, m, torch.zeros_like(y)) if with_slack else (y, m)
    x, slack = stage_input_window(sd, stage, inputs, b, (y0 - 1, y1 + 1, x0 - 1, x1 + 1), weights, stem, cache)
    w, sh = stage_weights(sd, stage, weights, cache)
    w, sh = torch.from_numpy(w), torch.from_numpy(sh)
    y = F.relu(F.conv2d(x, w, sh))
    if weights == "fp16_rne":
        y = y.clamp(max=F16_MAX)
    m = F.conv2d(x.abs(), w.abs(), sh.abs())
    if not with_slack:
        return y, m
    e = F.conv2d(slack, w.abs()) if slack.any() else torch.zeros_like(y)
    return y, m, e


def tile_window(ty, tx, th, tw, h, w, ring=2):
    """(y0, y1, x0, x1) of tile (ty, tx) of a TH x TW grid over h x w with a `ring`-pixel band of its neighbours, cut to
    the image: every in-tile position and all four seams of the tile lie inside."""
    return _clip((ty * th - ring, (ty + 1) * th + ring, tx * tw - ring, (tx + 1) * tw + ring), h, w)


def check_stage_windows(sd, stage, acts, windows, prec, weights, stem="tap", label="", cache=None, report=None,
                        tile=None, family=None):
    """check_stage on windows: the unchanged stage_bound per element of every window (b, y0, y1, x0, x1) of the stage's
    own read-back output `acts[name]` (whole, on the host or the device; only the windows are copied), against
    stage_reference_window on the taps in `acts`.  tile: (TH, TW) of the stage's launch, for the failure's position inside
    its tile.  report / family: as check_stage, under (precision, family or stage_family(stage))."""
    name = stage if isinstance(stage, str) else TAP[stage]
    worst = (0.0, None)
    n_bad = 0
    for win in windows:
        b, y0, y1, x0, x1 = win
        y_dev = _crop(acts[name], b, y0, y1, x0, x1)
        y, m, e = stage_reference_window(sd, stage, acts, win, weights, stem, True, cache)
        assert y_dev.shape == y.shape, (name, win, y_dev.shape, y.shape)
        bound = stage_bound(prec, stage, y, m, e)
        err = (y_dev - y).abs()
        ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.inf, 0.0))
        over_m = err / m.clamp_min(1e-300)
        if report is not None:
            r = report.setdefault((prec, family or stage_family(stage)), {"max_err_over_bound": 0.0, "max_err_over_M": 0.0})
            r["max_err_over_bound"] = max(r["max_err_over_bound"], ratio.max().item())
            r["max_err_over_M"] = max(r["max_err_over_M"], over_m.max().item())
        n_bad += int((ratio > 1).sum())
        if ratio.max().item() > max(worst[0], 1.0):
            i = int(ratio.argmax())
            worst = (ratio.max().item(), (win, i, y_dev.reshape(-1)[i].item(), y.reshape(-1)[i].item(),
                                          over_m.reshape(-1)[i].item(), tuple(y.shape)))
    if worst[1] is not None:
        win, i, dv, rv, om, shape = worst[1]
        _, c, wy, wx = np.unravel_index(i, shape)
        py, px = win[1] + int(wy), win[3] + int(wx)
        extra = ""
        if isinstance(stage, int):
            p, _, bi = STAGES[stage]
            g = sd[f"{p}.double_conv.{bi}.weight"][c].item()
            var = sd[f"{p}.double_conv.{bi}.running_var"][c].item()
            extra = f" gamma {g:.4g} running_var {var:.4g}"
        where = f" in-tile (y%{tile[0]}={py % tile[0]}, x%{tile[1]}={px % tile[1]})" if tile else ""
        raise AssertionError(
            f"{label} {prec} stage {name}: {n_bad} element(s) over the bound; worst at (b={win[0]}, c={c}, y={py}, x={px}): "
            f"device {dv:.9g} ref {rv:.9g} err/M {om:.3e} err/bound {worst[0]:.3g}{extra}; window "
            f"rows {win[1]}:{win[2]} cols {win[3]}:{win[4]}{where}")


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
