"""The yardstick of the flow tests (tests/test_flow_host.py, test_gpu_flow.py, test_gpu_flow_holdout.py): the restatement
`optical_flow.py` evaluated in FLOAT64, the test inputs, and the bound rule.

  yardstick  `flow64` re-runs `calc_optical_flow_farneback`'s level loop on float64 tensors.  The module's functions
             follow the dtype of what they are given; the one exception is `poly_exp`, whose weights come out of
             `_poly_exp_setup` as fp32 tensors: `poly_exp64` casts exactly those to float64, so both precisions weigh
             with the same numbers.  `warp64` builds the sampling maps from a float64 flow in float64 and samples with
             the module's fixed-point rule.
  inputs     smooth translated textures: seeded uniform noise [h/4 + 8 (+ margin), w/4 + 8 (+ margin)], bicubic x4
             (align_corners=False), normalised to [0, 1]; frame i is the crop at (oy - i dy, ox - i dx), quantised as
             round(peak x).  The content of frame i + 1 is that of frame i moved by (dy, dx): the flow is (dx, dy).
  bound      a kernel and the fp32 torch evaluation of the same stage are two fp32 evaluations of the same sums in
             different orders.  The kernel gets 8x the fp32 torch stage's own distance to float64 on the maximum and 3x
             on the mean (`assert_within`): the margin covers the spread of a maximum over 10^3 .. 10^5 elements.
"""
import torch
import torch.nn.functional as F

from ai_based_frame_interpolation_amd import optical_flow as OF

MAX_FACTOR, MEAN_FACTOR = 8.0, 3.0
#: (h, w, (dy, dx), pyramid levels above level 0)
CASES = [(40, 56, (1, 2), 0), (72, 100, (1, 2), 1), (135, 240, (2, 3), 2), (256, 272, (2, 3), 3), (132, 130, (1, 2), 2)]


def texture_clip(h, w, dy, dx, frames=2, seed=1, peak=255):
    """-> uint8 (peak 255) or int16 (peak 1023) [frames, h, w]"""
    g = torch.Generator().manual_seed(seed)
    my, mx = max(0, (frames - 1) * dy - 8), max(0, (frames - 1) * dx - 8)   # (two frames: the plain [h/4+8, w/4+8])
    n = torch.rand(h // 4 + 8 + (my + 3) // 4, w // 4 + 8 + (mx + 3) // 4, generator=g)
    up = F.interpolate(n[None, None], scale_factor=4, mode="bicubic", align_corners=False)[0, 0]
    up = (up - up.min()) / (up.max() - up.min())
    oy, ox = 8 + my, 8 + mx
    out = torch.stack([up[oy - i * dy:oy - i * dy + h, ox - i * dx:ox - i * dx + w] for i in range(frames)])
    assert out.shape == (frames, h, w)
    q = torch.round(out * peak)
    return q.to(torch.uint8) if peak == 255 else q.to(torch.int16)


def texture_pair(h, w, dy, dx, seed=1, peak=255):
    a, b = texture_clip(h, w, dy, dx, 2, seed, peak)
    return a, b


def as_float(frame, bits, dtype):
    """A frame as the flow takes it: 8-bit codes, 10-bit codes / 4."""
    return frame.to(dtype) if bits == 8 else OF._codes(frame, 10).to(dtype) / 4.0


def poly_exp64(img):
    g, xg, xxg, ig11, ig03, ig33, ig55 = OF._poly_exp_setup(5, 1.1, img.device)
    g, xg, xxg = g.double(), xg.double(), xxg.double()
    r0, r1, r2 = OF._conv_rows(img, g), OF._conv_rows(img, xg), OF._conv_rows(img, xxg)
    b1, b2, b4 = OF._conv_cols(r0, g), OF._conv_cols(r0, xg), OF._conv_cols(r0, xxg)
    b3, b6, b5 = OF._conv_cols(r1, g), OF._conv_cols(r1, xg), OF._conv_cols(r2, g)
    return torch.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55], dim=-1)


def levels_of(H, W, pyr_scale=0.5, levels=3, min_size=32):
    """The Python loop's pyramid -> [(h, w, ksize, sigma)] for level 0 .. levels."""
    k, scale = 0, 1.0
    while k < levels:
        scale *= pyr_scale
        if W * scale < min_size or H * scale < min_size:
            break
        k += 1
    out = []
    for lv in range(k + 1):
        scale = pyr_scale ** lv
        sigma = (1.0 / scale - 1.0) * 0.5
        out.append((int(round(H * scale)), int(round(W * scale)), max(int(round(sigma * 5)) | 1, 3), sigma))
    return out


def pyramid_level(img, level):
    """Level `level` of a float [H, W] image in its own dtype: blur of the full-resolution image, then resize."""
    h, w, ksize, sigma = levels_of(*img.shape)[level]
    return OF._resize_linear(OF._gaussian_blur(img, ksize, sigma), w, h)


@torch.no_grad()
def flow64(prev, nxt, bits=8):
    """`calc_optical_flow_farneback` on float64 tensors -> float64 [H, W, 2]."""
    imgs = [as_float(prev, bits, torch.float64), as_float(nxt, bits, torch.float64)]
    lv = levels_of(*prev.shape)
    flow = None
    for k in range(len(lv) - 1, -1, -1):
        h, w, _, _ = lv[k]
        flow = (torch.zeros(h, w, 2, dtype=torch.float64) if flow is None else OF._resize_linear(flow, w, h) * 2.0)
        R = [poly_exp64(pyramid_level(img, k)) for img in imgs]
        M = OF.update_matrices(R[0], R[1], flow)
        for i in range(3):
            flow, M = OF.update_flow_blur(R[0], R[1], flow, M, 15, i < 2)
    return flow


@torch.no_grad()
def warp64(f0, f1, flow, mode, bits=8):
    """Both modes from a float64 [H, W, 2] flow, maps in float64 -> int64 [H, W]."""
    h, w = f0.shape
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    hx, hy = flow[..., 0] * 0.5, flow[..., 1] * 0.5
    fwd = OF._remap_bilinear(OF._codes(f0 if mode == "reference" else f1, bits), (xs + hx).clamp(0, w - 1),
                             (ys + hy).clamp(0, h - 1))
    if mode == "reference":
        return fwd
    back = OF._remap_bilinear(OF._codes(f0, bits), (xs - hx).clamp(0, w - 1), (ys - hy).clamp(0, h - 1))
    return (back + fwd + 1) >> 1


def dist(x, ref):
    """-> (max, mean) of |x - ref| in float64"""
    d = (x.double().cpu() - ref.double().cpu()).abs()
    return float(d.max()), float(d.mean())


def assert_within(name, kernel, torch32, ref64):
    """The bound rule; prints every figure before it asserts.  -> (max ratio, mean ratio) (nan where torch is exact)."""
    kmax, kmean = dist(kernel, ref64)
    tmax, tmean = dist(torch32, ref64)
    rmax = kmax / tmax if tmax else float("nan")
    rmean = kmean / tmean if tmean else float("nan")
    print(f"{name}: kernel max {kmax:.3e} mean {kmean:.3e} | fp32 torch max {tmax:.3e} mean {tmean:.3e} | "
          f"ratios {rmax:.2f} {rmean:.2f}")
    assert kmax <= MAX_FACTOR * tmax, (name, kmax, tmax)
    assert kmean <= MEAN_FACTOR * tmean, (name, kmean, tmean)
    return rmax, rmean


def pixel_gap(a, b):
    """-> (share of differing pixels, largest difference in codes)"""
    d = (a.long().cpu() - b.long().cpu()).abs()
    return float((d != 0).double().mean()), int(d.max())
