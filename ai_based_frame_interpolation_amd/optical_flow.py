"""The reference evaluators' third method, the optical-flow baseline (model/evaluation_simple.py:76-103,
model/evaluation.py:134-192), WITHOUT OpenCV.

The reference calls `cv2.calcOpticalFlowFarneback(f0, f1, None, pyr_scale=0.5, levels=3, winsize=15,
iterations=3, poly_n=5, poly_sigma=1.1, flags=0)`, halves the flow and samples frame 0 at (x, y) + flow / 2
with `cv2.remap(..., INTER_LINEAR, BORDER_REPLICATE)`.  OpenCV is a third-party dependency of the reference
(`requirements.txt`, unpinned) that no image this code has run on contains, and the reference holds no flow
or frame fixtures, so this module RESTATES the published algorithm - G. Farneback, "Two-Frame Motion Estimation
Based on Polynomial Expansion" (SCIA 2003), in the form OpenCV's `optflowgf.cpp` implements it: Gaussian
pyramid, per-level polynomial expansion (separable Gaussian-weighted least squares), iterative displacement
update over a box-filtered normal-equation field, border attenuation - and remap's 5-bit fixed-point bilinear
sampling.  **Parity unpinned**: nothing here has been compared with OpenCV's output; what the tests pin is the
behaviour the algorithm must have (a translated texture yields that translation; remap with zero flow is the
identity) and the reference's own quirk, which is kept: it samples frame 0 at grid + flow / 2, i.e. AGAINST the
motion, so on translating content this baseline scores BELOW the linear blend (evaluation.py's docstring and
tests/test_host.py::test_optical_flow_baseline_is_the_references_formula).  When `cv2` IS importable the evaluator calls
OpenCV itself (evaluation.py) and this module is not used.

The functions of the restatement are plain torch on whatever device the frames are on, one pair at a time (the
reference runs it frame by frame on the CPU).  They are the DEFINITION.  The batched entry points at the end of the
file - `farneback_flow`, `warp`, `interpolate` - run the same definition in HIP kernels (csrc/flow.hip.h, DESIGN.md
3.3n: backend "hip") or loop the restatement (backend "torch"); hold-out scoring (holdout.py) and
`evaluation.evaluate_triplets(flow_backend="hip")` use them.  Beside the reference's formula (mode "reference") they
have the symmetric warp a motion-compensated baseline needs (mode "motion": frame 0 at p - flow / 2 averaged with
frame 1 at p + flow / 2).
"""
from __future__ import annotations

import ctypes
import math
from typing import Tuple

import torch
import torch.nn.functional as F

_BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)   # attenuation of the 5 outermost rows / columns


def _gauss_kernel_cv(ksize: int, sigma: float, dtype, device) -> torch.Tensor:
    """cv2.getGaussianKernel: fixed small kernels for sigma <= 0 and ksize <= 7, else exp(-x^2 / 2 sigma^2)
    normalised to 1 (sigma <= 0: 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8)."""
    small = {1: [1.0], 3: [0.25, 0.5, 0.25], 5: [0.0625, 0.25, 0.375, 0.25, 0.0625],
             7: [0.03125, 0.109375, 0.21875, 0.28125, 0.21875, 0.109375, 0.03125]}
    if sigma <= 0 and ksize in small:
        return torch.tensor(small[ksize], dtype=dtype, device=device)
    if sigma <= 0:
        sigma = 0.3 * ((ksize - 1) * 0.5 - 1) + 0.8
    x = torch.arange(ksize, dtype=torch.float64, device=device) - (ksize - 1) * 0.5
    k = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    return (k / k.sum()).to(dtype)


def _gaussian_blur(img: torch.Tensor, ksize: int, sigma: float) -> torch.Tensor:
    """cv2.GaussianBlur(img, (ksize, ksize), sigma) on an [H, W] float image, BORDER_REFLECT_101."""
    k = _gauss_kernel_cv(ksize, sigma, img.dtype, img.device)
    r = ksize // 2
    x = img[None, None]
    if r > 0:
        # reflect-101 needs the image to be larger than the radius; tiny pyramid levels fall back to replicate
        mode = "reflect" if min(img.shape) > r else "replicate"
        x = F.pad(x, (r, r, r, r), mode=mode)
    x = F.conv2d(x, k.view(1, 1, 1, -1))
    x = F.conv2d(x, k.view(1, 1, -1, 1))
    return x[0, 0]


def _resize_linear(img: torch.Tensor, width: int, height: int) -> torch.Tensor:
    """cv2.resize(img, (width, height), interpolation=INTER_LINEAR) for float images (any trailing channel
    dim): source coordinate (dst + 0.5) * scale - 0.5, indices clamped to the image."""
    h, w = img.shape[0], img.shape[1]
    if (h, w) == (height, width):
        return img.clone()

    def axis(n_dst, n_src):
        scale = n_src / n_dst
        f = (torch.arange(n_dst, dtype=torch.float64, device=img.device) + 0.5) * scale - 0.5
        i0 = torch.floor(f)
        t = (f - i0).to(img.dtype)
        i0 = i0.long()
        # OpenCV: below 0 -> index 0 with weight 0; past the end -> last index with weight 0
        t = torch.where(i0 < 0, torch.zeros_like(t), t)
        t = torch.where(i0 >= n_src - 1, torch.zeros_like(t), t)
        i0c = i0.clamp(0, n_src - 1)
        i1c = (i0 + 1).clamp(0, n_src - 1)
        return i0c, i1c, t

    y0, y1, ty = axis(height, h)
    x0, x1, tx = axis(width, w)
    shape_y = (-1, 1) + (1,) * (img.dim() - 2)
    shape_x = (1, -1) + (1,) * (img.dim() - 2)
    ty, tx = ty.view(shape_y), tx.view(shape_x)
    top = img[y0][:, x0] * (1 - tx) + img[y0][:, x1] * tx
    bot = img[y1][:, x0] * (1 - tx) + img[y1][:, x1] * tx
    return top * (1 - ty) + bot * ty


def _poly_exp_setup(n: int, sigma: float, device):
    """FarnebackPrepareGaussian: the 1-D weights g, x g, x^2 g and the four entries of the inverse of the
    6x6 Gram matrix of the basis {1, x, y, x^2, y^2, xy} under the weight g(x) g(y)."""
    x = torch.arange(-n, n + 1, dtype=torch.float64)
    g = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    g = g / g.sum()
    xg, xxg = x * g, x * x * g
    gy, gx = torch.meshgrid(g, g, indexing="ij")
    yy, xx = torch.meshgrid(x, x, indexing="ij")
    wgt = gy * gx
    basis = [torch.ones_like(xx), xx, yy, xx * xx, yy * yy, xx * yy]
    G = torch.tensor([[float((wgt * a * b).sum()) for b in basis] for a in basis], dtype=torch.float64)
    invG = torch.linalg.inv(G)
    ig11, ig03, ig33, ig55 = float(invG[1, 1]), float(invG[0, 3]), float(invG[3, 3]), float(invG[5, 5])
    f32 = lambda t: t.to(torch.float32).to(device)
    return f32(g), f32(xg), f32(xxg), ig11, ig03, ig33, ig55


def _conv_rows(img: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    """correlation along y with replicated borders: out[y] = sum_j k[j] img[y + j - n]"""
    n = k.numel() // 2
    x = F.pad(img[None, None], (0, 0, n, n), mode="replicate")
    return F.conv2d(x, k.view(1, 1, -1, 1))[0, 0]


def _conv_cols(img: torch.Tensor, k: torch.Tensor) -> torch.Tensor:
    n = k.numel() // 2
    x = F.pad(img[None, None], (n, n, 0, 0), mode="replicate")
    return F.conv2d(x, k.view(1, 1, 1, -1))[0, 0]


def poly_exp(img: torch.Tensor, n: int = 5, sigma: float = 1.1) -> torch.Tensor:
    """FarnebackPolyExp: local quadratic model f(d) ~ d^T A d + b^T d + c of every pixel's neighbourhood
    (Gaussian-weighted least squares, radius n).  Returns [H, W, 5] = (b_y-like r2, b_x-like r3, A_yy r4,
    A_xx r5, A_xy r6) in OpenCV's channel order: (b3 ig11, b2 ig11, b1 ig03 + b5 ig33, b1 ig03 + b4 ig33,
    b6 ig55)."""
    g, xg, xxg, ig11, ig03, ig33, ig55 = _poly_exp_setup(n, sigma, img.device)
    # vertical pass: r0 = g * f, r1 = (y g) * f, r2 = (y^2 g) * f
    r0, r1, r2 = _conv_rows(img, g), _conv_rows(img, xg), _conv_rows(img, xxg)
    # horizontal pass
    b1 = _conv_cols(r0, g)
    b2 = _conv_cols(r0, xg)      # x moment
    b4 = _conv_cols(r0, xxg)     # x^2 moment
    b3 = _conv_cols(r1, g)       # y moment
    b6 = _conv_cols(r1, xg)      # xy moment
    b5 = _conv_cols(r2, g)       # y^2 moment
    return torch.stack([b3 * ig11, b2 * ig11, b1 * ig03 + b5 * ig33, b1 * ig03 + b4 * ig33, b6 * ig55], dim=-1)


def _border_scale(height: int, width: int, device) -> torch.Tensor:
    nb = len(_BORDER)
    sy = torch.ones(height, device=device)
    sx = torch.ones(width, device=device)
    b = torch.tensor(_BORDER, device=device)
    ky, kx = min(nb, height), min(nb, width)
    sy[:ky] *= b[:ky]
    sy[height - ky:] *= b[:ky].flip(0)
    sx[:kx] *= b[:kx]
    sx[width - kx:] *= b[:kx].flip(0)
    return sy[:, None] * sx[None, :]


def update_matrices(R0: torch.Tensor, R1: torch.Tensor, flow: torch.Tensor) -> torch.Tensor:
    """FarnebackUpdateMatrices: R1 sampled (bilinearly) at the displaced position, averaged with R0, and the
    per-pixel normal equations [G11, G12, G22, h1, h2] of the displacement update.  flow[..., 0] = dx, [..., 1] = dy."""
    h, w = flow.shape[0], flow.shape[1]
    ys, xs = torch.meshgrid(torch.arange(h, device=flow.device, dtype=flow.dtype),
                            torch.arange(w, device=flow.device, dtype=flow.dtype), indexing="ij")
    dx, dy = flow[..., 0], flow[..., 1]
    fx, fy = xs + dx, ys + dy
    x1, y1 = torch.floor(fx), torch.floor(fy)
    ax, ay = (fx - x1)[..., None], (fy - y1)[..., None]
    x1, y1 = x1.long(), y1.long()
    inside = (x1 >= 0) & (x1 < w - 1) & (y1 >= 0) & (y1 < h - 1)
    xc, yc = x1.clamp(0, w - 2), y1.clamp(0, h - 2)
    s = (R1[yc, xc] * (1 - ax) * (1 - ay) + R1[yc, xc + 1] * ax * (1 - ay) +
         R1[yc + 1, xc] * (1 - ax) * ay + R1[yc + 1, xc + 1] * ax * ay)
    ins = inside[..., None]
    r2 = torch.where(inside, s[..., 0], torch.zeros_like(dx))
    r3 = torch.where(inside, s[..., 1], torch.zeros_like(dx))
    r4 = torch.where(inside, (R0[..., 2] + s[..., 2]) * 0.5, R0[..., 2])
    r5 = torch.where(inside, (R0[..., 3] + s[..., 3]) * 0.5, R0[..., 3])
    r6 = torch.where(inside, (R0[..., 4] + s[..., 4]) * 0.25, R0[..., 4] * 0.5)
    del ins
    r2 = (R0[..., 0] - r2) * 0.5
    r3 = (R0[..., 1] - r3) * 0.5
    r2 = r2 + r4 * dy + r6 * dx
    r3 = r3 + r6 * dy + r5 * dx
    sc = _border_scale(h, w, flow.device).to(flow.dtype)
    r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
    return torch.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3], dim=-1)


def _box_mean(M: torch.Tensor, size: int) -> torch.Tensor:
    """mean over a size x size window, replicated borders, on [H, W, C]"""
    m = size // 2
    x = M.permute(2, 0, 1)[None]
    x = F.pad(x, (m, m, m, m), mode="replicate")
    x = F.avg_pool2d(x, kernel_size=size, stride=1)
    return x[0].permute(1, 2, 0)


def update_flow_blur(R0, R1, flow, M, block_size: int, update_mats: bool):
    """FarnebackUpdateFlow_Blur: box-filter the normal equations, solve the 2x2 system per pixel."""
    S = _box_mean(M, block_size)
    g11, g12, g22, h1, h2 = S[..., 0], S[..., 1], S[..., 2], S[..., 3], S[..., 4]
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    new = torch.stack([(g11 * h2 - g12 * h1) * idet, (g22 * h1 - g12 * h2) * idet], dim=-1)
    if update_mats:
        M = update_matrices(R0, R1, new)
    return new, M


@torch.no_grad()
def calc_optical_flow_farneback(prev_u8: torch.Tensor, next_u8: torch.Tensor, pyr_scale: float = 0.5,
                                levels: int = 3, winsize: int = 15, iterations: int = 3, poly_n: int = 5,
                                poly_sigma: float = 1.1) -> torch.Tensor:
    """Dense flow prev -> next of two [H, W] uint8 (or float) frames, [H, W, 2] = (dx, dy) float32; the
    argument meaning of cv2.calcOpticalFlowFarneback with flags = 0 (box window, no initial flow)."""
    if prev_u8.shape != next_u8.shape or prev_u8.dim() != 2:
        raise ValueError("expected two [H, W] frames of equal shape")
    imgs = [prev_u8.to(torch.float32), next_u8.to(torch.float32)]
    H, W = prev_u8.shape
    min_size = 32
    k, scale = 0, 1.0
    while k < levels:
        scale *= pyr_scale
        if W * scale < min_size or H * scale < min_size:
            break
        k += 1
    levels = k
    flow = None
    for k in range(levels, -1, -1):
        scale = pyr_scale ** k
        sigma = (1.0 / scale - 1.0) * 0.5
        smooth = max(int(round(sigma * 5)) | 1, 3)
        w, h = int(round(W * scale)), int(round(H * scale))
        if flow is None:
            flow = torch.zeros(h, w, 2, dtype=torch.float32, device=prev_u8.device)
        else:
            flow = _resize_linear(flow, w, h) * (1.0 / pyr_scale)
        R = []
        for img in imgs:
            blurred = _gaussian_blur(img, smooth, sigma)
            R.append(poly_exp(_resize_linear(blurred, w, h), poly_n, poly_sigma))
        M = update_matrices(R[0], R[1], flow)
        for i in range(iterations):
            flow, M = update_flow_blur(R[0], R[1], flow, M, winsize, i < iterations - 1)
    return flow


_INTER_BITS, _REMAP_COEF_BITS = 5, 15


def _remap_bilinear(src: torch.Tensor, map_x: torch.Tensor, map_y: torch.Tensor) -> torch.Tensor:
    """remap's fixed-point bilinear sampling of an [H, W] integer image -> int64 [H, W] (samples of any depth)."""
    h, w = src.shape
    tab = 1 << _INTER_BITS
    sx = torch.round(map_x.to(torch.float64) * tab).long()
    sy = torch.round(map_y.to(torch.float64) * tab).long()
    x0, y0 = sx >> _INTER_BITS, sy >> _INTER_BITS
    fx, fy = (sx & (tab - 1)).to(torch.float64) / tab, (sy & (tab - 1)).to(torch.float64) / tab
    one = float(1 << _REMAP_COEF_BITS)
    # OpenCV builds the table in float and rounds every weight to an integer (the four weights of a cell
    # are then corrected to sum to 2^15 exactly; the correction goes to the largest weight)
    wts = torch.stack([(1 - fx) * (1 - fy), fx * (1 - fy), (1 - fx) * fy, fx * fy], dim=-1) * one
    iw = torch.round(wts).long()
    diff = (1 << _REMAP_COEF_BITS) - iw.sum(-1)
    big = iw.argmax(-1, keepdim=True)
    iw.scatter_add_(-1, big, diff[..., None])
    xa, xb = x0.clamp(0, w - 1), (x0 + 1).clamp(0, w - 1)
    ya, yb = y0.clamp(0, h - 1), (y0 + 1).clamp(0, h - 1)
    s = src.long()
    acc = s[ya, xa] * iw[..., 0] + s[ya, xb] * iw[..., 1] + s[yb, xa] * iw[..., 2] + s[yb, xb] * iw[..., 3]
    return (acc + (1 << (_REMAP_COEF_BITS - 1))) >> _REMAP_COEF_BITS


@torch.no_grad()
def remap_bilinear_u8(src_u8: torch.Tensor, map_x: torch.Tensor, map_y: torch.Tensor) -> torch.Tensor:
    """cv2.remap(src, map_x, map_y, INTER_LINEAR, borderMode=BORDER_REPLICATE) on an [H, W] uint8 image:
    coordinates rounded to 1/32 pixel, integer weights of 15 bits, result (sum + 2^14) >> 15."""
    return _remap_bilinear(src_u8, map_x, map_y).clamp(0, 255).to(torch.uint8)


@torch.no_grad()
def optical_flow_interpolation_baseline(frame0_u8: torch.Tensor, frame1_u8: torch.Tensor) -> torch.Tensor:
    """evaluation_simple.py:76-103 on two [H, W] uint8 frames: Farneback flow 0 -> 1 with the reference's
    parameters, frame 0 sampled at (x, y) + flow / 2 clipped to the image, bilinear, replicated border."""
    flow = calc_optical_flow_farneback(frame0_u8, frame1_u8, pyr_scale=0.5, levels=3, winsize=15, iterations=3,
                                       poly_n=5, poly_sigma=1.1)
    h, w = frame0_u8.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=flow.device, dtype=torch.float32),
                            torch.arange(w, device=flow.device, dtype=torch.float32), indexing="ij")
    new_x = (xs + flow[..., 0] * 0.5).clamp(0, w - 1)
    new_y = (ys + flow[..., 1] * 0.5).clamp(0, h - 1)
    return remap_bilinear_u8(frame0_u8, new_x, new_y)


# ---- batched entry points: the HIP kernels (csrc/flow.hip.h), or the restatement in a loop -----------------------------
BACKENDS = ("hip", "torch")
MODES = ("reference", "motion")
# (device, H, W) -> the flow workspace, one torch buffer per frame size, sized for the largest batch seen (a smaller
# batch uses its front; a larger one replaces it).  Calls of one size are assumed to be on ONE stream at a time: the
# buffer is scratch of the call in flight and nothing orders two streams that share it.
_workspaces = {}


def _check_backend(backend) -> str:
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {list(BACKENDS)}, got {backend!r}")
    return backend


def _check_mode(mode) -> str:
    if mode not in MODES:
        raise ValueError(f"mode must be one of {list(MODES)}, got {mode!r}")
    return mode


def _check_pair(a: torch.Tensor, b: torch.Tensor, bits: int) -> None:
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    if a.shape != b.shape or a.dim() != 3:
        raise ValueError(f"expected two [B, H, W] frame stacks of equal shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    ok = (torch.uint8,) if bits == 8 else (torch.uint16, torch.int16)
    if a.dtype not in ok or b.dtype not in ok or a.dtype != b.dtype:
        raise ValueError(f"{bits}-bit frames are {' or '.join(str(d) for d in ok)} tensors of one dtype, got {a.dtype} "
                         f"and {b.dtype}")


def _codes(t: torch.Tensor, bits: int) -> torch.Tensor:
    """The samples as int64 codes (10-bit: the 16-bit words unsigned, a word above 1023 read as 1023)."""
    if bits == 8:
        return t.long()
    return (t.view(torch.int16).to(torch.int64) & 0xFFFF).clamp(max=1023)


def _same_layout(a: torch.Tensor, b: torch.Tensor):
    """Both stacks as the kernels take them: one (image stride, row pitch) in samples for the two; views are passed
    where they lie (metrics._plane_layout), anything else is copied."""
    from . import metrics
    try:
        la, lb = metrics._plane_layout(a, "frame0"), metrics._plane_layout(b, "frame1")
    except ValueError:
        la, lb = 0, 1
    if la != lb:
        a, b = a.contiguous(), b.contiguous()
        la = metrics._plane_layout(a, "frame0")
    return a, b, la


def _need_gpu(*ts) -> None:
    if not all(t.is_cuda and t.device == ts[0].device for t in ts):
        raise RuntimeError("the hip backend needs CUDA/HIP tensors on one device; there is no CPU fallback for it "
                           "(backend='torch' runs the restatement anywhere)")


@torch.no_grad()
def farneback_flow(prev: torch.Tensor, next: torch.Tensor, backend: str = "hip", *, bits: int = 8) -> torch.Tensor:
    """Dense flow prev -> next of B frame pairs: [B, H, W] uint8 stacks (bits 10: uint16 / int16 words of 10-bit
    codes, which enter as code / 4) -> float32 [B, H, W, 2] = (dx, dy), the reference's parameters.  backend "hip":
    fiunet_farneback_flow on the frames where they lie; "torch": `calc_optical_flow_farneback` pair by pair."""
    _check_backend(backend)
    _check_pair(prev, next, bits)
    b, h, w = prev.shape
    if backend == "torch":
        conv = (lambda t: t) if bits == 8 else (lambda t: _codes(t, 10).to(torch.float32) / 4.0)
        if b == 0:
            return torch.empty((0, h, w, 2), dtype=torch.float32, device=prev.device)
        return torch.stack([calc_optical_flow_farneback(conv(prev[i]), conv(next[i])) for i in range(b)])
    from . import _native
    _need_gpu(prev, next)
    out = torch.empty((b, h, w, 2), dtype=torch.float32, device=prev.device)
    if b == 0:
        return out
    prev, next, (stride, pitch) = _same_layout(prev, next)
    L = _native.lib()
    nbytes = L.fiunet_flow_workspace_bytes(b, h, w)
    if nbytes == 0:
        _native.check(1, "fiunet_flow_workspace_bytes")
    key = (prev.device, h, w)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[key] = torch.empty(nbytes, dtype=torch.uint8, device=prev.device)
    with torch.cuda.device(prev.device):
        _native.check(L.fiunet_farneback_flow(prev.data_ptr(), next.data_ptr(), bits, b, h, w, stride, pitch,
                                              out.data_ptr(), ws.data_ptr(), ctypes.c_size_t(nbytes),
                                              _native._stream(prev)), "fiunet_farneback_flow")
    return out


def resample_flow(flow: torch.Tensor, height: int, width: int) -> torch.Tensor:
    """An [h, w, 2] flow field for a plane of another size (the luma flow, a sub-sampled chroma plane): cv2.resize's
    linear rule, dx scaled by width / w and dy by height / h.  The same size: the field itself."""
    h, w = flow.shape[:2]
    if (h, w) == (height, width):
        return flow
    mul = torch.tensor([width / w, height / h], dtype=flow.dtype, device=flow.device)
    return _resize_linear(flow, width, height) * mul


def _warp_torch(f0: torch.Tensor, f1: torch.Tensor, flow: torch.Tensor, mode: str, bits: int) -> torch.Tensor:
    """One [H, W] pair along an [h, w, 2] flow field, the definition of both modes -> int64 [H, W]."""
    h, w = f0.shape
    flow = resample_flow(flow.to(torch.float32), h, w)
    ys, xs = torch.meshgrid(torch.arange(h, device=flow.device, dtype=torch.float32),
                            torch.arange(w, device=flow.device, dtype=torch.float32), indexing="ij")
    hx, hy = flow[..., 0] * 0.5, flow[..., 1] * 0.5
    fwd = _remap_bilinear(_codes(f0, bits) if mode == "reference" else _codes(f1, bits),
                          (xs + hx).clamp(0, w - 1), (ys + hy).clamp(0, h - 1))
    if mode == "reference":
        return fwd
    back = _remap_bilinear(_codes(f0, bits), (xs - hx).clamp(0, w - 1), (ys - hy).clamp(0, h - 1))
    return (back + fwd + 1) >> 1


def _warp_time_torch(f0: torch.Tensor, f1: torch.Tensor, flow: torch.Tensor, wn: int, den: int, bits: int) -> torch.Tensor:
    """One [H, W] plane of the frame at time wn / den between A = f0 and B = f1 along the [h, w, 2] flow A -> B, the
    definition of retime "motion" (`fiunet_warp_table_*` is held to it bit for bit) -> int64 [H, W].
    0 < wn < den <= 2**20.  s0 = fp32(wn / den) and s1 = fp32((den - wn) / den), each computed in double and rounded
    once; A is sampled at p - s0 * flow(p) and B at p + s1 * flow(p), every product rounded to fp32 and then every sum
    (separate torch float32 operations: no fused multiply-add), clamped to the plane, through `_remap_bilinear`;
    out = ((den - wn) a + wn b + den // 2) // den, the blend's rounding.  2 wn == den is `_warp_torch(..., "motion")`,
    a zero flow is the blend of `retime.resample_table`."""
    wn, den = int(wn), int(den)
    if not 0 < wn < den <= 1 << 20:
        raise ValueError(f"need 0 < wn < den <= 2**20, got wn = {wn}, den = {den}")
    h, w = f0.shape
    flow = resample_flow(flow.to(torch.float32), h, w)
    dev = flow.device
    ys, xs = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32),
                            torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    s0 = torch.tensor(wn / den, dtype=torch.float64).to(torch.float32).to(dev)
    s1 = torch.tensor((den - wn) / den, dtype=torch.float64).to(torch.float32).to(dev)
    dx, dy = flow[..., 0], flow[..., 1]

    def clamp(v, hi):   # fmin(fmax(v, 0), hi): a NaN comes out as 0
        return torch.nan_to_num(v, nan=0.0).clamp(0, hi)
    a = _remap_bilinear(_codes(f0, bits), clamp(xs - s0 * dx, w - 1), clamp(ys - s0 * dy, h - 1))
    b = _remap_bilinear(_codes(f1, bits), clamp(xs + s1 * dx, w - 1), clamp(ys + s1 * dy, h - 1))
    return ((den - wn) * a + wn * b + den // 2) // den


@torch.no_grad()
def warp(frame0: torch.Tensor, frame1: torch.Tensor, flow: torch.Tensor, mode: str = "reference",
         backend: str = "hip", *, bits: int = 8, out: torch.Tensor = None) -> torch.Tensor:
    """The frame halfway between B pairs of [B, H, W] planes along `flow` [B, h, w, 2] (another size than the plane:
    `resample_flow`).  mode "reference": frame 0 at p + flow / 2 (the reference's formula, which samples against the
    motion); "motion": (frame 0 at p - flow / 2 + frame 1 at p + flow / 2 + 1) >> 1.  remap's arithmetic: clamped
    coordinates rounded to 1/32 pixel, 15-bit weights.  `out`: a [B, H, W] tensor or view of the frames' dtype to
    write into (last stride 1, not overlapping the frames)."""
    _check_mode(mode)
    _check_backend(backend)
    _check_pair(frame0, frame1, bits)
    b, h, w = frame0.shape
    if flow.dim() != 4 or flow.shape[0] != b or flow.shape[3] != 2 or flow.dtype != torch.float32:
        raise ValueError(f"flow: expected float32 [{b}, h, w, 2], got {flow.dtype} {tuple(flow.shape)}")
    if out is None:
        out = torch.empty((b, h, w), dtype=frame0.dtype, device=frame0.device)
    elif out.shape != frame0.shape or out.dtype != frame0.dtype:
        raise ValueError(f"out: expected {frame0.dtype} {tuple(frame0.shape)}, got {out.dtype} {tuple(out.shape)}")
    if b == 0:
        return out
    if backend == "torch":
        for i in range(b):
            v = _warp_torch(frame0[i], frame1[i], flow[i], mode, bits)
            out[i] = v.to(torch.uint8) if bits == 8 else v.to(torch.int16).view(out.dtype)
        return out
    from . import _native, metrics
    _need_gpu(frame0, frame1, flow, out)
    frame0, frame1, (stride, pitch) = _same_layout(frame0, frame1)
    ostride, opitch = metrics._plane_layout(out, "out")
    flow = flow.contiguous()
    with torch.cuda.device(frame0.device):
        _native.check(_native.lib().fiunet_flow_warp(
            frame0.data_ptr(), frame1.data_ptr(), flow.data_ptr(), MODES.index(mode), bits, b, h, w, stride, pitch,
            flow.shape[1], flow.shape[2], out.data_ptr(), ostride, opitch, _native._stream(frame0)), "fiunet_flow_warp")
    return out


@torch.no_grad()
def interpolate(frame0: torch.Tensor, frame1: torch.Tensor, mode: str = "reference", backend: str = "hip", *,
                bits: int = 8) -> torch.Tensor:
    """The flow-compensated middle frame of B pairs of [B, H, W] frames: `farneback_flow`, then `warp`.  mode
    "reference" with backend "torch" is `optical_flow_interpolation_baseline` pair by pair."""
    _check_mode(mode)
    return warp(frame0, frame1, farneback_flow(frame0, frame1, backend, bits=bits), mode, backend, bits=bits)
