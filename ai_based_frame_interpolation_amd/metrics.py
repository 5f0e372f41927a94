"""PSNR / SSIM of uint8 frames on the GPU (the reference's evaluators do this on the host with
scikit-image, model/evaluation.py:194-218, evaluation_simple.py:134-156).  Same definitions and
defaults: PSNR with data_range 255; SSIM with a 7x7 uniform window, sample covariance, K1 0.01,
K2 0.03, mean over the image minus a 3-pixel border.  Inputs stay on the device; results are
float64 tensors, one value per [H, W] plane.  No CPU fallback.

`psnr_planes` / `ssim_planes` are the same two metrics on planes WHERE THEY LIE - any row stride, one stride over the
leading dimensions, uint8 or 10-bit codes in 16-bit words (peak 1023) - for hold-out scoring of video (holdout.py,
DESIGN.md 3.3k): the Y, U and V planes of packed 4:2:0 rows are scored without a copy.  Interleaved samples (DESIGN.md
3.3o: U V of NV12, the bytes of packed RGB, uyvy422 / yuyv422) are scored where they lie too: `psnr_interleaved` gives
every component of [..., H, W, S] rows in one pass, `ssim_planes` takes a last-dimension stride of 1..4.

Also here: the reference's OTHER SSIM, the Gaussian-window one of its training loss
(model/train.py:18-87: `SSIMLoss`, `CombinedLoss`) - the only SSIM in the reference that is pure torch,
so the only one whose values are pinned by fixtures recorded from the reference itself
(tests/golden/ssim_gauss_*.npz).  `ssim_gauss`, `SSIMLoss` and `CombinedLoss` evaluate it with one HIP
pass over the two fp32 tensors (forward values only: this is the inference tier, nothing here is
differentiable)."""
from __future__ import annotations

import ctypes

import torch

from . import _native


def _planes(pred: torch.Tensor, target: torch.Tensor):
    if pred.shape != target.shape or pred.dim() < 2:
        raise RuntimeError(f"expected two uint8 tensors of equal shape [..., H, W], got "
                           f"{tuple(pred.shape)} and {tuple(target.shape)}")
    if pred.dtype != torch.uint8 or target.dtype != torch.uint8:
        raise RuntimeError("metrics are defined on the uint8 frames (postprocess_image output)")
    if not pred.is_cuda or not target.is_cuda:
        raise RuntimeError("device metrics need CUDA/HIP tensors; there is no CPU fallback here")
    h, w = pred.shape[-2:]
    n = pred.numel() // (h * w) if h * w else 0
    return pred.contiguous(), target.contiguous(), n, h, w


def _run(fn_name, pred, target):
    p, t, n, h, w = _planes(pred, target)
    L = _native.lib()
    nbytes = L.fiunet_metrics_workspace_bytes(n, h, w)
    if nbytes == 0:
        _native.check(1, "fiunet_metrics_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=p.device)
    out = torch.empty(n, dtype=torch.float64, device=p.device)
    with torch.cuda.device(p.device):
        s = torch.cuda.current_stream(p.device).cuda_stream
        _native.check(getattr(L, fn_name)(p.data_ptr(), t.data_ptr(), n, h, w, out.data_ptr(),
                                          ws.data_ptr(), ctypes.c_size_t(nbytes), s), fn_name)
    return out.view(pred.shape[:-2])


def psnr_u8(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """compute_psnr(pred, target) (evaluation.py:194-205) for every [H, W] plane."""
    return _run("fiunet_psnr_u8", pred, target)


def ssim_u8(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """compute_ssim(pred, target) (evaluation.py:207-218) for every [H, W] plane."""
    return _run("fiunet_ssim_u8", pred, target)


def _image_stride(t: torch.Tensor, name: str, tail: int, image: int) -> int:
    """The one stride the dimensions before the last `tail` advance by; `image` samples where there is one image."""
    st = t.stride()
    lead = [(n, s) for n, s in zip(t.shape[:-tail], st[:-tail]) if n != 1]
    for (_, s0), (n1, s1) in zip(lead[:-1], lead[1:]):
        if s0 != s1 * n1:
            raise ValueError(f"{name}: the leading dimensions must advance by one stride (shape {tuple(t.shape)}, "
                             f"strides {tuple(st)})")
    return lead[-1][1] if lead else image


def _stepped_layout(t: torch.Tensor, name: str, max_step: int):
    """[..., H, W] -> (image stride, row pitch, sample step) in samples, as the tensor lies: no copy.  The leading
    dimensions must advance by one stride (a stack, every second frame of one, channel c of [N, C, H, W], a slice of
    packed rows); the last dimension has a stride of 1..max_step (above 1: one component of interleaved samples)."""
    h, w = t.shape[-2:]
    st = t.stride()
    step = st[-1] if w > 1 else 1
    if not 1 <= step <= max_step:
        raise ValueError(f"{name}: the last dimension must have stride 1{f'..{max_step}' if max_step > 1 else ''} "
                         f"(strides {tuple(st)})")
    row = (w - 1) * step + 1
    pitch = st[-2] if h > 1 else row
    return _image_stride(t, name, 2, (h - 1) * pitch + row), pitch, step


def _plane_layout(t: torch.Tensor, name: str):
    """`_stepped_layout` of a plane whose last dimension has stride 1 -> (image stride, row pitch)."""
    return _stepped_layout(t, name, 1)[:2]


def _plane_args(pred: torch.Tensor, target: torch.Tensor, bits: int, max_step: int = 1, tail: int = 2):
    """tail: the trailing dimensions of one image (2: [H, W]; 3: [H, W, S] interleaved)."""
    if bits not in (8, 10):
        raise ValueError(f"bits must be 8 or 10, got {bits!r}")
    if pred.shape != target.shape or pred.dim() < tail:
        raise ValueError(f"expected two tensors of equal shape [..., H, W{', S' if tail == 3 else ''}], got "
                         f"{tuple(pred.shape)} and {tuple(target.shape)}")
    ok = (torch.uint8,) if bits == 8 else (torch.uint16, torch.int16)
    if pred.dtype not in ok or target.dtype not in ok:
        raise ValueError(f"{bits}-bit planes are {' or '.join(str(d) for d in ok)} tensors, got {pred.dtype} and "
                         f"{target.dtype}")
    if not pred.is_cuda or not target.is_cuda or pred.device != target.device:
        raise RuntimeError("device metrics need CUDA/HIP tensors on one device; there is no CPU fallback here")
    if tail == 3:
        return None
    h, w = pred.shape[-2:]
    if h < 1 or w < 1:
        raise ValueError(f"empty planes {tuple(pred.shape)}")
    n = pred.numel() // (h * w)
    return n, h, w, _stepped_layout(pred, "pred", max_step), _stepped_layout(target, "target", max_step)


def _plane_call(fn_name: str, args: tuple, count: int, h: int, w: int, device, *, takes_sse: bool,
                want_sse: bool = False):
    """What every plane metric ends in: `count` float64 results, the workspace, the current stream and the call
    `fn_name(*args, out, [sse,] workspace, bytes, stream)`.  takes_sse: the entry point has an sse pointer; want_sse: it
    gets `count` int64 sums to fill (NULL otherwise).  -> (out, sums or None)"""
    out = torch.empty(count, dtype=torch.float64, device=device)
    sums = torch.empty(count, dtype=torch.int64, device=device) if want_sse else None
    if count:
        L = _native.lib()
        nbytes = L.fiunet_plane_metrics_workspace_bytes(count, h, w)
        if nbytes == 0:
            _native.check(1, "fiunet_plane_metrics_workspace_bytes")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        sse_arg = (None if sums is None else sums.data_ptr(),) if takes_sse else ()
        with torch.cuda.device(device):
            s = torch.cuda.current_stream(device).cuda_stream
            _native.check(getattr(L, fn_name)(*args, out.data_ptr(), *sse_arg, ws.data_ptr(), ctypes.c_size_t(nbytes),
                                              s), fn_name)
    return out, sums


def psnr_planes(pred: torch.Tensor, target: torch.Tensor, bits: int, *, return_sse: bool = False):
    """PSNR of every [H, W] plane of two device tensors [..., H, W] WHERE THEY LIE (fiunet_plane_psnr): uint8 at bits 8
    (peak 255), uint16 or int16 words of 10-bit codes at bits 10 (peak 1023).  The last dimension has stride 1; any row
    stride and any single stride of the leading dimensions go to the kernel as they are (no `.contiguous()`).
    -> float64 [...]; with return_sse also the exact sums of squared differences, int64 [...] (the bits of the
    library's uint64)."""
    n, h, w, (ps, pp, _), (ts, tp, _) = _plane_args(pred, target, bits)
    lead = pred.shape[:-2]
    out, sse = _plane_call("fiunet_plane_psnr", (pred.data_ptr(), ps, pp, target.data_ptr(), ts, tp, bits, n, h, w),
                           n, h, w, pred.device, takes_sse=True, want_sse=bool(return_sse))
    return (out.view(lead), sse.view(lead)) if return_sse else out.view(lead)


def _interleaved_layout(t: torch.Tensor, name: str):
    """[..., H, W, S] -> (image stride, row pitch) in samples: stride 1 over S, S over W, anything over the rows."""
    h, w, comp = t.shape[-3:]
    st = t.stride()
    if st[-1] != 1 or (w > 1 and st[-2] != comp):
        raise ValueError(f"{name}: interleaved samples have stride 1 in the last dimension and S = {comp} in the one "
                         f"before it (strides {tuple(st)})")
    pitch = st[-3] if h > 1 else w * comp
    return _image_stride(t, name, 3, (h - 1) * pitch + w * comp), pitch


def psnr_interleaved(pred: torch.Tensor, target: torch.Tensor, bits: int, *, return_sse: bool = False):
    """PSNR of every component of interleaved device tensors [..., H, W, S], S in {2, 3, 4}, where they lie, in ONE pass
    over the samples (fiunet_interleaved_psnr): the last dimension has stride 1, the W dimension stride S, the rows and
    the leading dimensions as for `psnr_planes`.  -> float64 [..., S]; with return_sse also int64 [..., S].  Component c
    is, to the last bit, `psnr_planes` of a contiguous copy of `[..., c]`."""
    if pred.dim() >= 3 and pred.shape[-1] not in (2, 3, 4):
        raise ValueError(f"interleaved samples have 2, 3 or 4 components, got {pred.shape[-1]} (shape "
                         f"{tuple(pred.shape)})")
    _plane_args(pred, target, bits, tail=3)
    h, w, comp = pred.shape[-3:]
    if h < 1 or w < 1:
        raise ValueError(f"empty planes {tuple(pred.shape)}")
    n = pred.numel() // (h * w * comp)
    (ps, pp), (ts, tp) = _interleaved_layout(pred, "pred"), _interleaved_layout(target, "target")
    lead = pred.shape[:-3] + (comp,)
    out, sse = _plane_call("fiunet_interleaved_psnr",
                           (pred.data_ptr(), ps, pp, target.data_ptr(), ts, tp, bits, comp, n, h, w),
                           n * comp, h, w, pred.device, takes_sse=True, want_sse=bool(return_sse))
    return (out.view(lead), sse.view(lead)) if return_sse else out.view(lead)


def ssim_planes(pred: torch.Tensor, target: torch.Tensor, bits: int) -> torch.Tensor:
    """SSIM (skimage's defaults, data_range = the peak) of every [H, W] plane where it lies (fiunet_stepped_ssim);
    the arguments are `psnr_planes`', and the last dimension may have a stride of 1..4 on either side (the view
    `t[..., c]` of interleaved [..., H, W, S]); H, W >= 7.  -> float64 [...]."""
    n, h, w, (ps, pp, pstep), (ts, tp, tstep) = _plane_args(pred, target, bits, max_step=4)
    if h < 7 or w < 7:
        raise ValueError(f"SSIM: the 7x7 window exceeds the {h}x{w} plane")
    out, _ = _plane_call("fiunet_stepped_ssim",
                         (pred.data_ptr(), ps, pp, pstep, target.data_ptr(), ts, tp, tstep, bits, n, h, w),
                         n, h, w, pred.device, takes_sse=False)
    return out.view(pred.shape[:-2])


_WINDOWS = {}


def _gauss_1d(window_size: int, sigma: float = 1.5) -> torch.Tensor:
    """SSIMLoss._gaussian (train.py:27-29): fp32 tensor of exp(-(x - ws//2)^2 / (2 sigma^2)) divided by
    its own torch sum (host tensor; the kernel applies it separably)."""
    if window_size not in _WINDOWS:
        import math
        g = torch.tensor([math.exp(-(x - window_size // 2) ** 2 / float(2 * sigma ** 2))
                          for x in range(window_size)], dtype=torch.float32)
        _WINDOWS[window_size] = (g / g.sum()).contiguous()
    return _WINDOWS[window_size]


def _gauss_planes(img1: torch.Tensor, img2: torch.Tensor, window_size: int):
    """-> (per-plane mean of the SSIM map [B, C] float64, per-plane sum of squared error [B, C] float64)"""
    if img1.shape != img2.shape or img1.dim() != 4:
        raise RuntimeError(f"expected two [B, C, H, W] tensors of equal shape, got {tuple(img1.shape)} and "
                           f"{tuple(img2.shape)}")
    if img1.dtype != torch.float32 or img2.dtype != torch.float32:
        raise RuntimeError("the Gaussian-window SSIM is defined on the fp32 tensors of the loss (train.py:192)")
    if not img1.is_cuda or not img2.is_cuda:
        raise RuntimeError("device metrics need CUDA/HIP tensors; there is no CPU fallback here")
    b, c, h, w = img1.shape
    n = b * c
    if n == 0 or h == 0 or w == 0:
        raise RuntimeError("empty input")
    a, t = img1.contiguous(), img2.contiguous()
    L = _native.lib()
    nbytes = L.fiunet_ssim_gauss_workspace_bytes(n, h, w)
    if nbytes == 0:
        _native.check(1, "fiunet_ssim_gauss_workspace_bytes")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=a.device)
    out = torch.empty((2, n), dtype=torch.float64, device=a.device)
    win = _gauss_1d(int(window_size))
    with torch.cuda.device(a.device):
        s = torch.cuda.current_stream(a.device).cuda_stream
        _native.check(L.fiunet_ssim_gauss_f32(a.data_ptr(), t.data_ptr(), n, h, w, int(window_size),
                                              win.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                              ws.data_ptr(), ctypes.c_size_t(nbytes), s), "fiunet_ssim_gauss_f32")
    return out[0].view(b, c), out[1].view(b, c)


def ssim_gauss(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True,
               dtype=None) -> torch.Tensor:
    """SSIMLoss._ssim (train.py:37-56): `ssim_map.mean()` (a 0-dim tensor) if size_average else the
    per-sample mean over (C, H, W) ([B]).  Returned in the inputs' dtype like the reference's result
    unless `dtype` says otherwise (the device value is float64)."""
    planes, _ = _gauss_planes(img1, img2, window_size)
    val = planes.mean() if size_average else planes.mean(dim=1)
    return val.to(dtype or img1.dtype)


class SSIMLoss:
    """train.py:18-73: `1 - ssim` with the 11x11 sigma-1.5 Gaussian window.  The reference rebuilds its
    window when the channel count changes (:59-70); here the window is depth-wise by construction, so
    `channel` is accepted and ignored."""

    def __init__(self, window_size: int = 11, size_average: bool = True, channel: int = 1):
        self.window_size, self.size_average, self.channel = window_size, size_average, channel

    def __call__(self, img1: torch.Tensor, img2: torch.Tensor) -> torch.Tensor:
        return 1 - ssim_gauss(img1, img2, self.window_size, self.size_average)

    forward = __call__


class CombinedLoss:
    """train.py:75-87: mse_weight * MSELoss(pred, target) + ssim_weight * SSIMLoss()(pred, target), both
    terms from ONE pass over the two tensors."""

    def __init__(self, mse_weight: float = 0.5, ssim_weight: float = 0.5):
        self.mse_weight, self.ssim_weight = mse_weight, ssim_weight

    def terms(self, pred: torch.Tensor, target: torch.Tensor):
        """-> (mse, ssim) as float64 0-dim device tensors"""
        planes, sq = _gauss_planes(pred, target, 11)
        return sq.sum() / float(pred.numel()), planes.mean()

    def __call__(self, pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        mse, ssim = self.terms(pred, target)
        return (self.mse_weight * mse + self.ssim_weight * (1 - ssim)).to(pred.dtype)

    forward = __call__
