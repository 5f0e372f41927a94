"""Drop-in mirror of the reference's model/unet.py for the MI355X HIP path.

Same class name, constructor, call signature, attribute tree and state-dict schema as
/root/reference/model/unet.py:97-112 (`FrameInterpolationUNet`) and :65-95 (`UNet`), so
`load_state_dict` of a reference `best_model.pth` works and callers such as
model/inference.py:77-97,120 need no change.  The forward itself does not run any torch op
on the data: it hands raw device pointers to the hand-written HIP kernels behind the C ABI
(include/fiunet.h).  PyTorch only provides device memory, the stream and the parameter
containers (nn.Conv2d / nn.BatchNorm2d objects are used purely as named parameter holders
so that initialisation and state-dict keys are identical to the reference's; they are never
called).

There is no CPU fallback: CPU tensors, train mode and a missing/unbuilt extension raise.
"""
from __future__ import annotations

import contextlib
import os

import torch
import torch.nn as nn

from . import _native

# ---- layer table (unet.py:72-82, bilinear=True) ----------------------------------------------
# (attribute path of the DoubleConv holder, in, mid, out)
_ENCODER = (("down1", 64, 128), ("down2", 128, 256), ("down3", 256, 512), ("down4", 512, 512))
_DECODER = (("up1", 1024, 256), ("up2", 512, 128), ("up3", 256, 64), ("up4", 128, 64))
# bilinear=False, the constructor's default (unet.py:66,76-81 with factor 1): down4 -> 1024, Up(in, out) =
# ConvTranspose2d(in, in // 2, 2, 2) + DoubleConv(in, out)
_ENCODER_CT = (("down1", 64, 128), ("down2", 128, 256), ("down3", 256, 512), ("down4", 512, 1024))
_DECODER_CT = (("up1", 1024, 512), ("up2", 512, 256), ("up3", 256, 128), ("up4", 128, 64))

#: channels / pyramid level of the 18 conv+BN+ReLU outputs, in state-dict order (debug taps)
TAP_CHANNELS = (64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 256, 256, 128, 128, 64, 64, 64)
TAP_CHANNELS_CT = (64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64)
TAP_LEVEL = (0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0)
TAP_NAMES = tuple(
    f"{p}.double_conv.{c}"
    for p in ("unet.inc", "unet.down1.maxpool_conv.1", "unet.down2.maxpool_conv.1",
              "unet.down3.maxpool_conv.1", "unet.down4.maxpool_conv.1", "unet.up1.conv",
              "unet.up2.conv", "unet.up3.conv", "unet.up4.conv")
    for c in (0, 3))

#: read-back taps 18..21: `self.up(x1)` + F.pad of up1..up4 (unet.py:47-53), where it is stored as a tensor
UP_TAP_NAMES = ("unet.up1.up", "unet.up2.up", "unet.up3.up", "unet.up4.up")

_PRECISIONS = {"fp32": _native.FP32, "float32": _native.FP32, "bf16x2": _native.BF16X2, "bf16": _native.BF16,
               "bfloat16": _native.BF16, "fp16": _native.FP16, "float16": _native.FP16, "half": _native.FP16}


class _Holder(nn.Module):
    """Parameter container; exists only to give parameters the reference's names."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: the forward runs in the HIP kernels, not in torch")


class _Slot(nn.Module):
    """Place-holder child at a position where the reference has a tensor-less module (ReLU,
    MaxPool2d, Upsample): keeps `named_modules()`, integer indexing and `len()` of the holders
    identical to the reference's nn.Sequential / Up, while owning no tensors (state-dict unchanged).
    The op itself is fused into the neighbouring HIP conv kernel."""

    def __init__(self, what: str):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return f"{self.what} (fused into the HIP conv kernels)"

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError(f"{self.what}: fused into the HIP kernels, not callable on its own")


class _Seq(nn.ModuleDict):
    """ModuleDict keyed "0".."n-1" that also indexes like nn.Sequential (int and slice), so
    `model.unet.inc.double_conv[0].weight` and `down1.maxpool_conv[1]` work as on the reference
    (/root/reference/model/unet.py:11-18, :27-30)."""

    def __getitem__(self, idx):
        if isinstance(idx, slice):
            keys = list(self._modules.keys())[idx]
            return _Seq({k: self._modules[k] for k in keys})
        if isinstance(idx, int):
            n = len(self._modules)
            if not -n <= idx < n:
                raise IndexError(f"index {idx} is out of range")
            return list(self._modules.values())[idx % n]
        return super().__getitem__(idx)

    def __iter__(self):  # nn.Sequential iterates over modules, ModuleDict over keys
        return iter(self._modules.values())

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter holder: the forward runs in the HIP kernels, not in torch")


def _double_conv(cin: int, cout: int, mid: int | None = None) -> _Holder:
    """Holder with `.double_conv[0..5]` like DoubleConv (unet.py:5-18): conv, BN, ReLU, conv, BN,
    ReLU; slots 2 and 5 (ReLU) own no tensors."""
    mid = mid or cout
    h = _Holder()
    h.double_conv = _Seq({
        "0": nn.Conv2d(cin, mid, kernel_size=3, padding=1, bias=False),
        "1": nn.BatchNorm2d(mid),
        "2": _Slot("ReLU(inplace=True)"),
        "3": nn.Conv2d(mid, cout, kernel_size=3, padding=1, bias=False),
        "4": nn.BatchNorm2d(cout),
        "5": _Slot("ReLU(inplace=True)"),
    })
    return h


class UNet(_Holder):
    """Parameter tree of the reference UNet (unet.py:65-82); widths 64-128-256-512-512 with the bilinear
    decoder (every reference caller), 64-128-256-512-1024 with the ConvTranspose2d decoder (the default)."""

    def __init__(self, n_channels: int = 2, n_classes: int = 1, bilinear: bool = False):
        super().__init__()
        self.n_channels = n_channels
        self.n_classes = n_classes
        self.bilinear = bilinear
        self.inc = _double_conv(n_channels, 64)
        for name, cin, cout in (_ENCODER if bilinear else _ENCODER_CT):
            d = _Holder()
            d.maxpool_conv = _Seq({"0": _Slot("MaxPool2d(2)"), "1": _double_conv(cin, cout)})
            setattr(self, name, d)
        for name, cin, cout in (_DECODER if bilinear else _DECODER_CT):
            u = _Holder()
            if bilinear:
                u.up = _Slot("Upsample(scale_factor=2, mode='bilinear', align_corners=True)")
                u.conv = _double_conv(cin, cout, cin // 2)
            else:   # unet.py:42-44: parameter holder only, the transposed conv runs in convt2x2_kernel
                u.up = nn.ConvTranspose2d(cin, cin // 2, kernel_size=2, stride=2)
                u.conv = _double_conv(cin, cout)
            setattr(self, name, u)
        self.outc = _Holder()
        self.outc.conv = nn.Conv2d(64, n_classes, kernel_size=1)


class FrameInterpolationUNet(nn.Module):
    """`model(frame1, frame2)` -> middle frame; see module docstring.

    Extra (non-reference) keyword arguments:
      frame_channels: 1 (grayscale, the reference's 2->1 network) or 3 (RGB 6->3 variant the
                      reference README describes); same kernels.
      precision:      "fp32" (default; exact-fp32 MFMA, |d| <= 1e-3 contract), "bf16" (bf16 storage + MFMA,
                      fp32 accumulate) or "bf16x2" (the fp32 contract on the bf16 pipe - activations
                      and weights as two bf16 pieces, three MFMAs per product, ~1e-5 relative end to end, about
                      3x the speed of "fp32"; both decoders) or "fp16" (aliases "float16", "half": IEEE fp16 storage
                      + MFMA, fp32 accumulate - bf16's kernels with 11 significant bits instead of 8, round to
                      nearest, no dither).  Env FIUNET_PRECISION is the default when the
                      argument is None.  The attribute may be reassigned between forwards.
      weight_prep:    where a checkpoint becomes what the kernels read (BatchNorm fold, repack, bf16 rounding): "host"
                      (default; one thread of `fiunet_load_weights`, every tensor through host memory) or "device"
                      (`fiunet_load_weights_device`: HIP kernels on the tensors where they are, into the same buffers
                      at every reload) - the same bytes either way.  Env FIUNET_WEIGHT_PREP is the default when the
                      argument is None.  The attribute may be reassigned; the next forward then prepares again.
    """

    def __init__(self, bilinear: bool = False, frame_channels: int = 1, precision: str | None = None,
                 weight_prep: str | None = None):
        super().__init__()
        self.unet = UNet(n_channels=2 * frame_channels, n_classes=frame_channels, bilinear=bilinear)
        self.frame_channels = frame_channels
        self.precision = precision or os.environ.get("FIUNET_PRECISION", "fp32")
        if self.precision not in _PRECISIONS:
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}")
        self.weight_prep = weight_prep or os.environ.get("FIUNET_WEIGHT_PREP", "host")
        self._weight_prep_checked()
        self._prep_loaded = None  # the weight_prep the device copy was made with
        self._ctx = None          # _native.Context, per device
        self._ctx_dirty = True    # weights on the device are stale w.r.t. the parameters
        self._weights_gen = 0     # bumped at every upload (GraphedForward re-captures on change)
        self._tracked = None      # parameters + buffers whose (version, data_ptr) are fingerprinted
        self._fingerprint = None
        self._ws = None           # cached workspace tensor (kept at the largest size seen)
        self._options = 0

    # -- keep the device copy of the weights in sync with the nn.Module state --------------
    # Like the reference nn.Module, a forward always uses the LIVE parameters: besides the explicit
    # hooks below, every forward compares a cheap fingerprint (autograd version counter + storage
    # pointer of each parameter and buffer) with the one recorded at the last upload, so in-place
    # edits (`p.add_(..)`, `p.data = ..`, `model.unet.load_state_dict(..)`) are picked up too.
    def _apply(self, fn, *a, **k):
        self._ctx_dirty = True
        self._tracked = None
        return super()._apply(fn, *a, **k)

    def _current_fingerprint(self):
        """(identity, autograd version, storage pointer) of every parameter and buffer.  Sees `p.add_()`,
        `p.data = ...`, `p.copy_()`, replaced Parameters and `load_state_dict(assign=True)`.  Does NOT see
        in-place edits made through `.data` / under `torch.no_grad()` on a `.data` alias
        (`p.data.add_()`: `.data` carries its own version counter) - call `refresh_weights()` after those.
        Inference-mode tensors have no version counter; they count as version 0 (their storage pointer
        and identity still change when they are replaced)."""
        tracked = list(self.parameters()) + list(self.buffers())  # re-listed every call: catches replaced tensors
        fp = []
        for t in tracked:
            try:
                ver = t._version
            except RuntimeError:  # "Inference tensors do not track version counter"
                ver = 0
            fp.append((id(t), ver, t.data_ptr()))
        return tuple(fp)

    # the HIP context holds raw pointers: never pickled / deep-copied with the module
    def __getstate__(self):
        st = self.__dict__.copy()
        st["_ctx"], st["_ws"], st["_tracked"], st["_fingerprint"], st["_ctx_dirty"] = None, None, None, None, True
        return st

    def __deepcopy__(self, memo):
        import copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        for k, v in self.__getstate__().items():
            new.__dict__[k] = copy.deepcopy(v, memo)
        return new

    def load_state_dict(self, *a, **k):
        self._ctx_dirty = True
        self._tracked = None
        return super().load_state_dict(*a, **k)

    def refresh_weights(self):
        """Call after editing parameters in place so the next forward re-uploads them."""
        self._ctx_dirty = True

    def set_options(self, *, unfused: bool = False, keep_all: bool = False, gather_upsample: bool = False,
                    rne_weights: bool = False, no_dither: bool = False):
        """unfused / keep_all / gather_upsample: ablation and test switches (include/fiunet.h).
        rne_weights: bf16 weights rounded to nearest instead of with the per-filter error feedback;
        no_dither: no ordered input dither in the bf16 stem - both for comparing a real checkpoint both
        ways (the defaults are what the PSNR criterion was measured with)."""
        old = self._options
        self._options = ((_native.OPT_UNFUSED if unfused else 0) | (_native.OPT_KEEP_ALL if keep_all else 0)
                         | (_native.OPT_GATHER_UPSAMPLE if gather_upsample else 0)
                         | (_native.OPT_RNE_WEIGHTS if rne_weights else 0)
                         | (_native.OPT_NO_DITHER if no_dither else 0))
        if (old ^ self._options) & _native.OPT_RNE_WEIGHTS:
            self._ctx_dirty = True  # the rounding mode is applied when the weights are prepared
        if self._ctx is not None:
            self._ctx.set_options(self._options)

    def _ctx_or_none_set_options(self):
        if self._ctx is not None:
            self._ctx.set_options(self._options)

    def _context(self, device: torch.device) -> "_native.Context":
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._ctx is None or self._ctx.device_index != idx:
            if self._ctx is not None:
                self._ctx.close()
            self._ctx = _native.Context(idx, self.frame_channels, self.unet.bilinear)
            self._ctx_dirty = True
        fp = self._current_fingerprint()
        prep = self._weight_prep_checked()
        if self._ctx_dirty or fp != self._fingerprint or prep != self._prep_loaded:
            self._ctx.set_options(self._options)  # (the weight-rounding option is read at load time)
            self._ctx.load_state_dict(self.state_dict(), prep=prep)
            self._ctx_dirty = False
            self._prep_loaded = prep
            self._fingerprint = fp
            self._weights_gen += 1
        return self._ctx

    def _workspace(self, ctx, device, b, h, w, prec, u8=False, yuv=False, p10=False):
        """One scratch block, kept at the largest size any call has needed (a smaller batch or the
        ragged last chunk of a video reuses it instead of freeing and reallocating gigabytes)."""
        nbytes = ctx.workspace_bytes(b, h, w, prec, u8, yuv, p10)
        if self._ws is None or self._ws.device != device or self._ws.numel() < nbytes:
            self._ws = None  # release before allocating the next one
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return self._ws

    def _weight_prep_checked(self) -> str:
        """`weight_prep` is a plain attribute like `precision`: validated where it is used."""
        if self.weight_prep not in _native.WEIGHT_PREPS:
            raise ValueError(f"weight_prep must be one of {list(_native.WEIGHT_PREPS)}, got {self.weight_prep!r}")
        return self.weight_prep

    def _precision_code(self) -> int:
        """`precision` is a plain attribute and may be reassigned between forwards: validated where it is used."""
        try:
            return _PRECISIONS[self.precision]
        except (KeyError, TypeError):
            raise ValueError(f"precision must be one of {sorted(_PRECISIONS)}, got {self.precision!r}") from None

    def _check_pair(self, frame1, frame2, dtype_ok):
        if frame1.dim() != 4 or frame1.shape != frame2.shape:
            raise RuntimeError(
                f"expected two [B,{self.frame_channels},H,W] tensors of equal shape, got "
                f"{tuple(frame1.shape)} and {tuple(frame2.shape)}")
        if frame1.shape[1] != self.frame_channels:
            raise RuntimeError(
                f"expected {self.frame_channels} channel(s) per frame, got {frame1.shape[1]}")
        self._check_device_mode_dtype(frame1, frame2, dtype_ok)

    def _check_device_mode_dtype(self, frame1, frame2, dtype_ok):
        if not frame1.is_cuda or not frame2.is_cuda:
            raise RuntimeError(
                "FrameInterpolationUNet (MI355X build) runs only on a HIP device: move the model "
                "and the frames with .to('cuda').  There is no CPU fallback in this package.")
        if self.training:
            raise RuntimeError(
                "inference-only build: call model.eval() first (reference: inference.py:97); "
                "train-mode BatchNorm (batch statistics) is not implemented")
        if frame1.dtype not in dtype_ok or frame2.dtype != frame1.dtype:
            raise RuntimeError(f"unsupported frame dtype {frame1.dtype}/{frame2.dtype}")

    @torch.no_grad()
    def forward(self, frame1: torch.Tensor, frame2: torch.Tensor) -> torch.Tensor:
        self._check_pair(frame1, frame2, (torch.float32, torch.float16, torch.bfloat16, torch.float64))
        in_dtype = frame1.dtype
        f1 = frame1.to(torch.float32).contiguous()
        f2 = frame2.to(torch.float32).contiguous()
        b, _, h, w = f1.shape
        prec = self._precision_code()
        ctx = self._context(f1.device)
        ws = self._workspace(ctx, f1.device, b, h, w, prec)
        out = torch.empty_like(f1)
        with torch.cuda.device(f1.device):
            ctx.forward(f1, f2, out, prec, ws)
        return out if in_dtype == torch.float32 else out.to(in_dtype)

    def batch_invariant_from(self, height: int, width: int, device=None) -> int:
        """Smallest batch at which the result of a pair no longer depends on the batch it is part of (no layer cuts
        its K loop over workgroups: include/fiunet.h, fiunet_min_unsplit_batch).  1 from 1080p up, 5 at 720p."""
        dev = device if device is not None else next(self.parameters()).device
        return self._context(torch.device(dev)).min_unsplit_batch(int(height), int(width), self._precision_code())

    @torch.no_grad()
    def forward_strip(self, frame1: torch.Tensor, frame2: torch.Tensor, y_origin: int,
                      image_height: int) -> torch.Tensor:
        """The same forward on the band of rows [y_origin, y_origin + H) of a taller image
        (spatial tiling): upsampling and F.pad are evaluated in whole-image
        coordinates, so rows at least 112 away from a cut edge equal the un-tiled result.  See
        tiling.py for the strip plan; `fiunet_forward_strip` in include/fiunet.h for the rules."""
        self._check_pair(frame1, frame2, (torch.float32,))
        f1, f2 = frame1.contiguous(), frame2.contiguous()
        b, _, h, w = f1.shape
        prec = self._precision_code()
        ctx = self._context(f1.device)
        ws = self._workspace(ctx, f1.device, b, h, w, prec)
        out = torch.empty_like(f1)
        with torch.cuda.device(f1.device):
            ctx.forward_strip(f1, f2, out, int(y_origin), int(image_height), prec, ws)
        return out

    @torch.no_grad()
    def forward_u8(self, frame1: torch.Tensor, frame2: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """uint8 [B,C,H,W] frames in -> uint8 interpolated frame, with the reference's
        pre/post-processing (inference.py:31-35, :54-61) on device.  `out`: write the result there instead of into a
        new tensor - uint8, same shape and device, every image contiguous; the images may lie apart (the video loop
        passes every second frame of its interleaved result, `fiunet_forward_u8_strided`)."""
        self._check_pair(frame1, frame2, (torch.uint8,))
        f1, f2 = frame1.contiguous(), frame2.contiguous()
        b, _, h, w = f1.shape
        prec = self._precision_code()
        ctx = self._context(f1.device)
        ws = self._workspace(ctx, f1.device, b, h, w, prec, u8=True)
        if out is None:
            out = torch.empty_like(f1)
        elif out.dtype != torch.uint8 or out.shape != f1.shape or out.device != f1.device:
            raise ValueError(f"out must be a uint8 {tuple(f1.shape)} tensor on {f1.device}")
        with torch.cuda.device(f1.device):
            ctx.forward_u8(f1, f2, out, prec, ws)
        return out

    @torch.no_grad()
    def forward_yuv420(self, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, *,
                       siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited",
                       out: torch.Tensor | None = None) -> torch.Tensor:
        """The RGB network on colour video: uint8 [B, F] packed I420 frames in (F = H*W + 2*ceil(H/2)*ceil(W/2), a Y4M
        frame payload) -> uint8 [B, F] interpolated frames, `fiunet_forward_yuv420`: YUV -> planar RGB, `forward_u8`,
        RGB -> YUV, all on device in the integer conversion of csrc/colour.hip.h.  siting / matrix / colour_range: see
        colour.py (matrix defaults to "bt709", a convention for HD video: Y4M does not carry it).  `out`: write there -
        uint8 [B, F] on the same device, every frame contiguous; the frames may lie apart (the video loop passes every
        second frame of its interleaved result)."""
        return self._forward_i420("forward_yuv420", 8, frame1, frame2, height, width, out, siting, matrix, colour_range)

    @torch.no_grad()
    def forward_p10(self, frame1: torch.Tensor, frame2: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """10-bit frames: uint16 [B,C,H,W] of 10-bit codes in (above 1023 reads as 1023) -> uint16 interpolated frames,
        `fiunet_forward_p10`: x / 1023 * 2 - 1 on device, the fp32-in forward, trunc(clamp((y+1)/2, 0, 1) * 1023) on
        device - bit for bit `postprocess_p10(forward(preprocess_p10(a), preprocess_p10(b)))`.  Both networks.
        Accuracy: fp32, bf16x2 and fp16 within 1 code of the fp32 oracle; bf16 about 5 codes (8 significant bits in every
        activation, a stem dither of 2 codes peak to peak): use fp16 (or bf16x2) for 10-bit video.  `out`: as for `forward_u8`
        (uint16, every image contiguous, the images may lie apart)."""
        self._check_pair(frame1, frame2, (torch.uint16,))
        if not frame1.is_contiguous() or not frame2.is_contiguous():
            raise ValueError("forward_p10 takes contiguous frames")
        b, _, h, w = frame1.shape
        prec = self._precision_code()
        ctx = self._context(frame1.device)
        ws = self._workspace(ctx, frame1.device, b, h, w, prec, p10=True)
        if out is None:
            out = torch.empty_like(frame1)
        elif out.dtype != torch.uint16 or out.shape != frame1.shape or out.device != frame1.device:
            raise ValueError(f"out must be a uint16 {tuple(frame1.shape)} tensor on {frame1.device}")
        with torch.cuda.device(frame1.device):
            ctx.forward_p10(frame1, frame2, out, prec, ws)
        return out

    @torch.no_grad()
    def forward_yuv420p10(self, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, *,
                          siting: str = "jpeg", matrix: str = "bt709", colour_range: str = "limited",
                          out: torch.Tensor | None = None) -> torch.Tensor:
        """The RGB network on 10-bit colour video: uint16 [B, F] packed 4:2:0 10-bit frames in (F = H*W +
        2*ceil(H/2)*ceil(W/2) samples, a C420p10 Y4M frame payload) -> uint16 [B, F] interpolated frames,
        `fiunet_forward_yuv420p10`: YUV -> planar RGB, `forward_p10`, RGB -> YUV on device.  matrix
        also takes "bt2020".  The network interpolates code values, as it does for 8-bit video (no PQ / HLG
        linearisation).  Use fp16 (or bf16x2, fp32): bf16 is about 5 codes off.  `out`: as for `forward_yuv420`."""
        return self._forward_i420("forward_yuv420p10", 10, frame1, frame2, height, width, out, siting, matrix,
                                  colour_range)

    def _forward_i420(self, name, bits, frame1, frame2, height, width, out, siting, matrix, colour_range):
        from .colour import colour_flags, i420_frame_bytes
        dtype, kind = (torch.uint16, "4:2:0 10-bit") if bits == 10 else (torch.uint8, "I420")
        flags = colour_flags(siting, matrix, colour_range, bits=bits)
        self._need_rgb(name)
        h, w = int(height), int(width)
        fs = i420_frame_bytes(h, w)   # samples per packed 4:2:0 frame, at either depth
        return self._forward_frames(
            name, f"packed {kind} frames", dtype, frame1, frame2, h, w, fs, fs, True, out, bits == 10,
            lambda ctx, f1, f2, o, prec, ws: ctx.forward_yuv420(f1, f2, o, h, w, flags, prec, ws, bits), copy=bits == 8)

    def _forward_surface(self, name, bits, frame1, frame2, height, width, layout, out, out_layout, siting, matrix,
                         colour_range):
        from .colour import colour_flags, resolve_layout
        dtype, kind = (torch.uint16, "P010") if bits == 10 else (torch.uint8, "NV12")
        flags = colour_flags("mpeg2" if siting is None else siting, matrix, colour_range, bits=bits)
        self._need_rgb(name)
        h, w = int(height), int(width)
        lay = resolve_layout(layout, h, w)
        olay = resolve_layout(out_layout, h, w)
        return self._forward_frames(
            name, f"{kind} surfaces", dtype, frame1, frame2, h, w, lay.frame_stride, olay.frame_stride,
            olay == resolve_layout(None, h, w), out, bits == 10,
            lambda ctx, f1, f2, o, prec, ws: ctx.forward_surface(f1, f2, lay, o, olay, h, w, flags, prec, ws, bits))

    def _need_rgb(self, name):
        if self.frame_channels != 3:
            raise RuntimeError(f"{name} runs the RGB network (frame_channels=3); this model is grayscale")

    def _forward_frames(self, name, what, dtype, frame1, frame2, h, w, fs, out_fs, tight_out, out, p10, call, copy=False):
        """The body every frame-format forward shares, behind the public method's own pre-checks: two [B, fs] tensors of
        `dtype` (fs: the input layout's frame stride; `what`: the message's words for the frames) -> `out` [B, out_fs], new
        unless given, through one native call `call(ctx, frame1, frame2, out, prec, ws)`.  tight_out: the output layout
        leaves no sample unwritten.  copy: make non-contiguous frames contiguous instead of refusing them."""
        if (not isinstance(frame1, torch.Tensor) or not isinstance(frame2, torch.Tensor) or frame1.dim() != 2
                or frame1.shape != frame2.shape or frame1.shape[1] != fs):
            raise RuntimeError(f"expected two [B,{fs}] tensors ({what} of {h}x{w}) of equal shape, got "
                               f"{tuple(getattr(frame1, 'shape', ()))} and {tuple(getattr(frame2, 'shape', ()))}")
        self._check_device_mode_dtype(frame1, frame2, (dtype,))
        if copy:
            frame1, frame2 = frame1.contiguous(), frame2.contiguous()
        elif not frame1.is_contiguous() or not frame2.is_contiguous():
            raise ValueError(f"{name} takes contiguous frames")
        b = frame1.shape[0]
        prec = self._precision_code()
        ctx = self._context(frame1.device)
        ws = self._workspace(ctx, frame1.device, b, h, w, prec, yuv=True, p10=p10)
        shape = (b, out_fs)
        if out is None:
            # (a pitched frame has samples no pixel covers: they are never written, so a new one starts as zeros)
            out = (torch.empty if tight_out else torch.zeros)(shape, dtype=dtype, device=frame1.device)
        elif (out.dtype != dtype or tuple(out.shape) != shape or out.device != frame1.device
              or out.stride(1) != 1 or (b > 1 and out.stride(0) < out_fs)):
            raise ValueError(f"out must be a {str(dtype).split('.')[-1]} {shape} tensor on {frame1.device} whose "
                             "frames are contiguous")
        with torch.cuda.device(frame1.device):
            call(ctx, frame1, frame2, out, prec, ws)
        return out

    @torch.no_grad()
    def forward_nv12(self, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, *, layout=None,
                     out: torch.Tensor | None = None, out_layout=None, siting: str | None = None,
                     matrix: str = "bt709", colour_range: str = "limited") -> torch.Tensor:
        """The RGB network on decoder surfaces: uint8 NV12 frames in (the Y plane, then interleaved U,V pairs; what a
        hardware decoder leaves in device memory) -> uint8 NV12 interpolated frames, `fiunet_forward_nv12`: bit for
        bit `forward_yuv420` on the same samples, only their place in memory differs.  layout /
        out_layout: a `colour.SurfaceLayout` (pitches, chroma offset and frame stride in samples) or None for tight
        frames; the tensors are [B, frame_stride], [B, F] when tight.  siting None means "mpeg2", which is what
        decoders produce.  `out`: write there - frames contiguous, possibly further apart; samples outside the used
        columns and between the planes are left untouched."""
        return self._forward_surface("forward_nv12", 8, frame1, frame2, height, width, layout, out, out_layout, siting,
                                     matrix, colour_range)

    @torch.no_grad()
    def forward_p010(self, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, *, layout=None,
                     out: torch.Tensor | None = None, out_layout=None, siting: str | None = None,
                     matrix: str = "bt709", colour_range: str = "limited") -> torch.Tensor:
        """`forward_nv12` on 10-bit surfaces: uint16 P010 frames (a word is code << 6: read as word >> 6, written with
        the low six bits zero), `fiunet_forward_p010`: bit for bit `forward_yuv420p10` on the same codes.  matrix also
        takes "bt2020"; siting None means "mpeg2", which is what decoders produce.  Use fp16 (or bf16x2, fp32): bf16
        is about 5 codes off."""
        return self._forward_surface("forward_p010", 10, frame1, frame2, height, width, layout, out, out_layout, siting,
                                     matrix, colour_range)

    @torch.no_grad()
    def forward_rgb_packed(self, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, *,
                           format: str = "rgb24", layout=None, out: torch.Tensor | None = None,
                           out_layout=None) -> torch.Tensor:
        """The RGB network on packed RGB frames: uint8 "rgb24" / "bgr24" / "rgba" / "bgra" frames in (interleaved pixels:
        raw video, screen grabs, renders, `cv2.imread` images) -> interpolated frames of the same format,
        `fiunet_forward_rgb_packed`: bit for bit `packed.packed_to_rgb` on both -> `forward_u8` ->
        `packed.rgb_to_packed(alpha_from=(frame1, frame2))`, with no colour conversion at all.  The alpha
        of rgba / bgra does not go through the network: the result's is the rounded average of the inputs'.  layout /
        out_layout: a `packed.PackedLayout` (row pitch and frame stride in bytes) or None for tight frames; the tensors
        are [B, frame_stride], [B, H*W*bpp] when tight.  `out`: write there - frames contiguous, possibly further apart;
        bytes outside the used columns and between frames are left untouched."""
        from .packed import FORMATS, resolve_layout
        if format not in FORMATS:
            raise ValueError(f"format must be one of {list(FORMATS)}, got {format!r}")
        code = FORMATS[format][0]
        self._need_rgb("forward_rgb_packed")
        h, w = int(height), int(width)
        lay = resolve_layout(layout, format, h, w)
        olay = resolve_layout(out_layout, format, h, w)
        return self._forward_frames(
            "forward_rgb_packed", f"packed {format} frames", torch.uint8, frame1, frame2, h, w, lay.frame_stride,
            olay.frame_stride, olay == resolve_layout(None, format, h, w), out, False,
            lambda ctx, f1, f2, o, prec, ws: ctx.forward_rgb_packed(f1, f2, lay, o, olay, h, w, code, prec, ws))

    @torch.no_grad()
    def forward_yuv(self, frame1: torch.Tensor, frame2: torch.Tensor, height: int, width: int, *, format: str,
                    siting: str | None = None, matrix: str = "bt709", colour_range: str = "limited", layout=None,
                    out_layout=None, out: torch.Tensor | None = None) -> torch.Tensor:
        """The RGB network on 4:2:2 / 4:4:4 video: frames of `format` in (a `colour.YUV_FORMATS` name - "yuv422p",
        "yuv444p", "yuv422p10le", "yuv444p10le", "uyvy422", "yuyv422"; uint8 at 8 bits, uint16 words of 10-bit codes at
        10) -> interpolated frames of the same format, `fiunet_forward_yuv` / `fiunet_forward_yuv_p10`: bit for bit
        `colour.yuv_to_rgb` on both -> `forward_u8` / `forward_p10` -> `colour.rgb_to_yuv`.  siting None
        means "mpeg2" (what decoders and ffmpeg assume for 4:2:2; 4:4:4 has none); matrix also takes "bt2020" at 10
        bits.  layout / out_layout: a `packed.PackedLayout` in samples or None for tight frames (uyvy422 / yuyv422: row
        pitch and frame stride of a capture buffer; planar formats: a frame stride only); the tensors are [B,
        frame_stride].  `out`: write there - frames contiguous, possibly further apart; bytes outside the used columns
        and between frames are left untouched.  Use fp16 (or bf16x2, fp32) for the 10-bit formats: bf16 is about 5
        codes off."""
        from .colour import YUV_FORMATS, resolve_yuv_layout, yuv_flags
        if format not in YUV_FORMATS:
            raise ValueError(f"format must be one of {list(YUV_FORMATS)}, got {format!r}")
        code, bits, _ = YUV_FORMATS[format]
        dtype = torch.uint16 if bits == 10 else torch.uint8
        h, w = int(height), int(width)
        lay = resolve_yuv_layout(layout, format, h, w)
        olay = resolve_yuv_layout(out_layout, format, h, w)
        flags = yuv_flags(format, siting, matrix, colour_range)
        self._need_rgb("forward_yuv")
        return self._forward_frames(
            "forward_yuv", f"{format} frames", dtype, frame1, frame2, h, w, lay.frame_stride, olay.frame_stride,
            olay == resolve_yuv_layout(None, format, h, w), out, bits == 10,
            lambda ctx, f1, f2, o, prec, ws: ctx.forward_yuv(f1, f2, code, lay, o, olay, h, w, flags, prec, ws, bits))

    @contextlib.contextmanager
    def debug_taps(self, frame1, frame2, strip=None):
        """Parity-test hook: run one forward keeping every stage (strip=(y_origin, image_height): `forward_strip`) and
        yield (read, output) while the workspace still holds it.  read(tap) -> the fp32 NCHW tensor of tap 0..17 (the 18
        conv stages) or 18..21 (the upsampled + padded halves of up1..up4), on the device, so that a caller can cut what it
        needs there before copying; None for an upsampled half that is not stored in this configuration.  No other
        forward of this model may run inside the block."""
        saved = self._options
        self._options = saved | _native.OPT_KEEP_ALL
        self._ctx_or_none_set_options()
        try:
            with torch.no_grad():
                out = self.forward(frame1, frame2) if strip is None else self.forward_strip(frame1, frame2, *strip)
            b, _, h, w = frame1.shape
            prec = self._precision_code()

            def read(tap):
                try:
                    return self._ctx.read_activation(self._ws, b, h, w, prec, tap)
                except _native.NativeError as e:
                    if tap < 18 or e.status != _native.ERR_UNSUPPORTED:   # (unsupported = not stored in this configuration)
                        raise
                    return None
            yield read, out
        finally:
            self._options = saved
            self._ctx_or_none_set_options()

    def debug_activations(self, frame1, frame2, taps=None, with_up=False):
        """Parity-test hook: run one forward keeping every stage and return
        ({tap name: fp32 NCHW tensor}, output).  with_up: also the four upsampled + padded halves
        (`unet.up{k}.up`, as F.pad leaves them: unet.py:47-53) where they are stored - always with the
        ConvTranspose2d decoder and in precision "bf16x2"; a stage that interpolates inside its gather is skipped."""
        with self.debug_taps(frame1, frame2) as (read, out):
            acts = {TAP_NAMES[t]: read(t) for t in (range(18) if taps is None else taps)}
            for k in (range(4) if with_up else ()):
                up = read(18 + k)
                if up is not None:
                    acts[UP_TAP_NAMES[k]] = up
        return acts, out


class GraphedForward:
    """One forward of a fixed [B,C,H,W] shape captured into a HIP graph (torch.cuda.CUDAGraph):
    the ~20-25 kernel launches of a forward replay as one graph launch, which matters for the
    reference's own workload (a single 256x256 pair is launch-bound).  `fiunet_forward` neither
    allocates nor synchronises, so it captures as is.  Call with tensors of the captured shape;
    the returned tensor is the graph's static output buffer (clone it to keep it).

    The graph holds raw device pointers, so this object OWNS every buffer it captured: its own
    input/output tensors and its own workspace (never the model's cached one, which a later eager
    call of another shape may free).  The prepared weights belong to the model's HIP context and are
    re-uploaded (freed + reallocated) whenever the parameters change; `__call__` compares the
    model's upload generation, precision and context with the ones captured and transparently
    re-captures when they differ, so a replay never reads freed memory."""

    def __init__(self, model: "FrameInterpolationUNet", batch: int, height: int, width: int):
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("move the model to the GPU before capturing a graph")
        c = model.frame_channels
        self.model = model
        self.f1 = torch.zeros(batch, c, height, width, device=dev)
        self.f2 = torch.zeros(batch, c, height, width, device=dev)
        self.out = torch.empty_like(self.f1)
        self.ws = None
        self.captures = 0
        self._capture()

    def _capture(self):
        model, dev = self.model, self.f1.device
        model._check_pair(self.f1, self.f2, (torch.float32,))
        b, _, h, w = self.f1.shape
        ctx = model._context(dev)              # uploads the weights if they are stale
        prec = model._precision_code()
        nbytes = ctx.workspace_bytes(b, h, w, prec)
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self._ctx, self._gen, self._prec = ctx, model._weights_gen, model.precision
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side), torch.cuda.device(dev):  # warm-up: LDS attributes, lazy init
            for _ in range(2):
                ctx.forward(self.f1, self.f2, self.out, prec, self.ws)
        torch.cuda.current_stream(dev).wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.device(dev), torch.cuda.graph(self.graph):
            ctx.forward(self.f1, self.f2, self.out, prec, self.ws)
        self.captures += 1

    def _stale(self) -> bool:
        m = self.model
        return (m._ctx is not self._ctx or m._ctx_dirty or m.precision != self._prec or m.weight_prep != m._prep_loaded
                or m._weights_gen != self._gen or m._current_fingerprint() != m._fingerprint)

    def __call__(self, frame1: torch.Tensor, frame2: torch.Tensor) -> torch.Tensor:
        if self._stale():
            self._capture()
        self.f1.copy_(frame1)
        self.f2.copy_(frame2)
        self.graph.replay()
        return self.out


def count_parameters(model: nn.Module) -> int:
    """unet.py:114-116."""
    return sum(p.numel() for p in model.parameters() if p.requires_grad)
