"""Host-side counterpart of the reference's model/inference.py hot-path helpers.

Same names, argument meaning and error behaviour as the reference functions they replace:
  preprocess_image   /root/reference/model/inference.py:11-41
  postprocess_image  /root/reference/model/inference.py:43-63
  load_model         /root/reference/model/inference.py:65-99
  interpolate_frames /root/reference/model/inference.py:101-122
  generate_multiple_intermediate_frames  inference.py:124-149
plus the `FrameInterpolator` class that the reference's main.py imports (main.py:100,122) but
never defines: `.interpolate_frames(img1, img2)` and
`.interpolate_video(input, output, factor)`.

The arithmetic of pre/post-processing and the network runs in HIP kernels; this file is
plumbing (file I/O, shapes, batching).  One loop (`_sequence`) is behind the five `interpolate_sequence*` functions;
the video routes live in stream.py alone, and `FrameInterpolator.interpolate_video` checks its arguments and dispatches
into them (`chunk_frames=None`, the resident call, is the whole clip as one chunk).  No cv2/imageio in this image: image files go through cv2 if
it happens to be importable, else through imageio_lite (PNG, BMP, PGM/PPM, `.npy`; cv2.resize's
fixed-point INTER_LINEAR restated); videos are raw `.npy` frame stacks [N,H,W] / [N,H,W,3] uint8.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from struct import error as struct_error
from zlib import error as zlib_error

from . import _native, imageio_lite, scene
from .unet import FrameInterpolationUNet


def _read_gray(path: str) -> np.ndarray:
    """cv2.imread(path, cv2.IMREAD_GRAYSCALE) (inference.py:23): OpenCV when it is installed, else the
    readers of imageio_lite (PNG, BMP, PGM/PPM, .npy).  None when the file cannot be decoded."""
    img = None
    # formats OpenCV does not know (.npy frames are what save_frames and the serving path write) never go
    # through it; for everything else a None from cv2.imread falls through to the built-in readers
    if not str(path).lower().endswith(".npy"):
        try:
            import cv2  # type: ignore
            img = cv2.imread(path, cv2.IMREAD_GRAYSCALE)
        except ImportError:
            pass
    if img is not None:
        return img
    try:
        return imageio_lite.read_gray(path)
    except (ValueError, KeyError, struct_error, zlib_error, OSError):
        return None


def _resize_linear_u8(img: np.ndarray, target_size) -> np.ndarray:
    """cv2.resize(img, (W, H)) (inference.py:29, default INTER_LINEAR): OpenCV when installed, else its
    fixed-point algorithm restated in imageio_lite.  Host glue, not part of the device hot path."""
    try:
        import cv2  # type: ignore
        return cv2.resize(img, (int(target_size[0]), int(target_size[1])))
    except ImportError:
        return imageio_lite.resize_linear_u8(img, target_size)


def preprocess_image(image_path, target_size=(256, 256)):
    """Gray read -> resize to target_size (width, height) -> /255 -> 2x-1 -> [1,1,H,W] fp32.

    Accepts a path (reference behaviour, inference.py:23) or an already decoded uint8 array.
    Raises ValueError("Could not read image from ...") like inference.py:25-26."""
    if isinstance(image_path, np.ndarray):
        image = image_path
    else:
        image = _read_gray(image_path) if os.path.exists(str(image_path)) else None
        if image is None:
            raise ValueError(f"Could not read image from {image_path}")
    if target_size is not None:
        image = _resize_linear_u8(image, target_size)
    image = image.astype(np.float32) / 255.0
    image = 2.0 * image - 1.0
    return torch.from_numpy(image).unsqueeze(0).unsqueeze(0)


def postprocess_image(tensor: torch.Tensor) -> np.ndarray:
    """[-1,1] fp32 tensor -> uint8 image: (x+1)/2, clamp [0,1], *255, truncating cast
    (inference.py:54-61).  Runs the HIP post-processing kernel; the tensor must be on the GPU
    (interpolate_frames returns it there)."""
    if not tensor.is_cuda:
        raise RuntimeError("postprocess_image (MI355X build) expects the device tensor that "
                           "interpolate_frames returned; there is no CPU fallback")
    t = tensor.detach().to(torch.float32).contiguous()
    return _native.postprocess_u8(t).squeeze().cpu().numpy()


def load_model(model_path, device, precision=None, frame_channels=1, weight_prep=None):
    """Construct bilinear=True, load `{'model_state_dict': ...}` or a bare state-dict, move to
    device, eval (inference.py:77-97).  FileNotFoundError if the file is missing (:80-81).  weight_prep: "host" /
    "device" / None = the default (FrameInterpolationUNet)."""
    model = FrameInterpolationUNet(bilinear=True, frame_channels=frame_channels, precision=precision,
                                   weight_prep=weight_prep)
    if not os.path.exists(model_path):
        raise FileNotFoundError(f"Model file not found: {model_path}")
    checkpoint = torch.load(model_path, map_location="cpu")
    if "model_state_dict" in checkpoint:
        model.load_state_dict(checkpoint["model_state_dict"])
        print(f"Model loaded from {model_path}")
        print(f"Trained for {checkpoint.get('epoch', 'Unknown')} epochs")
        val = checkpoint.get("val_loss", "Unknown")
        print(f"Best validation loss: {val:.6f}" if isinstance(val, float) else
              f"Best validation loss: {val}")
    else:
        model.load_state_dict(checkpoint)
        print(f"Model state dict loaded from {model_path}")
    model = model.to(device)
    model.eval()
    return model


def interpolate_frames(model, frame1, frame2, device):
    """inference.py:115-120: move to device, no_grad, model(frame1, frame2)."""
    frame1 = frame1.to(device)
    frame2 = frame2.to(device)
    with torch.no_grad():
        return model(frame1, frame2)


def generate_multiple_intermediate_frames(model, frame1, frame2, num_intermediate, device):
    """inference.py:124-149: the reference runs the SAME pair N times (the network has no time
    input), so all N frames are identical; one forward is enough."""
    frame = interpolate_frames(model, frame1, frame2, device)
    return [frame for _ in range(num_intermediate)]


def _pair_batches(n_pairs: int, batch: int):
    for s in range(0, n_pairs, batch):
        yield s, min(batch, n_pairs - s)


def _forward_u8_chunk(model, a: torch.Tensor, b: torch.Tensor, batch: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """forward_u8 of one chunk of a sequence.  Below 1080p some layers of a forward have fewer workgroups
    than the chip has CUs and cut their K loop over several (split-K, fiunet.hip); how many depends on the
    batch (at 720p batches of fewer than five pairs still split the deepest level), so the fp32 summation
    order - hence a pixel sitting on a uint8 truncation boundary - of a pair may depend on how many pairs
    share its call.  A ragged chunk - the last one of a sequence, and the only one of a sequence shorter than
    a batch - is therefore padded (its last pair repeated, the extra outputs dropped) up to the smallest batch
    at which no layer splits (`model.batch_invariant_from`, the library's own rule: 1 from 1080p up, 5 at 720p),
    or to the full `batch` where even that still splits (256x256 at batch 8): every pair of a sequence is
    computed exactly as in a full batch, the result does not depend on the sequence length or on how the
    sequence is sharded over ranks (`sequence_pair_fn`) - and a one-pair 720p clip costs 5 forwards, not 8."""
    return _padded_chunk(model, model.forward_u8, a, b, a.shape[-2], a.shape[-1], batch, out)


def _padded_chunk(model, fwd, a: torch.Tensor, b: torch.Tensor, h: int, w: int, batch: int,
                  out: torch.Tensor | None = None) -> torch.Tensor:
    """`fwd(a, b, out=...)` of one chunk of pairs of h x w frames, a ragged chunk padded as `_forward_u8_chunk` says
    (the rule is shared by every frame layout: the frames are only ever indexed along dim 0 here)."""
    cnt = a.shape[0]
    target = cnt
    if cnt < batch:
        bmin = model.batch_invariant_from(h, w, a.device)
        target = batch if bmin > batch else max(cnt, bmin)
    if target > cnt:
        rep = [1] * a.dim()
        rep[0] = target - cnt
        a = torch.cat([a, a[-1:].repeat(*rep)])
        b = torch.cat([b, b[-1:].repeat(*rep)])
        res = fwd(a, b)[:cnt]
        if out is not None:
            out.copy_(res)
            return out
        return res
    # `out` (the video loops: every second frame of the interleaved result): the fused head stores each frame in place
    return fwd(a, b, out=out)


def sequence_pair_fn(model, batch: int = 8):
    """`pair_fn` for `video.interpolate_video_sharded`: uint8 `[b, H, W]` frame stacks in, uint8 middles out,
    through the same chunk helper as the single-process loops, so a rank's ragged sub-batches of small
    frames are padded to `batch` exactly as `interpolate_sequence` pads its own (use the same `batch` for
    both and the sharded result equals the single-process one bit for bit at every frame size)."""
    @torch.no_grad()
    def pair_fn(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        if a.dim() == 3:
            return _forward_u8_chunk(model, a.unsqueeze(1), b.unsqueeze(1), batch,
                                     None if out is None else out.unsqueeze(1)).squeeze(1)
        return _forward_u8_chunk(model, a, b, batch, out)
    pair_fn.accepts_out = True   # video.interpolate_video_sharded: the root's own middles go straight into the interleaved result
    return pair_fn


def _cut_flags(thr, stacks, bits):
    """Device uint8 flags of the cut intervals of the input frames (scene.detect_cuts), or None when scene_cut is off."""
    if thr is None:
        return None
    return scene.detect_cuts([p.contiguous() for p in stacks], thr, bits)[1]


def _hold(flags, factor, *videos):
    """scene.hold_cut_frames on each interleaved result (the planes of one video) when scene_cut is on."""
    if flags is not None:
        for v in videos:
            scene.hold_cut_frames(v, flags, factor)


# torch's uint16 is a dtype of limited support on the GPU (no guaranteed cat / repeat kernels): the 10-bit loops pad and
# interleave int16 views of their uint16 frames (same bits) and hand uint16 views to the model.
def _i16(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16)


def _u16(t: torch.Tensor | None) -> torch.Tensor | None:
    return None if t is None else t.view(torch.uint16)


def _sequence(model, fr: torch.Tensor, fwd, h: int, w: int, batch: int, thr, bits: int) -> torch.Tensor:
    """The one factor-2 loop behind every `interpolate_sequence*`: device frames [N, ...] of h x w pictures in the dtype
    the loop may cat / repeat (uint8; int16 words at 10 bits) -> [2N-1, ...] = F0, M0, F1, ..., F(N-1) in that dtype.  The
    originals are copied as they are; `fwd(a, b, out=)` writes each chunk's middles where they belong (no temporary, no
    strided copy), a ragged chunk padded as `_forward_u8_chunk` says; thr: a checked scene_cut threshold (None: off) -
    the middle of every interval scene.detect_cuts flags, over every sample of a frame, is a copy of the frame before."""
    flags = _cut_flags(thr, [fr], bits)
    n = fr.shape[0]
    out = torch.empty((2 * n - 1,) + tuple(fr.shape[1:]), dtype=fr.dtype, device=fr.device)
    out[0::2] = fr
    for s, cnt in _pair_batches(n - 1, batch):
        _padded_chunk(model, fwd, fr[s:s + cnt], fr[s + 1:s + cnt + 1], h, w, batch, out=out[2 * s + 1: 2 * (s + cnt): 2])
    _hold(flags, 2, out)
    return out


@torch.no_grad()
def interpolate_sequence(model, frames_u8: torch.Tensor, batch: int = 8, *, scene_cut: float | None = None) -> torch.Tensor:
    """factor-2 video loop on one GPU: device uint8 frames [N,H,W] (or [N,C,H,W]) ->
    [2N-1, ...] = F0, M0, F1, M1, ..., F(N-1), where Mi = model(Fi, Fi+1) through the fused
    uint8 path (pre/post-processing on device).  Semantics per SURVEY.md 8a row 11.
    scene_cut: None (off) or a threshold in (0, 100]: the middle of every interval scene.detect_cuts flags is a copy of
    Fi (scene.py); every other frame is unchanged."""
    thr = scene.check_threshold(scene_cut)
    squeeze = frames_u8.dim() == 3
    fr = frames_u8.unsqueeze(1) if squeeze else frames_u8
    out = _sequence(model, fr, model.forward_u8, fr.shape[-2], fr.shape[-1], batch, thr, 8)
    return out.squeeze(1) if squeeze else out


@torch.no_grad()
def interpolate_sequence_yuv420(model, frames: torch.Tensor, height: int, width: int, batch: int = 8, *,
                                scene_cut: float | None = None, **colour) -> torch.Tensor:
    """factor-2 video loop of the RGB network on colour video: device uint8 [N, F] packed I420 frames of
    height x width (a Y4M frame payload each) -> [2N-1, F] = F0, M0, F1, ..., F(N-1), where Mi =
    model.forward_yuv420(Fi, Fi+1, **colour).  The originals are copied byte for byte; each middle is written in
    place; a ragged last chunk is padded as in `interpolate_sequence`, so the result does not depend on N.
    colour: siting / matrix / colour_range (colour.py).  scene_cut: as for `interpolate_sequence`, on all three planes."""
    thr = scene.check_threshold(scene_cut)
    h, w = int(height), int(width)

    def fwd(a, b, out=None):
        return model.forward_yuv420(a, b, h, w, out=out, **colour)
    return _sequence(model, frames, fwd, h, w, batch, thr, 8)


@torch.no_grad()
def interpolate_sequence_nv12(model, frames: torch.Tensor, height: int, width: int, batch: int = 8, *,
                              scene_cut: float | None = None, **colour) -> torch.Tensor:
    """`interpolate_sequence_yuv420` on decoder frames: device uint8 [N, F] tight NV12 frames of height x width (the Y
    plane, then interleaved U,V pairs) -> [2N-1, F] = F0, M0, F1, ..., F(N-1), Mi = model.forward_nv12(Fi, Fi+1,
    **colour).  The same contract: originals byte for byte, middles written in place, a ragged last chunk padded.  A
    tight NV12 frame holds the samples of its I420 frame in another order, so the scene-cut flags - sums over every
    sample - are those of the I420 run.  colour: siting (None: "mpeg2") / matrix / colour_range."""
    thr = scene.check_threshold(scene_cut)
    h, w = int(height), int(width)

    def fwd(a, b, out=None):
        return model.forward_nv12(a.contiguous(), b.contiguous(), h, w, out=out, **colour)
    return _sequence(model, frames, fwd, h, w, batch, thr, 8)


@torch.no_grad()
def interpolate_sequence_rgb_packed(model, frames: torch.Tensor, height: int, width: int, format: str, batch: int = 8, *,
                                    scene_cut: float | None = None) -> torch.Tensor:
    """factor-2 video loop of the RGB network on packed RGB video: device uint8 [N, F] tight "rgb24" / "bgr24" / "rgba" /
    "bgra" frames of height x width (F = H*W*bpp) -> [2N-1, F] = F0, M0, F1, ..., F(N-1), Mi =
    model.forward_rgb_packed(Fi, Fi+1, format=format): no colour conversion anywhere.  The same contract as
    `interpolate_sequence_yuv420`: originals byte for byte, middles written in place, a ragged last chunk padded.  The
    scene-cut sums run over every byte of a frame: for rgb24 / bgr24 they are those of the same frames as planar RGB; for
    rgba / bgra they include the alpha byte (a quarter of the bytes; constant alpha adds nothing to a sum and lowers
    every percentage by a quarter)."""
    thr = scene.check_threshold(scene_cut)
    h, w = int(height), int(width)

    def fwd(a, b, out=None):
        return model.forward_rgb_packed(a.contiguous(), b.contiguous(), h, w, format=format, out=out)
    return _sequence(model, frames, fwd, h, w, batch, thr, 8)


@torch.no_grad()
def interpolate_sequence_yuv(model, frames: torch.Tensor, height: int, width: int, format: str, batch: int = 8, *,
                             scene_cut: float | None = None, **colour) -> torch.Tensor:
    """factor-2 video loop of the RGB network on 4:2:2 / 4:4:4 video: device [N, F] tight frames of `format` (a
    `colour.YUV_FORMATS` name; uint8 at 8 bits, uint16 at 10) of height x width -> [2N-1, F] = F0, M0, F1, ..., F(N-1), Mi
    = model.forward_yuv(Fi, Fi+1, format=format, **colour).  The same contract as `interpolate_sequence_yuv420`:
    originals sample for sample, middles written in place, a ragged last chunk padded.  The scene-cut sums run over every
    sample of a frame.  colour: siting (None: "mpeg2") / matrix / colour_range."""
    from .colour import YUV_FORMATS
    thr = scene.check_threshold(scene_cut)
    h, w = int(height), int(width)
    if format not in YUV_FORMATS:
        raise ValueError(f"format must be one of {list(YUV_FORMATS)}, got {format!r}")
    if YUV_FORMATS[format][1] == 10:
        def fwd10(a, b, out=None):
            return _i16(model.forward_yuv(_u16(a.contiguous()), _u16(b.contiguous()), h, w, format=format,
                                          out=_u16(out), **colour))
        return _u16(_sequence(model, _i16(frames), fwd10, h, w, batch, thr, 10))

    def fwd(a, b, out=None):
        return model.forward_yuv(a.contiguous(), b.contiguous(), h, w, format=format, out=out, **colour)
    return _sequence(model, frames, fwd, h, w, batch, thr, 8)


@torch.no_grad()
def interpolate_sequence_p10(model, frames: torch.Tensor, batch: int = 8, *, scene_cut: float | None = None) -> torch.Tensor:
    """factor-2 video loop on 10-bit frames: device uint16 [N,H,W] (or [N,C,H,W]) 10-bit codes -> [2N-1, ...] = F0, M0,
    F1, ..., F(N-1), where Mi = model.forward_p10(Fi, Fi+1).  Both networks.  The originals are copied sample for
    sample; each middle is written in place; a ragged last chunk is padded as in `interpolate_sequence`, so the result
    does not depend on N.  Use precision fp16 (or bf16x2, fp32) for 10-bit video: bf16 is about 5 codes off.
    scene_cut: as for `interpolate_sequence` (samples above 1023 read as 1023 by the detection)."""
    thr = scene.check_threshold(scene_cut)
    squeeze = frames.dim() == 3
    fr = frames.unsqueeze(1) if squeeze else frames
    _, _, h, w = fr.shape

    def fwd(a, b, out=None):
        return _i16(model.forward_p10(_u16(a), _u16(b), out=_u16(out)))
    out = _u16(_sequence(model, _i16(fr), fwd, h, w, batch, thr, 10))
    return out.squeeze(1) if squeeze else out


@torch.no_grad()
def interpolate_sequence_yuv420p10(model, frames: torch.Tensor, height: int, width: int, batch: int = 8, *,
                                   scene_cut: float | None = None, **colour) -> torch.Tensor:
    """`interpolate_sequence_yuv420` on 10-bit video: device uint16 [N, F] packed 4:2:0 10-bit frames (a C420p10 Y4M
    frame payload each) -> [2N-1, F], Mi = model.forward_yuv420p10(Fi, Fi+1, **colour).  The originals are copied
    sample for sample; the result does not depend on N.  colour: siting / matrix (also "bt2020") / colour_range.
    scene_cut: as for `interpolate_sequence`, on all three planes."""
    thr = scene.check_threshold(scene_cut)
    h, w = int(height), int(width)

    def fwd(a, b, out=None):
        return _i16(model.forward_yuv420p10(_u16(a), _u16(b), h, w, out=_u16(out), **colour))
    return _u16(_sequence(model, _i16(frames), fwd, h, w, batch, thr, 10))


@torch.no_grad()
def interpolate_sequence_host(model, frames_u8_cpu: torch.Tensor, batch: int = 8,
                              out: torch.Tensor | None = None) -> torch.Tensor:
    """factor-2 video loop for frames that live in HOST memory: uint8 [N,H,W] (CPU) -> uint8
    [2N-1,H,W] (CPU, pinned).  Chunks of `batch` pairs are double-buffered: while the GPU runs
    chunk i on the compute stream, chunk i+1 goes host->device and the results of chunk i-1 go
    device->host on a copy stream (pinned buffers, PCIe Gen5).  Same result as
    interpolate_sequence(model, frames.cuda()).cpu().  Pass a pinned `out` [2N-1,H,W] to reuse it
    across calls (pinning 1.6 GB for 400 1080p frames costs more than interpolating them)."""
    dev = next(model.parameters()).device
    n = frames_u8_cpu.shape[0]
    src = frames_u8_cpu if frames_u8_cpu.is_pinned() else frames_u8_cpu.contiguous().pin_memory()
    if out is None:
        out = torch.empty((2 * n - 1,) + tuple(src.shape[1:]), dtype=torch.uint8).pin_memory()
    compute, copy = torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)
    chunks = list(_pair_batches(n - 1, batch))
    dbuf, dmid, up_done, comp_done = {}, {}, {}, {}

    def upload(i):
        s, cnt = chunks[i]
        with torch.cuda.stream(copy):
            dbuf[i] = src[s:s + cnt + 1].to(dev, non_blocking=True).unsqueeze(1)
            up_done[i] = torch.cuda.Event(); up_done[i].record(copy)

    def download(i):
        s, cnt = chunks[i]
        with torch.cuda.stream(copy):
            copy.wait_event(comp_done[i])
            dmid[i].record_stream(copy)  # allocated on the compute stream, read by the copy stream
            for j in range(cnt):  # one contiguous 2-MB copy per frame (a strided view would be staged)
                out[2 * (s + j) + 1].copy_(dmid[i][j, 0], non_blocking=True)
        dbuf.pop(i, None)

    if chunks:
        upload(0)
    for i in range(len(chunks)):
        if i + 1 < len(chunks):
            upload(i + 1)
        compute.wait_event(up_done[i])
        fr = dbuf[i]
        dmid[i] = _forward_u8_chunk(model, fr[:-1], fr[1:], batch)
        comp_done[i] = torch.cuda.Event(); comp_done[i].record(compute)
        fr.record_stream(compute)
        download(i)
        if i >= 1:
            dmid.pop(i - 1, None)
    out[0::2] = src  # host-side interleave of the original frames, while the GPU is still busy
    copy.synchronize()
    torch.cuda.current_stream(dev).synchronize()
    return out


def _interleave_average_u8(planes: torch.Tensor) -> torch.Tensor:
    """[N, h, w] uint8 -> [2N-1, h, w]: the originals with the rounded average of each neighbouring pair
    in between (chroma of an inserted frame)."""
    n = planes.shape[0]
    out = torch.empty((2 * n - 1,) + tuple(planes.shape[1:]), dtype=torch.uint8, device=planes.device)
    out[0::2] = planes
    if n > 1:
        out[1::2] = ((planes[:-1].to(torch.int16) + planes[1:].to(torch.int16) + 1) >> 1).to(torch.uint8)
    return out


def _interleave_average_p10(planes: torch.Tensor) -> torch.Tensor:
    """`_interleave_average_u8` for 10-bit chroma: [N, h, w] int32 -> [2N-1, h, w] int32, the originals as they are and
    the rounded average of each neighbouring pair in between (samples above 1023 read as 1023)."""
    n = planes.shape[0]
    out = torch.empty((2 * n - 1,) + tuple(planes.shape[1:]), dtype=torch.int32, device=planes.device)
    out[0::2] = planes
    if n > 1:
        c = planes.clamp(max=1023)
        out[1::2] = (c[:-1] + c[1:] + 1) >> 1
    return out


class FrameInterpolator:
    """What main.py:95-129 expects from `model.inference` (it is missing in the reference).

    interpolate_frames(img1, img2): uint8 [H,W] (gray) or [H,W,3] images -> uint8 image of the
    same shape; colour images are processed per channel with the 2->1 grayscale network unless
    the checkpoint is the 6->3 variant.
    interpolate_video(input_path, output_path, factor=2): raw .npy frame stack or uncompressed
    YUV4MPEG2 (`.y4m`) video in/out (4:2:0 colour through the RGB network: `interpolate_sequence_yuv420`; 10-bit
    `C420p10` / `C422p10` / `C444p10` / `Cmono10` through `interpolate_sequence_p10` (gray) or
    `interpolate_sequence_yuv420p10` (RGB, 4:2:0 only)); factor must be a power of two (recursive bisection; factor 2
    is the only semantics the reference's flags imply, main.py:57-62)."""

    def __init__(self, model_path=None, device="cuda", precision=None, model=None, batch=8):
        self.device = torch.device("cuda" if device in ("auto", None) else device)
        self.model = model if model is not None else load_model(model_path, self.device, precision)
        self.batch = batch

    def _as_planes(self, img: np.ndarray) -> torch.Tensor:
        t = torch.from_numpy(np.ascontiguousarray(img)).to(self.device)
        if t.dim() == 2:
            return t[None, None]
        planes = t.permute(2, 0, 1)  # [C,H,W]
        return planes[None] if self.model.frame_channels == planes.shape[0] else planes[:, None]

    def interpolate_frames(self, img1: np.ndarray, img2: np.ndarray) -> np.ndarray:
        if img1.shape != img2.shape or img1.dtype != np.uint8:
            raise ValueError("expected two uint8 images of equal shape")
        a, b = self._as_planes(img1), self._as_planes(img2)
        o = self.model.forward_u8(a, b)
        if img1.ndim == 2:
            return o[0, 0].cpu().numpy()
        o = o[0] if self.model.frame_channels == img1.shape[2] else o[:, 0]
        return o.permute(1, 2, 0).contiguous().cpu().numpy()

    def interpolate_video(self, input_path, output_path, factor=2, *, matrix="bt709", siting=None, scene_cut=None,
                          chunk_frames=None, fps=None, src_fps=None, time_depth=2, retime="blend", raw=None,
                          width=None, height=None, dedup=None, max_gap=4, dedup_log=None, scene_log=None, resize=None,
                          resize_filter="linear", packing=None, chroma="average", chroma_log=None, shutter=None):
        """matrix: the YUV matrix of colour Y4M video through the RGB network ("bt709" by convention for HD video,
        "bt601", or for 10-bit video "bt2020", the matrix of HDR10 / HLG content; the container does not carry it).
        siting: the chroma siting of colour Y4M video through the RGB network, "jpeg" or "mpeg2"; None takes it from the
        tag (8-bit: C420jpeg / C420 -> "jpeg", C420mpeg2 -> "mpeg2"; 10-bit: C420p10 does not carry it -> "mpeg2",
        what HEVC, AV1 and H.264 decoders give).  The grayscale network's Y4M path uses neither.  10-bit video keeps
        10 bits end to end; run it in precision fp16 (or bf16x2, fp32): bf16 is about 5 codes off.
        scene_cut: None (off) or a threshold in (0, 100].  Cuts are detected once on the input frames, over every
        sample as stored (all planes, all channels; scene.py), and every frame inserted into a cut
        interval - factor - 1 of them, chroma included - is a byte copy of the frame before the cut.  10 separates
        a hard cut from ordinary motion.
        chunk_frames: None holds the whole clip (host and device) as one chunk; an int streams it `chunk_frames` pairs
        at a time in memory bounded by the chunk (the same routes: stream.py), with a byte-identical
        result.  The input may also be a readable binary file object (Y4M: a pipe) and the output a writable one (Y4M).
        A path output is written as `<output>.part` and renamed on success.  Output naming: `.npy` is a stack of the
        luma frames (grayscale network), anything else Y4M; a whole-clip Y4M call (no chunk_frames, no fps) keeps its
        older rule - whatever does not end in `.y4m` is a `.npy` stack, `.npy` appended where the name lacks it.
        fps: None, or the frame rate of the output, above the source's: an int, a Fraction, an (n, d) pair or an "n/d"
        string such as "60000/1001" (no floats: 59.94 is not 60000/1001).  `factor` then stays 2; every route builds
        the frames of a 2**time_depth bisection (time_depth 1..4; what factor = 2**time_depth computes, cut holds
        included) and resamples them on the device to the times j x source rate / fps (retime.py):
        retime "blend" weighs the two bisection frames around each time, "nearest" takes the closer one, "motion"
        warps both along the optical flow between them to the frame's own time (no double edges where
        things move, one Farneback flow per pair of bisection frames; it loses a few dB on sub-pixel motion and where
        the flow fails, so "blend" stays the default); no frame blends or warps across a flagged cut.  The Y4M header carries fps reduced.  src_fps: the source rate, required for
        .npy input; for Y4M it overrides the header's.
        raw: None, or "nv12": input and output are headerless tight NV12 frames of `height` x `width` (files, or file
        objects: pipes), what `ffmpeg -f rawvideo -pix_fmt nv12` reads and writes and what a hardware decoder's
        surfaces hold; they go through the RGB network on the device without a repack (`interpolate_sequence_nv12`,
        stream.interpolate_raw_stream).  width, height and src_fps are then required (the stream has no
        header); siting None means "mpeg2", the range is limited; factor, fps, scene_cut and chunk_frames work as for
        Y4M.  raw "rgb24", "bgr24", "rgba" or "bgra": headerless tight packed RGB frames (`ffmpeg -f rawvideo -pix_fmt
        rgb24`), through the RGB network with their colour as it is (`interpolate_sequence_rgb_packed`):
        matrix and siting are not used; the alpha of an inserted rgba / bgra frame is the rounded average of its
        neighbours', and scene_cut then counts the alpha bytes too.  raw "yuv422p", "yuv444p", "yuv422p10le",
        "yuv444p10le", "uyvy422" or "yuyv422": headerless tight 4:2:2 / 4:4:4 frames (`ffmpeg -f rawvideo -pix_fmt
        yuv422p10le`: ProRes / DNxHR decodes, capture cards), through the RGB network at their own chroma resolution
        (`interpolate_sequence_yuv`): matrix and siting apply as for nv12 (siting None: "mpeg2"; bt2020
        at 10 bits), the range is limited; run the 10-bit formats in precision fp16.  Y4M tagged C422 / C444 is still
        refused by the RGB network: such clips take this raw route.
        dedup: None, or a tolerance >= 0 in code values: re-time repeated frames (telecined film, animation on twos and
        threes, a stalled capture; retime.py).  An interval whose frames differ by at most `dedup` per
        sample on average over every aligned 64-sample segment (0: equal frames) is dead; a run of dead intervals and
        the live one after it, max_gap frames at most (2..8), is covered evenly by the motion of that live interval,
        taken from its bisection frames and blended as `retime` says.  A longer hold (a title card), a run before a
        flagged cut and a run at the clip's end stay as they are.  Works with `factor` (at most 16) and with `fps`; the
        frame count does not change.  Costs one small device-to-host read per chunk.
        dedup_log: None, or a list that receives one (peaks, dead) pair of host arrays per chunk, over the chunk's own
        intervals (a resident run: one pair, the whole clip's); concatenated they are `scene.pair_peak` of the clip and
        its dead flags.  scene_log: the same for `scene_cut`: one (scores float64, flags uint8) pair per chunk, what the
        stream routes' `scene_log` has always received (it costs one more device-to-host read per chunk); from the
        two logs `retime.dedup_spans` gives the spans a run re-timed, which is how the command line counts them.
        resize: None, or (width, height) / "WxH": every frame is resized on the device right after its upload, with the
        bilinear filter of `preprocess_image` (resize.py, DESIGN.md 3.3q: each plane on its own grid, chroma at the size
        the format gives at the new size, no siting offset; a large down-scale aliases as the reference's does), before
        scene cuts, dedup and the first forward.  The route and its refusals are those of the new size, the output has
        the new size (the Y4M header says so); width / height stay the size of a raw source.  The result is, byte for
        byte, what the same call without `resize` writes for the clip resized beforehand, for every chunk_frames.
        resize_filter: "linear", or "area" for an alias-free down-scale (every destination sample is the
        exact rounded mean of the source area it covers; refused where a plane would grow on either axis or shrink more
        than 64 times).  Anything but "linear" is an error without `resize`.
        packing: None, or with raw="yuv422p10le" one of "v210", "y210le", "p210le" (wire10.py): the
        samples are yuv422p10le's, packed on the wire as 10-bit capture cards and uncompressed broadcast files carry
        them (`ffmpeg -c:v v210 -f rawvideo`).  Input and output are tight frames of that packing; each chunk is unpacked
        on the device after its upload and packed before its download, everything between is the yuv422p10le route, and
        the output is that route's output packed, byte for byte.  An error with any other raw, with Y4M and with .npy.
        chroma: how colour Y4M video through the GRAYSCALE network gets the chroma of an inserted frame (chroma.py,
        DESIGN.md 3.3u).  "average": the rounded average of its neighbours' (what this call has always written).
        "motion": carried along the motion - 8x8 luma block by block, the chroma planes are warped along the optical flow
        between the two neighbours where the network's own luma for the frame agrees with that flow, and averaged
        elsewhere, so a coloured object that moves keeps its colour in place instead of a double exposure.  The luma of
        every frame and the source frames are unchanged; works with factor, fps, retime, scene_cut, dedup, resize and
        chunk_frames, 8 and 10 bits, 4:2:0, 4:2:2 and 4:4:4; a mono stream has no chroma and is unchanged.  Costs one
        Farneback flow per inserted frame.  "motion" is refused by name for an RGB model, .npy input and every raw=
        route: none of them has separate chroma planes.  chroma_log: None, or a list that receives one (warped blocks,
        blocks) pair after a "motion" run.
        shutter: None, or an exact rational in [0, 1] (an int, a Fraction, an (n, d) pair or an "n/d" string; no floats):
        conversion to ANY frame rate, a lower one included, with a synthesized shutter (retime.py).  `fps`
        is then required and may be at, below or above the source rate (60 -> 24, 60000/1001 -> 50, 30 -> 25).  Point
        sampling a lower rate strobes, since every frame keeps the source's short exposure; so each output frame is the
        mean of the clip - the bisection frames and the straight lines between them - over the time a shutter that is
        open for `shutter` of the OUTPUT frame period would expose it, from the frame's own time on (1/2: 180 degrees).
        No exposure crosses a flagged cut or the clip's end.  shutter=0 is point sampling, with every `retime`; above 0
        `retime` must be "blend".  Works on every route, with scene_cut, resize and every chunk_frames (byte-identical);
        refused with dedup; a window of more than 8 source intervals or 48 bisection frames is refused with the remedy
        (a lower time_depth or shutter).  A streamed chunk reads ceil(shutter x source rate / fps) frames ahead."""
        from . import chroma as _chroma
        _chroma.check_mode(chroma)
        thr = scene.check_threshold(scene_cut)
        if factor < 2 or factor & (factor - 1):
            raise ValueError("factor must be a power of two (the network has no time input)")
        from . import stream
        run = dict(batch=self.batch, chunk_frames=chunk_frames, scene_cut=thr, fps=fps, src_fps=src_fps,
                   time_depth=time_depth, retime=retime, dedup=dedup, max_gap=max_gap, dedup_log=dedup_log,
                   scene_log=scene_log, resize=resize, resize_filter=resize_filter)
        if shutter is not None:   # (a new keyword: without it the call is what it always was)
            run["shutter"] = shutter
        from . import resize as _resize
        if resize is not None:
            _resize.check_size(resize)
        _resize.check_resize_filter(resize, resize_filter)
        if raw is not None:
            _chroma.refuse_motion(chroma, f"raw {raw} video")
            if packing is not None:   # (a new keyword beside raw: without it the call is what it always was)
                run["packing"] = packing
            return stream.interpolate_raw_stream(self.model, input_path, output_path, factor, raw=raw, width=width,
                                                 height=height, matrix=matrix, siting=siting, **run)
        stream.check_packing(packing, raw)   # (refuses: Y4M and .npy video take no packing)
        if width is not None or height is not None:
            raise ValueError("width and height describe raw video: pass raw=\"nv12\" with them")
        stream.check_retime(fps, src_fps, time_depth, retime, factor)
        stream.check_dedup(dedup, max_gap, fps, factor)
        stream.check_shutter(shutter, fps, retime, dedup)
        if chunk_frames is not None:
            stream.check_chunk_frames(chunk_frames)
        is_path = isinstance(input_path, (str, os.PathLike))
        if is_path and not os.path.exists(input_path):
            raise FileNotFoundError(f"Video file not found: {input_path}")
        if is_path and not str(input_path).lower().endswith(".y4m"):
            _chroma.refuse_motion(chroma, ".npy video")
            return stream.interpolate_npy_stream(self.model, input_path, output_path, factor, **run)
        if chunk_frames is None and fps is None and isinstance(output_path, (str, os.PathLike)):
            # the whole-clip call's older naming rule: whatever is not `.y4m` is a `.npy` stack, named as np.save names it
            name = os.fspath(output_path)
            if not name.lower().endswith(".y4m") and not name.endswith(".npy"):
                output_path = name + ".npy"
        if chroma != "average":   # (a new keyword: without it the call is what it always was)
            if self.model.frame_channels == 3:
                _chroma.refuse_motion(chroma, "the RGB network (its colour goes through the network itself)")
            run.update(chroma=chroma, chroma_log=chroma_log)
        return stream.interpolate_y4m_stream(self.model, input_path, output_path, factor, matrix=matrix, siting=siting,
                                             **run)
