"""ctypes binding of libfiunet_hip.so (C ABI declared in include/fiunet.h).

PyTorch is only the plumbing here: it owns device memory (caching allocator) and the HIP
stream; every arithmetic op of the forward runs in the hand-written HIP kernels behind this
ABI.  There is NO fallback: if the shared library is missing or a call fails, a RuntimeError
is raised (the reference raises RuntimeError from torch for bad shapes too).

`import torch` must happen before the library is loaded so that the process-wide HIP runtime
is the one PyTorch-ROCm ships (same SONAME libamdhip64.so.7); the library then shares
torch's device context, allocator pointers and streams.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import torch  # noqa: F401  (must precede CDLL: see module docstring)

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FIUNET_LIB") or os.path.join(_PKG, "libfiunet_hip.so")  # FIUNET_LIB: A/B builds
CSRC = os.path.join(_PKG, "csrc")

ABI_VERSION = 8        # include/fiunet.h FIUNET_ABI_VERSION this binding is written for
ABI_MIN_COMPAT = 4     # oldest A/B library (FIUNET_LIB) whose shared entry points have today's signatures
FP32, BF16, BF16X2, FP16 = 0, 1, 2, 3   # include/fiunet.h: enum fiunet_precision
OPT_UNFUSED, OPT_KEEP_ALL, OPT_GATHER_UPSAMPLE = 1, 2, 16
OPT_RNE_WEIGHTS, OPT_NO_DITHER = 32, 64
WEIGHT_PREPS = ("host", "device")   # Context.load_state_dict(prep=): fiunet_load_weights / fiunet_load_weights_device
YUV_MPEG2, YUV_BT709, YUV_FULL_RANGE, YUV_BT2020 = 1, 2, 4, 8   # include/fiunet.h: enum fiunet_colour

#: every symbol include/fiunet.h declares (tests/test_abi.py checks the header against this)
SYMBOLS = (
    "fiunet_abi_version", "fiunet_last_error_string", "fiunet_create", "fiunet_destroy",
    "fiunet_set_options", "fiunet_load_weights", "fiunet_load_weights_device", "fiunet_prepare_precision", "fiunet_workspace_bytes", "fiunet_forward",
    "fiunet_min_unsplit_batch",
    "fiunet_forward_strip",
    "fiunet_workspace_bytes_u8", "fiunet_forward_u8", "fiunet_forward_u8_strided", "fiunet_preprocess_u8",
    "fiunet_postprocess_u8", "fiunet_debug_read_activation", "fiunet_profile_enable",
    "fiunet_profile_read", "fiunet_metrics_workspace_bytes", "fiunet_psnr_u8", "fiunet_ssim_u8",
    "fiunet_ssim_gauss_workspace_bytes", "fiunet_ssim_gauss_f32",
    "fiunet_plane_metrics_workspace_bytes", "fiunet_plane_psnr", "fiunet_plane_ssim",
    "fiunet_interleaved_psnr", "fiunet_stepped_ssim",
    "fiunet_yuv420_to_rgb_u8", "fiunet_rgb_to_yuv420_u8", "fiunet_workspace_bytes_yuv420", "fiunet_forward_yuv420",
    "fiunet_preprocess_p10", "fiunet_postprocess_p10", "fiunet_workspace_bytes_p10", "fiunet_forward_p10",
    "fiunet_yuv420p10_to_rgb_p10", "fiunet_rgb_p10_to_yuv420p10", "fiunet_workspace_bytes_yuv420p10",
    "fiunet_forward_yuv420p10",
    "fiunet_pair_sad_u8", "fiunet_pair_sad_p10", "fiunet_scene_cuts", "fiunet_hold_cut_frames",
    "fiunet_retime_u8", "fiunet_retime_p10",
    # repeated frames in video
    "fiunet_pair_peak_u8", "fiunet_pair_peak_p10", "fiunet_retime_table_u8", "fiunet_retime_table_p10",
    # YUV 4:2:2 / 4:4:4 frames
    "fiunet_yuv_to_rgb_u8", "fiunet_rgb_to_yuv_u8", "fiunet_yuv_to_rgb_p10", "fiunet_rgb_p10_to_yuv",
    "fiunet_workspace_bytes_yuv", "fiunet_forward_yuv", "fiunet_forward_yuv_p10",
    # Farneback flow and flow-compensated warps
    "fiunet_flow_workspace_bytes", "fiunet_farneback_flow", "fiunet_flow_warp",
    # resizing frame planes
    "fiunet_resize_planes_u8", "fiunet_resize_planes_p10",
    # 10-bit 4:2:2 wire packings
    "fiunet_unpack_422p10", "fiunet_pack_422p10",
    # motion-compensated resampling
    "fiunet_warp_table_u8", "fiunet_warp_table_p10",
    # motion-guided chroma
    "fiunet_chroma_pick_u8", "fiunet_chroma_pick_p10", "fiunet_chroma_fill_u8", "fiunet_chroma_fill_p10",
    # deinterlacing
    "fiunet_deinterlace_u8", "fiunet_deinterlace_p10",
    # inverse telecine
    "fiunet_field_match_u8", "fiunet_field_match_p10", "fiunet_field_weave_u8", "fiunet_field_weave_p10",
    # a synthesized shutter for lower frame rates
    "fiunet_shutter_u8", "fiunet_shutter_p10",
    # (the packed RGB entry points stand before the surface ones: tests/test_nv12_host.py reads those off the tail)
    "fiunet_packed_to_rgb_u8", "fiunet_rgb_to_packed_u8", "fiunet_workspace_bytes_rgb_packed",
    "fiunet_forward_rgb_packed",
    "fiunet_nv12_to_rgb_u8", "fiunet_rgb_to_nv12_u8", "fiunet_workspace_bytes_nv12", "fiunet_forward_nv12",
    "fiunet_p010_to_rgb_p10", "fiunet_rgb_p10_to_p010", "fiunet_workspace_bytes_p010", "fiunet_forward_p010",
)


class SurfaceLayout(ctypes.Structure):
    """include/fiunet.h: fiunet_surface_layout (NV12 / P010 surfaces; every field in samples, 0 = tight)."""
    _fields_ = [("luma_pitch", ctypes.c_size_t), ("chroma_offset", ctypes.c_size_t),
                ("chroma_pitch", ctypes.c_size_t), ("frame_stride", ctypes.c_size_t)]


def _surface(layout, frame_stride: int):
    """A resolved colour.SurfaceLayout (or None: tight) with the frames `frame_stride` samples apart -> the C struct."""
    if layout is None:
        return ctypes.byref(SurfaceLayout(0, 0, 0, frame_stride))
    return ctypes.byref(SurfaceLayout(layout.luma_pitch, layout.chroma_offset, layout.chroma_pitch, frame_stride))



class RetimeEntry(ctypes.Structure):
    """include/fiunet.h: fiunet_retime_entry (output row = grid row `row`, blended with the row after it by wn / den)."""
    _fields_ = [("row", ctypes.c_uint32), ("wn", ctypes.c_uint32), ("den", ctypes.c_uint32)]


class WarpEntry(ctypes.Structure):
    """include/fiunet.h: fiunet_warp_entry (grid rows `row` and the one after, warped to wn / den along flow field `flow`;
    flag: an index into the device flags, or WARP_NO_FLAG)."""
    _fields_ = [("row", ctypes.c_uint32), ("wn", ctypes.c_uint32), ("den", ctypes.c_uint32), ("flow", ctypes.c_uint32),
                ("flag", ctypes.c_int32)]


WARP_NO_FLAG = -1   # include/fiunet.h: FIUNET_WARP_NO_FLAG


class ResizePlane(ctypes.Structure):
    """include/fiunet.h: fiunet_resize_plane (sample (y, x) of frame f at offset + f * frame_stride + y * pitch + x *
    step, everything in samples; filter: RESIZE_LINEAR / RESIZE_AREA in a destination plane, 0 in a source plane)."""
    _fields_ = [("offset", ctypes.c_size_t), ("pitch", ctypes.c_size_t), ("frame_stride", ctypes.c_size_t),
                ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("step", ctypes.c_int32), ("filter", ctypes.c_int32)]


RESIZE_LINEAR, RESIZE_AREA = 0, 1   # include/fiunet.h: fiunet_resize_filter


class PackedLayout(ctypes.Structure):
    """include/fiunet.h: fiunet_packed_layout (packed RGB frames; both fields in bytes, 0 = tight)."""
    _fields_ = [("row_pitch", ctypes.c_size_t), ("frame_stride", ctypes.c_size_t)]


def _packed(layout, frame_stride: int):
    """A resolved packed.PackedLayout with the frames `frame_stride` bytes apart -> the C struct."""
    return ctypes.byref(PackedLayout(layout.row_pitch, frame_stride))

_lib = None


def build_jobs(environ=None) -> int:
    """How many translation units `build` lets make compile at once: MAX_JOBS if set, else CMAKE_BUILD_PARALLEL_LEVEL if
    set, else 8; never above 16 (never the machine's CPU count: a shared machine grants a process far fewer)."""
    env = os.environ if environ is None else environ
    asked = env.get("MAX_JOBS") or env.get("CMAKE_BUILD_PARALLEL_LEVEL")
    return max(1, min(int(asked) if asked else 8, 16))


def build(force: bool = False) -> str:
    """Compile the HIP extension in-tree for gfx950 (hipcc cross-compiles without a GPU); force: from scratch, the
    library's objects included."""
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], capture_output=True, text=True)
        if os.path.exists(LIB_PATH):   # (FIUNET_LIB: not the Makefile's OUT)
            os.remove(LIB_PATH)
    res = subprocess.run(["make", "-C", CSRC, f"-j{build_jobs()}"], capture_output=True, text=True)
    if res.returncode != 0 or not os.path.exists(LIB_PATH):
        raise RuntimeError("building libfiunet_hip.so failed:\n" + res.stdout + res.stderr)
    return LIB_PATH


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the MI355X HIP extension has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C "
            f"{CSRC}`).  There is no CPU fallback for this path.")
    L = ctypes.CDLL(LIB_PATH)
    # the argument lists below are this ABI version's: a library of another version would take misaligned arguments
    # silently (v4 inserted a parameter into fiunet_debug_read_activation under the same symbol name)
    L.fiunet_abi_version.restype = ctypes.c_int
    ver = int(L.fiunet_abi_version())
    ab = bool(os.environ.get("FIUNET_LIB"))
    if ver != ABI_VERSION and not (ab and ABI_MIN_COMPAT <= ver < ABI_VERSION):
        raise RuntimeError(f"{LIB_PATH} implements fiunet ABI v{ver}; this binding is written for v{ABI_VERSION}"
                           + (f" (A/B libraries from v{ABI_MIN_COMPAT} on are accepted)" if ab else "") + ": rebuild it")
    if ab:
        # an A/B build of an older source state (tools/ab_bench.py) may predate the newest entry points:
        # bind what it has; calling a missing one still fails loudly (AttributeError)
        have = [n for n in SYMBOLS if hasattr(L, n)]
        if len(have) != len(SYMBOLS):
            class _Partial:
                def __init__(self, lib): self.__dict__["_lib"] = lib
                def __getattr__(self, n):
                    if n in SYMBOLS and n not in have:
                        class _Missing:
                            def __setattr__(self, *a): pass
                            def __call__(self, *a): raise AttributeError(f"{LIB_PATH} does not export {n}")
                        return _Missing()
                    return getattr(self._lib, n)
            L = _Partial(L)
    vp, ci, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.fiunet_abi_version.restype = ci
    L.fiunet_last_error_string.restype = ctypes.c_char_p
    L.fiunet_create.argtypes = [ctypes.POINTER(vp), ci, ci, ci]
    L.fiunet_destroy.argtypes = [vp]
    L.fiunet_set_options.argtypes = [vp, ctypes.c_uint]
    L.fiunet_load_weights.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p),
                                      ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64)]
    L.fiunet_load_weights_device.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_char_p),
                                             ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64), vp]
    L.fiunet_prepare_precision.argtypes = [vp, ci]
    L.fiunet_workspace_bytes.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes.restype = sz
    L.fiunet_min_unsplit_batch.argtypes = [vp, ci, ci, ci]
    L.fiunet_min_unsplit_batch.restype = ci
    L.fiunet_workspace_bytes_u8.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_u8.restype = sz
    L.fiunet_forward.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp, sz, vp]
    L.fiunet_forward_strip.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp, sz, vp]
    L.fiunet_forward_u8.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp, sz, vp]
    L.fiunet_forward_u8_strided.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, ci, vp, sz, vp]
    L.fiunet_preprocess_u8.argtypes = [vp, vp, sz, vp]
    cu = ctypes.c_uint
    L.fiunet_yuv420_to_rgb_u8.argtypes = [vp, sz, vp, ci, ci, ci, cu, vp]
    L.fiunet_rgb_to_yuv420_u8.argtypes = [vp, vp, sz, ci, ci, ci, cu, vp]
    L.fiunet_workspace_bytes_yuv420.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_yuv420.restype = sz
    L.fiunet_forward_yuv420.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, cu, ci, vp, sz, vp]
    L.fiunet_postprocess_u8.argtypes = [vp, vp, sz, vp]
    L.fiunet_preprocess_p10.argtypes = [vp, vp, sz, vp]
    L.fiunet_postprocess_p10.argtypes = [vp, vp, sz, vp]
    L.fiunet_workspace_bytes_p10.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_p10.restype = sz
    L.fiunet_forward_p10.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, ci, vp, sz, vp]
    L.fiunet_yuv420p10_to_rgb_p10.argtypes = [vp, sz, vp, ci, ci, ci, cu, vp]
    L.fiunet_rgb_p10_to_yuv420p10.argtypes = [vp, vp, sz, ci, ci, ci, cu, vp]
    L.fiunet_workspace_bytes_yuv420p10.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_yuv420p10.restype = sz
    L.fiunet_forward_yuv420p10.argtypes = [vp, vp, vp, vp, sz, ci, ci, ci, cu, ci, vp, sz, vp]
    L.fiunet_pair_sad_u8.argtypes = [vp, ci, sz, vp, vp]
    L.fiunet_pair_sad_p10.argtypes = [vp, ci, sz, vp, vp]
    L.fiunet_scene_cuts.argtypes = [vp, ci, sz, ci, ctypes.c_double, vp, vp, vp]
    L.fiunet_hold_cut_frames.argtypes = [vp, ci, sz, ci, vp, vp]
    u64, u32 = ctypes.c_uint64, ctypes.c_uint32
    L.fiunet_retime_u8.argtypes = [vp, ci, sz, ci, u64, u64, ci, u32, u32, ci, vp, vp, vp]
    L.fiunet_retime_p10.argtypes = [vp, ci, sz, ci, u64, u64, ci, u32, u32, ci, vp, vp, vp]
    L.fiunet_pair_peak_u8.argtypes = [vp, ci, sz, vp, vp]
    L.fiunet_pair_peak_p10.argtypes = [vp, ci, sz, vp, vp]
    L.fiunet_retime_table_u8.argtypes = [vp, ci, sz, vp, ci, vp, vp]
    L.fiunet_retime_table_p10.argtypes = [vp, ci, sz, vp, ci, vp, vp]
    L.fiunet_shutter_u8.argtypes = [vp, ci, sz, vp, ci, vp, vp]
    L.fiunet_shutter_p10.argtypes = [vp, ci, sz, vp, ci, vp, vp]
    L.fiunet_resize_planes_u8.argtypes = [vp, vp, vp, vp, ci, ci, vp]
    L.fiunet_resize_planes_p10.argtypes = [vp, vp, vp, vp, ci, ci, vp]
    L.fiunet_warp_table_u8.argtypes = [vp, ci, vp, vp, ci, ci, ci, vp, ci, vp, ci, vp, vp, vp]
    L.fiunet_warp_table_p10.argtypes = [vp, ci, vp, vp, ci, ci, ci, vp, ci, vp, ci, vp, vp, vp]
    L.fiunet_chroma_pick_u8.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    L.fiunet_chroma_pick_p10.argtypes = [vp, vp, vp, vp, vp, vp, vp, ci, vp, vp]
    L.fiunet_chroma_fill_u8.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, ci, vp, vp, vp]
    L.fiunet_chroma_fill_p10.argtypes = [vp, vp, vp, vp, vp, ci, ci, vp, ci, ci, ci, vp, vp, vp]
    L.fiunet_deinterlace_u8.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    L.fiunet_deinterlace_p10.argtypes = [vp, ci, vp, vp, vp, ci, ci, ci, ci, ci, ci, vp]
    L.fiunet_field_match_u8.argtypes = [vp, ci, vp, ci, ci, ci, ci, vp, vp]
    L.fiunet_field_match_p10.argtypes = [vp, ci, vp, ci, ci, ci, ci, vp, vp]
    L.fiunet_field_weave_u8.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, vp]
    L.fiunet_field_weave_p10.argtypes = [vp, ci, vp, vp, vp, ci, vp, ci, ci, vp]
    L.fiunet_nv12_to_rgb_u8.argtypes = [vp, vp, vp, ci, ci, ci, cu, vp]
    L.fiunet_rgb_to_nv12_u8.argtypes = [vp, vp, vp, ci, ci, ci, cu, vp]
    L.fiunet_p010_to_rgb_p10.argtypes = [vp, vp, vp, ci, ci, ci, cu, vp]
    L.fiunet_rgb_p10_to_p010.argtypes = [vp, vp, vp, ci, ci, ci, cu, vp]
    L.fiunet_workspace_bytes_nv12.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_nv12.restype = sz
    L.fiunet_workspace_bytes_p010.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_p010.restype = sz
    L.fiunet_forward_nv12.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, cu, ci, vp, sz, vp]
    L.fiunet_forward_p010.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, cu, ci, vp, sz, vp]
    L.fiunet_packed_to_rgb_u8.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.fiunet_rgb_to_packed_u8.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.fiunet_workspace_bytes_rgb_packed.argtypes = [vp, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_rgb_packed.restype = sz
    L.fiunet_forward_rgb_packed.argtypes = [vp, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, vp, sz, vp]
    L.fiunet_unpack_422p10.argtypes = [vp, ci, vp, vp, vp, sz, ci, ci, ci, vp]
    L.fiunet_pack_422p10.argtypes = [vp, sz, vp, ci, vp, vp, ci, ci, ci, vp]
    L.fiunet_yuv_to_rgb_u8.argtypes = [vp, ci, sz, sz, vp, ci, ci, ci, cu, vp]
    L.fiunet_yuv_to_rgb_p10.argtypes = [vp, ci, sz, sz, vp, ci, ci, ci, cu, vp]
    L.fiunet_rgb_to_yuv_u8.argtypes = [vp, vp, ci, sz, sz, ci, ci, ci, cu, vp]
    L.fiunet_rgb_p10_to_yuv.argtypes = [vp, vp, ci, sz, sz, ci, ci, ci, cu, vp]
    L.fiunet_workspace_bytes_yuv.argtypes = [vp, ci, ci, ci, ci, ci]
    L.fiunet_workspace_bytes_yuv.restype = sz
    L.fiunet_forward_yuv.argtypes = [vp, vp, vp, ci, sz, sz, vp, sz, sz, ci, ci, ci, cu, ci, vp, sz, vp]
    L.fiunet_forward_yuv_p10.argtypes = [vp, vp, vp, ci, sz, sz, vp, sz, sz, ci, ci, ci, cu, ci, vp, sz, vp]
    L.fiunet_debug_read_activation.argtypes = [vp, vp, ci, ci, ci, ci, ci, vp, sz,
                                               ctypes.POINTER(ci), vp]
    L.fiunet_metrics_workspace_bytes.argtypes = [ci, ci, ci]
    L.fiunet_metrics_workspace_bytes.restype = sz
    L.fiunet_psnr_u8.argtypes = [vp, vp, ci, ci, ci, vp, vp, sz, vp]
    L.fiunet_ssim_u8.argtypes = [vp, vp, ci, ci, ci, vp, vp, sz, vp]
    L.fiunet_plane_metrics_workspace_bytes.argtypes = [ci, ci, ci]
    L.fiunet_plane_metrics_workspace_bytes.restype = sz
    L.fiunet_plane_psnr.argtypes = [vp, sz, sz, vp, sz, sz, ci, ci, ci, ci, vp, vp, vp, sz, vp]
    L.fiunet_plane_ssim.argtypes = [vp, sz, sz, vp, sz, sz, ci, ci, ci, ci, vp, vp, sz, vp]
    L.fiunet_interleaved_psnr.argtypes = [vp, sz, sz, vp, sz, sz, ci, ci, ci, ci, ci, vp, vp, vp, sz, vp]
    L.fiunet_stepped_ssim.argtypes = [vp, sz, sz, ci, vp, sz, sz, ci, ci, ci, ci, ci, vp, vp, sz, vp]
    L.fiunet_flow_workspace_bytes.argtypes = [ci, ci, ci]
    L.fiunet_flow_workspace_bytes.restype = sz
    L.fiunet_farneback_flow.argtypes = [vp, vp, ci, ci, ci, ci, sz, sz, vp, vp, sz, vp]
    L.fiunet_flow_warp.argtypes = [vp, vp, vp, ci, ci, ci, ci, ci, sz, sz, ci, ci, vp, sz, sz, vp]
    L.fiunet_ssim_gauss_workspace_bytes.argtypes = [ci, ci, ci]
    L.fiunet_ssim_gauss_workspace_bytes.restype = sz
    L.fiunet_ssim_gauss_f32.argtypes = [vp, vp, ci, ci, ci, ci, vp, vp, vp, vp, sz, vp]
    L.fiunet_profile_enable.argtypes = [vp, ci]
    L.fiunet_profile_read.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_float),
                                      ctypes.POINTER(ctypes.c_double), ctypes.c_char_p, ci]
    if not os.environ.get("FIUNET_LIB"):
        for name in SYMBOLS:
            getattr(L, name)  # AttributeError here = the .so does not export what the header declares
    _lib = L
    return L


ERR_UNSUPPORTED = 7   # include/fiunet.h: enum fiunet_status


class NativeError(RuntimeError):
    """A non-OK status from the C ABI; `.status` is the fiunet_status code (the message carries the library's text)."""

    def __init__(self, what: str, status: int, text: str):
        super().__init__(f"{what} failed (status {status}): {text}")
        self.status = status


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = lib().fiunet_last_error_string()
        raise NativeError(what, rc, msg.decode() if msg else "?")


def _stream(t: "torch.Tensor", stream=None) -> int:
    """The stream a call runs on: the caller's raw handle, or the current stream of `t`'s device."""
    return torch.cuda.current_stream(t.device).cuda_stream if stream is None else stream


PLAN_KINDS = ("act", "pool", "up", "scratch", "slab")   # csrc/fiunet.hip BufKind


def debug_plan(frame_channels: int, bilinear: bool, flags: int, precision: int, b: int, h: int, w: int):
    """Diagnostic (tests; not part of the ABI): the workspace plan of one forward - fiunet_debug_plan in csrc/fiunet.hip,
    pure host arithmetic with no device call.  -> ([{"kind": one of PLAN_KINDS, "index", "offset", "bytes", "first",
    "last"}] per buffer the plan placed, total bytes); stages count 0..17, last = 18: live after the last conv."""
    fn = lib().fiunet_debug_plan
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 4 + [
        ctypes.POINTER(ctypes.c_longlong), ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_ulonglong)]
    cap = 64
    recs, n, total = (ctypes.c_longlong * (6 * cap))(), ctypes.c_int(), ctypes.c_ulonglong()
    check(fn(frame_channels, int(bilinear), flags, precision, b, h, w, recs, cap, ctypes.byref(n), ctypes.byref(total)),
          "fiunet_debug_plan")
    keys = ("index", "offset", "bytes", "first", "last")
    return ([dict(zip(keys, recs[6 * k + 1:6 * k + 6]), kind=PLAN_KINDS[recs[6 * k]]) for k in range(n.value)],
            total.value)


FLOW_MODES = ("reference", "motion")   # include/fiunet.h: enum fiunet_flow_mode
FLOW_STAGES = ("pyramid", "poly_exp", "update_matrices", "box_solve", "flow_resize")   # fiunet_debug_flow_stage 1..5


def debug_flow_plan(h: int, w: int):
    """Diagnostic (tests; not part of the ABI): the pyramid fiunet_farneback_flow builds for an h x w frame -
    fiunet_debug_flow_plan in csrc/flow.hip, pure host arithmetic.  -> [(h, w, ksize, sigma)] for level 0 .. levels."""
    fn = lib().fiunet_debug_flow_plan
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                   ctypes.POINTER(ctypes.c_double)]
    n, dims, sigma = ctypes.c_int(), (ctypes.c_int * 12)(), (ctypes.c_double * 4)()
    check(fn(h, w, ctypes.byref(n), dims, sigma), "fiunet_debug_flow_plan")
    return [(dims[3 * k], dims[3 * k + 1], dims[3 * k + 2], sigma[k]) for k in range(n.value + 1)]


def debug_flow_stage(stage: str, in0, in1, in2, out, scratch, bits: int, level: int, b: int, H: int, W: int, h: int,
                     w: int, image_stride: int = 0, row_pitch: int = 0, mul=(1.0, 1.0)) -> None:
    """Diagnostic (tests; not part of the ABI): one stage of the flow (FLOW_STAGES) on the caller's buffers -
    fiunet_debug_flow_stage in csrc/flow.hip says what each stage reads and writes."""
    fn = lib().fiunet_debug_flow_stage
    vp, ci, sz, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_float
    fn.argtypes = [ci, vp, vp, vp, vp, vp, ci, ci, ci, ci, ci, ci, ci, sz, sz, cf, cf, vp]
    ptr = lambda t: None if t is None else t.data_ptr()
    check(fn(FLOW_STAGES.index(stage) + 1, ptr(in0), ptr(in1), ptr(in2), ptr(out), ptr(scratch), bits, level, b, H, W,
             h, w, image_stride, row_pitch, mul[0], mul[1], _stream(out)), "fiunet_debug_flow_stage")


class Context:
    """Owns one fiunet_ctx (device-resident prepared weights) on one GPU."""

    def __init__(self, device_index: int, frame_channels: int = 1, bilinear: bool = True):
        self._h = ctypes.c_void_p()
        check(lib().fiunet_create(ctypes.byref(self._h), device_index, frame_channels,
                                  1 if bilinear else 0), "fiunet_create")
        self.device_index = device_index
        self.frame_channels = frame_channels
        self._prepared = set()   # precisions whose extra weight copies exist (fiunet_prepare_precision)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            lib().fiunet_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_options(self, flags: int):
        check(lib().fiunet_set_options(self._h, flags), "fiunet_set_options")

    def force_cfg(self, layer: int, tile: int = 0, ksplit: int = 0) -> None:
        """Diagnostic (tests, tools/cfg_sweep.py; not part of the ABI): override the launch configuration of conv
        `layer` (1..17; < 0 clears all) - tile 0 = choose, 1 = the tuned tile, 2 = the small tile, 3 = the in-workgroup
        K cut where the launch has its form; ksplit 0 = choose, k = cut the K loop k ways where the launch can be cut."""
        fn = lib().fiunet_debug_force_cfg
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
        check(fn(self._h, layer, tile, ksplit), "fiunet_debug_force_cfg")

    def load_state_dict(self, sd, prep: str = "host") -> None:
        """prep "host": fiunet_load_weights - every tensor goes to the host, where one thread folds, packs and rounds, then
        uploads.  prep "device": fiunet_load_weights_device - the tensors stay (or are put by torch) on this context's GPU
        as contiguous fp32 and the library's kernels prepare the same bytes there, asynchronously on the current stream,
        into the buffers of the load before when there was one."""
        if prep not in WEIGHT_PREPS:
            raise ValueError(f"prep must be one of {list(WEIGHT_PREPS)}, got {prep!r}")
        dev = torch.device("cuda", self.device_index) if prep == "device" else torch.device("cpu")
        names, ptrs, numels, keep = [], [], [], []
        for k, v in sd.items():
            if k.endswith("num_batches_tracked"):
                continue
            t = v.detach().to(device=dev, dtype=torch.float32).contiguous()
            keep.append(t)   # (alive until the call returns; a converted copy's memory is then reused in stream order)
            names.append(k.encode())
            ptrs.append(t.data_ptr())
            numels.append(t.numel())
        n = len(names)
        args = (self._h, n, (ctypes.c_char_p * n)(*names), (ctypes.c_void_p * n)(*ptrs), (ctypes.c_int64 * n)(*numels))
        if prep == "device":
            with torch.cuda.device(dev):
                check(lib().fiunet_load_weights_device(*args, torch.cuda.current_stream(dev).cuda_stream),
                      "fiunet_load_weights_device")
        else:
            check(lib().fiunet_load_weights(*args), "fiunet_load_weights")
        self._prepared = set()

    def weight_buffer(self, layer: int, which: int):
        """Diagnostic (tests; not part of the ABI): (device pointer, bytes) of one prepared weight buffer -
        fiunet_debug_weight_buffer in csrc/fiunet.hip lists the layers and buffers; (None, 0) where there is none."""
        fn = lib().fiunet_debug_weight_buffer
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                       ctypes.POINTER(ctypes.c_size_t)]
        p, b = ctypes.c_void_p(), ctypes.c_size_t()
        check(fn(self._h, layer, which, ctypes.byref(p), ctypes.byref(b)), "fiunet_debug_weight_buffer")
        return p.value, b.value

    def prepare(self, precision: int) -> None:
        """Weight copies a precision needs beyond the load's (bf16x2: the two-piece copies; fp16: the fp16 copies; built on
        first use so that fp32 / bf16 users pay neither their memory nor their packing time).  Allocates: not under capture."""
        if precision not in self._prepared:
            check(lib().fiunet_prepare_precision(self._h, precision), "fiunet_prepare_precision")
            self._prepared.add(precision)

    def workspace_bytes(self, b, h, w, precision, u8=False, yuv=False, p10=False) -> int:
        """yuv: fiunet_forward_yuv420's workspace (u8: fiunet_forward_u8's; neither: fiunet_forward's); with p10 the
        10-bit entry points' (fiunet_forward_yuv420p10 / fiunet_forward_p10)."""
        self.prepare(precision)   # every forward path sizes its workspace first
        if p10:
            fn = lib().fiunet_workspace_bytes_yuv420p10 if yuv else lib().fiunet_workspace_bytes_p10
        else:
            fn = (lib().fiunet_workspace_bytes_yuv420 if yuv else
                  lib().fiunet_workspace_bytes_u8 if u8 else lib().fiunet_workspace_bytes)
        n = fn(self._h, b, h, w, precision)
        if n == 0:
            if h < 16 or w < 16:
                raise RuntimeError(f"input {h}x{w} is too small for four 2x2 max-pools (need >= 16)")
            if h * w >= 1 << 26:
                raise RuntimeError(f"input {h}x{w} has 2^26 pixels or more: cut it into row bands "
                                   "(tiling.forward_tiled / forward_strip)")
            check(1, "fiunet_workspace_bytes")
        return n

    def min_unsplit_batch(self, h, w, precision) -> int:
        """Smallest batch at which no layer of an h x w forward K-splits (65: none up to 64)."""
        n = lib().fiunet_min_unsplit_batch(self._h, h, w, precision)
        if n == 0:
            check(1, "fiunet_min_unsplit_batch")
        return n

    def forward(self, f1, f2, out, precision, workspace, stream=None):
        b, _, h, w = f1.shape
        s = _stream(f1, stream)
        check(lib().fiunet_forward(self._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), b, h, w,
                                   precision, workspace.data_ptr(), workspace.numel(), s),
              "fiunet_forward")

    def forward_strip(self, f1, f2, out, y_origin, h_image, precision, workspace, stream=None):
        """The forward on rows [y_origin, y_origin + h) of an image of h_image rows."""
        b, _, h, w = f1.shape
        s = _stream(f1, stream)
        check(lib().fiunet_forward_strip(self._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), b, h,
                                         w, y_origin, h_image, precision, workspace.data_ptr(),
                                         workspace.numel(), s), "fiunet_forward_strip")

    def forward_u8(self, f1, f2, out, precision, workspace, stream=None):
        """`out`: uint8 [B, C, H, W] whose images are contiguous; they may lie further apart than one image (a strided
        view such as every second frame of the video loop's interleaved result): the fused head writes them in place."""
        b, c, h, w = f1.shape
        s = _stream(f1, stream)
        if out.is_contiguous():
            check(lib().fiunet_forward_u8(self._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), b, h,
                                          w, precision, workspace.data_ptr(), workspace.numel(), s),
                  "fiunet_forward_u8")
            return
        st = out.stride()
        if tuple(st[1:]) != (h * w, w, 1) or (b > 1 and st[0] < c * h * w):
            raise ValueError(f"out: every image must be contiguous (strides {tuple(st)} for shape {tuple(out.shape)})")
        check(lib().fiunet_forward_u8_strided(self._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), st[0], b, h,
                                              w, precision, workspace.data_ptr(), workspace.numel(), s),
              "fiunet_forward_u8_strided")

    def forward_yuv420(self, f1, f2, out, h, w, colour, precision, workspace, bits, stream=None):
        """fiunet_forward_yuv420 (bits 8: uint8) / fiunet_forward_yuv420p10 (bits 10: uint16): f1, f2 [B, F] packed
        4:2:0 frames, contiguous; `out` [B, F] whose rows are contiguous and may lie further apart (every second frame
        of the video loop's interleaved result).  Strides in samples."""
        b = f1.shape[0]
        s = _stream(f1, stream)
        st = out.stride(0) if b > 1 else out.shape[1]
        fn, name = ((lib().fiunet_forward_yuv420p10, "fiunet_forward_yuv420p10") if bits == 10 else
                    (lib().fiunet_forward_yuv420, "fiunet_forward_yuv420"))
        check(fn(self._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), st, b, h, w, colour, precision,
                 workspace.data_ptr(), workspace.numel(), s), name)

    def forward_p10(self, f1, f2, out, precision, workspace, stream=None):
        """10-bit frames: uint16 [B, C, H, W] contiguous in; `out` uint16 [B, C, H, W] whose images are contiguous and
        may lie further apart (every second frame of the video loop's interleaved result).  Strides in samples."""
        b, c, h, w = f1.shape
        s = _stream(f1, stream)
        image_stride = 0   # contiguous
        if not out.is_contiguous():
            st = out.stride()
            # (the stride of a size-1 dim is arbitrary: a one-channel image is contiguous whatever st[1] says)
            if (c > 1 and st[1] != h * w) or tuple(st[2:]) != (w, 1) or (b > 1 and st[0] < c * h * w):
                raise ValueError(f"out: every image must be contiguous (strides {tuple(st)} for shape "
                                 f"{tuple(out.shape)})")
            image_stride = st[0] if b > 1 else 0
        check(lib().fiunet_forward_p10(self._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), image_stride, b, h,
                                       w, precision, workspace.data_ptr(), workspace.numel(), s),
              "fiunet_forward_p10")

    def forward_surface(self, f1, f2, layout, out, out_layout, h, w, colour, precision, workspace, bits, stream=None):
        """fiunet_forward_nv12 (bits 8: uint8) / fiunet_forward_p010 (bits 10: uint16 words) on [B, frame_stride] rows:
        f1, f2 contiguous in `layout`; `out` in `out_layout`, its rows contiguous and possibly further apart.  The
        layouts are resolved colour.SurfaceLayout tuples or None (tight); the workspace is the 4:2:0 entry point's."""
        b = f1.shape[0]
        s = _stream(f1, stream)
        st = out.stride(0) if b > 1 else out.shape[1]
        fn, name = ((lib().fiunet_forward_p010, "fiunet_forward_p010") if bits == 10 else
                    (lib().fiunet_forward_nv12, "fiunet_forward_nv12"))
        check(fn(self._h, f1.data_ptr(), f2.data_ptr(), _surface(layout, f1.shape[1]), out.data_ptr(),
                 _surface(out_layout, st), b, h, w, colour, precision, workspace.data_ptr(), workspace.numel(), s), name)

    def forward_rgb_packed(self, f1, f2, layout, out, out_layout, h, w, fmt, precision, workspace, stream=None):
        """fiunet_forward_rgb_packed on uint8 [B, frame_stride] rows: f1, f2 contiguous in `layout`; `out` in
        `out_layout`, its rows contiguous and possibly further apart.  The layouts are resolved packed.PackedLayout
        tuples; fmt: the fiunet_packed_format code; the workspace is the 4:2:0 entry point's."""
        b = f1.shape[0]
        s = _stream(f1, stream)
        st = out.stride(0) if b > 1 else out.shape[1]
        check(lib().fiunet_forward_rgb_packed(self._h, f1.data_ptr(), f2.data_ptr(), _packed(layout, f1.shape[1]),
                                              out.data_ptr(), _packed(out_layout, st), b, h, w, fmt, precision,
                                              workspace.data_ptr(), workspace.numel(), s),
              "fiunet_forward_rgb_packed")

    def forward_yuv(self, f1, f2, fmt, layout, out, out_layout, h, w, colour, precision, workspace, bits, stream=None):
        """fiunet_forward_yuv (bits 8: uint8) / fiunet_forward_yuv_p10 (bits 10: uint16) on [B, frame_stride] rows of the
        fiunet_yuv_format `fmt`: f1, f2 contiguous in `layout`; `out` in `out_layout`, its rows contiguous and possibly
        further apart.  The layouts are resolved packed.PackedLayout tuples (row_pitch 0 for the planar formats); the
        workspace is the 4:2:0 entry point's."""
        b = f1.shape[0]
        s = _stream(f1, stream)
        fn, name = ((lib().fiunet_forward_yuv_p10, "fiunet_forward_yuv_p10") if bits == 10 else
                    (lib().fiunet_forward_yuv, "fiunet_forward_yuv"))
        check(fn(self._h, f1.data_ptr(), f2.data_ptr(), fmt, layout.row_pitch, f1.shape[1], out.data_ptr(),
                 out_layout.row_pitch, _row_stride(out), b, h, w, colour, precision, workspace.data_ptr(),
                 workspace.numel(), s), name)

    def profile_enable(self, on: bool):
        check(lib().fiunet_profile_enable(self._h, 1 if on else 0), "fiunet_profile_enable")

    def profile_read(self):
        """-> (n_forwards, [(kernel name, avg ms, algorithmic flops)] for the 18 conv stages)"""
        n = ctypes.c_int(0)
        ms = (ctypes.c_float * 18)()
        fl = (ctypes.c_double * 18)()
        names = ctypes.create_string_buffer(18 * 96)
        check(lib().fiunet_profile_read(self._h, ctypes.byref(n), ms, fl, names, 96),
              "fiunet_profile_read")
        rows = []
        for i in range(18):
            nm = names.raw[i * 96:(i + 1) * 96].split(b"\0", 1)[0].decode()
            rows.append((nm, float(ms[i]), float(fl[i])))
        return n.value, rows

    def read_activation(self, workspace, b, h, w, precision, tap):
        dims = (ctypes.c_int * 3)()
        # the library knows the architecture (the ConvTranspose2d decoder is wider at taps 8, 9, 11, 13, 15): ask it
        # for the tap's dims first (dst = NULL), then hand over a buffer of exactly that size WITH its capacity
        check(lib().fiunet_debug_read_activation(self._h, None, b, h, w, precision, tap, None, 0, dims, None),
              "fiunet_debug_read_activation (dims query)")
        c, hh, ww = tuple(dims)
        dst = torch.empty((b, c, hh, ww), dtype=torch.float32, device=workspace.device)
        s = _stream(workspace)
        check(lib().fiunet_debug_read_activation(self._h, workspace.data_ptr(), b, h, w, precision,
                                                 tap, dst.data_ptr(), dst.numel(), dims, s),
              "fiunet_debug_read_activation")
        return dst


def _pointwise(name: str, src: "torch.Tensor", dtype) -> "torch.Tensor":
    """One of the four pre / post-processing kernels on contiguous samples -> `dtype`, same shape."""
    out = torch.empty(src.shape, dtype=dtype, device=src.device)
    s = _stream(src)
    check(getattr(lib(), name)(src.data_ptr(), out.data_ptr(), src.numel(), s), name)
    return out


def preprocess_u8(src_u8: "torch.Tensor") -> "torch.Tensor":
    """fiunet_preprocess_u8: uint8 -> fp32 x / 255 * 2 - 1."""
    return _pointwise("fiunet_preprocess_u8", src_u8, torch.float32)


def postprocess_u8(src_f32: "torch.Tensor") -> "torch.Tensor":
    """fiunet_postprocess_u8: fp32 -> uint8 trunc(clamp((t + 1) / 2, 0, 1) * 255)."""
    return _pointwise("fiunet_postprocess_u8", src_f32, torch.uint8)


def preprocess_p10(src: "torch.Tensor") -> "torch.Tensor":
    """fiunet_preprocess_p10: uint16 10-bit codes -> fp32 x / 1023 * 2 - 1."""
    return _pointwise("fiunet_preprocess_p10", src, torch.float32)


def postprocess_p10(src_f32: "torch.Tensor") -> "torch.Tensor":
    """fiunet_postprocess_p10: fp32 -> uint16 trunc(clamp((t + 1) / 2, 0, 1) * 1023)."""
    return _pointwise("fiunet_postprocess_p10", src_f32, torch.uint16)


def yuv420_to_rgb(frames: "torch.Tensor", out: "torch.Tensor", h: int, w: int, colour: int, bits: int) -> None:
    """fiunet_yuv420_to_rgb_u8 (bits 8: uint8) / fiunet_yuv420p10_to_rgb_p10 (bits 10: uint16): [B, F] packed 4:2:0
    frames (rows contiguous, any row stride) -> planar RGB [B, 3, h, w]."""
    b = frames.shape[0]
    st = frames.stride(0) if b > 1 else frames.shape[1]
    s = _stream(frames)
    fn, name = ((lib().fiunet_yuv420p10_to_rgb_p10, "fiunet_yuv420p10_to_rgb_p10") if bits == 10 else
                (lib().fiunet_yuv420_to_rgb_u8, "fiunet_yuv420_to_rgb_u8"))
    check(fn(frames.data_ptr(), st, out.data_ptr(), b, h, w, colour, s), name)


def rgb_to_yuv420(rgb: "torch.Tensor", out: "torch.Tensor", colour: int, bits: int) -> None:
    """fiunet_rgb_to_yuv420_u8 (bits 8: uint8) / fiunet_rgb_p10_to_yuv420p10 (bits 10: uint16): planar RGB [B, 3, h, w]
    contiguous -> [B, F] packed 4:2:0 frames (rows contiguous, any row stride)."""
    b, _, h, w = rgb.shape
    st = out.stride(0) if b > 1 else out.shape[1]
    s = _stream(rgb)
    fn, name = ((lib().fiunet_rgb_p10_to_yuv420p10, "fiunet_rgb_p10_to_yuv420p10") if bits == 10 else
                (lib().fiunet_rgb_to_yuv420_u8, "fiunet_rgb_to_yuv420_u8"))
    check(fn(rgb.data_ptr(), out.data_ptr(), st, b, h, w, colour, s), name)


def surface_to_rgb(frames: "torch.Tensor", layout, out: "torch.Tensor", h: int, w: int, colour: int, bits: int) -> None:
    """fiunet_nv12_to_rgb_u8 (bits 8) / fiunet_p010_to_rgb_p10 (bits 10): [B, frame_stride] surfaces (rows contiguous,
    any row stride) in the resolved `layout` (None: tight) -> planar RGB [B, 3, h, w]."""
    b = frames.shape[0]
    st = frames.stride(0) if b > 1 else frames.shape[1]
    s = _stream(frames)
    fn, name = ((lib().fiunet_p010_to_rgb_p10, "fiunet_p010_to_rgb_p10") if bits == 10 else
                (lib().fiunet_nv12_to_rgb_u8, "fiunet_nv12_to_rgb_u8"))
    check(fn(frames.data_ptr(), _surface(layout, st), out.data_ptr(), b, h, w, colour, s), name)


def rgb_to_surface(rgb: "torch.Tensor", out: "torch.Tensor", layout, colour: int, bits: int) -> None:
    """fiunet_rgb_to_nv12_u8 (bits 8) / fiunet_rgb_p10_to_p010 (bits 10): planar RGB [B, 3, h, w] contiguous -> [B,
    frame_stride] surfaces (rows contiguous, any row stride) in the resolved `layout` (None: tight)."""
    b, _, h, w = rgb.shape
    st = out.stride(0) if b > 1 else out.shape[1]
    s = _stream(rgb)
    fn, name = ((lib().fiunet_rgb_p10_to_p010, "fiunet_rgb_p10_to_p010") if bits == 10 else
                (lib().fiunet_rgb_to_nv12_u8, "fiunet_rgb_to_nv12_u8"))
    check(fn(rgb.data_ptr(), out.data_ptr(), _surface(layout, st), b, h, w, colour, s), name)


def _row_stride(t: "torch.Tensor") -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def packed_to_rgb(frames: "torch.Tensor", layout, out: "torch.Tensor", alpha, h: int, w: int, fmt: int) -> None:
    """fiunet_packed_to_rgb_u8: uint8 [B, frame_stride] packed frames (rows contiguous, any row stride) in the resolved
    `layout` -> planar RGB [B, 3, h, w]; alpha: None, or the contiguous [B, h, w] tensor the alpha plane goes to."""
    s = _stream(frames)
    check(lib().fiunet_packed_to_rgb_u8(frames.data_ptr(), _packed(layout, _row_stride(frames)), out.data_ptr(),
                                        None if alpha is None else alpha.data_ptr(), frames.shape[0], h, w, fmt, s),
          "fiunet_packed_to_rgb_u8")


def rgb_to_packed(rgb: "torch.Tensor", out: "torch.Tensor", layout, alphas, alpha_layout, fmt: int) -> None:
    """fiunet_rgb_to_packed_u8: planar RGB [B, 3, h, w] contiguous -> uint8 [B, frame_stride] packed frames (rows
    contiguous, any row stride) in the resolved `layout`; alphas: a tuple of 0, 1 or 2 packed tensors of one row stride
    in the resolved `alpha_layout`."""
    b, _, h, w = rgb.shape
    s = _stream(rgb)
    a = [t.data_ptr() for t in alphas] + [None, None]
    al = _packed(alpha_layout, _row_stride(alphas[0])) if alphas else None
    check(lib().fiunet_rgb_to_packed_u8(rgb.data_ptr(), out.data_ptr(), _packed(layout, _row_stride(out)), a[0], a[1],
                                        al, b, h, w, fmt, s), "fiunet_rgb_to_packed_u8")


def yuv_to_rgb(frames: "torch.Tensor", fmt: int, layout, out: "torch.Tensor", h: int, w: int, colour: int,
               bits: int) -> None:
    """fiunet_yuv_to_rgb_u8 (bits 8) / fiunet_yuv_to_rgb_p10 (bits 10): [B, frame_stride] frames of the
    fiunet_yuv_format `fmt` (rows contiguous, any row stride) in the resolved `layout` -> planar RGB [B, 3, h, w]."""
    s = _stream(frames)
    fn, name = ((lib().fiunet_yuv_to_rgb_p10, "fiunet_yuv_to_rgb_p10") if bits == 10 else
                (lib().fiunet_yuv_to_rgb_u8, "fiunet_yuv_to_rgb_u8"))
    check(fn(frames.data_ptr(), fmt, layout.row_pitch, _row_stride(frames), out.data_ptr(), frames.shape[0], h, w,
             colour, s), name)


def rgb_to_yuv(rgb: "torch.Tensor", out: "torch.Tensor", fmt: int, layout, colour: int, bits: int) -> None:
    """fiunet_rgb_to_yuv_u8 (bits 8) / fiunet_rgb_p10_to_yuv (bits 10): planar RGB [B, 3, h, w] contiguous -> [B,
    frame_stride] frames of the fiunet_yuv_format `fmt` (rows contiguous, any row stride) in the resolved `layout`."""
    b, _, h, w = rgb.shape
    s = _stream(rgb)
    fn, name = ((lib().fiunet_rgb_p10_to_yuv, "fiunet_rgb_p10_to_yuv") if bits == 10 else
                (lib().fiunet_rgb_to_yuv_u8, "fiunet_rgb_to_yuv_u8"))
    check(fn(rgb.data_ptr(), out.data_ptr(), fmt, layout.row_pitch, _row_stride(out), b, h, w, colour, s), name)


PACK10_V210, PACK10_Y210, PACK10_P210 = 0, 1, 2   # include/fiunet.h: enum fiunet_packing10


def _wire10_layouts(packing: int, layout, frame_stride_bytes: int):
    """(packed layout, surface layout) arguments of the two wire10 entry points: `layout` is a resolved
    packed.PackedLayout in bytes (v210 / y210le) or colour.SurfaceLayout in samples (p210le), the frames
    `frame_stride_bytes` apart."""
    if packing == PACK10_P210:
        return None, ctypes.byref(SurfaceLayout(layout.luma_pitch, layout.chroma_offset, layout.chroma_pitch,
                                                frame_stride_bytes // 2))
    return ctypes.byref(PackedLayout(layout.row_pitch, frame_stride_bytes)), None


def _row_stride_bytes(t: "torch.Tensor") -> int:
    return _row_stride(t) * t.element_size()


def unpack_422p10(frames: "torch.Tensor", packing: int, layout, out: "torch.Tensor", h: int, w: int, stream=None) -> None:
    """fiunet_unpack_422p10: [B, frame_stride] wire frames of the fiunet_packing10 `packing` (rows contiguous, any row
    stride) in the resolved `layout` -> 16-bit [B, >= samples] yuv422p10le frames (rows contiguous, any row stride)."""
    pl, sl = _wire10_layouts(packing, layout, _row_stride_bytes(frames))
    check(lib().fiunet_unpack_422p10(frames.data_ptr(), packing, pl, sl, out.data_ptr(), _row_stride(out),
                                     frames.shape[0], h, w, _stream(frames, stream)), "fiunet_unpack_422p10")


def pack_422p10(planar: "torch.Tensor", out: "torch.Tensor", packing: int, layout, h: int, w: int, stream=None) -> None:
    """fiunet_pack_422p10: 16-bit [B, >= samples] yuv422p10le frames (rows contiguous, any row stride) -> [B,
    frame_stride] wire frames of `packing` in the resolved `layout` (rows contiguous, any row stride)."""
    pl, sl = _wire10_layouts(packing, layout, _row_stride_bytes(out))
    check(lib().fiunet_pack_422p10(planar.data_ptr(), _row_stride(planar), out.data_ptr(), packing, pl, sl,
                                   planar.shape[0], h, w, _stream(planar, stream)), "fiunet_pack_422p10")


def pair_sad(frames: "torch.Tensor", sums: "torch.Tensor", bits: int) -> None:
    """fiunet_pair_sad_u8 / fiunet_pair_sad_p10: ACCUMULATES sum |F[i+1] - F[i]| of a contiguous stack [N, ...] (uint8 at
    8 bits; 16-bit words, int16 or uint16, at 10) into the int64 `sums` [N-1]."""
    n = frames.shape[0]
    fs = frames[0].numel() if n else 0
    fn = lib().fiunet_pair_sad_p10 if bits == 10 else lib().fiunet_pair_sad_u8
    s = _stream(frames)
    check(fn(frames.data_ptr(), n, fs, sums.data_ptr(), s), "fiunet_pair_sad_" + ("p10" if bits == 10 else "u8"))


def scene_cuts(sums: "torch.Tensor", n_frames: int, count: int, bits: int, threshold: float,
               scores: "torch.Tensor", flags: "torch.Tensor") -> None:
    """fiunet_scene_cuts: int64 sums [N-1] -> fp64 scores [N-1], uint8 flags [N-1]."""
    s = _stream(sums)
    check(lib().fiunet_scene_cuts(sums.data_ptr(), n_frames, count, bits, float(threshold), scores.data_ptr(),
                                  flags.data_ptr(), s), "fiunet_scene_cuts")


def hold_cut_frames(video: "torch.Tensor", n_frames: int, factor: int, flags: "torch.Tensor") -> None:
    """fiunet_hold_cut_frames on a contiguous interleaved result [(n_frames-1)*factor+1, ...], in place."""
    fb = video[0].numel() * video.element_size() if video.shape[0] else 0
    s = _stream(video)
    check(lib().fiunet_hold_cut_frames(video.data_ptr(), n_frames, fb, factor, flags.data_ptr(), s),
          "fiunet_hold_cut_frames")


def retime(grid: "torch.Tensor", n_intervals: int, depth: int, first_interval: int, j0: int, n_out: int, p: int,
           q: int, mode: int, flags, out: "torch.Tensor", bits: int) -> None:
    """fiunet_retime_u8 / fiunet_retime_p10: a contiguous grid [(n_intervals << depth) + 1, ...] (uint8 at 8 bits; 16-bit
    words at 10) -> `out` [n_out, ...], clip output frames j0 .. j0 + n_out - 1; flags uint8 [n_intervals] or None."""
    fs = grid[0].numel()
    fn = lib().fiunet_retime_p10 if bits == 10 else lib().fiunet_retime_u8
    s = _stream(grid)
    check(fn(grid.data_ptr(), n_intervals, fs, depth, first_interval, j0, n_out, p, q, mode,
             None if flags is None else flags.data_ptr(), out.data_ptr(), s),
          "fiunet_retime_" + ("p10" if bits == 10 else "u8"))


def pair_peak(frames: "torch.Tensor", peaks: "torch.Tensor", bits: int) -> None:
    """fiunet_pair_peak_u8 / fiunet_pair_peak_p10: MAX-ACCUMULATES the largest 64-sample segment sum of |F[i+1] - F[i]|
    of a contiguous stack [N, ...] (uint8 at 8 bits; 16-bit words, int16 or uint16, at 10) into the 32-bit `peaks`
    [N-1] (int32 on the torch side: a peak is below 2**16)."""
    n = frames.shape[0]
    fs = frames[0].numel() if n else 0
    fn = lib().fiunet_pair_peak_p10 if bits == 10 else lib().fiunet_pair_peak_u8
    s = _stream(frames)
    check(fn(frames.data_ptr(), n, fs, peaks.data_ptr(), s), "fiunet_pair_peak_" + ("p10" if bits == 10 else "u8"))


def resize_plane_array(planes, filter: int = 0):
    """A sequence of (offset, h, w, pitch, step, frame_stride) int tuples, in samples -> the C array of
    fiunet_resize_plane, every one with `filter` in its filter member (the library reads it from destination planes;
    source planes carry 0).  ValueError on a value that does not fit its field (the library checks the rest)."""
    arr = (ResizePlane * max(len(planes), 1))()
    if not -(1 << 31) <= filter < 1 << 31:
        raise ValueError(f"filter = {filter} does not fit fiunet_resize_plane")
    for k, (off, h, w, pitch, step, fs) in enumerate(planes):
        if not all(0 <= v < 1 << 64 for v in (off, pitch, fs)) or not all(-(1 << 31) <= v < 1 << 31 for v in (h, w, step)):
            raise ValueError(f"plane {k} = {(off, h, w, pitch, step, fs)} does not fit fiunet_resize_plane")
        arr[k] = ResizePlane(off, pitch, fs, h, w, step, filter)
    return arr


def _resize_extent(planes, n_frames: int) -> int:
    """Samples from the buffer's start to the end of the last frame's last plane (0 for no frames)."""
    if n_frames < 1:
        return 0
    return max(off + (n_frames - 1) * fs + (h - 1) * pitch + (w - 1) * step + 1 for off, h, w, pitch, step, fs in planes)


def _planes_fit(name: str, planes, n: int, room: int) -> None:
    """ValueError where n frames of `planes` ("src planes", "grid plane": `name`), taken together, reach past a buffer of
    `room` samples.  Only well-formed planes are judged: the library refuses the others."""
    if all(min(p) >= 0 and p[1] >= 1 and p[2] >= 1 for p in planes) and _resize_extent(planes, n) > room:
        verb = "reach" if name.endswith("s") else "reaches"
        raise ValueError(f"the {name} {verb} sample {_resize_extent(planes, n)} of a buffer of {room}")


def resize_planes(src: "torch.Tensor", src_planes, dst: "torch.Tensor", dst_planes, n_frames: int, bits: int,
                  stream=None, filter: int = 0) -> None:
    """fiunet_resize_planes_u8 / fiunet_resize_planes_p10: plane i of `src_planes` of every one of n_frames frames of the
    dense buffer `src` (uint8 at 8 bits; 16-bit words at 10) -> plane i of `dst_planes` of `dst`.  A plane is (offset, h,
    w, pitch, step, frame_stride) in samples from the tensor's first element; filter: RESIZE_LINEAR (0) or RESIZE_AREA,
    carried by every destination plane (the library refuses any other value).  ValueError, before the call, where well-
    formed planes reach past either tensor."""
    src_planes, dst_planes = [tuple(int(v) for v in p) for p in src_planes], [tuple(int(v) for v in p) for p in dst_planes]
    if len(src_planes) != len(dst_planes):
        raise ValueError(f"{len(src_planes)} source planes for {len(dst_planes)} destination planes")
    for name, t, planes in (("src", src, src_planes), ("dst", dst, dst_planes)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be a dense buffer (the planes carry the pitches)")
        _planes_fit(name + " planes", planes, n_frames, t.numel())
    fn = lib().fiunet_resize_planes_p10 if bits == 10 else lib().fiunet_resize_planes_u8
    check(fn(src.data_ptr(), resize_plane_array(src_planes), dst.data_ptr(), resize_plane_array(dst_planes, int(filter)),
             len(src_planes), n_frames, _stream(src, stream)), "fiunet_resize_planes_" + ("p10" if bits == 10 else "u8"))


def retime_entries(entries):
    """A sequence of (row, wn, den) int triples -> the C array of fiunet_retime_entry (None when empty).  ValueError on a
    value that does not fit 32 bits unsigned (the library checks the rest)."""
    n = len(entries)
    if not n:
        return None
    arr = (RetimeEntry * n)()
    for k, (row, wn, den) in enumerate(entries):
        if not (0 <= row < 1 << 32 and 0 <= wn < 1 << 32 and 0 <= den < 1 << 32):
            raise ValueError(f"entry {k} = {(row, wn, den)} does not fit 32 bits unsigned")
        arr[k] = RetimeEntry(row, wn, den)
    return arr


def retime_table(grid: "torch.Tensor", entries, out: "torch.Tensor", bits: int) -> None:
    """fiunet_retime_table_u8 / fiunet_retime_table_p10: a contiguous grid [n_rows, ...] and (row, wn, den) triples, read
    on the host during the call -> `out` [len(entries), ...]."""
    arr = retime_entries(entries)
    fs = grid[0].numel() if grid.shape[0] else 0
    fn = lib().fiunet_retime_table_p10 if bits == 10 else lib().fiunet_retime_table_u8
    s = _stream(grid)
    check(fn(grid.data_ptr(), grid.shape[0], fs, arr, len(entries), out.data_ptr(), s),
          "fiunet_retime_table_" + ("p10" if bits == 10 else "u8"))


SHUTTER_MAX_TAPS = 48   # csrc/shutter.hip.h: kShutterMaxTaps


def shutter_entries(entries):
    """A sequence of (first_row, weights) -> the C array of 32-bit words fiunet_shutter_* takes (first_row, n_taps, the
    weights; None when empty).  ValueError on a value that does not fit 32 bits unsigned (the library checks the rest)."""
    words = []
    for k, (row, w) in enumerate(entries):
        w = [int(v) for v in w]
        if not (0 <= row < 1 << 32 and all(0 <= v < 1 << 32 for v in w)):
            raise ValueError(f"entry {k} = {(row, w)} does not fit 32 bits unsigned")
        words += [int(row), len(w)] + w
    return (ctypes.c_uint32 * len(words))(*words) if words else None


def shutter(grid: "torch.Tensor", entries, out: "torch.Tensor", bits: int, stream=None) -> None:
    """fiunet_shutter_u8 / fiunet_shutter_p10: a contiguous grid [n_rows, ...] and (first_row, weights) entries, read on
    the host during the call -> `out` [len(entries), ...]."""
    arr = shutter_entries(entries)
    fs = grid[0].numel() if grid.shape[0] else 0
    fn = lib().fiunet_shutter_p10 if bits == 10 else lib().fiunet_shutter_u8
    check(fn(grid.data_ptr(), grid.shape[0], fs, arr, len(entries), out.data_ptr(), _stream(grid, stream)),
          "fiunet_shutter_" + ("p10" if bits == 10 else "u8"))


def warp_entries(entries):
    """A sequence of (row, wn, den, flow, flag) int tuples -> the C array of fiunet_warp_entry (None when empty).
    ValueError on a value that does not fit its field (the library checks the rest)."""
    n = len(entries)
    if not n:
        return None
    arr = (WarpEntry * n)()
    for k, (row, wn, den, flow, flag) in enumerate(entries):
        if not all(0 <= v < 1 << 32 for v in (row, wn, den, flow)) or not -(1 << 31) <= flag < 1 << 31:
            raise ValueError(f"entry {k} = {(row, wn, den, flow, flag)} does not fit fiunet_warp_entry")
        arr[k] = WarpEntry(row, wn, den, flow, flag)
    return arr


def warp_table(grid: "torch.Tensor", n_rows: int, grid_plane, flow: "torch.Tensor", flags, entries, out: "torch.Tensor",
               out_plane, bits: int, stream=None) -> None:
    """fiunet_warp_table_u8 / fiunet_warp_table_p10: one plane of len(entries) output frames, each warped along a field of
    `flow` (contiguous float32 [n_flows, flow_h, flow_w, 2]) between two rows of the dense buffer `grid` to its time
    wn / den.  A plane is (offset, h, w, pitch, step, frame_stride) in samples from the tensor's first element; entries:
    (row, wn, den, flow, flag) with flag WARP_NO_FLAG or an index into the uint8 device tensor `flags` (or None).
    ValueError, before the call, where well-formed planes reach past either tensor."""
    grid_plane, out_plane = tuple(int(v) for v in grid_plane), tuple(int(v) for v in out_plane)
    entries = [tuple(int(v) for v in e) for e in entries]
    for name, t, plane, n in (("grid", grid, grid_plane, n_rows), ("out", out, out_plane, len(entries))):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be a dense buffer (the plane carries the pitch)")
        _planes_fit(name + " plane", [plane], n, t.numel())
    if flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[3] != 2 or not flow.is_contiguous():
        raise ValueError(f"flow: expected a contiguous float32 [n, h, w, 2] tensor, got {flow.dtype} {tuple(flow.shape)}")
    if flags is not None and (flags.dtype != torch.uint8 or not flags.is_contiguous()):
        raise ValueError("flags must be a contiguous uint8 tensor")
    fn = lib().fiunet_warp_table_p10 if bits == 10 else lib().fiunet_warp_table_u8
    check(fn(grid.data_ptr(), n_rows, resize_plane_array([grid_plane]), flow.data_ptr(), flow.shape[0], flow.shape[1],
             flow.shape[2], None if flags is None else flags.data_ptr(), 0 if flags is None else flags.numel(),
             warp_entries(entries), len(entries), out.data_ptr(), resize_plane_array([out_plane]), _stream(grid, stream)),
          "fiunet_warp_table_" + ("p10" if bits == 10 else "u8"))


def _room(t: "torch.Tensor") -> int:
    """Samples from the first element of `t` (a tensor or a view) to the end of its storage."""
    return t.untyped_storage().nbytes() // t.element_size() - t.storage_offset()


def _chroma_planes(name, t, planes, n):
    planes = [tuple(int(v) for v in p) for p in planes]
    for p in planes:
        _planes_fit(name + " plane", [p], n, _room(t))   # (plane by plane: U and V may lie in any order)
    return planes


def chroma_pick(a: "torch.Tensor", a_plane, b: "torch.Tensor", b_plane, m: "torch.Tensor", m_plane, flow: "torch.Tensor",
                pick: "torch.Tensor", bits: int, stream=None) -> None:
    """fiunet_chroma_pick_u8 / fiunet_chroma_pick_p10: the pick map [n, ceil(h / 8), ceil(w / 8)] (contiguous uint8) of n
    frames from the luma of A, B and M and `flow` (contiguous float32 [n, h, w, 2]).  A plane is (offset, h, w, pitch,
    step, frame_stride) in samples from the first element of its tensor, which may be a view: a, b and m may be three
    views of one buffer.  ValueError, before the call, where well-formed planes reach past a tensor's storage."""
    if flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[3] != 2 or not flow.is_contiguous():
        raise ValueError(f"flow: expected a contiguous float32 [n, h, w, 2] tensor, got {flow.dtype} {tuple(flow.shape)}")
    n = flow.shape[0]
    (ap,), (bp,), (mp,) = (_chroma_planes(k, t, [p], n) for k, t, p in (("a", a, a_plane), ("b", b, b_plane), ("m", m, m_plane)))
    if tuple(flow.shape[1:3]) != (ap[1], ap[2]):
        raise ValueError(f"flow: expected [n, {ap[1]}, {ap[2]}, 2], the luma size, got {tuple(flow.shape)}")
    want = (n, -(-ap[1] // 8), -(-ap[2] // 8))
    if pick.dtype != torch.uint8 or tuple(pick.shape) != want or not pick.is_contiguous():
        raise ValueError(f"pick: expected a contiguous uint8 {want} tensor, got {pick.dtype} {tuple(pick.shape)}")
    fn = lib().fiunet_chroma_pick_p10 if bits == 10 else lib().fiunet_chroma_pick_u8
    check(fn(a.data_ptr(), resize_plane_array([ap]), b.data_ptr(), resize_plane_array([bp]), m.data_ptr(),
             resize_plane_array([mp]), flow.data_ptr(), n, pick.data_ptr(), _stream(a, stream)),
          "fiunet_chroma_pick_" + ("p10" if bits == 10 else "u8"))


def chroma_fill(a: "torch.Tensor", a_planes, b: "torch.Tensor", b_planes, flow: "torch.Tensor", pick: "torch.Tensor",
                sub, out: "torch.Tensor", out_planes, bits: int, stream=None) -> None:
    """fiunet_chroma_fill_u8 / fiunet_chroma_fill_p10: both chroma planes of n frames, sub-sampled by sub = (sy, sx)
    against the luma that `flow` (contiguous float32 [n, h, w, 2]) and `pick` (contiguous uint8 [n, ceil(h / 8),
    ceil(w / 8)]) belong to.  a_planes, b_planes, out_planes: two planes each, as for `chroma_pick`."""
    if flow.dtype != torch.float32 or flow.dim() != 4 or flow.shape[3] != 2 or not flow.is_contiguous():
        raise ValueError(f"flow: expected a contiguous float32 [n, h, w, 2] tensor, got {flow.dtype} {tuple(flow.shape)}")
    n, fh, fw = flow.shape[:3]
    want = (n, -(-fh // 8), -(-fw // 8))
    if pick.dtype != torch.uint8 or tuple(pick.shape) != want or not pick.is_contiguous():
        raise ValueError(f"pick: expected a contiguous uint8 {want} tensor, got {pick.dtype} {tuple(pick.shape)}")
    ap, bp, op = (_chroma_planes(k, t, p, n) for k, t, p in (("a", a, a_planes), ("b", b, b_planes), ("out", out, out_planes)))
    if not len(ap) == len(bp) == len(op) == 2:
        raise ValueError("a_planes, b_planes and out_planes are two planes each (U, V)")
    fn = lib().fiunet_chroma_fill_p10 if bits == 10 else lib().fiunet_chroma_fill_u8
    check(fn(a.data_ptr(), resize_plane_array(ap), b.data_ptr(), resize_plane_array(bp), flow.data_ptr(), fh, fw,
             pick.data_ptr(), int(sub[0]), int(sub[1]), n, out.data_ptr(), resize_plane_array(op), _stream(a, stream)),
          "fiunet_chroma_fill_" + ("p10" if bits == 10 else "u8"))


# include/fiunet.h: enum fiunet_deint
DEINT_TFF, DEINT_BFF = 0, 1
DEINT_FIELD_RATE, DEINT_FRAME_RATE = 0, 1
DEINT_ADAPTIVE, DEINT_BOB, DEINT_NO_SPATIAL_CHECK = 0, 1, 256


def deinterlace(src: "torch.Tensor", n_src: int, src_planes, dst: "torch.Tensor", dst_planes, first: int, n_frames: int,
                order: int, rate: int, method_flags: int, bits: int, stream=None) -> None:
    """fiunet_deinterlace_u8 / fiunet_deinterlace_p10: frames first .. first + n_frames - 1 of the window of n_src frames
    in the dense buffer `src` -> n_frames (DEINT_FRAME_RATE) or 2 * n_frames (DEINT_FIELD_RATE) frames of `dst`, 1..4
    planes (offset, h, w, pitch, step, frame_stride) in samples from each tensor's first element.  ValueError, before the
    call, where well-formed planes reach past either tensor."""
    src_planes, dst_planes = [tuple(int(v) for v in p) for p in src_planes], [tuple(int(v) for v in p) for p in dst_planes]
    if len(src_planes) != len(dst_planes):
        raise ValueError(f"{len(src_planes)} source planes for {len(dst_planes)} destination planes")
    n_out = n_frames * (2 if rate == DEINT_FIELD_RATE else 1)
    for name, t, planes, n in (("src", src, src_planes, n_src), ("dst", dst, dst_planes, n_out)):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be a dense buffer (the planes carry the pitches)")
        _planes_fit(name + " planes", planes, n, t.numel())
    fn = lib().fiunet_deinterlace_p10 if bits == 10 else lib().fiunet_deinterlace_u8
    check(fn(src.data_ptr(), n_src, resize_plane_array(src_planes), dst.data_ptr(), resize_plane_array(dst_planes),
             len(src_planes), first, n_frames, order, rate, method_flags, _stream(src, stream)),
          "fiunet_deinterlace_" + ("p10" if bits == 10 else "u8"))


class WeaveEntry(ctypes.Structure):
    """include/fiunet.h: fiunet_weave_entry (an output frame: the rows of the kept parity from window frame `keep`, the
    others from `other`)."""
    _fields_ = [("keep", ctypes.c_uint32), ("other", ctypes.c_uint32)]


def weave_entries(entries):
    """A sequence of (keep, other) int pairs -> the C array of fiunet_weave_entry (None when empty).  ValueError on a value
    that does not fit 32 bits unsigned (the library checks the rest)."""
    n = len(entries)
    if not n:
        return None
    arr = (WeaveEntry * n)()
    for k, (keep, other) in enumerate(entries):
        if not (0 <= keep < 1 << 32 and 0 <= other < 1 << 32):
            raise ValueError(f"entry {k} = {(keep, other)} does not fit 32 bits unsigned")
        arr[k] = WeaveEntry(keep, other)
    return arr


def field_match(src: "torch.Tensor", n_src: int, plane, first: int, n_frames: int, order: int, threshold: int,
                scores: "torch.Tensor", bits: int, stream=None) -> None:
    """fiunet_field_match_u8 / fiunet_field_match_p10: MAX-ACCUMULATES the comb scores (p, c, n) of frames first .. first +
    n_frames - 1 of the window of n_src frames in the dense buffer `src`, on one plane (offset, h, w, pitch, step,
    frame_stride) in samples from the tensor's first element, into the contiguous int32 `scores` [n_frames, 3] (int32 on
    the torch side: a score is at most 1024).  ValueError, before the call, where a well-formed plane reaches past `src`."""
    plane = tuple(int(v) for v in plane)
    if not src.is_contiguous():
        raise ValueError("src must be a dense buffer (the plane carries the pitch)")
    _planes_fit("src plane", [plane], n_src, src.numel())
    if scores.dtype != torch.int32 or tuple(scores.shape) != (n_frames, 3) or not scores.is_contiguous():
        raise ValueError(f"scores: expected a contiguous int32 [{n_frames}, 3] tensor, got {scores.dtype} {tuple(scores.shape)}")
    fn = lib().fiunet_field_match_p10 if bits == 10 else lib().fiunet_field_match_u8
    check(fn(src.data_ptr(), n_src, resize_plane_array([plane]), first, n_frames, order, threshold, scores.data_ptr(),
             _stream(src, stream)), "fiunet_field_match_" + ("p10" if bits == 10 else "u8"))


def field_weave(src: "torch.Tensor", n_src: int, src_planes, dst: "torch.Tensor", dst_planes, entries, parity: int,
                bits: int, stream=None) -> None:
    """fiunet_field_weave_u8 / fiunet_field_weave_p10: len(entries) frames of `dst`, frame j with the rows of parity
    `parity` from frame keep_j of the window of n_src frames in the dense buffer `src` and the other rows from frame
    other_j; entries: (keep, other) pairs, read on the host during the call; 1..4 planes (offset, h, w, pitch, step,
    frame_stride) in samples from each tensor's first element.  ValueError, before the call, where well-formed planes reach
    past either tensor."""
    src_planes, dst_planes = [tuple(int(v) for v in p) for p in src_planes], [tuple(int(v) for v in p) for p in dst_planes]
    entries = [tuple(int(v) for v in e) for e in entries]
    if len(src_planes) != len(dst_planes):
        raise ValueError(f"{len(src_planes)} source planes for {len(dst_planes)} destination planes")
    for name, t, planes, n in (("src", src, src_planes, n_src), ("dst", dst, dst_planes, len(entries))):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be a dense buffer (the planes carry the pitches)")
        _planes_fit(name + " planes", planes, n, t.numel())
    fn = lib().fiunet_field_weave_p10 if bits == 10 else lib().fiunet_field_weave_u8
    check(fn(src.data_ptr(), n_src, resize_plane_array(src_planes), dst.data_ptr(), resize_plane_array(dst_planes),
             len(src_planes), weave_entries(entries), len(entries), parity, _stream(src, stream)),
          "fiunet_field_weave_" + ("p10" if bits == 10 else "u8"))
