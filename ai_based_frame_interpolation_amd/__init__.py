"""MI355X-native UNet frame-interpolation forward (drop-in for the reference's model/unet.py
hot path).  See DESIGN.md / INTEGRATION.md.  The HIP extension (libfiunet_hip.so) is loaded
lazily on the first forward; nothing here falls back to CPU."""
from .unet import FrameInterpolationUNet, GraphedForward, UNet, count_parameters  # noqa: F401
from .inference import (  # noqa: F401
    FrameInterpolator, generate_multiple_intermediate_frames, interpolate_frames,
    interpolate_sequence, interpolate_sequence_host, interpolate_sequence_nv12, interpolate_sequence_p10,
    interpolate_sequence_rgb_packed, interpolate_sequence_yuv, interpolate_sequence_yuv420, interpolate_sequence_yuv420p10, load_model,
    postprocess_image, preprocess_image, sequence_pair_fn,
)
from .serving import InterpolationService  # noqa: F401
from .colour import (  # noqa: F401
    SurfaceLayout, i420_frame_bytes, nv12_to_rgb, p010_to_rgb, rgb_to_nv12, rgb_to_p010, rgb_to_yuv420,
    rgb_to_yuv420p10, yuv420_to_rgb, yuv420p10_frame_samples, yuv420p10_to_rgb,
    YUV_FORMATS, rgb_to_yuv, yuv_frame_samples, yuv_to_rgb,
)
from .packed import PackedLayout  # noqa: F401
from . import chroma, colour, deinterlace, evaluation, holdout, ivtc, layout, metrics, optical_flow, packed, resize, retime, scene, serving, stream, synthetic, tiling, transport, video, wire10  # noqa: F401

__all__ = [
    "FrameInterpolationUNet", "GraphedForward", "UNet", "count_parameters", "FrameInterpolator",
    "generate_multiple_intermediate_frames", "interpolate_frames", "interpolate_sequence",
    "interpolate_sequence_host", "interpolate_sequence_yuv420", "interpolate_sequence_p10",
    "interpolate_sequence_yuv420p10", "sequence_pair_fn", "colour", "i420_frame_bytes",
    "yuv420_to_rgb", "rgb_to_yuv420", "yuv420p10_frame_samples", "yuv420p10_to_rgb", "rgb_to_yuv420p10",
    "transport", "optical_flow",
    "load_model", "postprocess_image", "preprocess_image", "evaluation", "metrics", "tiling", "video",
    "InterpolationService", "serving", "synthetic", "scene", "stream", "retime",
    "SurfaceLayout", "nv12_to_rgb", "rgb_to_nv12", "p010_to_rgb", "rgb_to_p010", "interpolate_sequence_nv12",
    "packed", "PackedLayout", "interpolate_sequence_rgb_packed", "holdout",
    "YUV_FORMATS", "yuv_to_rgb", "rgb_to_yuv", "yuv_frame_samples", "interpolate_sequence_yuv", "resize",
    "wire10", "layout", "chroma", "deinterlace", "ivtc",
]
