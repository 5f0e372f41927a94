"""Command line: `python -m ai_based_frame_interpolation_amd.cli video --input IN --output OUT [--factor 2] ...`

The reference's `main.py video` flags (--input, --output, --factor, --model, --device), plus --precision, --matrix,
--siting, --scene-cut, --batch, --chunk-frames, the frame-rate conversion's --fps, --src-fps, --time-depth and
--retime, --dedup and --max-gap for repeated frames, and --raw / --size (and --packing) for headerless NV12, packed RGB or 4:2:2 / 4:4:4 YUV video.  The command always streams (stream.py), so a clip of any length runs in memory bounded by
the chunk, and `-` is standard input / output: it sits in an ffmpeg pipe

    ffmpeg -i in.mkv -f yuv4mpegpipe - | python -m ai_based_frame_interpolation_amd.cli video --input - --output - \\
        --model best_model.pth | ffmpeg -f yuv4mpegpipe -i - out.mkv

With `--fps 60000/1001` (a fraction or an integer, never a decimal) the output has that frame rate instead of
--factor times the input's (retime.py): 23.976 -> 59.94, 24 -> 60, 25 -> 60, 50 -> 120.

With `--shutter 1/2` (a fraction in 0 .. 1 of the OUTPUT frame period, never a decimal) --fps may be any rate, a lower one
included - 59.94 -> 50, 60 -> 24, 30 -> 25 - and every output frame is the clip averaged over the time such a shutter is
open, the exposure of the slower camera (retime.py); `--shutter 0` point-samples.  After `deinterlace`:

    ... cli deinterlace --input - --output - | python -m ai_based_frame_interpolation_amd.cli video --input - \\
        --output - --fps 50 --shutter 1/2 --model best_model.pth | ffmpeg -f yuv4mpegpipe -i - out.mkv

With `--dedup 0` (a tolerance in code values; `--max-gap 4`) runs of repeated frames - telecined film, animation on twos,
a stalled capture - are re-timed instead of interpolated across (retime.py); one line on standard error
says how many repeated frames were re-timed.

With `--chroma motion` a grayscale checkpoint carries the chroma of colour Y4M video along the motion instead of averaging
it (chroma.py); one line on standard error says in how many blocks the chroma was warped.

With `--raw nv12 --size 1920x1080 --src-fps 24` input and output are headerless tight NV12 frames, the layout hardware
decoders and encoders use, converted on the device without a repack:

    ffmpeg -i in.mkv -f rawvideo -pix_fmt nv12 - | python -m ai_based_frame_interpolation_amd.cli video --input - \\
        --output - --raw nv12 --size 1920x1080 --src-fps 24 --model rgb.pth | \\
        ffmpeg -f rawvideo -pix_fmt nv12 -s 1920x1080 -r 48 -i - out.mkv

`--raw rgb24` (or bgr24, rgba, bgra) does the same for packed RGB frames - screen capture, renders, image sequences -
which keep their colour: no chroma subsampling and no colour matrix on the way (--matrix and --siting
are not used; the alpha of an inserted rgba / bgra frame is the rounded average of its neighbours'):

    ffmpeg -i capture.mkv -f rawvideo -pix_fmt rgb24 - | python -m ai_based_frame_interpolation_amd.cli video \\
        --input - --output - --raw rgb24 --size 1920x1080 --src-fps 30 --model rgb.pth | \\
        ffmpeg -f rawvideo -pix_fmt rgb24 -s 1920x1080 -r 60 -i - out.mkv

`--raw yuv422p10le` (or yuv422p, yuv444p, yuv444p10le, uyvy422, yuyv422) takes 4:2:2 and 4:4:4 video at its own chroma
resolution: what ProRes, DNxHR and XDCAM decode to and what capture cards deliver.  --matrix and
--siting apply as for nv12 (siting defaults to mpeg2; bt2020 with the 10-bit formats); run 10-bit video in fp16:

    ffmpeg -i prores.mov -f rawvideo -pix_fmt yuv422p10le - | python -m ai_based_frame_interpolation_amd.cli video \\
        --input - --output - --raw yuv422p10le --size 1920x1080 --src-fps 24 --precision fp16 --model rgb.pth | \\
        ffmpeg -f rawvideo -pix_fmt yuv422p10le -s 1920x1080 -r 48 -i - -c:v prores_ks -profile:v 3 out.mov

    ffmpeg -f decklink -i 'DeckLink Mini Recorder' -f rawvideo -pix_fmt uyvy422 - | \\
        python -m ai_based_frame_interpolation_amd.cli video --input - --output - --raw uyvy422 --size 1920x1080 \\
        --src-fps 30 --model rgb.pth | ffmpeg -f rawvideo -pix_fmt uyvy422 -s 1920x1080 -r 60 -i - out.mkv

`--raw yuv422p10le --packing v210` (or y210le, p210le) takes the same samples as 10-bit capture cards and uncompressed
broadcast files pack them (wire10.py): the frames are unpacked and packed on the GPU, so ffmpeg neither
unpacks v210 to yuv422p10le before the pipe nor repacks behind it.  The result is the yuv422p10le route's, byte for byte:

    ffmpeg -f decklink -raw_format yuv422p10 -i 'DeckLink Mini Recorder' -c:v v210 -f rawvideo - | \\
        python -m ai_based_frame_interpolation_amd.cli video --input - --output - --raw yuv422p10le --packing v210 \\
        --size 1920x1080 --src-fps 30 --precision fp16 --model rgb.pth | \\
        ffmpeg -f rawvideo -c:v v210 -s 1920x1080 -r 60 -i - -c:v v210 out.mov

Standard output then carries nothing but video: the model-loading lines go to standard error.  The network (grayscale
2->1 or RGB 6->3) is read from the checkpoint.

`evaluate` scores a checkpoint on a clip by hold-out (holdout.py): every held-out frame is rebuilt from
its two neighbours by the network, by blending and by repeating a frame, and compared with the frame that was there:

    ffmpeg -i clip.mkv -f yuv4mpegpipe - | python -m ai_based_frame_interpolation_amd.cli evaluate --input - \\
        --model best_model.pth --json scores.json --csv frames.csv

The summary table goes to standard error, the whole result to --json and one line per scored frame to --csv.  Raw
video is scored as the `video` command reads it (--raw, --size; --src-fps for the time stamps), and --scene-cut leaves
the held-out frames next to a hard cut out of the summary:

    ffmpeg -i clip.mkv -f rawvideo -pix_fmt nv12 - | python -m ai_based_frame_interpolation_amd.cli evaluate \\
        --input - --raw nv12 --size 1920x1080 --src-fps 24 --model rgb_model.pth --scene-cut 10 --json scores.json

`deinterlace` turns the fields of interlaced video into frames (deinterlace.py) and needs no model.  It
sits in front of `video`, which - like `evaluate` - warns where a Y4M header says interlaced and treats the frames as
they are:

    ffmpeg -i 1080i.mxf -f yuv4mpegpipe - | python -m ai_based_frame_interpolation_amd.cli deinterlace --input - \\
        --output - | python -m ai_based_frame_interpolation_amd.cli video --input - --output - --model best_model.pth \\
        --fps 100 | ffmpeg -f yuv4mpegpipe -i - out.mkv

--order auto (the default) reads `It` / `Ib` off the Y4M header; --rate field (the default) writes one frame per field
at twice the rate; --raw / --size / --packing take headerless video as `video` does, with --order tff or bff.

`ivtc` undoes 2:3 pulldown (ivtc.py): hard-telecined film - 24 fps carried as 29.97 fps interlaced video -
becomes its film frames again, byte for byte, at 23.976 fps, which `video --fps` then takes to any rate.  It needs no
model, takes `deinterlace`'s --order / --raw / --size / --packing / --src-fps / --chunk-frames, and prints what it matched,
flagged and dropped to standard error:

    ffmpeg -i telecined.vob -f yuv4mpegpipe - | python -m ai_based_frame_interpolation_amd.cli ivtc --input - \\
        --output - | python -m ai_based_frame_interpolation_amd.cli video --input - --output - --model best_model.pth \\
        --fps 60000/1001 | ffmpeg -f yuv4mpegpipe -i - out.mkv

--no-decimate writes every matched frame at the source rate; --cycle, --comb-threshold, --combed and --fallback are the
parameters of the definition.

`--resize WIDTHxHEIGHT` on either command resizes every frame on the GPU right after its upload (resize.py, DESIGN.md
3.3q): `video` then writes a clip of that size, `evaluate` scores the checkpoint at that size - 256x256 is what the
reference trains and evaluates at - and says so in its table.  --size stays the size of the --raw source.
`--resize-filter area` (with --resize) down-scales without aliasing: every sample is the rounded mean of the source area
it covers; the default, linear, is the two-tap filter of the reference's cv2.resize.

    python -m ai_based_frame_interpolation_amd.cli evaluate --input clip.y4m --resize 256x256 --model best_model.pth
    python -m ai_based_frame_interpolation_amd.cli video --input uhd.y4m --output hd.y4m --resize 1920x1080 \
        --resize-filter area --model rgb_model.pth
"""
from __future__ import annotations

import argparse
import contextlib
import sys

import torch

from . import retime

FIRST_CONV = "unet.inc.double_conv.0.weight"


def frame_channels_of(state_dict) -> int:
    """1 (grayscale 2->1 network) or 3 (RGB 6->3) from the input channels of the first convolution."""
    sd = state_dict.get("model_state_dict", state_dict)
    if FIRST_CONV not in sd:
        raise ValueError(f"checkpoint has no {FIRST_CONV}: not a frame-interpolation UNet")
    cin = int(sd[FIRST_CONV].shape[1])
    if cin not in (2, 6):
        raise ValueError(f"{FIRST_CONV} has {cin} input channels: expected 2 (grayscale) or 6 (RGB)")
    return cin // 2


def _scene_cut(v: str):
    return None if v.lower() in ("none", "off") else float(v)


def _siting(v: str):
    return None if v.lower() == "none" else v


def _fps(v: str):
    try:
        return retime.parse_fps(v)
    except ValueError as e:   # argparse prints an ArgumentTypeError's own text
        raise argparse.ArgumentTypeError(str(e)) from None


def _shutter(v: str):
    try:
        return retime.check_shutter(v)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _dedup(v: str):
    try:
        return retime.check_dedup(float(v))[0]
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e)) from None


def _size(v: str):
    """"WxH" -> (width, height)"""
    parts = v.lower().split("x")
    if len(parts) != 2 or not all(p.isdigit() and int(p) > 0 for p in parts):
        raise argparse.ArgumentTypeError(f"expected WIDTHxHEIGHT such as 1920x1080, got {v!r}")
    return int(parts[0]), int(parts[1])


def _methods(v: str):
    names = tuple(s.strip() for s in v.split(",") if s.strip())
    from .holdout import ALL_METHODS as known
    bad = [n for n in names if n not in known]
    if not names or bad or len(set(names)) != len(names):
        raise argparse.ArgumentTypeError(f"expected a comma-separated choice of {', '.join(known)}, got {v!r}")
    return names


PACKING_CHOICES = ("v210", "y210le", "p210le")   # wire10.PACKINGS
CHROMA_CHOICES = ("average", "motion")           # chroma.MODES
RAW_CHOICES = ("nv12", "rgb24", "bgr24", "rgba", "bgra", "yuv422p", "yuv444p", "yuv422p10le", "yuv444p10le", "uyvy422",
               "yuyv422")


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m ai_based_frame_interpolation_amd.cli",
                                 description="AI frame interpolation on the MI355X")
    sub = ap.add_subparsers(dest="command", required=True)
    v = sub.add_parser("video", help="Interpolate frames in a video (Y4M or .npy; '-' is stdin / stdout)")
    v.add_argument("--input", required=True, help="Input video path, or - for standard input (Y4M)")
    v.add_argument("--output", required=True, help="Output video path, or - for standard output (Y4M)")
    v.add_argument("--factor", type=int, default=2, help="Interpolation factor (a power of two)")
    v.add_argument("--model", default="best_model.pth", help="Path to trained model")
    v.add_argument("--device", default="auto", help="Device to use (cuda/auto)")
    v.add_argument("--precision", default=None, help="fp32 / bf16x2 / bf16 / fp16 (default: the library's)")
    v.add_argument("--weight-prep", default=None, choices=("host", "device"),
                   help="Where the checkpoint is folded, packed and rounded (default: host, or FIUNET_WEIGHT_PREP)")
    v.add_argument("--matrix", default="bt709", help="YUV matrix of colour video through the RGB network")
    v.add_argument("--siting", type=_siting, default=None, help="Chroma siting jpeg / mpeg2 (default: from the tag)")
    v.add_argument("--scene-cut", type=_scene_cut, default=None, help="Scene-cut threshold in (0, 100], or none")
    v.add_argument("--batch", type=int, default=8, help="Frame pairs per forward")
    v.add_argument("--chunk-frames", type=int, default=None, help="Frame pairs per streamed chunk (default 4 x batch)")
    v.add_argument("--fps", type=_fps, default=None,
                   help="Output frame rate as n or n/d (60, 60000/1001); replaces --factor")
    v.add_argument("--src-fps", type=_fps, default=None,
                   help="Source frame rate as n or n/d (default: the Y4M header's)")
    v.add_argument("--time-depth", type=int, default=2, choices=(1, 2, 3, 4), help="Bisection levels under --fps")
    v.add_argument("--retime", default="blend", choices=retime.VIDEO_MODES,
                   help="How --fps makes a frame between two bisection frames: blend (a cross-fade), nearest (the "
                        "closer one) or motion (both warped along the optical flow between them to the frame's own "
                        "time: no double edges where things move, at the cost of one flow per pair)")
    v.add_argument("--shutter", type=_shutter, default=None, metavar="N/D",
                   help="Synthesize a shutter open for N/D (0 .. 1) of the output frame period; --fps may then be any "
                        "rate, a lower one included (60 -> 24, 60000/1001 -> 50); 1/2 is 180 degrees, 0 point-samples")
    v.add_argument("--dedup", type=_dedup, default=None, metavar="TOL",
                   help="Re-time repeated frames (telecine, animation on twos, stalled capture): frames that differ "
                        "by at most TOL code values count as repeats (0: equal frames)")
    v.add_argument("--max-gap", type=int, default=4, choices=tuple(range(2, 9)),
                   help="Longest run of equal frames that --dedup re-times (a longer hold stays a hold)")
    v.add_argument("--raw", default=None, choices=RAW_CHOICES,
                   help="Headerless raw video in and out (tight NV12, packed RGB or 4:2:2 / 4:4:4 YUV frames, named as "
                        "ffmpeg's -pix_fmt); needs --size and --src-fps")
    v.add_argument("--packing", default=None, choices=PACKING_CHOICES,
                   help="With --raw yuv422p10le: the frames are packed on the wire as v210, y210le or p210le, in and out")
    v.add_argument("--size", type=_size, default=None, help="Frame size of --raw video as WIDTHxHEIGHT")
    v.add_argument("--resize", type=_size, default=None, metavar="WIDTHxHEIGHT",
                   help="Resize every frame on the GPU before it is interpolated; the output has this size (--size "
                        "stays the size of the --raw source)")
    v.add_argument("--resize-filter", default=None, choices=("linear", "area"),
                   help="Filter of --resize: linear (default; cv2.resize's two taps per axis) or area (alias-free "
                        "down-scaling: the mean of the covered source area)")
    v.add_argument("--chroma", default="average", choices=CHROMA_CHOICES,
                   help="Chroma of the frames the grayscale network inserts into colour Y4M video: average (of the two "
                        "neighbours) or motion (warped along the optical flow where the network's luma agrees with it: "
                        "no colour ghosts around what moves, at the cost of one flow per inserted frame)")
    e = sub.add_parser("evaluate", help="Score a checkpoint on a clip by hold-out (Y4M, .npy or --raw; '-' is stdin)")
    e.add_argument("--input", required=True,
                   help="Clip to score: a .y4m or .npy path, or - for standard input (Y4M, or --raw video)")
    e.add_argument("--model", default="best_model.pth", help="Path to trained model")
    e.add_argument("--device", default="auto", help="Device to use (cuda/auto)")
    e.add_argument("--triplets", default="sliding", choices=("sliding", "disjoint"),
                   help="sliding: every frame but the first and last is held out; disjoint: every second frame")
    e.add_argument("--methods", type=_methods, default=("unet", "linear", "repeat"),
                   help="Comma-separated: unet, linear (blend), repeat (frame duplication), motion (Farneback flow, "
                        "symmetric warp), optical_flow (the reference evaluators' flow formula)")
    e.add_argument("--precision", default=None, help="fp32 / bf16x2 / bf16 / fp16 (default: the library's)")
    e.add_argument("--weight-prep", default=None, choices=("host", "device"),
                   help="Where the checkpoint is folded, packed and rounded (default: host, or FIUNET_WEIGHT_PREP)")
    e.add_argument("--matrix", default="bt709", help="YUV matrix of colour video through the RGB network")
    e.add_argument("--siting", type=_siting, default=None, help="Chroma siting jpeg / mpeg2 (default: from the tag)")
    e.add_argument("--batch", type=int, default=8, help="Frame pairs per forward")
    e.add_argument("--chunk-frames", type=int, default=None, help="Held-out frames per chunk (default 4 x batch)")
    e.add_argument("--src-fps", type=_fps, default=None,
                   help="Source frame rate as n or n/d, for the time stamps (default: the Y4M header's)")
    e.add_argument("--raw", default=None, choices=RAW_CHOICES,
                   help="Headerless raw video (tight frames, named as ffmpeg's -pix_fmt); needs --size")
    e.add_argument("--packing", default=None, choices=PACKING_CHOICES,
                   help="With --raw yuv422p10le: the frames are packed on the wire as v210, y210le or p210le")
    e.add_argument("--size", type=_size, default=None, help="Frame size of --raw video as WIDTHxHEIGHT")
    e.add_argument("--resize", type=_size, default=None, metavar="WIDTHxHEIGHT",
                   help="Resize the clip on the GPU before frames are held out and score it at this size, such as the "
                        "256x256 a checkpoint was trained at (--size stays the size of the --raw source)")
    e.add_argument("--resize-filter", default=None, choices=("linear", "area"),
                   help="Filter of --resize: linear (default; cv2.resize's two taps per axis) or area (alias-free "
                        "down-scaling: the mean of the covered source area)")
    e.add_argument("--scene-cut", type=_scene_cut, default=None,
                   help="Scene-cut threshold in (0, 100], or none: held-out frames next to a cut are left out of the "
                        "summary")
    e.add_argument("--chroma", default="average", choices=CHROMA_CHOICES,
                   help="Chroma of the unet method's frames on colour Y4M video through the grayscale network: average "
                        "or motion (see video --chroma); the u and v rows of the table show the difference")
    e.add_argument("--json", default=None, metavar="FILE", help="Write the whole result here (arrays as lists)")
    e.add_argument("--csv", default=None, metavar="FILE", help="Write one line per scored frame here")
    d = sub.add_parser("deinterlace", help="Deinterlace interlaced video: fields to frames (Y4M or --raw; '-' is stdin / "
                                            "stdout; needs no model)")
    d.add_argument("--input", required=True, help="Interlaced video path, or - for standard input")
    d.add_argument("--output", required=True, help="Output video path, or - for standard output (the input's format)")
    d.add_argument("--order", default="auto", choices=("auto", "tff", "bff"),
                   help="Field order: tff (even rows first in time), bff, or auto (the Y4M header's It / Ib)")
    d.add_argument("--rate", default="field", choices=("field", "frame"),
                   help="field: one frame per field, the frame rate doubles (default); frame: one per frame")
    d.add_argument("--method", default="adaptive", choices=("adaptive", "bob"),
                   help="adaptive: motion-adaptive with an edge-directed spatial estimate (default); bob: the average of "
                        "the rows above and below")
    d.add_argument("--no-spatial-check", action="store_true",
                   help="Leave out the spatial interlacing check of the adaptive method (static areas then pass through "
                        "exactly)")
    d.add_argument("--device", default="auto", help="Device to use (cuda/auto)")
    d.add_argument("--chunk-frames", type=int, default=32, help="Source frames per step (memory is bounded by it)")
    d.add_argument("--src-fps", type=_fps, default=None,
                   help="Source frame rate as n or n/d, for the Y4M header of the result (default: the input header's)")
    d.add_argument("--raw", default=None, choices=RAW_CHOICES,
                   help="Headerless raw video in and out (tight frames, named as ffmpeg's -pix_fmt); needs --size and "
                        "--order tff or bff")
    d.add_argument("--packing", default=None, choices=PACKING_CHOICES,
                   help="With --raw yuv422p10le: the frames are packed on the wire as v210, y210le or p210le, in and out")
    d.add_argument("--size", type=_size, default=None, help="Frame size of --raw video as WIDTHxHEIGHT")
    t = sub.add_parser("ivtc", help="Inverse telecine: hard-telecined film (2:3 pulldown) back to its film frames (Y4M or "
                                    "--raw; '-' is stdin / stdout; needs no model)")
    t.add_argument("--input", required=True, help="Telecined video path, or - for standard input")
    t.add_argument("--output", required=True, help="Output video path, or - for standard output (the input's format)")
    t.add_argument("--order", default="auto", choices=("auto", "tff", "bff"),
                   help="Field order: tff (even rows first in time), bff, or auto (the Y4M header's It / Ib)")
    t.add_argument("--no-decimate", action="store_true",
                   help="Match the fields only: write every frame, at the source rate")
    t.add_argument("--cycle", type=int, default=5, help="Frames per decimation cycle: one of them is dropped (default 5)")
    t.add_argument("--comb-threshold", type=int, default=None,
                   help="T of the comb test (u - m) * (d - m) > T * T (default: 12 at 8 bits, 48 at 10)")
    t.add_argument("--combed", type=int, default=48,
                   help="Largest count of combed samples in a 16 x 64 block that a matched frame may have (default 48)")
    t.add_argument("--fallback", default="deinterlace", choices=("deinterlace", "keep"),
                   help="A frame no pairing cleans: deinterlace it (default) or keep the best weave")
    t.add_argument("--device", default="auto", help="Device to use (cuda/auto)")
    t.add_argument("--chunk-frames", type=int, default=32, help="Source frames per step (memory is bounded by it)")
    t.add_argument("--src-fps", type=_fps, default=None,
                   help="Source frame rate as n or n/d, for the Y4M header of the result (default: the input header's)")
    t.add_argument("--raw", default=None, choices=RAW_CHOICES,
                   help="Headerless raw video in and out (tight frames, named as ffmpeg's -pix_fmt); needs --size and "
                        "--order tff or bff")
    t.add_argument("--packing", default=None, choices=PACKING_CHOICES,
                   help="With --raw yuv422p10le: the frames are packed on the wire as v210, y210le or p210le, in and out")
    t.add_argument("--size", type=_size, default=None, help="Frame size of --raw video as WIDTHxHEIGHT")
    return ap


def parse_args(argv=None) -> argparse.Namespace:
    ap = parser()
    a = ap.parse_args(argv)
    if a.command in ("deinterlace", "ivtc"):
        if a.packing is not None and a.raw != "yuv422p10le":
            ap.error("--packing says how yuv422p10le samples are packed on the wire: pass --raw yuv422p10le with it")
        if a.raw is not None and a.size is None:
            ap.error("--raw needs --size WIDTHxHEIGHT (raw video has no header)")
        if a.raw is None and a.size is not None:
            ap.error("--size describes --raw video")
        if a.raw is not None and a.order == "auto":
            ap.error("--raw video has no header to read the field order from: pass --order tff or --order bff")
        return a
    if a.chunk_frames is None:
        a.chunk_frames = 4 * a.batch
    if a.command in ("evaluate", "video"):
        if a.packing is not None and a.raw != "yuv422p10le":
            ap.error("--packing says how yuv422p10le samples are packed on the wire: pass --raw yuv422p10le with it")
        if a.resize_filter is not None and a.resize is None:
            ap.error("--resize-filter names the filter of --resize WIDTHxHEIGHT")
        a.resize_filter = a.resize_filter or "linear"
        if a.chroma == "motion" and (a.raw is not None or a.input.lower().endswith(".npy")):
            ap.error("--chroma motion carries the separate chroma planes of Y4M video through the grayscale network "
                     "along the motion: --raw and .npy video have none")
    if a.command == "evaluate":
        if a.raw is not None and a.size is None:
            ap.error("--raw needs --size WIDTHxHEIGHT (raw video has no header)")
        if a.raw is None and a.size is not None:
            ap.error("--size describes --raw video")
        return a
    if a.command != "video":
        return a
    if a.raw is not None and (a.size is None or a.src_fps is None):
        ap.error("--raw needs --size WIDTHxHEIGHT and --src-fps (raw video has no header)")
    if a.raw is None and a.size is not None:
        ap.error("--size describes --raw video")
    return a


def _refuse_rgb_chroma(chroma: str, frame_channels: int) -> None:
    """ValueError for --chroma motion with an RGB checkpoint, before the model is loaded."""
    if frame_channels == 3:
        from . import chroma as _chroma
        _chroma.refuse_motion(chroma, "the RGB network (its colour goes through the network itself)")


def retimed_repeats(dedup_log, scene_log, max_gap: int) -> int:
    """The number of repeated source frames a run re-timed: the dead intervals inside spans, from the run's logs."""
    dead = [bool(v) for _, d in dedup_log for v in d]
    cuts = [bool(v) for _, f in scene_log for v in f] if scene_log else None
    return sum(ln - 1 for _, ln in retime.dedup_spans(dead, cuts, max_gap))


def run_video(a: argparse.Namespace) -> int:
    from . import stream
    from .inference import FrameInterpolator, load_model
    stream.check_chunk_frames(a.chunk_frames)
    device = torch.device("cuda" if a.device in ("auto", None) else a.device)
    fc = frame_channels_of(torch.load(a.model, map_location="cpu"))
    _refuse_rgb_chroma(a.chroma, fc)
    with contextlib.redirect_stdout(sys.stderr):   # standard output carries the video only
        model = load_model(a.model, device, a.precision, frame_channels=fc, weight_prep=a.weight_prep)
    fi = FrameInterpolator(model=model, device=device, batch=a.batch)
    src = sys.stdin.buffer if a.input == "-" else a.input
    dst = sys.stdout.buffer if a.output == "-" else a.output
    logs = {} if a.packing is None else dict(packing=a.packing)
    if a.chroma != "average":   # (and its count, printed below)
        logs.update(chroma=a.chroma, chroma_log=[])
    if a.shutter is not None:
        logs.update(shutter=a.shutter)
    if a.dedup is not None:   # for the count below (the cut flags too: a run before a cut is not re-timed)
        logs.update(dedup_log=[], scene_log=[] if a.scene_cut is not None else None)
    n = fi.interpolate_video(src, dst, a.factor, matrix=a.matrix, siting=a.siting, scene_cut=a.scene_cut,
                             chunk_frames=a.chunk_frames, fps=a.fps, src_fps=a.src_fps, time_depth=a.time_depth,
                             retime=a.retime, raw=a.raw, width=a.size[0] if a.size else None,
                             height=a.size[1] if a.size else None, dedup=a.dedup, max_gap=a.max_gap,
                             resize=a.resize, resize_filter=a.resize_filter, **logs)
    if a.dedup is not None:
        print(f"re-timed {retimed_repeats(logs['dedup_log'], logs['scene_log'], a.max_gap)} repeated frames",
              file=sys.stderr)
    for warped, blocks in logs.get("chroma_log") or []:
        print(f"chroma warped along the motion in {warped} of {blocks} blocks ({warped / max(blocks, 1):.1%})",
              file=sys.stderr)
    print(f"wrote {n} frames", file=sys.stderr)
    return n


def run_evaluate(a: argparse.Namespace) -> dict:
    import json

    from . import holdout, stream
    from .inference import load_model
    stream.check_chunk_frames(a.chunk_frames)
    device = torch.device("cuda" if a.device in ("auto", None) else a.device)
    fc = frame_channels_of(torch.load(a.model, map_location="cpu"))
    _refuse_rgb_chroma(a.chroma, fc)
    with contextlib.redirect_stdout(sys.stderr):
        model = load_model(a.model, device, a.precision, frame_channels=fc, weight_prep=a.weight_prep)
    src = sys.stdin.buffer if a.input == "-" else a.input
    res = holdout.score_video(model, src, triplets=a.triplets, methods=a.methods, batch=a.batch,
                              chunk_frames=a.chunk_frames, matrix=a.matrix, siting=a.siting, src_fps=a.src_fps,
                              raw=a.raw, width=a.size[0] if a.size else None, height=a.size[1] if a.size else None,
                              scene_cut=a.scene_cut, resize=a.resize, resize_filter=a.resize_filter,
                              **({} if a.packing is None else dict(packing=a.packing)),
                              **({} if a.chroma == "average" else dict(chroma=a.chroma)))
    print(holdout.summary_table(res), file=sys.stderr)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(holdout.to_jsonable(res), f, allow_nan=False)
    if a.csv:
        with open(a.csv, "w") as f:
            f.writelines(line + "\n" for line in holdout.csv_lines(res))
    return res


def run_deinterlace(a: argparse.Namespace) -> int:
    from . import deinterlace
    device = torch.device("cuda" if a.device in ("auto", None) else a.device)
    src = sys.stdin.buffer if a.input == "-" else a.input
    dst = sys.stdout.buffer if a.output == "-" else a.output
    n = deinterlace.deinterlace_video(src, dst, order=a.order, rate=a.rate, method=a.method,
                                      spatial_check=not a.no_spatial_check, chunk_frames=a.chunk_frames, raw=a.raw,
                                      width=a.size[0] if a.size else None, height=a.size[1] if a.size else None,
                                      src_fps=a.src_fps, packing=a.packing, device=device)
    print(f"wrote {n} frames", file=sys.stderr)
    return n


def run_ivtc(a: argparse.Namespace) -> dict:
    from . import ivtc
    device = torch.device("cuda" if a.device in ("auto", None) else a.device)
    src = sys.stdin.buffer if a.input == "-" else a.input
    dst = sys.stdout.buffer if a.output == "-" else a.output
    rep = ivtc.ivtc_video(src, dst, order=a.order, decimate=not a.no_decimate, cycle=a.cycle, threshold=a.comb_threshold,
                          combed=a.combed, fallback=a.fallback, chunk_frames=a.chunk_frames, raw=a.raw,
                          width=a.size[0] if a.size else None, height=a.size[1] if a.size else None, src_fps=a.src_fps,
                          packing=a.packing, device=device)
    m = rep["matches"]
    print(f"matched {rep['frames_in']} frames: p {m['p']}, c {m['c']}, n {m['n']}; combed {len(rep['combed'])}"
          + (f" (frames {', '.join(map(str, rep['combed']))})" if rep["combed"] else "")
          + f"; dropped {len(rep['dropped'])}", file=sys.stderr)
    print(f"wrote {rep['frames_out']} frames", file=sys.stderr)
    return rep


def main(argv=None) -> int:
    a = parse_args(argv)
    if a.command == "deinterlace":
        run_deinterlace(a)
    elif a.command == "ivtc":
        run_ivtc(a)
    elif a.command == "video":
        run_video(a)
    elif a.command == "evaluate":
        run_evaluate(a)
    return 0


if __name__ == "__main__":
    sys.exit(main())
