"""Time the colour-video conversion kernels and their share of the RGB network's step (DESIGN.md "Colour video").

  yuv420_to_rgb / rgb_to_yuv420   B=8 1080p: ms per call and GB/s (bytes read + written: F + 3*H*W per frame)
  forward_u8 vs forward_yuv420    the RGB network at B=8 1080p bf16 on planar RGB and on packed I420 frames; the
                                  difference is the cost of the three conversions inside forward_yuv420

Device time from HIP events around `--iters` back-to-back calls after `--warmup` calls of the same shape; each
measurement is repeated `--reps` times, interleaved, and the median and the spread are printed.  One JSON line last.

    python tools/colour_timing.py [--batch 8 --height 1080 --width 1920 --precision bf16]
"""
import argparse

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--conv-iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("colour_timing")
    report = H.Report(a.out)
    b, h, w = a.batch, a.height, a.width
    fb = P.i420_frame_bytes(h, w)
    m, _ = H.seeded_model(3, a.precision, dev, b)
    g = torch.Generator(device=dev).manual_seed(0)
    y1 = torch.randint(0, 256, (b, fb), dtype=torch.uint8, device=dev, generator=g)
    y2 = torch.randint(0, 256, (b, fb), dtype=torch.uint8, device=dev, generator=g)
    r1, r2 = P.yuv420_to_rgb(y1, h, w), P.yuv420_to_rgb(y2, h, w)
    rgb_out = torch.empty_like(r1)
    yuv_out = torch.empty_like(y1)

    cases = {
        "yuv420_to_rgb": lambda: P.yuv420_to_rgb(y1, h, w, out=rgb_out),
        "rgb_to_yuv420": lambda: P.rgb_to_yuv420(r1, out=yuv_out),
        "forward_u8": lambda: m.forward_u8(r1, r2, out=rgb_out),
        "forward_yuv420": lambda: m.forward_yuv420(y1, y2, h, w, out=yuv_out),
    }
    iters = {k: a.iters if k.startswith("forward") else a.conv_iters for k in cases}
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=iters)
    med = {k: H.summary(v)[0] for k, v in ms.items()}
    conv_bytes = b * (fb + 3 * h * w)
    res = {"shape": [b, h, w], "precision": a.precision, "ms": med,
           "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
           "gb_per_s": {k: conv_bytes / (med[k] * 1e-3) / 1e9 for k in ("yuv420_to_rgb", "rgb_to_yuv420")},
           "conversion_share_of_step": (med["forward_yuv420"] - med["forward_u8"]) / med["forward_yuv420"],
           "protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=f"{a.conv_iters} (conversions) / {a.iters} (forwards)")}
    for k in cases:
        extra = f"  {res['gb_per_s'][k]:.0f} GB/s" if k in res["gb_per_s"] else ""
        report.say(f"{k:16s} {med[k]:8.3f} ms  (reps {min(ms[k]):.3f}-{max(ms[k]):.3f}){extra}")
    report.say(f"conversion share of the forward_yuv420 step: {100 * res['conversion_share_of_step']:.2f} %")
    report.finish(res)


if __name__ == "__main__":
    main()
