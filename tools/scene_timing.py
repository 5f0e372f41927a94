"""Time scene-cut detection and the hold against the video loop they ride on.

  detect        scene.detect_cuts on an N-frame 1080p I420 clip resident in HBM (int64 zeroing, fiunet_pair_sad_u8
                over the clip, fiunet_scene_cuts)
  hold_none     fiunet_hold_cut_frames on the 2N-1-frame result with no interval flagged (every workgroup exits)
  hold_all      the same with every interval flagged (N-1 frames copied; a real clip has a cut every few seconds)
  loop          interpolate_sequence_yuv420 on the same clip, RGB network, batch 8, --precision

Device time from HIP events around `--iters` back-to-back calls after `--warmup` calls; each measurement is repeated
`--reps` times, interleaved, and the median and the spread are printed (the protocol of tools/colour_timing.py).  One
JSON line last.

    python tools/scene_timing.py [--frames 33 --height 1080 --width 1920 --precision bf16]
"""
import argparse

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=33)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--precision", default="bf16")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--loop-iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("scene_timing")
    report = H.Report(a.out)
    n, h, w = a.frames, a.height, a.width
    fb = P.i420_frame_bytes(h, w)
    m, _ = H.seeded_model(3, a.precision, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    frames = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device=dev, generator=g)
    out = P.interpolate_sequence_yuv420(m, frames, h, w)
    none = torch.zeros(n - 1, dtype=torch.uint8, device=dev)
    every = torch.ones(n - 1, dtype=torch.uint8, device=dev)

    cases = {
        "detect": lambda: P.scene.detect_cuts(frames, 10.0, 8),
        "hold_none": lambda: P.scene.hold_cut_frames(out, none, 2),
        "hold_all": lambda: P.scene.hold_cut_frames(out, every, 2),
        "loop": lambda: P.interpolate_sequence_yuv420(m, frames, h, w),
    }
    iters = {k: a.loop_iters if k == "loop" else a.iters for k in cases}
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=iters)
    med = {k: H.summary(v)[0] for k, v in ms.items()}
    pairs = n - 1
    res = {"shape": [n, h, w], "precision": a.precision, "ms": med,
           "spread_ms": {k: [min(v), max(v)] for k, v in ms.items()},
           "detect_gb_per_s": n * fb / (med["detect"] * 1e-3) / 1e9,
           "loop_pairs_per_s": pairs / (med["loop"] * 1e-3),
           "held_frame_us": 1e3 * (med["hold_all"] - med["hold_none"]) / pairs,
           "share_detect_plus_empty_hold": (med["detect"] + med["hold_none"]) / med["loop"],
           "share_every_interval_held": (med["detect"] + med["hold_all"]) / med["loop"],
           "protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=f"{a.iters} (scene kernels) / {a.loop_iters} (loop)")}
    for k in cases:
        report.say(f"{k:10s} {med[k]:9.3f} ms  (reps {min(ms[k]):.3f}-{max(ms[k]):.3f})")
    report.say(f"detect reads {res['detect_gb_per_s']:.0f} GB/s of input; loop {res['loop_pairs_per_s']:.0f} pairs/s; "
               f"one held frame {res['held_frame_us']:.1f} us")
    report.say(f"share of the loop: detect + empty hold {100 * res['share_detect_plus_empty_hold']:.3f} %, "
               f"every interval held {100 * res['share_every_interval_held']:.3f} %")
    report.finish(res)


if __name__ == "__main__":
    main()
