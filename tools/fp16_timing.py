"""Time precision "fp16" against "bf16" on the benchmark's network.

  B=8 1080p   frames/s of the fp32-in forward, gray network (bench.py's headline workload and weights)
  256x256     latency of ONE pair (the reference's own operating point)

Device time from HIP events around `--iters` back-to-back forwards after `--warmup` forwards of the same shape; the
precisions alternate inside every repetition (drift on a shared host hits both alike), `--reps` repetitions, median and
spread printed.  One JSON line last.

    python tools/fp16_timing.py [--precisions bf16,fp16 --reps 5]
"""
import argparse

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from bench import make_bench_model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,fp16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("fp16_timing")
    report = H.Report(a.out)
    precs = a.precisions.split(",")
    m = make_bench_model(precs[0]).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    shapes = {"b8_1080p": (8, 1080, 1920, a.iters), "b1_256": (1, 256, 256, 20 * a.iters)}
    frames = {k: [torch.rand((b, 1, h, w), device=dev, generator=g) * 2 - 1 for _ in range(2)]
              for k, (b, h, w, _) in shapes.items()}

    def case(p, f1, f2):
        def fn():
            if m.precision != p:   # (a plain attribute, read by each forward; stored once per timing, not per call)
                m.precision = p
            m(f1, f2)
        return fn
    cases = {(p, k): case(p, *frames[k]) for p in precs for k in shapes}
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters={(p, k): shapes[k][3] for p, k in cases})
    res = {"protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=f"{a.iters} (1080p) / {20 * a.iters} (256x256)",
                                  what="forwards"),
           "network": "bench.py gray 2->1, bilinear", "b8_1080p_frames_per_s": {}, "b1_256_ms": {}, "spread_ms": {}}
    for p in precs:
        med = {k: H.summary(ms[p, k])[0] for k in shapes}
        res["b8_1080p_frames_per_s"][p] = round(8 * 1000.0 / med["b8_1080p"], 2)
        res["b1_256_ms"][p] = round(med["b1_256"], 4)
        res["spread_ms"][p] = {k: [round(min(ms[p, k]), 4), round(max(ms[p, k]), 4)] for k in shapes}
        report.say(f"{p:6s} B=8 1080p {res['b8_1080p_frames_per_s'][p]:8.2f} frames/s ({med['b8_1080p']:.3f} ms)   "
                   f"one 256x256 pair {med['b1_256']:.4f} ms")
    if "bf16" in precs and "fp16" in precs:
        res["fp16_over_bf16_1080p"] = round(res["b8_1080p_frames_per_s"]["fp16"] / res["b8_1080p_frames_per_s"]["bf16"], 4)
        res["fp16_over_bf16_256_latency"] = round(res["b1_256_ms"]["fp16"] / res["b1_256_ms"]["bf16"], 4)
    report.finish(res)


if __name__ == "__main__":
    main()
