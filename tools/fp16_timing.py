"""Time precision "fp16" against "bf16" on the benchmark's network.

  B=8 1080p   frames/s of the fp32-in forward, gray network (bench.py's headline workload and weights)
  256x256     latency of ONE pair (the reference's own operating point)

Device time from HIP events around `--iters` back-to-back forwards after `--warmup` forwards of the same shape; the
precisions alternate inside every repetition (drift on a shared host hits both alike), `--reps` repetitions, median and
spread printed.  One JSON line last.

    python tools/fp16_timing.py [--precisions bf16,fp16 --reps 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import make_bench_model  # noqa: E402


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16,fp16")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "fp16_timing measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    precs = a.precisions.split(",")
    m = make_bench_model(precs[0]).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(0)
    cases = {}
    for key, (b, h, w, iters) in {"b8_1080p": (8, 1080, 1920, a.iters), "b1_256": (1, 256, 256, 20 * a.iters)}.items():
        f1, f2 = (torch.rand((b, 1, h, w), device=dev, generator=g) * 2 - 1 for _ in range(2))
        cases[key] = (b, iters, lambda f1=f1, f2=f2: m(f1, f2))
    ms = {p: {k: [] for k in cases} for p in precs}
    for p in precs:
        m.precision = p
        for _, _, fn in cases.values():
            for _ in range(a.warmup):
                fn()
    torch.cuda.synchronize()
    for _ in range(a.reps):
        for p in precs:
            m.precision = p
            for k, (_, iters, fn) in cases.items():
                ms[p][k].append(_time(fn, iters))
    res = {"protocol": f"HIP events, {a.warmup} warm-up forwards per case, median of {a.reps} interleaved reps of "
                       f"{a.iters} (1080p) / {20 * a.iters} (256x256) forwards", "network": "bench.py gray 2->1, bilinear",
           "b8_1080p_frames_per_s": {}, "b1_256_ms": {}, "spread_ms": {}}
    for p in precs:
        med = {k: statistics.median(v) for k, v in ms[p].items()}
        res["b8_1080p_frames_per_s"][p] = round(8 * 1000.0 / med["b8_1080p"], 2)
        res["b1_256_ms"][p] = round(med["b1_256"], 4)
        res["spread_ms"][p] = {k: [round(min(v), 4), round(max(v), 4)] for k, v in ms[p].items()}
        print(f"{p:6s} B=8 1080p {res['b8_1080p_frames_per_s'][p]:8.2f} frames/s ({med['b8_1080p']:.3f} ms)   "
              f"one 256x256 pair {med['b1_256']:.4f} ms")
    if "bf16" in precs and "fp16" in precs:
        res["fp16_over_bf16_1080p"] = round(res["b8_1080p_frames_per_s"]["fp16"] / res["b8_1080p_frames_per_s"]["bf16"], 4)
        res["fp16_over_bf16_256_latency"] = round(res["b1_256_ms"]["fp16"] / res["b1_256_ms"]["bf16"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
