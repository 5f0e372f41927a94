"""Time the frame-rate conversion (retime.py): its kernel alone and what it costs a streamed run.

  kernel    retime.resample of a 24 -> 60 chunk (p / q = 2 / 5, time_depth 2), 1080p I420 8 bit and C420p10.  A
            streamed chunk's grid comes fresh from the network, not from a cache, so the calls rotate over a set of
            grids and outputs of at least `--set-gb` GB together (several times the 256 MB Infinity Cache): every call
            reads and writes memory that the calls before it have pushed out.
              blend       every interval unflagged: of each 5 output frames 4 blend two grid rows and 1 is a copy
              copy        every interval flagged: every frame is a copy (a cut's hold; nearest costs the same)
            as time per output frame and as bytes moved per second (a blended frame reads two frames and writes one, a
            copied frame reads one and writes one), beside fiunet_hold_cut_frames on the same grid with every interval
            flagged (G - 1 frames read and written per interval): the nearest existing HBM-bound copy.
            Device time from HIP events around `--iters` back-to-back calls (each on the next grid of the set) after
            `--warmup` calls.
  streamed  interpolate_video(file, file, chunk_frames=C) of a 1080p I420 clip through the RGB network, bf16, batch 8:
              factor4     factor=4
              fps60       fps=60, time_depth=2 (the same forwards: the difference is what the feature costs)
            host wall clock around each call (it ends in a device synchronise), as input frames per second.
Each measurement is repeated `--reps` times, interleaved over the cases; the median and the spread are printed.  One
JSON line last.

    python tools/retime_timing.py [--intervals 16 --set-gb 2 --frames 257 --chunk 32 --reps 5 --dir /tmp]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


class _Rotate:
    """Calls fn(k) with k = 0, 1, ..., n - 1, 0, ... : each call works on the next member of a set."""

    def __init__(self, fn, n):
        self.fn, self.n, self.k = fn, n, 0

    def __call__(self):
        self.fn(self.k)
        self.k = (self.k + 1) % self.n


def _kernel_cases(dev, bits, h, w, n_int, plan, set_bytes):
    fs = P.i420_frame_bytes(h, w)   # samples of a 4:2:0 frame at either depth
    rows = n_int * plan.G + 1
    g = torch.Generator(device=dev).manual_seed(bits)
    j0, n_out = plan.span(0, n_int, True)
    dtype, hi = (torch.uint8, 256) if bits == 8 else (torch.int16, 1024)
    fb = fs * (1 if bits == 8 else 2)
    n_set = max(2, -(-set_bytes // ((rows + n_out) * fb)))
    grids = [torch.randint(0, hi, (rows, fs), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
    outs = [torch.empty((n_out, fs), dtype=dtype, device=dev) for _ in range(n_set)]
    none = torch.zeros(n_int, dtype=torch.uint8, device=dev)
    every = torch.ones(n_int, dtype=torch.uint8, device=dev)
    blends = sum(1 for j in range(j0, j0 + n_out) if plan.frame(j)[3])

    def resample(flags):
        return _Rotate(lambda k: P.retime.resample(grids[k], plan, 0, j0, n_out, bits=bits, flags=flags, out=outs[k]),
                       n_set)
    cases = {
        "blend": (resample(none), n_out, (3 * blends + 2 * (n_out - blends)) * fb),
        "copy": (resample(every), n_out, 2 * n_out * fb),
        # (in place: it turns the grids into held ones, which costs the resampling cases nothing)
        "hold": (_Rotate(lambda k: P.scene.hold_cut_frames(grids[k], every, plan.G), n_set), n_int * (plan.G - 1),
                 2 * n_int * (plan.G - 1) * fb),
    }
    return cases, dict(frame_bytes=fb, out_frames=n_out, blended_frames=blends, grids=n_set,
                       set_mb=round(n_set * (rows + n_out) * fb / 2**20))


def _write_clip(path, n, h, w):
    """n frames cycling through 8 random pictures (the network's cost does not depend on the content)."""
    with IO.Y4MWriter(path, w, h, (24, 1), "420jpeg", bits=8) as wr:
        pics = np.random.default_rng(0).integers(0, 256, (8, P.i420_frame_bytes(h, w))).astype(np.uint8)
        for s in range(0, n, 8):
            wr.write(pics[:min(8, n - s)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--intervals", type=int, default=16, help="input intervals of the kernel's chunk")
    ap.add_argument("--set-gb", type=float, default=2.0, help="least size of the rotating set of grids and outputs")
    ap.add_argument("--frames", type=int, default=257, help="input frames of the streamed clip")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory of the clip files (default: the system temp dir)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "retime_timing measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    plan = P.retime.plan(24, 60, 2)
    res = {"shape": [h, w], "ratio": [plan.p, plan.q], "time_depth": plan.depth, "kernel": {}, "streamed": {},
           "protocol": f"kernel: HIP events, {a.warmup} warm-up calls per case, median of {a.reps} interleaved reps of "
                       f"{a.iters} calls rotating over a set of grids of at least {a.set_gb} GB; streamed: host wall "
                       f"clock, one warm-up run per case, median of {a.reps} interleaved runs"}
    for bits in (8, 10):
        cases, info = _kernel_cases(dev, bits, h, w, a.intervals, plan, int(a.set_gb * 1e9))
        for fn, _, _ in cases.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in cases}
        for _ in range(a.reps):   # interleaved repetitions: drift on a shared host hits every case alike
            for k, (fn, _, _) in cases.items():
                ms[k].append(_time(fn, a.iters))
        leg = dict(info)
        for k, (_, frames, moved) in cases.items():
            med = statistics.median(ms[k])
            leg[k] = dict(ms=round(med, 4), spread_ms=[round(min(ms[k]), 4), round(max(ms[k]), 4)],
                          us_per_frame=round(1e3 * med / frames, 2), gb_per_s=round(moved / (med * 1e-3) / 1e9, 1))
            print(f"{bits:2d} bit {k:6s} {med:8.3f} ms  (reps {min(ms[k]):.3f}-{max(ms[k]):.3f})  "
                  f"{leg[k]['us_per_frame']:8.2f} us / frame  {leg[k]['gb_per_s']:7.1f} GB/s")
        leg["blend_vs_hold"] = round(leg["blend"]["gb_per_s"] / leg["hold"]["gb_per_s"], 3)
        res["kernel"][f"{bits}bit"] = leg
        del cases
        torch.cuda.empty_cache()

    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="bf16")
    m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
    fi = P.FrameInterpolator(model=m.to(dev).eval(), device=dev, batch=8)
    tmp = tempfile.mkdtemp(dir=a.dir)
    src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
    _write_clip(src, a.frames, h, w)
    runs = {
        "factor4": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk),
        "fps60": lambda: fi.interpolate_video(src, out, fps=60, time_depth=2, chunk_frames=a.chunk),
    }
    written = {k: fn() for k, fn in runs.items()}   # warm-up
    wall = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            wall[k].append(time.perf_counter() - t0)
    for k in runs:
        med = statistics.median(wall[k])
        res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                  spread_s=[round(min(wall[k]), 3), round(max(wall[k]), 3)], frames_out=written[k])
        print(f"streamed {k:8s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  "
              f"(runs {min(wall[k]):.3f}-{max(wall[k]):.3f})  {written[k]} frames out")
    res["streamed"].update(frames=a.frames, chunk_frames=a.chunk, network="rgb", precision="bf16",
                           fps60_vs_factor4=round(res["streamed"]["fps60"]["input_frames_per_s"]
                                                  / res["streamed"]["factor4"]["input_frames_per_s"], 3))
    for f in (src, out):
        if os.path.exists(f):
            os.remove(f)
    os.rmdir(tmp)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
