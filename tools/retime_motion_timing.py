"""Time motion-compensated resampling (retime "motion", retime.py): its kernel beside the warp it was
modelled on, and what `retime="motion"` costs a streamed 24 -> 60 run.

  kernel    B = 8 warped 1080p planes per call.  A member of the rotating set is a 9-row grid, 8 flow fields
            [8, 1080, 1920, 2] and 8 output planes; the calls rotate over at least `--set-gb` GB (several times the
            256 MB Infinity Cache), so the frames come from memory.
              warp / warp_again   fiunet_flow_warp in FIUNET_FLOW_MOTION on the same planes and fields: the yardstick,
                                  timed twice for the in-job spread
              table               fiunet_warp_table_u8 at wn / den = 2 / 5, contiguous samples (step 1)
              table_step2 / _step3   the same on planes whose samples lie 2 and 3 apart (U of NV12, a byte of rgb24)
              warp10 / table10 / warp10_again   the yardstick and the kernel on 16-bit words of 10-bit codes
            Device time from HIP events around `--replays` replays of a captured graph of `--iters` calls, after
            `--warmup` calls; reported per call and per warped plane.  The aim is "no slower than the yardstick beyond
            the spread of its two timings" at step 1.
              flow                farneback_flow(..., "hip") of the 8 pairs, eager, HIP events: the other half of the cost
  streamed  interpolate_video(file, file, fps=60, time_depth=2, chunk_frames=32) of a 257-frame 1080p I420 clip at
            24 fps, RGB network, bf16, batch 8: retime "blend" and "motion", each twice, interleaved; host wall clock
            around each call.  The share of flow and warp is the difference of the two wall times over motion's.
The median and the spread of `--reps` interleaved repetitions are printed, and written to `--out` when given.  One JSON
line last.

    python tools/retime_motion_timing.py [--set-gb 1 --frames 257 --chunk 32 --reps 5 --out profiles/retime_motion_timing.txt]
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
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO, optical_flow as OF  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

LINES = []
B = 8


def say(text):
    print(text, flush=True)
    LINES.append(text)


def _time(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _capture(fn, iters):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g


class _Rotate:
    def __init__(self, fn, n):
        self.fn, self.n, self.k = fn, n, 0

    def __call__(self):
        self.fn(self.k)
        self.k = (self.k + 1) % self.n


def _kernel_cases(dev, h, w, set_bytes):
    g = torch.Generator(device=dev).manual_seed(1)
    member = (B + 1) * h * w * 3 + B * h * w * 8 + B * h * w * 3
    n_set = max(2, -(-set_bytes // member))
    flows = [(torch.rand((B, h, w, 2), device=dev, generator=g) - 0.5) * 8 for _ in range(n_set)]
    entries = [(r, 2, 5, r, -1) for r in range(B)]
    cases = {}

    def add(name, bits, step, yardstick):
        dtype, hi = (torch.uint8, 256) if bits == 8 else (torch.int16, 1024)
        row = h * w * step
        grids = [torch.randint(0, hi, (B + 1, row), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
        outs = [torch.empty((B, row), dtype=dtype, device=dev) for _ in range(n_set)]
        plane = (step - 1, h, w, w * step, step, row)
        if yardstick:
            def fn(k):
                f = grids[k].reshape(B + 1, h, w)
                OF.warp(f[:B], f[1:], flows[k], "motion", "hip", bits=bits, out=outs[k].reshape(B, h, w))
        else:
            def fn(k):
                _native.warp_table(grids[k], B + 1, plane, flows[k], None, entries, outs[k], plane, bits)
        cases[name] = _Rotate(fn, n_set)
    add("warp", 8, 1, True)
    add("table", 8, 1, False)
    add("warp_again", 8, 1, True)
    add("table_step2", 8, 2, False)
    add("table_step3", 8, 3, False)
    add("warp10", 10, 1, True)
    add("table10", 10, 1, False)
    add("warp10_again", 10, 1, True)
    return cases, flows, dict(members=n_set, set_mb=round(n_set * member / 2**20))


def _write_clip(path, n, h, w):
    pics = np.random.default_rng(0).integers(0, 256, (8, P.i420_frame_bytes(h, w))).astype(np.uint8)
    with IO.Y4MWriter(path, w, h, (24, 1), "420jpeg", bits=8) as wr:
        for i in range(n):
            wr.write(pics[i % 8:i % 8 + 1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set")
    ap.add_argument("--frames", type=int, default=257, help="input frames of the streamed clip (0: skip it)")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--replays", type=int, default=5, help="replays of the captured graph per timing")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory of the clip files (default: the system temp dir)")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "retime_motion_timing measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    res = {"shape": [h, w], "planes_per_call": B, "kernel": {}, "streamed": {},
           "protocol": f"kernel: HIP events, {a.warmup} warm-up calls per case, median of {a.reps} interleaved reps of "
                       f"{a.replays} replays of a graph of {a.iters} calls rotating over a set of at least {a.set_gb} GB; "
                       f"streamed: host wall clock, one warm-up run per case, interleaved runs"}
    say(f"retime_motion_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    cases, flows, info = _kernel_cases(dev, h, w, int(a.set_gb * 1e9))
    for fn in cases.values():
        for _ in range(a.warmup):
            fn()
    torch.cuda.synchronize()
    graphs = {k: _capture(fn, a.iters) for k, fn in cases.items()}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(a.reps):
        for k in cases:
            ms[k].append(_time(graphs[k].replay, a.replays) / a.iters)
    leg = dict(info)
    for k in cases:
        med = statistics.median(ms[k])
        leg[k] = dict(ms=round(med, 4), us_per_plane=round(1e3 * med / B, 2),
                      spread_ms=[round(min(ms[k]), 4), round(max(ms[k]), 4)])
        say(f"{k:14s} graph {med:8.4f} ms a call, {1e3 * med / B:8.2f} us a warped plane  "
            f"(reps {min(ms[k]):.4f}-{max(ms[k]):.4f})")
    for new, old in (("table", "warp"), ("table10", "warp10")):
        a_, b_ = leg[old]["ms"], leg[old + "_again"]["ms"]
        spread, ratio = abs(a_ - b_) / min(a_, b_), leg[new]["ms"] / max(a_, b_)
        leg[f"{new}_vs_{old}"] = dict(ratio_to_slower_yardstick=round(ratio, 3), yardstick_spread=round(spread, 3),
                                      within_spread=bool(leg[new]["ms"] <= max(a_, b_)))
        say(f"{new} / {old}: {ratio:.3f} of the slower of the yardstick's two timings (they differ by {100 * spread:.1f} %)")
    del graphs
    lead = torch.randint(0, 256, (B + 1, h, w), dtype=torch.uint8, device=dev)
    flow_fn = lambda: OF.farneback_flow(lead[:B], lead[1:], "hip")  # noqa: E731
    for _ in range(a.warmup):
        flow_fn()
    fl = [_time(flow_fn, 3) for _ in range(a.reps)]
    leg["flow"] = dict(ms=round(statistics.median(fl), 3), ms_per_pair=round(statistics.median(fl) / B, 3),
                       spread_ms=[round(min(fl), 3), round(max(fl), 3)])
    say(f"flow           eager {statistics.median(fl):8.3f} ms a call of {B} pairs, {statistics.median(fl) / B:.3f} ms a pair  "
        f"(reps {min(fl):.3f}-{max(fl):.3f})")
    res["kernel"] = leg
    del cases, flows, lead
    torch.cuda.empty_cache()

    if a.frames:
        m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="bf16")
        m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
        fi = P.FrameInterpolator(model=m.to(dev).eval(), device=dev, batch=8)
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        _write_clip(src, a.frames, h, w)

        def run(mode):
            return lambda: fi.interpolate_video(src, out, fps=60, time_depth=2, retime=mode, chunk_frames=a.chunk)
        runs = {"blend": run("blend"), "motion": run("motion"), "blend_again": run("blend"), "motion_again": run("motion")}
        written = {k: fn() for k, fn in list(runs.items())[:2]}   # warm-up
        wall = {k: [] for k in runs}
        for _ in range(max(1, a.reps // 2)):
            for k, fn in runs.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                wall[k].append(time.perf_counter() - t0)
        for k in runs:
            med = statistics.median(wall[k])
            res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                      spread_s=[round(min(wall[k]), 3), round(max(wall[k]), 3)])
            say(f"streamed {k:13s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  "
                f"(runs {min(wall[k]):.3f}-{max(wall[k]):.3f})")
        s = res["streamed"]
        blend = statistics.median(wall["blend"] + wall["blend_again"])
        motion = statistics.median(wall["motion"] + wall["motion_again"])
        s.update(frames=a.frames, frames_out=written["motion"], chunk_frames=a.chunk, network="rgb", precision="bf16",
                 motion_vs_blend=round(motion / blend, 3), flow_and_warp_share=round((motion - blend) / motion, 3))
        say(f"streamed: motion takes {motion / blend:.3f} of blend's wall time; flow and warp are "
            f"{100 * (motion - blend) / motion:.1f} % of the motion run")
        for f in (src, out):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
    say(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
