"""Time the re-timing of repeated frames (retime.py): its two kernels beside the kernels they were
modelled on, and what `dedup=` costs a streamed run.

  kernel    B = 8 intervals of 1080p I420 (9 frames), 8 bit and 10 bit.  The frames of a streamed chunk come from memory,
            not from a cache, so the calls rotate over a set of at least `--set-gb` GB (several times the 256 MB
            Infinity Cache).
              sad / sad_again    fiunet_pair_sad_*: the yardstick of the detection, timed twice for the in-job spread
              peak               fiunet_pair_peak_*: the same bytes read (two frames per interval)
              retime / retime_again   fiunet_retime_* on the 8 x 4 + 1-row grid, 24 -> 60 (of 5 frames 4 blend, 1 copies)
              table              fiunet_retime_table_* on entries built from the same plan: the same frames
            Device time from HIP events around `--replays` replays of a captured graph of `--iters` calls (the
            kernels back to back on the device, nothing from the host in between), after `--warmup` calls; the same
            calls issued eagerly from Python are timed beside it.  The target is "no slower than the yardstick beyond
            the spread of its two timings", on the graph's figures.
  streamed  interpolate_video(file, file, 4, chunk_frames=32) of a 257-frame 1080p I420 clip in which every third frame
            repeats the one before it, RGB network, bf16, batch 8: without dedup (twice) and with dedup=0; host wall
            clock around each call (it ends in a device synchronise).
Each measurement is repeated `--reps` times, interleaved over the cases; the median and the spread are printed, and
written to `--out` when given.  One JSON line last.

    python tools/dedup_timing.py [--set-gb 1 --frames 257 --chunk 32 --reps 5 --out profiles/dedup_timing.txt]
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
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

LINES = []


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
    """A graph of `iters` calls of fn (every entry point here promises: asynchronous on the stream, no allocation, no
    synchronisation - so it captures)."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g


class _Rotate:
    """Calls fn(k) with k = 0, 1, ..., n - 1, 0, ... : each call works on the next member of a set."""

    def __init__(self, fn, n):
        self.fn, self.n, self.k = fn, n, 0

    def __call__(self):
        self.fn(self.k)
        self.k = (self.k + 1) % self.n


def _kernel_cases(dev, bits, h, w, n_int, plan, set_bytes):
    fs = P.i420_frame_bytes(h, w)   # samples of a 4:2:0 frame at either depth
    g = torch.Generator(device=dev).manual_seed(bits)
    dtype, hi = (torch.uint8, 256) if bits == 8 else (torch.int16, 1024)
    fb = fs * (1 if bits == 8 else 2)
    rows = n_int * plan.G + 1
    j0, n_out = plan.span(0, n_int, True)
    n_set = max(2, -(-set_bytes // ((rows + n_out) * fb)))
    grids = [torch.randint(0, hi, (rows, fs), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
    outs = [torch.empty((n_out, fs), dtype=dtype, device=dev) for _ in range(n_set)]
    n_det = max(2, -(-set_bytes // ((n_int + 1) * fb)))   # the detection's own set: a member is the 9 frames it reads
    stacks = [torch.randint(0, hi, (n_int + 1, fs), dtype=dtype, device=dev, generator=g) for _ in range(n_det)]
    sums = torch.zeros(n_int, dtype=torch.int64, device=dev)
    peaks = torch.zeros(n_int, dtype=torch.int32, device=dev)
    entries = P.retime.table_entries(plan, [], 0, j0, n_out, n_int)
    blends = sum(1 for _, wn, _ in entries if wn)
    assert blends == sum(1 for j in range(j0, j0 + n_out) if plan.frame(j)[3])

    def sad():
        return _Rotate(lambda k: _native.pair_sad(stacks[k], sums, bits), n_det)

    def retime():
        return _Rotate(lambda k: P.retime.resample(grids[k], plan, 0, j0, n_out, bits=bits, out=outs[k]), n_set)
    detect_bytes = 2 * n_int * fb
    moved = (3 * blends + 2 * (n_out - blends)) * fb
    cases = {
        "sad": (sad(), detect_bytes),
        "peak": (_Rotate(lambda k: _native.pair_peak(stacks[k], peaks, bits), n_det), detect_bytes),
        "sad_again": (sad(), detect_bytes),
        "retime": (retime(), moved),
        "table": (_Rotate(lambda k: P.retime.resample_table(grids[k], entries, bits, out=outs[k]), n_set), moved),
        "retime_again": (retime(), moved),
    }
    return cases, dict(frame_bytes=fb, intervals=n_int, out_frames=n_out, blended_frames=blends, members=n_set,
                       set_mb=round(n_set * (rows + n_out) * fb / 2**20), detect_members=n_det,
                       detect_set_mb=round(n_det * (n_int + 1) * fb / 2**20))


def _write_clip(path, n, h, w):
    """n frames in which every third repeats the one before it: A B B C D D ... (random pictures: the network's cost
    does not depend on the content)."""
    pics = np.random.default_rng(0).integers(0, 256, (8, P.i420_frame_bytes(h, w))).astype(np.uint8)
    with IO.Y4MWriter(path, w, h, (24, 1), "420jpeg", bits=8) as wr:
        k = 0
        for i in range(n):
            if i % 3 != 2:
                k += 1
            wr.write(pics[k % 8:k % 8 + 1])
    return sum(1 for i in range(n) if i % 3 == 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--intervals", type=int, default=8)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set")
    ap.add_argument("--frames", type=int, default=257, help="input frames of the streamed clip (0: skip it)")
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--replays", type=int, default=10, help="replays of the captured graph per timing")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory of the clip files (default: the system temp dir)")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dedup_timing measures on the GPU; there is no CPU path"
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    plan = P.retime.plan(24, 60, 2)
    res = {"shape": [h, w], "kernel": {}, "streamed": {},
           "protocol": f"kernel: HIP events, {a.warmup} warm-up calls per case, median of {a.reps} interleaved reps of "
                       f"{a.replays} replays of a graph of {a.iters} calls (eager: of {a.iters} calls from Python) "
                       f"rotating over a set of at least {a.set_gb} GB; streamed: host wall clock, one "
                       f"warm-up run per case, median of {a.reps} interleaved runs"}
    say(f"dedup_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    for bits in (8, 10):
        cases, info = _kernel_cases(dev, bits, h, w, a.intervals, plan, int(a.set_gb * 1e9))
        for fn, _ in cases.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        # the figure is taken from a captured graph of `--iters` calls (on the members of the set in turn), replayed
        # `--replays` times: the device runs the kernels back to back, with no Python call, ctypes array or launch from
        # the host in between.  The same calls issued eagerly from Python are timed beside it, to show the host's share.
        graphs = {k: _capture(fn, a.iters) for k, (fn, _) in cases.items()}
        for g in graphs.values():
            g.replay()
        torch.cuda.synchronize()
        ms, eager = {k: [] for k in cases}, {k: [] for k in cases}
        for _ in range(a.reps):   # interleaved repetitions: drift on a shared host hits every case alike
            for k, (fn, _) in cases.items():
                ms[k].append(_time(graphs[k].replay, a.replays) / a.iters)
                eager[k].append(_time(fn, a.iters))
        leg = dict(info)
        for k, (_, moved) in cases.items():
            med, med_e = statistics.median(ms[k]), statistics.median(eager[k])
            leg[k] = dict(ms=round(med, 4), spread_ms=[round(min(ms[k]), 4), round(max(ms[k]), 4)],
                          gb_per_s=round(moved / (med * 1e-3) / 1e9, 1), eager_ms=round(med_e, 4),
                          eager_spread_ms=[round(min(eager[k]), 4), round(max(eager[k]), 4)])
            say(f"{bits:2d} bit {k:12s} graph {med:8.4f} ms  (reps {min(ms[k]):.4f}-{max(ms[k]):.4f})  "
                f"{leg[k]['gb_per_s']:7.1f} GB/s   eager {med_e:8.4f} ms  (reps {min(eager[k]):.4f}-{max(eager[k]):.4f})")
        del graphs
        for new, old in (("peak", "sad"), ("table", "retime")):
            a_, b_ = leg[old]["ms"], leg[old + "_again"]["ms"]
            spread = abs(a_ - b_) / min(a_, b_)
            ratio = leg[new]["ms"] / max(a_, b_)
            leg[f"{new}_vs_{old}"] = dict(ratio_to_slower_yardstick=round(ratio, 3), yardstick_spread=round(spread, 3),
                                          within_spread=bool(leg[new]["ms"] <= max(a_, b_)))
            say(f"{bits:2d} bit {new} / {old}: {ratio:.3f} of the slower of the yardstick's two timings "
                f"(they differ by {100 * spread:.1f} %)")
        res["kernel"][f"{bits}bit"] = leg
        del cases
        torch.cuda.empty_cache()

    if a.frames:
        m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="bf16")
        m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
        fi = P.FrameInterpolator(model=m.to(dev).eval(), device=dev, batch=8)
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        repeats = _write_clip(src, a.frames, h, w)
        log = []
        runs = {
            "plain": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk),
            "dedup": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk, dedup=0, dedup_log=log),
            "plain_again": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk),
        }
        written = {k: fn() for k, fn in runs.items()}   # warm-up
        dead = int(sum(d.sum() for _, d in log))
        wall = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                log.clear()
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize(dev)
                wall[k].append(time.perf_counter() - t0)
        for k in runs:
            med = statistics.median(wall[k])
            res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                      spread_s=[round(min(wall[k]), 3), round(max(wall[k]), 3)], frames_out=written[k])
            say(f"streamed {k:12s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  "
                f"(runs {min(wall[k]):.3f}-{max(wall[k]):.3f})  {written[k]} frames out")
        s = res["streamed"]
        slower = max(s["plain"]["wall_s"], s["plain_again"]["wall_s"])
        s.update(frames=a.frames, repeated_frames=repeats, dead_intervals=dead, chunk_frames=a.chunk, network="rgb",
                 precision="bf16", dedup_vs_plain=round(s["dedup"]["wall_s"] / slower, 3))
        say(f"streamed: {repeats} repeated frames, {dead} dead intervals found; dedup takes {s['dedup_vs_plain']:.3f} of "
            f"the slower plain run's wall time")
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
