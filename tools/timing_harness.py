"""The measurement protocol of the `tools/*_timing.py` scripts, once.

A timing tool builds its cases (callables that enqueue work on the current stream), hands them to `interleaved` (device
time) or `interleaved_wall` (host clock around calls with host work in them), and does its own arithmetic on the lists it
gets back: what is compared with what, and against which aim, differs from tool to tool and stays there.  Nothing here
knows a frame format.

    import timing_harness as H      # first: a script's own directory is on sys.path, and this import puts the
                                    # repository there, for `import ai_based_frame_interpolation_amd`, `bench`, `oracle`
"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

clock = time.perf_counter


def synchronize(device=None):
    torch.cuda.synchronize(device)


def need_gpu(tool_name):
    assert torch.cuda.is_available(), f"{tool_name} measures on the GPU; there is no CPU path"
    return torch.device("cuda:0")


def device_ms(fn, iters):
    """ms per call between two HIP events around `iters` back-to-back calls on the current stream."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def wall_s(fn, iters=1, device=None):
    """Seconds per call on the host clock, behind a device synchronise on either side: for calls with host work in them."""
    synchronize(device)
    t0 = clock()
    for _ in range(iters):
        fn()
    synchronize(device)
    return (clock() - t0) / iters


class Rotate:
    """Calls fn(k) with k = 0, 1, ..., n - 1, 0, ... : each call works on the next member of a set.  With a set several
    times the 256 MB Infinity Cache, every call reads and writes memory that the calls before it have pushed out."""

    def __init__(self, fn, n):
        self.fn, self.n, self.k = fn, n, 0

    def __call__(self):
        self.fn(self.k)
        self.k = (self.k + 1) % self.n


def graph_of(fn, iters):
    """A captured graph of `iters` calls of fn: replayed, the device runs them back to back with nothing of the host in
    between.  (fn must capture: asynchronous on the stream, no allocation, no synchronisation.)"""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g


def interleaved(cases, *, warmup, reps, iters, graph=False, replays=1):
    """{name: fn} -> {name: [ms per call, one per rep]}.  `iters` is one count or {name: count}.  With `graph`, a timing
    is `replays` replays of a graph of `iters` calls instead of `iters` calls from Python."""
    count = iters if isinstance(iters, dict) else dict.fromkeys(cases, iters)
    for fn in cases.values():
        for _ in range(warmup):
            fn()
    synchronize()
    timed = dict(cases)
    if graph:
        timed = {k: graph_of(fn, count[k]).replay for k, fn in cases.items()}
        for replay in timed.values():
            replay()
        synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):   # interleaved repetitions: drift on a shared host hits every case alike
        for k, fn in timed.items():
            ms[k].append(device_ms(fn, replays) / count[k] if graph else device_ms(fn, count[k]))
    return ms


def interleaved_wall(runs, *, reps, device=None, results=None):
    """{name: fn} -> {name: [seconds, one per rep]} on the host clock: one untimed round (code objects, the allocator's
    pools), then `reps` rounds interleaved over the runs, each call behind a device synchronise on either side.
    `results`, a dict, receives the value each run last returned."""
    secs = {k: [] for k in runs}
    for rep in range(reps + 1):
        for k, fn in runs.items():
            def call(k=k, fn=fn):
                got = fn()
                if results is not None:
                    results[k] = got
            if rep:
                secs[k].append(wall_s(call, 1, device))
            else:
                call()
    return secs


def summary(values):
    """-> (median, min, max)"""
    return statistics.median(values), min(values), max(values)


def pair_spread(a, b):
    """The relative difference of a yardstick's two timings (or rates): what the same code shows against itself in this job."""
    return abs(a - b) / max(a, b) if a != b else 0.0


def protocol(*, warmup, reps, iters, what="calls", set_gb=None, replays=None, wall_reps=None):
    """The sentence a tool prints first and stores under "protocol".  `iters` is a count or a text such as
    "200 (conversions) / 20 (forwards)"."""
    text = f"HIP events, {warmup} warm-up {what} per case, median of {reps} interleaved reps of "
    text += f"{replays} replays of a graph of {iters} {what}" if replays else f"{iters} {what}"
    if set_gb is not None:
        text += f" rotating over a set of at least {set_gb} GB"
    if wall_reps is not None:
        text += (f"; streamed: host clock behind a device synchronise on either side, one untimed round, median of "
                 f"{wall_reps} interleaved runs")
    return text


class Report:
    """say(line) prints it and, with a path, appends it to the file at once: a run ended at its time limit leaves what it
    measured.  finish(result) says the JSON line, last.  The file starts empty unless `append` (stream_timing's profile is
    built from several calls, a leg each)."""

    def __init__(self, path=None, append=False):
        self.path = path
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            open(path, "a" if append else "w").close()

    def say(self, line):
        print(line, flush=True)
        if self.path:
            with open(self.path, "a") as f:
                f.write(line + "\n")

    def finish(self, result):
        self.say(json.dumps(result))


def seeded_model(frame_channels, precision, device, batch=8):
    """-> (model, FrameInterpolator) with the seeded weights of the benchmarks: seed 1234 (gray 2 -> 1) or 77 (RGB 6 -> 3)."""
    import ai_based_frame_interpolation_amd as P
    from oracle import unet_oracle as O
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=frame_channels, precision=precision)
    m.load_state_dict(O.make_seeded_state_dict(77, n_channels=6, n_classes=3) if frame_channels == 3
                      else O.make_seeded_state_dict(1234))
    m = m.to(device).eval()
    return m, P.FrameInterpolator(model=m, device=device, batch=batch)


def write_y4m_clip(path, n, h, w, tag="420jpeg", bits=8, fps=(24, 1), distinct=8):
    """n frames cycling through `distinct` random pictures (the network's cost does not depend on the content)."""
    from ai_based_frame_interpolation_amd import imageio_lite as IO
    samples = IO._y4m_stream_header(IO._y4m_header_line(w, h, fps, tag, None, bits), bits)["frame_samples"]
    hi, dtype = (256, np.uint8) if bits == 8 else (1024, np.uint16)
    pics = np.random.default_rng(0).integers(0, hi, (distinct, samples)).astype(dtype)
    with IO.Y4MWriter(path, w, h, fps, tag, bits=bits) as wr:
        for i in range(n):
            wr.write(pics[i % distinct:i % distinct + 1])


class MemoryClip:
    """A readable binary source of `frames` frames of `frame_bytes` bytes that repeats a few frames held in memory."""

    def __init__(self, members: bytes, frame_bytes: int, frames: int):
        self.data, self.left, self.pos = memoryview(members), frame_bytes * frames, 0

    def readinto(self, b):
        n = min(len(b), self.left, len(self.data) - self.pos)
        b[:n] = self.data[self.pos:self.pos + n]
        self.pos = (self.pos + n) % len(self.data)
        self.left -= n
        return n


class NullSink:
    def write(self, b):
        return len(b)

    def flush(self):
        pass
