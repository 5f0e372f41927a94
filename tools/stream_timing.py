"""Time the streamed video path (stream.py) against the resident whole-clip path on the same clip.

Legs (factor 2, batch 8, chunk_frames --chunk):
  rgb1080    1080p I420 through the RGB network, bf16
  gray1080   1080p C420jpeg through the grayscale network (luma through the network, chroma averaged), bf16
  rgb4k10    2160x3840 C420p10 through the RGB network, fp16
Modes per leg:
  resident   interpolate_video(file, file): the whole clip read, resident in HBM, written at the end
  file       interpolate_video(file, file, chunk_frames=C)
  pipe       interpolate_video(pipe, pipe, chunk_frames=C): the source is an OS pipe fed from memory by a thread, the
             sink an OS pipe drained by a thread (the ffmpeg-pipe situation without ffmpeg's own cost)
Host wall clock around each call (every call ends in a device synchronise: host I/O is part of what is timed); one
warm-up call per mode, then --reps repetitions, interleaved over the modes; the median and the spread are printed.  Also
per mode: the peak device allocation (torch.cuda.max_memory_allocated after a reset) and the peak growth of the
process's resident set (VmRSS sampled every 5 ms) during the call.  --long K adds a streamed pipe run of the first
leg's clip repeated to K x its length, to show that neither peak grows with the clip.  One JSON line per leg.

    python tools/stream_timing.py [--legs rgb1080,gray1080,rgb4k10] [--frames 257] [--dir /tmp] [--long 4]
"""
import argparse
import json
import os
import subprocess
import tempfile
import threading
import time

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below

LEGS = {   # name: (height, width, tag, bits, network channels, precision, default frames)
    "rgb1080": (1080, 1920, "420jpeg", 8, 3, "bf16", None),
    "gray1080": (1080, 1920, "420jpeg", 8, 1, "bf16", None),
    "rgb4k10": (2160, 3840, "420p10", 10, 3, "fp16", 65),
}


def _rss():
    with open("/proc/self/status") as f:
        for line in f:
            if line.startswith("VmRSS:"):
                return int(line.split()[1]) * 1024
    return 0


class _RssPeak:
    def __enter__(self):
        self.base = self.peak = _rss()
        self.stop = threading.Event()
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()
        return self

    def _run(self):
        while not self.stop.is_set():
            self.peak = max(self.peak, _rss())
            time.sleep(0.005)

    def __exit__(self, *exc):
        self.stop.set()
        self.t.join()
        self.peak = max(self.peak, _rss())
        self.growth = self.peak - self.base
        return False


def _filesystem(path):
    try:
        out = subprocess.run(["df", "-T", path], capture_output=True, text=True, timeout=10).stdout.splitlines()
        return out[-1].split()[1] if len(out) > 1 else "unknown"
    except Exception:  # noqa: BLE001
        return "unknown"


def _pipe_run(fi, data, chunk):
    rin, win = os.pipe()
    rout, wout = os.pipe()
    got = [0]

    def feed():
        with os.fdopen(win, "wb") as f:
            mv = memoryview(data)
            for s in range(0, len(mv), 1 << 22):
                f.write(mv[s:s + (1 << 22)])

    def drain():
        with os.fdopen(rout, "rb", buffering=0) as f:
            while True:
                b = f.read(1 << 22)
                if not b:
                    return
                got[0] += len(b)
    ts = [threading.Thread(target=feed), threading.Thread(target=drain)]
    for t in ts:
        t.start()
    with os.fdopen(rin, "rb") as src, os.fdopen(wout, "wb") as dst:
        n = fi.interpolate_video(src, dst, 2, chunk_frames=chunk)
    for t in ts:
        t.join()
    return n


def _measure(dev, fn):
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    with _RssPeak() as r:
        dt = H.wall_s(fn, 1, dev)
    return dt, torch.cuda.max_memory_allocated(dev) - base, r.growth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="rgb1080,gray1080,rgb4k10")
    ap.add_argument("--frames", type=int, default=257)
    ap.add_argument("--chunk", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--long", type=int, default=4)
    ap.add_argument("--dir", default=None, help="directory of the clip files (default: the system temp dir)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("stream_timing")
    report = H.Report(a.out, append=True)
    tmp = tempfile.mkdtemp(dir=a.dir)
    fs = _filesystem(tmp)
    for li, leg in enumerate(a.legs.split(",")):
        h, w, tag, bits, fc, prec, nd = LEGS[leg]
        n = nd or a.frames
        m, fi = H.seeded_model(fc, prec, dev)
        src = os.path.join(tmp, "in.y4m")
        H.write_y4m_clip(src, n, h, w, tag, bits)
        data = open(src, "rb").read()
        out = os.path.join(tmp, "out.y4m")
        modes = {
            "resident": lambda: fi.interpolate_video(src, out, 2),
            "file": lambda: fi.interpolate_video(src, out, 2, chunk_frames=a.chunk),
            "pipe": lambda: _pipe_run(fi, data, a.chunk),
        }
        for fn in modes.values():   # warm-up
            fn()
        times = {k: [] for k in modes}
        peaks = {k: (0, 0) for k in modes}
        for _ in range(a.reps):
            for k, fn in modes.items():
                dt, dpk, rss = _measure(dev, fn)
                times[k].append(dt)
                peaks[k] = (max(peaks[k][0], dpk), max(peaks[k][1], rss))
        res = dict(leg=leg, frames=n, height=h, width=w, tag=tag, network=fc, precision=prec, chunk_frames=a.chunk,
                   filesystem=fs, reps=a.reps)
        for k in modes:
            med, lo, hi = H.summary(times[k])
            res[k] = dict(pairs_per_s=round((n - 1) / med, 1), wall_s=round(med, 3), spread_s=round(hi - lo, 3),
                          device_peak_mb=round(peaks[k][0] / 2**20, 1), rss_growth_mb=round(peaks[k][1] / 2**20, 1))
        for k in ("file", "pipe"):
            res[k]["vs_resident"] = round(res[k]["pairs_per_s"] / res["resident"]["pairs_per_s"], 3)
        if li == 0 and a.long > 1:
            big = data[:data.index(b"\n") + 1] + data[data.index(b"\n") + 1:] * a.long
            dt, dpk, rss = _measure(dev, lambda: _pipe_run(fi, big, a.chunk))
            nl = n * a.long
            res["pipe_long"] = dict(frames=nl, pairs_per_s=round((nl - 1) / dt, 1), wall_s=round(dt, 3),
                                    device_peak_mb=round(dpk / 2**20, 1), rss_growth_mb=round(rss / 2**20, 1))
            del big
        report.say(json.dumps(res))
        os.remove(src)
        if os.path.exists(out):
            os.remove(out)
        del fi, m, data
        torch.cuda.empty_cache()
    os.rmdir(tmp)


if __name__ == "__main__":
    main()
