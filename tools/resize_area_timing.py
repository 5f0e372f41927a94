"""Time the area filter of the resize beside the linear kernel's copy of the same source, and
`resize_filter=` end to end, in one process.  The set-up is tools/resize_timing.py's.

  kernel    `resize.resize_frames` on B tight frames of I420 (the planes of 8-bit Y4M 4:2:0), yuv422p10le, nv12 and rgb24
            at 1080p, and of I420 at 2160p.  Per source, three calls:
              copy     the linear kernel at the source's own size: it reads every source byte once and writes as many.
                       This is the yardstick - the kernel of the parent commit, not the new one
              area     filter="area" to 256x256 (the 2160p source: to 1080p): reads every source byte once, writes few
              linear   the same resize with filter="linear", for information (it reads four samples per destination one)
            Each is timed twice per job (_a, _b; the difference is the spread of this job).  The target: area takes no
            longer than the copy of the same source beyond that spread; nv12 is also held to I420's copy (the same
            bytes, planar) and rgb24's line names yuv422p10le's (a third more bytes, planar) beside its own.
            Frames come from memory, not from a cache: the calls rotate over a set of sources and destinations of at
            least `--set-gb` GB together.  Device time from HIP events around `--iters` back-to-back calls after
            `--warmup` calls; `--reps` repetitions interleaved over the cases; medians.
  stream    a 33-frame 1080p 8-bit 4:2:0 Y4M clip through the grayscale network in bf16, streamed in chunks of 8 into a
            null sink with resize=(256, 256) under either filter: frames/s of source frames, median of `--stream-reps`
            interleaved runs after one warm-up run each.
One JSON line last; the text goes to `--out` as well (default profiles/resize_area_timing.txt).

    python tools/resize_area_timing.py [--batch 8 --set-gb 1 --iters 50 --reps 7]
"""
import argparse
import os
import tempfile

import numpy as np
import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import imageio_lite, resize

FORMATS = {"i420": (("y4m", "420jpeg"), 8), "yuv422p10le": ("yuv422p10le", 10), "nv12": ("nv12", 8), "rgb24": ("rgb24", 8)}
#: (format, source (h, w), destination (h, w))
CASES = [("i420", (1080, 1920), (256, 256)), ("yuv422p10le", (1080, 1920), (256, 256)), ("nv12", (1080, 1920), (256, 256)),
         ("rgb24", (1080, 1920), (256, 256)), ("i420", (2160, 3840), (1080, 1920))]
PLANAR_YARDSTICK = {"nv12": "i420", "rgb24": "yuv422p10le"}


def _kernel_case(dev, name, b, src_hw, dst_hw, set_bytes):
    kind, bits = FORMATS[name]
    sp, dp = resize.frame_planes(kind, *src_hw), resize.frame_planes(kind, *dst_hw)
    rs, rd = resize.frame_samples(sp), resize.frame_samples(dp)
    item = 1 if bits == 8 else 2
    dtype = torch.uint8 if bits == 8 else torch.int16
    rbytes = b * rs * item
    n_set = max(2, -(-set_bytes // (2 * rbytes)))
    g = torch.Generator(device=dev).manual_seed(rs)
    src = [torch.randint(0, 256 if bits == 8 else 1024, (b, rs), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
    same = [torch.empty((b, rs), dtype=dtype, device=dev) for _ in range(n_set)]
    small = [torch.empty((b, rd), dtype=dtype, device=dev) for _ in range(n_set)]

    def copy(k):
        resize.resize_frames(src[k], sp, sp, bits, out=same[k])

    def area(k):
        resize.resize_frames(src[k], sp, dp, bits, out=small[k], filter="area")

    def linear(k):
        resize.resize_frames(src[k], sp, dp, bits, out=small[k], filter="linear")
    cases = {f"{n}_{r}": H.Rotate(fn, n_set) for r in "ab" for n, fn in (("copy", copy), ("area", area), ("linear", linear))}
    return cases, rbytes


def _kernels(dev, a, say):
    out = {}
    for name, src_hw, dst_hw in CASES:
        label = f"{name} {src_hw[0]}x{src_hw[1]}->{dst_hw[0]}x{dst_hw[1]}"
        cases, rbytes = _kernel_case(dev, name, a.batch, src_hw, dst_hw, int(a.set_gb * 1e9))
        ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
        us = {k: H.summary(v)[0] * 1e3 for k, v in ms.items()}
        leg = {n: [round(us[n + "_a"], 1), round(us[n + "_b"], 1)] for n in ("copy", "area", "linear")}
        spread = max(abs(us[n + "_a"] - us[n + "_b"]) for n in ("copy", "area"))
        worst, yard = max(leg["area"]), min(leg["copy"])
        leg.update(spread_us=round(spread, 1), area_read_gb_per_s=round(rbytes / (worst * 1e-6) / 1e9, 1),
                   copy_read_gb_per_s=round(rbytes / (yard * 1e-6) / 1e9, 1), area_over_copy=round(worst / yard, 3),
                   met=bool(worst <= yard + spread))
        out[label] = leg
        say(f"{label:34s} copy {leg['copy'][0]:7.1f} / {leg['copy'][1]:7.1f} us | area {leg['area'][0]:7.1f} / "
            f"{leg['area'][1]:7.1f} us ({leg['area_read_gb_per_s']:7.1f} GB/s of source) | linear {leg['linear'][0]:7.1f} / "
            f"{leg['linear'][1]:7.1f} us | spread {leg['spread_us']:.1f} us | area / copy x{leg['area_over_copy']:.3f} "
            f"{'MET' if leg['met'] else 'MISSED'}")
        del cases
        torch.cuda.empty_cache()
    for name, other in PLANAR_YARDSTICK.items():
        mine, yard = out[f"{name} 1080x1920->256x256"], out[f"{other} 1080x1920->256x256"]
        ratio = max(mine["area"]) / min(yard["copy"])
        met = bool(max(mine["area"]) <= min(yard["copy"]) + max(mine["spread_us"], yard["spread_us"]))
        mine.update({"planar_yardstick": other, "area_over_planar_copy": round(ratio, 3), "met_planar": met})
        say(f"{name} area against the copy of {other} at 1080p ({min(yard['copy']):.1f} us): x{ratio:.3f} "
            f"{'MET' if met else 'MISSED'}")
    return out


def _stream(dev, a, say):
    n, (h, w), size = a.stream_frames, (1080, 1920), (256, 256)
    _, fi = H.seeded_model(1, "bf16", dev)
    sp = resize.frame_planes(("y4m", "420jpeg"), h, w)
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, resize.frame_samples(sp), dtype=np.uint8)
    rows = np.stack([np.roll(base, 7 * i) for i in range(n)])
    with tempfile.TemporaryDirectory() as d:
        big = os.path.join(d, "big.y4m")
        with imageio_lite.Y4MWriter(big, w, h, (24, 1), "420jpeg", None, bits=8) as wr:
            wr.write(rows)

        def run(**kw):
            fi.interpolate_video(big, H.NullSink(), 2, chunk_frames=8, resize=size, **kw)
        runs = {"linear": lambda: run(resize_filter="linear"), "area": lambda: run(resize_filter="area")}
        secs = H.interleaved_wall(runs, reps=a.stream_reps, device=dev)
    out = {}
    for k, v in secs.items():
        med, lo, hi = H.summary(v)
        out[k] = dict(s=round(med, 4), spread_s=[round(lo, 4), round(hi, 4)], frames_per_s=round(n / med, 1))
        say(f"stream {n} x 1080p -> 256x256, gray bf16, chunks of 8: {k:7s} {med:8.4f} s (reps {lo:.4f}-{hi:.4f})  "
            f"{out[k]['frames_per_s']:8.1f} source frames/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set of sources and destinations")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--stream-frames", type=int, default=33)
    ap.add_argument("--stream-reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "resize_area_timing.txt"))
    a = ap.parse_args()
    dev = H.need_gpu("resize_area_timing")
    report = H.Report(a.out)
    say = report.say
    say(f"# tools/resize_area_timing.py: B = {a.batch}; "
        f"{H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb, wall_reps=a.stream_reps)}; "
        f"{torch.cuda.get_device_name(0)}")
    report.finish({"kernel": _kernels(dev, a, say), "stream": _stream(dev, a, say)})


if __name__ == "__main__":
    main()
