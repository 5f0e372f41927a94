"""Time the 10-bit 4:2:2 wire packings beside the yuv422p10le colour conversions, in one process.

  kernels   unpack (wire -> yuv422p10le) and pack (yuv422p10le -> wire) of B frames of v210, y210le and p210le, 1080p and
            2160p, beside the yardstick: fiunet_yuv_to_rgb_p10 / fiunet_rgb_p10_to_yuv on yuv422p10le, measured as two
            cases (yard_a, yard_b): the difference between them is the run-to-run spread of this job.  A frame comes
            from memory, not from a cache: the calls rotate over a set of inputs and outputs of at least `--set-gb` GB
            together.  Device time from HIP events around `--iters` back-to-back calls after `--warmup` calls; `--reps`
            repetitions interleaved over the cases; median and spread.  Bytes moved: one wire frame plus one working
            frame (the yardstick: one yuv422p10le frame plus three planes of H x W words).  The aim: every unpack and
            pack no slower per byte moved than the slower yardstick measurement of its leg, less that leg's spread.
  stream    a 257-frame 1080p clip through `interpolate_video(raw="yuv422p10le", chunk_frames=32)` at factor 2 in fp16,
            with packing="v210" and without, alternating, from memory into a null sink.  The aim: within the spread of
            the runs.
Every line goes to standard output and to `--out`; one JSON line last.

    python tools/wire10_timing.py [--batch 8 --set-gb 1 --iters 200 --reps 7 --out profiles/wire10_timing.txt]
"""
import argparse
import os

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import _native, wire10
from ai_based_frame_interpolation_amd.colour import YUV_FORMATS, resolve_yuv_layout, yuv_flags

FMT = wire10.WORKING_FORMAT


def _words(dev, g, shape, top=1024):
    return torch.randint(0, top, shape, dtype=torch.int16, device=dev, generator=g)


def _kernel_cases(dev, b, h, w, set_bytes):
    """Sets of `n_set` working batches, wire batches wide enough for the largest packing, and RGB batches."""
    n = wire10.planar_samples(h, w)
    widest = max(wire10.frame_bytes(p, h, w) for p in wire10.PACKINGS) // 2
    n_set = max(2, -(-set_bytes // (2 * b * (widest + n))))
    g = torch.Generator(device=dev).manual_seed(10)
    work = [_words(dev, g, (b, n)) for _ in range(n_set)]
    wire = [_words(dev, g, (b, widest)) for _ in range(n_set)]       # (any bits: an unpack ignores what it must)
    rgb = [_words(dev, g, (b, 3, h, w)).view(torch.uint16) for _ in range(n_set)]
    code, lay, flags = YUV_FORMATS[FMT][0], resolve_yuv_layout(None, FMT, h, w), yuv_flags(FMT, "mpeg2", "bt709", "limited")

    def yard(decode):
        if decode:
            return H.Rotate(lambda k: _native.yuv_to_rgb(work[k].view(torch.uint16), code, lay, rgb[k], h, w, flags, 10), n_set)
        return H.Rotate(lambda k: _native.rgb_to_yuv(rgb[k], work[k].view(torch.uint16), code, lay, flags, 10), n_set)

    def new(unpack, p):
        m = wire10.frame_bytes(p, h, w) // 2
        if unpack:
            return H.Rotate(lambda k: wire10.unpack(wire[k][:, :m], h, w, p, out=work[k]), n_set)
        return H.Rotate(lambda k: wire10.pack(work[k], h, w, p, out=wire[k][:, :m]), n_set)
    cases, moved = {}, {}
    for name, first in (("unpack", True), ("pack", False)):
        cases[f"{name} yard_a"] = yard(first)
        for p in wire10.PACKINGS:
            cases[f"{name} {p}"] = new(first, p)
            moved[f"{name} {p}"] = b * (wire10.frame_bytes(p, h, w) + 2 * n)
        cases[f"{name} yard_b"] = yard(first)
        moved[f"{name} yard_a"] = moved[f"{name} yard_b"] = 2 * b * (n + 3 * h * w)
    return cases, moved, dict(batch=b, set_members=n_set, set_mb=round(2 * n_set * b * (widest + n) / 2**20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set of inputs and outputs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1080x1920,2160x3840")
    ap.add_argument("--stream-frames", type=int, default=257)
    ap.add_argument("--stream-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "wire10_timing.txt"))
    a = ap.parse_args()
    dev = H.need_gpu("wire10_timing")
    report = H.Report(a.out)
    say = report.say
    res = {"kernels": {}, "stream": {},
           "protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb, wall_reps=a.stream_reps)}
    say(res["protocol"])
    for shape in a.shapes.split(","):
        h, w = (int(v) for v in shape.split("x"))
        cases, moved, info = _kernel_cases(dev, a.batch, h, w, int(a.set_gb * 1e9))
        ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
        leg = dict(info)
        for k in cases:
            med, lo, hi = H.summary(ms[k])
            leg[k] = dict(ms=round(med, 4), spread_ms=[round(lo, 4), round(hi, 4)],
                          gb_per_s=round(moved[k] / (med * 1e-3) / 1e9, 1))
            say(f"{h}x{w} B={a.batch} {k:16s} {med:8.4f} ms  (reps {lo:.4f}-{hi:.4f})  {leg[k]['gb_per_s']:7.1f} GB/s")
        for name in ("unpack", "pack"):
            ya, yb = leg[f"{name} yard_a"]["gb_per_s"], leg[f"{name} yard_b"]["gb_per_s"]
            spread = H.pair_spread(ya, yb)
            leg[f"{name} yard_spread"] = round(spread, 4)
            bar = min(ya, yb) * (1 - spread)
            for p in wire10.PACKINGS:
                ratio = leg[f"{name} {p}"]["gb_per_s"] / min(ya, yb)
                leg[f"{name} {p}_vs_yard"] = round(ratio, 3)
                leg[f"{name} {p}_aim"] = "met" if leg[f"{name} {p}"]["gb_per_s"] >= bar else "missed"
            say(f"{h}x{w} {name}: yardstick spread {spread:.4f}; bytes/s vs the slower yardstick: "
                + ", ".join(f"{p} {leg[f'{name} {p}_vs_yard']:.3f} ({leg[f'{name} {p}_aim']})" for p in wire10.PACKINGS))
        res["kernels"][f"{h}x{w}"] = leg
        del cases
        torch.cuda.empty_cache()

    h, w, frames = 1080, 1920, a.stream_frames
    _, fi = H.seeded_model(3, "fp16", dev, a.batch)
    g = torch.Generator(device=dev).manual_seed(2)
    members = _words(dev, g, (4, wire10.planar_samples(h, w)))
    sources = {FMT: (members.cpu().numpy().tobytes(), 2 * wire10.planar_samples(h, w), {}),
               "v210": (wire10.pack(members, h, w, "v210").cpu().numpy().tobytes(), wire10.frame_bytes("v210", h, w),
                        dict(packing="v210"))}
    runs = {k: (lambda data=data, frame=frame, kw=kw: fi.interpolate_video(
        H.MemoryClip(data, frame, frames), H.NullSink(), raw=FMT, width=w, height=h, src_fps=24, chunk_frames=32, **kw))
        for k, (data, frame, kw) in sources.items()}
    written = {}
    secs = H.interleaved_wall(runs, reps=a.stream_reps, device=dev, results=written)
    assert all(n == 2 * frames - 1 for n in written.values()), written
    for k, v in secs.items():
        med, lo, hi = H.summary(v)
        res["stream"][k] = dict(s=round(med, 4), spread_s=[round(lo, 4), round(hi, 4)],
                                source_frames_per_s=round(frames / med, 1))
        say(f"stream {frames} x {h}x{w} fp16 factor 2 {k:12s} {med:7.4f} s  (runs {lo:.4f}-{hi:.4f})  "
            f"{frames / med:7.1f} source frames/s")
    base, new = res["stream"][FMT], res["stream"]["v210"]
    spread = max(base["spread_s"][1] - base["spread_s"][0], new["spread_s"][1] - new["spread_s"][0])
    res["stream"]["v210_vs_working"] = round(new["s"] / base["s"], 4)
    res["stream"]["aim"] = "met" if new["s"] - base["s"] <= spread else "missed"
    say(f"stream: v210 / {FMT} time {res['stream']['v210_vs_working']:.4f}; run-to-run spread {spread:.4f} s: the aim "
        f"(within that spread) is {res['stream']['aim']}")
    report.finish(res)


if __name__ == "__main__":
    main()
