"""Time inverse telecine (ivtc.py): its two kernels beside the kernels they were modelled on, and what
`cli ivtc` makes of a 1080i clip end to end.

  kernel    B = 8 frames of 1080p per call, out of a window of B + 2 (one context frame either side), 8 bit and 10 bit.
            The calls rotate over at least `--set-gb` GB (several times the 256 MB Infinity Cache), so the frames come
            from memory.
              match                fiunet_field_match_*: the three scores of B luma planes
              peak / peak_again    fiunet_pair_peak_* on B intervals of the same luma planes: the yardstick, timed twice
                                   for the in-job spread
              weave                fiunet_field_weave_*: B frames of I420 (three planes), half of them woven from two
                                   frames, half copies
              table / table_again  fiunet_retime_table_* writing the same frames as byte copies (wn = 0): the yardstick
            Device time from HIP events around `--replays` replays of a captured graph of `--iters` calls, after
            `--warmup` calls; reported per frame.  The aim: no slower per frame than the slower of the yardstick's two
            timings.
  clip      `cli ivtc --order tff` of a `--frames`-frame 1080i I420 Y4M clip, file to file, beside `cli deinterlace --rate
            frame` of the same clip; host wall clock around each run, in source frames per second.  No target.  The clip
            is 2:3 pulldown of synthetic film (a smooth picture - uniform noise box-blurred twice - that moves 3 x 1
            pixels per film frame), so the run is inverse telecine proper: its report (matches, combed, dropped) is
            printed with the figures.
The median and the spread of `--reps` interleaved repetitions are printed, and written to `--out` when given.  One JSON
line last.

    python tools/ivtc_timing.py [--set-gb 1 --frames 257 --reps 5 --out profiles/ivtc_timing.txt]
"""
import argparse
import os
import tempfile

import numpy as np
import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import _native, cli, imageio_lite as IO, ivtc as I
from ai_based_frame_interpolation_amd.layout import frame_layout

B = 8


def _cases(dev, bits, h, w, set_bytes):
    g = torch.Generator(device=dev).manual_seed(bits)
    dtype, hi, item = (torch.uint8, 256, 1) if bits == 8 else (torch.int16, 1024, 2)
    lay = frame_layout(("y4m", "420jpeg"), h, w)          # (the arrangement of I420 at either depth)
    luma = (0, h, w, w, 1, h * w)
    n_luma = max(2, -(-set_bytes // ((B + 2) * h * w * item)))
    lumas = [torch.randint(0, hi, (B + 2, h * w), dtype=dtype, device=dev, generator=g) for _ in range(n_luma)]
    scores = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    peaks = torch.zeros(B, dtype=torch.int32, device=dev)
    thr = I.default_threshold(bits)
    member = (B + 2 + B) * lay.samples * item
    n_set = max(2, -(-set_bytes // member))
    windows = [torch.randint(0, hi, (B + 2, lay.samples), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
    outs = [torch.empty((B, lay.samples), dtype=dtype, device=dev) for _ in range(n_set)]
    weave_entries = [(1 + i, 1 + i - (i & 1)) for i in range(B)]     # c, p, c, p, ...
    table_entries = [(1 + i, 0, 1) for i in range(B)]

    def peak():
        return H.Rotate(lambda k: _native.pair_peak(lumas[k][:B + 1], peaks, bits), n_luma)

    def table():
        return H.Rotate(lambda k: _native.retime_table(windows[k], table_entries, outs[k], bits), n_set)
    cases = {
        "peak": peak(),
        "match": H.Rotate(lambda k: _native.field_match(lumas[k], B + 2, luma, 1, B, 0, thr, scores, bits), n_luma),
        "peak_again": peak(),
        "table": table(),
        "weave": H.Rotate(lambda k: I.weave(windows[k], lay, bits, weave_entries, "tff", out=outs[k]), n_set),
        "table_again": table(),
    }
    return cases, dict(luma_members=n_luma, luma_set_mb=round(n_luma * (B + 2) * h * w * item / 2**20), members=n_set,
                       set_mb=round(n_set * member / 2**20), frame_samples=lay.samples)


def _smooth(h, w, seed, blur=13):
    box = np.random.default_rng(seed).integers(0, 256, (h + 2 * blur, w + 2 * blur)).astype(np.float64)
    for _ in range(2):
        c = np.cumsum(np.cumsum(np.pad(box, ((1, 0), (1, 0))), axis=0), axis=1)
        box = c[blur:, blur:] - c[:-blur, blur:] - c[blur:, :-blur] + c[:-blur, :-blur]
    return np.rint((box - box.min()) * (255.0 / (box.max() - box.min()))).astype(np.uint8)


def _write_telecined_clip(path, n, h, w, dx=3, dy=1):
    """n frames of tff 2:3 pulldown (phase 0) of film cut from one smooth picture per plane that moves (dx, dy) pixels
    per film frame (half that in the chroma planes), as I420 Y4M."""
    fields = [f for f in range(n) for _ in range(2 if f % 2 == 0 else 3)][:2 * n]   # (more film than the clip needs)
    films = fields[-1] + 1
    hc, wc = (h + 1) // 2, (w + 1) // 2
    big = [_smooth(h + films * dy, w + films * dx, 1), _smooth(hc + films * dy, wc + films * dx, 2),
           _smooth(hc + films * dy, wc + films * dx, 3)]
    sizes = [(h, w, dx, dy), (hc, wc, dx // 2 + 1, dy), (hc, wc, dx // 2 + 1, dy)]

    def film(f):
        return [b[f * sy:f * sy + ph, f * sx:f * sx + pw] for b, (ph, pw, sx, sy) in zip(big, sizes)]
    with IO.Y4MWriter(path, w, h, (30000, 1001), "420jpeg", bits=8) as wr:
        for t in range(n):
            a, b = film(fields[2 * t]), film(fields[2 * t + 1])
            planes = []
            for pa, pb in zip(a, b):
                fr = pa.copy()
                fr[1::2] = pb[1::2]
                planes.append(fr.reshape(-1))
            wr.write(np.concatenate(planes)[None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set")
    ap.add_argument("--frames", type=int, default=257, help="source frames of the clip (0: skip it)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--replays", type=int, default=5, help="replays of the captured graph per timing")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="directory of the clip files (default: the system temp dir)")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("ivtc_timing")
    report = H.Report(a.out)
    say = report.say
    h, w = a.height, a.width
    res = {"shape": [h, w], "frames_per_call": B, "kernel": {}, "clip": {},
           "protocol": "kernel: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, replays=a.replays,
                                               set_gb=a.set_gb, wall_reps=2)}
    say(f"ivtc_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    for bits in (8, 10):
        cases, info = _cases(dev, bits, h, w, int(a.set_gb * 1e9))
        ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters, graph=True, replays=a.replays)
        leg = dict(info)
        for k in cases:
            med, lo, hi = H.summary(ms[k])
            leg[k] = dict(ms=round(med, 4), us_per_frame=round(1e3 * med / B, 2), spread_ms=[round(lo, 4), round(hi, 4)])
            say(f"{bits:2d} bit {k:12s} graph {med:8.4f} ms a call, {1e3 * med / B:8.2f} us a frame  (reps {lo:.4f}-{hi:.4f})")
        for new, old in (("match", "peak"), ("weave", "table")):
            a_, b_ = leg[old]["us_per_frame"], leg[old + "_again"]["us_per_frame"]
            spread = H.pair_spread(a_, b_)
            got = leg[new]["us_per_frame"]
            leg[f"{new}_vs_{old}"] = dict(ratio_to_slower_yardstick=round(got / max(a_, b_), 3), yardstick_spread=round(spread, 3),
                                          aim_met=bool(got <= max(a_, b_)))
            say(f"{bits:2d} bit {new} / {old}: {got / max(a_, b_):.3f} of the slower of the yardstick's two timings per frame "
                f"(they differ by {100 * spread:.1f} %): the aim is {'met' if got <= max(a_, b_) else 'MISSED'}")
        res["kernel"][f"{bits}bit"] = leg
        del cases
        torch.cuda.empty_cache()

    if a.frames:
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        _write_telecined_clip(src, a.frames, h, w)
        reports = []

        def ivtc():
            reports.append(cli.run_ivtc(cli.parse_args(["ivtc", "--input", src, "--output", out, "--order", "tff"])))
            return reports[-1]["frames_out"]

        def deinterlace():
            return cli.run_deinterlace(cli.parse_args(["deinterlace", "--input", src, "--output", out, "--order", "tff",
                                                       "--rate", "frame"]))
        written = {}
        wall = H.interleaved_wall({"ivtc": ivtc, "deinterlace_frame": deinterlace, "ivtc_again": ivtc}, reps=2, device=dev,
                                  results=written)
        for k, secs in wall.items():
            med, lo, hi = H.summary(secs)
            res["clip"][k] = dict(source_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                  spread_s=[round(lo, 3), round(hi, 3)], frames_out=written[k])
            say(f"clip {k:18s} {a.frames / med:7.2f} source frames/s  wall {med:.3f} s  (runs {lo:.3f}-{hi:.3f})  "
                f"{written[k]} frames out")
        rep = reports[-1]
        res["clip"].update(frames=a.frames, format="C420jpeg", chunk_frames=32, matches=rep["matches"],
                           combed=len(rep["combed"]), dropped=len(rep["dropped"]),
                           content="2:3 pulldown (tff, phase 0) of synthetic film: a smooth picture moving 3 x 1 pixels a film frame")
        say(f"clip: matches {rep['matches']}, {len(rep['combed'])} combed, {len(rep['dropped'])} dropped of {a.frames} frames")
        for f in (src, out):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
    report.finish(res)


if __name__ == "__main__":
    main()
