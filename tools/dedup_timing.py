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
import os
import tempfile

import numpy as np
import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native, imageio_lite as IO


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
        return H.Rotate(lambda k: _native.pair_sad(stacks[k], sums, bits), n_det)

    def retime():
        return H.Rotate(lambda k: P.retime.resample(grids[k], plan, 0, j0, n_out, bits=bits, out=outs[k]), n_set)
    detect_bytes = 2 * n_int * fb
    moved = (3 * blends + 2 * (n_out - blends)) * fb
    cases = {
        "sad": (sad(), detect_bytes),
        "peak": (H.Rotate(lambda k: _native.pair_peak(stacks[k], peaks, bits), n_det), detect_bytes),
        "sad_again": (sad(), detect_bytes),
        "retime": (retime(), moved),
        "table": (H.Rotate(lambda k: P.retime.resample_table(grids[k], entries, bits, out=outs[k]), n_set), moved),
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
    dev = H.need_gpu("dedup_timing")
    report = H.Report(a.out)
    say = report.say
    h, w = a.height, a.width
    plan = P.retime.plan(24, 60, 2)
    res = {"shape": [h, w], "kernel": {}, "streamed": {},
           "protocol": "kernel: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, replays=a.replays,
                                               set_gb=a.set_gb, wall_reps=a.reps)
                       + f"; eager: of {a.iters} calls from Python, each case's after its graph"}
    say(f"dedup_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    for bits in (8, 10):
        cases, info = _kernel_cases(dev, bits, h, w, a.intervals, plan, int(a.set_gb * 1e9))
        H.interleaved({k: fn for k, (fn, _) in cases.items()}, warmup=a.warmup, reps=0, iters=a.iters)   # (the warm-up alone)
        # the figure is taken from a captured graph of `--iters` calls (on the members of the set in turn), replayed
        # `--replays` times: the device runs the kernels back to back, with no Python call, ctypes array or launch from
        # the host in between.  The same calls issued eagerly from Python are timed beside it, each case's directly
        # after its graph, to show the host's share.
        timed, count = {}, {}
        for k, (fn, _) in cases.items():
            graph = H.graph_of(fn, a.iters)
            graph.replay()
            timed[k], count[k] = graph.replay, a.replays
            timed[k + " eager"], count[k + " eager"] = fn, a.iters
        got = H.interleaved(timed, warmup=0, reps=a.reps, iters=count)
        ms, eager = {k: [v / a.iters for v in got[k]] for k in cases}, {k: got[k + " eager"] for k in cases}
        leg = dict(info)
        for k, (_, moved) in cases.items():
            (med, lo, hi), (med_e, lo_e, hi_e) = H.summary(ms[k]), H.summary(eager[k])
            leg[k] = dict(ms=round(med, 4), spread_ms=[round(lo, 4), round(hi, 4)],
                          gb_per_s=round(moved / (med * 1e-3) / 1e9, 1), eager_ms=round(med_e, 4),
                          eager_spread_ms=[round(lo_e, 4), round(hi_e, 4)])
            say(f"{bits:2d} bit {k:12s} graph {med:8.4f} ms  (reps {lo:.4f}-{hi:.4f})  "
                f"{leg[k]['gb_per_s']:7.1f} GB/s   eager {med_e:8.4f} ms  (reps {lo_e:.4f}-{hi_e:.4f})")
        for new, old in (("peak", "sad"), ("table", "retime")):
            a_, b_ = leg[old]["ms"], leg[old + "_again"]["ms"]
            spread = H.pair_spread(a_, b_)
            ratio = leg[new]["ms"] / max(a_, b_)
            leg[f"{new}_vs_{old}"] = dict(ratio_to_slower_yardstick=round(ratio, 3), yardstick_spread=round(spread, 3),
                                          within_spread=bool(leg[new]["ms"] <= max(a_, b_)))
            say(f"{bits:2d} bit {new} / {old}: {ratio:.3f} of the slower of the yardstick's two timings "
                f"(they differ by {100 * spread:.1f} %)")
        res["kernel"][f"{bits}bit"] = leg
        del cases, timed   # (`fn` and `graph`, the loop's last, hold `retime_again`'s set until the next leg has allocated
        #                    its own, as this tool's loop variables always have: where a set lands is part of its figures)
        torch.cuda.empty_cache()

    if a.frames:
        _, fi = H.seeded_model(3, "bf16", dev)
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        repeats = _write_clip(src, a.frames, h, w)
        log = []

        def dedup():
            log.clear()   # (each run logs the same intervals: the last run's are counted below)
            return fi.interpolate_video(src, out, 4, chunk_frames=a.chunk, dedup=0, dedup_log=log)
        runs = {
            "plain": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk),
            "dedup": dedup,
            "plain_again": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk),
        }
        written = {}
        wall = H.interleaved_wall(runs, reps=a.reps, device=dev, results=written)
        dead = int(sum(d.sum() for _, d in log))
        for k in runs:
            med, lo, hi = H.summary(wall[k])
            res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                      spread_s=[round(lo, 3), round(hi, 3)], frames_out=written[k])
            say(f"streamed {k:12s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  "
                f"(runs {lo:.3f}-{hi:.3f})  {written[k]} frames out")
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
    report.finish(res)


if __name__ == "__main__":
    main()
