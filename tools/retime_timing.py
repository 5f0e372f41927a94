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
import os
import tempfile

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P


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
        return H.Rotate(lambda k: P.retime.resample(grids[k], plan, 0, j0, n_out, bits=bits, flags=flags, out=outs[k]),
                       n_set)
    cases = {
        "blend": resample(none),
        "copy": resample(every),
        # (in place: it turns the grids into held ones, which costs the resampling cases nothing)
        "hold": H.Rotate(lambda k: P.scene.hold_cut_frames(grids[k], every, plan.G), n_set),
    }
    work = {   # name: (frames, bytes moved)
        "blend": (n_out, (3 * blends + 2 * (n_out - blends)) * fb),
        "copy": (n_out, 2 * n_out * fb),
        "hold": (n_int * (plan.G - 1), 2 * n_int * (plan.G - 1) * fb),
    }
    return cases, work, dict(frame_bytes=fb, out_frames=n_out, blended_frames=blends, grids=n_set,
                       set_mb=round(n_set * (rows + n_out) * fb / 2**20))


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
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("retime_timing")
    report = H.Report(a.out)
    h, w = a.height, a.width
    plan = P.retime.plan(24, 60, 2)
    res = {"shape": [h, w], "ratio": [plan.p, plan.q], "time_depth": plan.depth, "kernel": {}, "streamed": {},
           "protocol": "kernel: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb, wall_reps=a.reps)}
    for bits in (8, 10):
        cases, work, info = _kernel_cases(dev, bits, h, w, a.intervals, plan, int(a.set_gb * 1e9))
        ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
        leg = dict(info)
        for k, (frames, moved) in work.items():
            med, lo, hi = H.summary(ms[k])
            leg[k] = dict(ms=round(med, 4), spread_ms=[round(lo, 4), round(hi, 4)],
                          us_per_frame=round(1e3 * med / frames, 2), gb_per_s=round(moved / (med * 1e-3) / 1e9, 1))
            report.say(f"{bits:2d} bit {k:6s} {med:8.3f} ms  (reps {lo:.3f}-{hi:.3f})  "
                       f"{leg[k]['us_per_frame']:8.2f} us / frame  {leg[k]['gb_per_s']:7.1f} GB/s")
        leg["blend_vs_hold"] = round(leg["blend"]["gb_per_s"] / leg["hold"]["gb_per_s"], 3)
        res["kernel"][f"{bits}bit"] = leg
        del cases
        torch.cuda.empty_cache()

    _, fi = H.seeded_model(3, "bf16", dev)
    tmp = tempfile.mkdtemp(dir=a.dir)
    src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
    H.write_y4m_clip(src, a.frames, h, w)
    runs = {
        "factor4": lambda: fi.interpolate_video(src, out, 4, chunk_frames=a.chunk),
        "fps60": lambda: fi.interpolate_video(src, out, fps=60, time_depth=2, chunk_frames=a.chunk),
    }
    written = {}
    wall = H.interleaved_wall(runs, reps=a.reps, device=dev, results=written)
    for k in runs:
        med, lo, hi = H.summary(wall[k])
        res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                  spread_s=[round(lo, 3), round(hi, 3)], frames_out=written[k])
        report.say(f"streamed {k:8s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  "
                   f"(runs {lo:.3f}-{hi:.3f})  {written[k]} frames out")
    res["streamed"].update(frames=a.frames, chunk_frames=a.chunk, network="rgb", precision="bf16",
                           fps60_vs_factor4=round(res["streamed"]["fps60"]["input_frames_per_s"]
                                                  / res["streamed"]["factor4"]["input_frames_per_s"], 3))
    for f in (src, out):
        if os.path.exists(f):
            os.remove(f)
    os.rmdir(tmp)
    report.finish(res)


if __name__ == "__main__":
    main()
