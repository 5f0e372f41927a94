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
import os
import tempfile

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import _native, optical_flow as OF

B = 8


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
        cases[name] = H.Rotate(fn, n_set)
    add("warp", 8, 1, True)
    add("table", 8, 1, False)
    add("warp_again", 8, 1, True)
    add("table_step2", 8, 2, False)
    add("table_step3", 8, 3, False)
    add("warp10", 10, 1, True)
    add("table10", 10, 1, False)
    add("warp10_again", 10, 1, True)
    return cases, flows, dict(members=n_set, set_mb=round(n_set * member / 2**20))


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
    dev = H.need_gpu("retime_motion_timing")
    report = H.Report(a.out)
    say = report.say
    h, w = a.height, a.width
    res = {"shape": [h, w], "planes_per_call": B, "kernel": {}, "streamed": {},
           "protocol": "kernel: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, replays=a.replays,
                                               set_gb=a.set_gb, wall_reps=max(1, a.reps // 2))}
    say(f"retime_motion_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    cases, flows, info = _kernel_cases(dev, h, w, int(a.set_gb * 1e9))
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters, graph=True, replays=a.replays)
    leg = dict(info)
    for k in cases:
        med, lo, hi = H.summary(ms[k])
        leg[k] = dict(ms=round(med, 4), us_per_plane=round(1e3 * med / B, 2), spread_ms=[round(lo, 4), round(hi, 4)])
        say(f"{k:14s} graph {med:8.4f} ms a call, {1e3 * med / B:8.2f} us a warped plane  (reps {lo:.4f}-{hi:.4f})")
    for new, old in (("table", "warp"), ("table10", "warp10")):
        a_, b_ = leg[old]["ms"], leg[old + "_again"]["ms"]
        spread, ratio = H.pair_spread(a_, b_), leg[new]["ms"] / max(a_, b_)
        leg[f"{new}_vs_{old}"] = dict(ratio_to_slower_yardstick=round(ratio, 3), yardstick_spread=round(spread, 3),
                                      within_spread=bool(leg[new]["ms"] <= max(a_, b_)))
        say(f"{new} / {old}: {ratio:.3f} of the slower of the yardstick's two timings (they differ by {100 * spread:.1f} %)")
    lead = torch.randint(0, 256, (B + 1, h, w), dtype=torch.uint8, device=dev)
    fl = H.interleaved({"flow": lambda: OF.farneback_flow(lead[:B], lead[1:], "hip")}, warmup=a.warmup, reps=a.reps, iters=3)
    med, lo, hi = H.summary(fl["flow"])
    leg["flow"] = dict(ms=round(med, 3), ms_per_pair=round(med / B, 3), spread_ms=[round(lo, 3), round(hi, 3)])
    say(f"flow           eager {med:8.3f} ms a call of {B} pairs, {med / B:.3f} ms a pair  (reps {lo:.3f}-{hi:.3f})")
    res["kernel"] = leg
    del cases, flows, lead
    torch.cuda.empty_cache()

    if a.frames:
        _, fi = H.seeded_model(3, "bf16", dev)
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        H.write_y4m_clip(src, a.frames, h, w)

        def run(mode):
            return lambda: fi.interpolate_video(src, out, fps=60, time_depth=2, retime=mode, chunk_frames=a.chunk)
        runs = {"blend": run("blend"), "motion": run("motion"), "blend_again": run("blend"), "motion_again": run("motion")}
        written = {}
        # (each mode is run twice a round, so half of `--reps` rounds give `--reps` runs of it)
        wall = H.interleaved_wall(runs, reps=max(1, a.reps // 2), device=dev, results=written)
        for k in runs:
            med, lo, hi = H.summary(wall[k])
            res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                      spread_s=[round(lo, 3), round(hi, 3)])
            say(f"streamed {k:13s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  (runs {lo:.3f}-{hi:.3f})")
        s = res["streamed"]
        blend = H.summary(wall["blend"] + wall["blend_again"])[0]
        motion = H.summary(wall["motion"] + wall["motion_again"])[0]
        s.update(frames=a.frames, frames_out=written["motion"], chunk_frames=a.chunk, network="rgb", precision="bf16",
                 motion_vs_blend=round(motion / blend, 3), flow_and_warp_share=round((motion - blend) / motion, 3))
        say(f"streamed: motion takes {motion / blend:.3f} of blend's wall time; flow and warp are "
            f"{100 * (motion - blend) / motion:.1f} % of the motion run")
        for f in (src, out):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
    report.finish(res)


if __name__ == "__main__":
    main()
