"""Time motion-guided chroma (chroma.py): its two kernels beside the warp they are built on, and what
`chroma="motion"` costs a streamed factor-2 run of the grayscale network.

  kernel    B = 8 inserted 1080p 4:2:0 frames per call.  A member of the rotating set is a 9-row grid of I420 frames (A =
            rows 0..7, B = rows 1..8), 8 luma planes for the network's M, 8 flow fields [8, 1080, 1920, 2], the pick map
            and 8 output frames; the calls rotate over at least `--set-gb` GB (several times the 256 MB Infinity Cache), so
            the frames come from memory.  The planes hold random samples, so about half of the blocks take the warp.
              warp_table / warp_table_again   fiunet_warp_table_u8 at wn = 1, den = 2 on the luma and the two chroma
                                  planes of the same frames (three calls): the yardstick, timed twice for the in-job spread
              pick                fiunet_chroma_pick_u8: one luma-size warp, the average, the block sums
              fill                fiunet_chroma_fill_u8: both chroma planes
              pick_fill           the two together: what a level of the route adds beside the flow
            Device time from HIP events around `--replays` replays of a captured graph of `--iters` calls, after
            `--warmup` calls.  The aim is "pick_fill no slower than the yardstick beyond the spread of its two timings":
            both do one luma-size and two chroma-size warps.  It is recorded, not gated.
  streamed  interpolate_video(file, file, factor=2, chunk_frames=32) of a 257-frame 1080p I420 clip, grayscale network,
            bf16, batch 8: chroma "average" and "motion", each twice, interleaved; host wall clock around each call.  No
            target is set: a flow per inserted frame beside a forward per inserted frame.
The median and the spread of `--reps` interleaved repetitions are printed, and written to `--out` when given.  One JSON
line last.

    python tools/chroma_timing.py [--set-gb 1 --frames 257 --chunk 32 --reps 5 --out profiles/chroma_timing.txt]
"""
import argparse
import os
import tempfile

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import _native

B = 8


def _kernel_cases(dev, h, w, set_bytes):
    g = torch.Generator(device=dev).manual_seed(1)
    hc, wc, ph, pw = h // 2, w // 2, -(-h // 8), -(-w // 8)
    row = h * w + 2 * hc * wc
    member = (B + 1) * row + B * h * w + B * h * w * 8 + B * ph * pw + B * row
    n_set = max(2, -(-set_bytes // member))
    grids = [torch.randint(0, 256, (B + 1, row), dtype=torch.uint8, device=dev, generator=g) for _ in range(n_set)]
    mids = [torch.randint(0, 256, (B, h * w), dtype=torch.uint8, device=dev, generator=g) for _ in range(n_set)]
    flows = [(torch.rand((B, h, w, 2), device=dev, generator=g) - 0.5) * 8 for _ in range(n_set)]
    picks = [torch.empty((B, ph, pw), dtype=torch.uint8, device=dev) for _ in range(n_set)]
    outs = [torch.empty((B, row), dtype=torch.uint8, device=dev) for _ in range(n_set)]
    luma = (0, h, w, w, 1, row)
    chroma = [(h * w + p * hc * wc, hc, wc, wc, 1, row) for p in range(2)]
    entries = [(r, 1, 2, r, -1) for r in range(B)]

    def yardstick(k):
        for plane in [luma] + chroma:
            _native.warp_table(grids[k], B + 1, plane, flows[k], None, entries, outs[k], plane, 8)

    def pick(k):
        _native.chroma_pick(grids[k], luma, grids[k][1:], luma, mids[k], (0, h, w, w, 1, h * w), flows[k], picks[k], 8)

    def fill(k):
        _native.chroma_fill(grids[k], chroma, grids[k][1:], chroma, flows[k], picks[k], (2, 2), outs[k], chroma, 8)

    def both(k):
        pick(k)
        fill(k)
    for k in range(n_set):   # the fill case reads maps that the pick case may not have made yet
        pick(k)
    share = float(torch.stack(picks).float().mean())
    cases = {name: H.Rotate(fn, n_set) for name, fn in (("warp_table", yardstick), ("pick", pick), ("fill", fill),
                                                        ("pick_fill", both), ("warp_table_again", yardstick))}
    return cases, dict(members=n_set, set_mb=round(n_set * member / 2**20), share_warped=round(share, 3))


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
    dev = H.need_gpu("chroma_timing")
    report = H.Report(a.out)
    say = report.say
    h, w = a.height, a.width
    res = {"shape": [h, w], "frames_per_call": B, "kernel": {}, "streamed": {},
           "protocol": "kernel: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, replays=a.replays,
                                               set_gb=a.set_gb, wall_reps=max(1, a.reps // 2))}
    say(f"chroma_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    cases, info = _kernel_cases(dev, h, w, int(a.set_gb * 1e9))
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters, graph=True, replays=a.replays)
    leg = dict(info)
    for k in cases:
        med, lo, hi = H.summary(ms[k])
        leg[k] = dict(ms=round(med, 4), us_per_frame=round(1e3 * med / B, 2), spread_ms=[round(lo, 4), round(hi, 4)])
        say(f"{k:17s} graph {med:8.4f} ms a call, {1e3 * med / B:8.2f} us an inserted frame  (reps {lo:.4f}-{hi:.4f})")
    a_, b_ = leg["warp_table"]["ms"], leg["warp_table_again"]["ms"]
    spread, ratio = H.pair_spread(a_, b_), leg["pick_fill"]["ms"] / max(a_, b_)
    met = bool(leg["pick_fill"]["ms"] <= max(a_, b_))
    leg["pick_fill_vs_warp_table"] = dict(ratio_to_slower_yardstick=round(ratio, 3), yardstick_spread=round(spread, 3),
                                          within_spread=met)
    say(f"pick_fill / warp_table: {ratio:.3f} of the slower of the yardstick's two timings (they differ by "
        f"{100 * spread:.1f} %); {info['share_warped']:.2f} of the blocks warped; the aim is "
        f"{'met' if met else '**MISSED**'}")
    res["kernel"] = leg
    del cases
    torch.cuda.empty_cache()

    if a.frames:
        _, fi = H.seeded_model(1, "bf16", dev)
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        H.write_y4m_clip(src, a.frames, h, w)

        def run(mode):
            return lambda: fi.interpolate_video(src, out, 2, chroma=mode, chunk_frames=a.chunk)
        runs = {"average": run("average"), "motion": run("motion"), "average_again": run("average"),
                "motion_again": run("motion")}
        written = {}
        # (each mode is run twice a round, so half of `--reps` rounds give `--reps` runs of it)
        wall = H.interleaved_wall(runs, reps=max(1, a.reps // 2), device=dev, results=written)
        for k in runs:
            med, lo, hi = H.summary(wall[k])
            res["streamed"][k] = dict(input_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                      spread_s=[round(lo, 3), round(hi, 3)])
            say(f"streamed {k:14s} {a.frames / med:7.2f} input frames/s  wall {med:.3f} s  (runs {lo:.3f}-{hi:.3f})")
        average = H.summary(wall["average"] + wall["average_again"])[0]
        motion = H.summary(wall["motion"] + wall["motion_again"])[0]
        res["streamed"].update(frames=a.frames, frames_out=written["motion"], chunk_frames=a.chunk, network="gray",
                               precision="bf16", motion_vs_average=round(motion / average, 3))
        say(f"streamed: chroma \"motion\" takes {motion / average:.3f} of the wall time of \"average\"")
        for f in (src, out):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
    report.finish(res)


if __name__ == "__main__":
    main()
