"""Time the deinterlacer (deinterlace.py): its kernel beside another kernel that reads two frames and
more and writes one, and what `cli deinterlace` makes of a 1080i clip end to end.

  kernel    B = 8 source frames of 1080p per call, deinterlaced out of a window of B + 2 (one context frame either
            side).  A member of the rotating set is such a window and its output frames; the calls rotate over at least
            `--set-gb` GB (several times the 256 MB Infinity Cache), so the frames come from memory.
              <format>/<method>/<rate>   i420 (Y4M C420jpeg), yuv422p10le, nv12 and uyvy422; "adaptive" and "bob"; "field"
                                         (2 B output frames) and "frame" (B).  i420 and yuv422p10le are step-1 formats (the
                                         vector path), nv12's chroma and all of uyvy422 are stepped (the per-sample path)
              warp / warp_again          fiunet_warp_table_u8 at wn / den = 2 / 5 on B luma planes of the same size: the
                                         yardstick, timed twice for the in-job spread
              warp10 / warp10_again      the same on 16-bit words (fiunet_warp_table_p10)
            Device time from HIP events around `--replays` replays of a captured graph of `--iters` calls, after
            `--warmup` calls; reported per output frame and per 1080p plane's worth of output samples (what the yardstick
            writes in a plane).  The aim: "adaptive" on a step-1 format is no slower per plane than the slower of the
            yardstick's two timings.
  clip      `cli deinterlace --order tff` of a `--frames`-frame 1080i I420 Y4M clip, file to file, twice; host wall clock
            around each run, in source frames per second.
The median and the spread of `--reps` interleaved repetitions are printed, and written to `--out` when given.  One JSON
line last.

    python tools/deinterlace_timing.py [--set-gb 1 --frames 257 --reps 5 --out profiles/deinterlace_timing.txt]
"""
import argparse
import os
import tempfile

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import _native, cli, deinterlace as D
from ai_based_frame_interpolation_amd.layout import frame_layout

B = 8
FORMATS = {"i420": ("y4m", "420jpeg"), "yuv422p10le": "yuv422p10le", "nv12": "nv12", "uyvy422": "uyvy422"}
STEP1 = ("i420", "yuv422p10le")


def _cases(dev, h, w, set_bytes):
    g = torch.Generator(device=dev).manual_seed(1)
    cases, info = {}, {}
    for name, kind in FORMATS.items():
        lay = frame_layout(kind, h, w)
        dtype, hi, item = (torch.uint8, 256, 1) if lay.bits == 8 else (torch.int16, 1024, 2)
        member = (B + 2 + 2 * B) * lay.samples * item
        n_set = max(2, -(-set_bytes // member))
        windows = [torch.randint(0, hi, (B + 2, lay.samples), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
        outs = [torch.empty((2 * B, lay.samples), dtype=dtype, device=dev) for _ in range(n_set)]
        info[name] = dict(members=n_set, set_mb=round(n_set * member / 2**20), samples=lay.samples, planes=len(lay.planes))
        for method in D.METHODS:
            for rate, per in (("field", 2), ("frame", 1)):
                def fn(k, lay=lay, windows=windows, outs=outs, method=method, rate=rate, per=per):
                    D.deinterlace(windows[k], lay, lay.bits, "tff", rate, method, first=1, count=B, out=outs[k][:per * B])
                cases[f"{name}/{method}/{rate}"] = H.Rotate(fn, n_set)
    flow_member = B * h * w * 8
    n_flow = max(2, -(-set_bytes // (flow_member + (2 * B + 1) * h * w)))
    flows = [(torch.rand((B, h, w, 2), device=dev, generator=g) - 0.5) * 8 for _ in range(n_flow)]
    entries = [(r, 2, 5, r, -1) for r in range(B)]
    plane = (0, h, w, w, 1, h * w)
    for bits, tag in ((8, "warp"), (10, "warp10")):
        dtype, hi = (torch.uint8, 256) if bits == 8 else (torch.int16, 1024)
        grids = [torch.randint(0, hi, (B + 1, h * w), dtype=dtype, device=dev, generator=g) for _ in range(n_flow)]
        wouts = [torch.empty((B, h * w), dtype=dtype, device=dev) for _ in range(n_flow)]

        def fn(k, grids=grids, wouts=wouts, bits=bits):
            _native.warp_table(grids[k], B + 1, plane, flows[k], None, entries, wouts[k], plane, bits)
        cases[tag] = H.Rotate(fn, n_flow)
        cases[tag + "_again"] = H.Rotate(fn, n_flow)
    return cases, info


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
    dev = H.need_gpu("deinterlace_timing")
    report = H.Report(a.out)
    say = report.say
    h, w = a.height, a.width
    res = {"shape": [h, w], "source_frames_per_call": B, "kernel": {}, "clip": {},
           "protocol": "kernel: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, replays=a.replays,
                                               set_gb=a.set_gb, wall_reps=2)}
    say(f"deinterlace_timing: {torch.cuda.get_device_name(dev)}; {res['protocol']}")
    cases, info = _cases(dev, h, w, int(a.set_gb * 1e9))
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters, graph=True, replays=a.replays)
    leg = dict(info)
    for k in cases:
        med, lo, hi = H.summary(ms[k])
        if "/" in k:
            name, _, rate = k.split("/")
            frames = B * (2 if rate == "field" else 1)
            per_plane = 1e3 * med / (frames * info[name]["samples"] / (h * w))
            leg[k] = dict(ms=round(med, 4), us_per_output_frame=round(1e3 * med / frames, 2), us_per_plane=round(per_plane, 2),
                          spread_ms=[round(lo, 4), round(hi, 4)])
            say(f"{k:28s} graph {med:8.4f} ms a call, {1e3 * med / frames:8.2f} us an output frame, {per_plane:7.2f} us a "
                f"1080p plane of samples  (reps {lo:.4f}-{hi:.4f})")
        else:
            leg[k] = dict(ms=round(med, 4), us_per_plane=round(1e3 * med / B, 2), spread_ms=[round(lo, 4), round(hi, 4)])
            say(f"{k:28s} graph {med:8.4f} ms a call, {1e3 * med / B:8.2f} us a warped plane  (reps {lo:.4f}-{hi:.4f})")
    for name in STEP1:
        yard = "warp" if name == "i420" else "warp10"
        a_, b_ = leg[yard]["us_per_plane"], leg[yard + "_again"]["us_per_plane"]
        spread = H.pair_spread(a_, b_)
        for rate in ("field", "frame"):
            got = leg[f"{name}/adaptive/{rate}"]["us_per_plane"]
            leg[f"{name}/adaptive/{rate}_vs_{yard}"] = dict(ratio_to_slower_yardstick=round(got / max(a_, b_), 3),
                                                            yardstick_spread=round(spread, 3), aim_met=bool(got <= max(a_, b_)))
            say(f"{name}/adaptive/{rate} / {yard}: {got / max(a_, b_):.3f} of the slower of the yardstick's two timings per "
                f"plane (they differ by {100 * spread:.1f} %): the aim is {'met' if got <= max(a_, b_) else 'MISSED'}")
    res["kernel"] = leg
    del cases
    torch.cuda.empty_cache()

    if a.frames:
        tmp = tempfile.mkdtemp(dir=a.dir)
        src, out = os.path.join(tmp, "in.y4m"), os.path.join(tmp, "out.y4m")
        H.write_y4m_clip(src, a.frames, h, w)

        def run():
            return cli.run_deinterlace(cli.parse_args(["deinterlace", "--input", src, "--output", out, "--order", "tff"]))
        written = {}
        wall = H.interleaved_wall({"deinterlace": run, "deinterlace_again": run}, reps=2, device=dev, results=written)
        for k, secs in wall.items():
            med, lo, hi = H.summary(secs)
            res["clip"][k] = dict(source_frames_per_s=round(a.frames / med, 2), wall_s=round(med, 3),
                                  spread_s=[round(lo, 3), round(hi, 3)])
            say(f"clip {k:18s} {a.frames / med:7.2f} source frames/s  wall {med:.3f} s  (runs {lo:.3f}-{hi:.3f})")
        res["clip"].update(frames=a.frames, frames_out=written["deinterlace"], format="C420jpeg", chunk_frames=32)
        for f in (src, out):
            if os.path.exists(f):
                os.remove(f)
        os.rmdir(tmp)
    report.finish(res)


if __name__ == "__main__":
    main()
