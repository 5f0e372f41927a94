"""Time the motion-compensated baseline: the HIP flow and warp kernels beside the torch restatement they
restate, on the same device in the same process, and the baseline's share of a hold-out run.

  pairs     Farneback flow plus the "motion" warp of B frame pairs (B = 8 at 1080p, B = 8 at 256x256; a moving texture,
            uint8), per pair:
              hip      optical_flow.farneback_flow + optical_flow.warp, backend "hip" (fiunet_farneback_flow,
                       fiunet_flow_warp; the workspace is the cached one, the outputs are allocated per call as a caller's
                       would be); device time from HIP events around `--iters` back-to-back calls after `--warmup` calls
              torch    the same two calls with backend "torch": `calc_optical_flow_farneback` and the fixed-point remap pair
                       by pair, on the same device tensors - the YARDSTICK.  A few hundred small tensor operations per
                       pair, some of them with host synchronisation, so it is timed by the wall clock behind a device
                       synchronise, `--torch-iters` calls.
            `--reps` repetitions interleaved over the cases; median and spread.  The flow alone is timed the same way.
  score     one `holdout.score_video` run of a `--clip-frames`-frame 1080p C420jpeg clip (tools/holdout_timing.py's
            moving texture), sliding triplets, all five methods, RGB network at bf16: wall time behind a device
            synchronise, and the share of it inside the flow methods (`holdout._predict_flow`, timed behind synchronises of
            its own in a second run).
One JSON line last.

    python tools/flow_timing.py [--batch 8 --iters 20 --torch-iters 1 --reps 5 --clip-frames 65]
"""
import argparse
import os
import tempfile

import numpy as np
import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import holdout, optical_flow as OF
from oracle import unet_oracle as O
from holdout_timing import _clip


def _pairs(dev, b, h, w):
    """B pairs of a moving texture, uint8 [B, h, w] each: pair i moves by (2 + i, 1) pixels."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    tex = lambda dx, dy: 128 + 90 * np.sin((xx - dx) / 9.0) * np.cos((yy - dy) / 13.0) + 30 * np.cos((xx - dx + yy - dy) / 5.0)
    f0 = np.stack([tex(0.3 * i, 0) for i in range(b)])
    f1 = np.stack([tex(0.3 * i + 2 + i % 3, 1) for i in range(b)])
    q = lambda a: torch.from_numpy(np.clip(np.rint(a), 0, 255).astype(np.uint8)).to(dev)
    return q(f0), q(f1)


def _pair_leg(dev, b, h, w, a, say):
    f0, f1 = _pairs(dev, b, h, w)
    both = lambda backend: OF.warp(f0, f1, OF.farneback_flow(f0, f1, backend), "motion", backend)
    gap = (both("hip").int() - both("torch").int()).abs()
    ms = H.interleaved({"hip flow": lambda: OF.farneback_flow(f0, f1, "hip"), "hip flow+warp": lambda: both("hip")},
                       warmup=a.warmup, reps=a.reps, iters=a.iters)
    n = a.torch_iters
    secs = H.interleaved_wall({"torch flow": lambda: [OF.farneback_flow(f0, f1, "torch") for _ in range(n)],
                               "torch flow+warp": lambda: [both("torch") for _ in range(n)]}, reps=a.reps, device=dev)
    ms.update({k: [s * 1e3 / n for s in v] for k, v in secs.items()})
    leg = dict(batch=b, shape=f"{h}x{w}", pixels_differing=round(float((gap != 0).float().mean()), 6),
               largest_difference=int(gap.max()))
    for k in ms:
        med, lo, hi = (v / b for v in H.summary(ms[k]))
        leg[k] = dict(ms_per_pair=round(med, 4), spread_ms=[round(lo, 4), round(hi, 4)])
        say(f"{b}x{h}x{w} {k:16s} {med:10.4f} ms / pair  (reps {lo:.4f}-{hi:.4f})")
    for k in ("flow", "flow+warp"):
        leg[f"torch / hip time, {k}"] = round(leg[f"torch {k}"]["ms_per_pair"] / leg[f"hip {k}"]["ms_per_pair"], 2)
        say(f"{b}x{h}x{w} torch / hip time, {k}: {leg[f'torch / hip time, {k}']}")
    return leg


def _score(dev, frames, h, w, say):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="bf16")
    m.load_state_dict(O.make_interpolating_state_dict(n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    spent = [0.0]
    inner = holdout._predict_flow

    def timed(*a, **k):
        got = []
        spent[0] += H.wall_s(lambda: got.append(inner(*a, **k)))
        return got[0]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "clip.y4m")
        _clip(src, frames, h, w)
        holdout.score_video(m, src, methods=holdout.ALL_METHODS, chunk_frames=8)   # warm-up
        for name, methods in (("three methods", holdout.METHODS), ("five methods", holdout.ALL_METHODS)):
            got = []
            out[f"wall_s, {name}"] = round(H.wall_s(lambda: got.append(holdout.score_video(m, src, methods=methods))), 3)
            res = got[0]
        holdout._predict_flow = timed
        try:
            wall2 = H.wall_s(lambda: holdout.score_video(m, src, methods=holdout.ALL_METHODS))
        finally:
            holdout._predict_flow = inner
    say(holdout.summary_table(res))
    out.update(frames=frames, scored_frames=len(res["scored_frames"]), timed_run_wall_s=round(wall2, 3),
               flow_s=round(spent[0], 3), flow_share=round(spent[0] / wall2, 3))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--torch-iters", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--clip-frames", type=int, default=65)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("flow_timing")
    report = H.Report(a.out)
    res = {"protocol": "hip: " + H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters) + f"; torch: host clock behind a "
                       f"device synchronise on either side, one untimed round, median of {a.reps} interleaved runs of "
                       f"{a.torch_iters} call(s); per pair"}
    res["1080p"] = _pair_leg(dev, a.batch, 1080, 1920, a, report.say)
    res["256x256"] = _pair_leg(dev, a.batch, 256, 256, a, report.say)
    torch.cuda.empty_cache()
    res["score_video"] = _score(dev, a.clip_frames, 1080, 1920, report.say)
    report.say(f"score_video: {res['score_video']}")
    report.finish(res)


if __name__ == "__main__":
    main()
