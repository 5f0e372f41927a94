"""Time the plane metrics of hold-out scoring beside the contiguous uint8 kernels, in one process.

  kernels   PSNR and SSIM of B planes of H x W (B = 8, 1080p), through the C ABI with the workspace and the result
            allocated once (the calls are a few microseconds of device time: the Python wrappers' allocations would be
            most of what is timed):
              u8_a, u8_b        fiunet_psnr_u8 / fiunet_ssim_u8, the yardstick, measured as two cases: the difference
                                between them is the run-to-run spread of this job
              plane8            fiunet_plane_psnr / fiunet_plane_ssim on the same contiguous uint8 planes
              plane8_i420y      the same on the Y planes of packed I420 rows (image stride 1.5 H x W)
              plane10           contiguous 10-bit planes (16-bit words)
              plane10_i420y     the Y planes of packed 10-bit 4:2:0 rows
            The planes come from memory, not from a cache: the calls rotate over a set of pred / target pairs of at
            least `--set-gb` GB for the uint8 cases (several times the 256 MB Infinity Cache).  Device time from HIP
            events around `--iters` back-to-back calls after `--warmup` calls; `--reps` repetitions interleaved over
            the cases; median and spread.  Bytes moved: both planes, once.
  score     one `holdout.score_video` run of a `--clip-frames`-frame 1080p C420jpeg clip (a moving texture written to
            a temporary file), sliding triplets, all three methods, RGB network at bf16: wall time behind a device
            synchronise, scored frames per second, and the share of it spent inside the route's forward (`route.run`,
            timed behind synchronises of its own in a second run, so that the first run's figure carries none).
One JSON line last.

    python tools/holdout_timing.py [--batch 8 --set-gb 1 --iters 200 --reps 7 --clip-frames 65]
"""
import argparse
import ctypes
import os
import tempfile

import numpy as np
import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native, holdout, stream, imageio_lite as IO
from oracle import unet_oracle as O


def _kernel_cases(dev, b, h, w, set_bytes):
    """A set of `n_set` (pred, target) pairs of byte buffers, each wide enough for b packed 10-bit 4:2:0 frames; every
    case reads its planes out of them (a metric's time does not depend on the values; 16-bit words above 1023 read as
    1023).  -> (cases, bytes read per case, info)"""
    L = _native.lib()
    n, fs = h * w, P.i420_frame_bytes(h, w)
    n_set = max(2, -(-set_bytes // (2 * b * n)))
    g = torch.Generator(device=dev).manual_seed(h)
    pairs = [tuple(torch.randint(0, 256, (b * 2 * fs,), dtype=torch.uint8, device=dev, generator=g) for _ in (0, 1))
             for _ in range(n_set)]
    nbytes = L.fiunet_plane_metrics_workspace_bytes(b, h, w)
    assert nbytes == L.fiunet_metrics_workspace_bytes(b, h, w) and nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out = torch.empty(b, dtype=torch.float64, device=dev)
    sse = torch.empty(b, dtype=torch.int64, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    wp, op, sp, sz = ws.data_ptr(), out.data_ptr(), sse.data_ptr(), ctypes.c_size_t(nbytes)
    ptr = [(p.data_ptr(), t.data_ptr()) for p, t in pairs]
    cases, moved = {}, {}

    def add(name, fn, nb):
        cases[name], moved[name] = H.Rotate(fn, n_set), nb

    def u8(tag):
        add(f"psnr u8_{tag}", lambda k: _native.check(L.fiunet_psnr_u8(ptr[k][0], ptr[k][1], b, h, w, op, wp, sz, s), "psnr_u8"),
            2 * b * n)
        add(f"ssim u8_{tag}", lambda k: _native.check(L.fiunet_ssim_u8(ptr[k][0], ptr[k][1], b, h, w, op, wp, sz, s), "ssim_u8"),
            2 * b * n)

    def plane(name, bits, stride):
        add(f"psnr {name}", lambda k: _native.check(L.fiunet_plane_psnr(ptr[k][0], stride, w, ptr[k][1], stride, w, bits, b,
                                                                        h, w, op, sp, wp, sz, s), "plane_psnr"),
            2 * b * n * (bits // 8 + (bits % 8 > 0)))
        add(f"ssim {name}", lambda k: _native.check(L.fiunet_plane_ssim(ptr[k][0], stride, w, ptr[k][1], stride, w, bits, b,
                                                                        h, w, op, wp, sz, s), "plane_ssim"),
            2 * b * n * (bits // 8 + (bits % 8 > 0)))
    u8("a")
    plane("plane8", 8, n)
    plane("plane8_i420y", 8, fs)
    plane("plane10", 10, n)
    plane("plane10_i420y", 10, fs)
    u8("b")
    return cases, moved, pairs, dict(batch=b, set_members=n_set, u8_set_mb=round(n_set * 2 * b * n / 2**20))


def _clip(path, frames, h, w):
    """A moving texture as C420jpeg Y4M: luma and chroma drift by 2 / 1 pixels a frame."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    cy, cx = np.mgrid[0:(h + 1) // 2, 0:(w + 1) // 2].astype(np.float32)
    with IO.Y4MWriter(path, w, h, (24, 1), "420jpeg") as wr:
        for t in range(frames):
            y = 128 + 90 * np.sin((xx - 2 * t) / 9.0) * np.cos(yy / 13.0) + 30 * np.cos((xx - 2 * t + yy) / 5.0)
            u = 128 + 60 * np.sin((cx - t) / 11.0 + cy / 17.0)
            v = 128 + 60 * np.cos((cx - t) / 7.0 - cy / 19.0)
            row = np.concatenate([np.clip(np.rint(p), 0, 255).astype(np.uint8).ravel() for p in (y, u, v)])
            wr.write(row[None])


def _score(dev, frames, h, w, say):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="bf16")
    m.load_state_dict(O.make_interpolating_state_dict(n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    spent = [0.0]
    make_route = stream._y4m_route

    def timed_route(*a, **k):
        route = make_route(*a, **k)
        run = route.run

        def timed(d, factor):
            got = []
            spent[0] += H.wall_s(lambda: got.append(run(d, factor)))
            return got[0]
        route.run = timed
        return route
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "clip.y4m")
        _clip(src, frames, h, w)
        holdout.score_video(m, src, chunk_frames=8)   # warm-up: code objects, the allocator's pools
        got = []
        wall = H.wall_s(lambda: got.append(holdout.score_video(m, src)))
        res = got[0]
        stream._y4m_route = timed_route
        try:
            wall2 = H.wall_s(lambda: holdout.score_video(m, src))
        finally:
            stream._y4m_route = make_route
    scored = len(res["scored_frames"])
    say(holdout.summary_table(res))
    return dict(frames=frames, scored_frames=scored, wall_s=round(wall, 3), scored_frames_per_s=round(scored / wall, 2),
                timed_run_wall_s=round(wall2, 3), forward_s=round(spent[0], 3), forward_share=round(spent[0] / wall2, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set of uint8 plane pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shape", default="1080x1920")
    ap.add_argument("--clip-frames", type=int, default=65)
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("holdout_timing")
    report = H.Report(a.out)
    say = report.say
    h, w = (int(v) for v in a.shape.split("x"))
    res = {"protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb)}
    cases, moved, pairs, info = _kernel_cases(dev, a.batch, h, w, int(a.set_gb * 1e9))
    ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
    leg = dict(info)
    for k in cases:
        med, lo, hi = H.summary(ms[k])
        leg[k] = dict(ms=round(med, 5), spread_ms=[round(lo, 5), round(hi, 5)],
                      gb_per_s=round(moved[k] / (med * 1e-3) / 1e9, 1))
        say(f"{a.batch}x{h}x{w} {k:20s} {med:8.5f} ms  (reps {lo:.5f}-{hi:.5f})  {leg[k]['gb_per_s']:7.1f} GB/s")
    for name in ("psnr", "ssim"):
        ta, tb = leg[f"{name} u8_a"]["ms"], leg[f"{name} u8_b"]["ms"]
        leg[f"{name} u8_spread"] = round(H.pair_spread(ta, tb), 4)
        for k in cases:
            if k.startswith(name) and "u8_" not in k:
                leg[f"{k} time_vs_u8"] = round(leg[k]["ms"] / max(ta, tb), 3)
        say(f"{name}: in-job spread of the u8 yardstick {leg[f'{name} u8_spread']:.4f}; plane8 / u8 time "
            f"{leg[f'{name} plane8 time_vs_u8']:.3f}")
    res["kernels"] = leg
    del cases, pairs
    torch.cuda.empty_cache()
    res["score_video"] = _score(dev, a.clip_frames, h, w, say)
    say(f"score_video: {res['score_video']}")
    report.finish(res)


if __name__ == "__main__":
    main()
