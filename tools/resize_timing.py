"""Time the resize kernel beside a byte-moving yardstick, and `resize=` end to end, in one process.

  kernel    `resize.resize_frames` on B tight frames of I420 (the planes of 8-bit Y4M 4:2:0), nv12, rgb24 and yuv422p10le:
              1080p -> 256x256, 2160p -> 1080p, 1080p -> 1080p (the copy) and 540p -> 1080p.
            The yardstick is fiunet_hold_cut_frames with every interval flagged at factor 2: a plain device copy of B
            frames of the destination's size, so it WRITES the bytes the resize case writes (and reads as many).  It is
            timed twice per case (hold_a, hold_b): the difference between the two is the spread of this job.
            Frames come from memory, not from a cache: the calls rotate over a set of sources and destinations of at
            least `--set-gb` GB together.  Device time from HIP events around `--iters` back-to-back calls after
            `--warmup` calls; `--reps` repetitions interleaved over the cases; median and spread.  Reported: microseconds
            per call, GB/s read + written (a down-scale reads at most four source samples per destination sample; the
            figure counts every source byte once, whole source frames), GB/s written, and written GB/s over the
            yardstick's.
  stream    a 1080p 8-bit 4:2:0 Y4M clip through the grayscale network, streamed in chunks of 8 pairs into a null sink:
              device   interpolate_video(resize=(256, 256)) on the 1080p clip
              pre      the same call on the clip already at 256x256 (no resize: the same forwards)
              host     every frame resized with imageio_lite.resize_linear_u8 on the host, then `pre` on the result
            frames/s of source frames, median of `--stream-reps` interleaved runs after one warm-up run each.
One JSON line last; the text goes to `--out` as well (default profiles/resize_timing.txt).

    python tools/resize_timing.py [--batch 8 --set-gb 1 --iters 50 --reps 7]
"""
import argparse
import os
import tempfile

import numpy as np
import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
from ai_based_frame_interpolation_amd import _native, imageio_lite, resize

FORMATS = {"i420": (("y4m", "420jpeg"), 8), "nv12": ("nv12", 8), "rgb24": ("rgb24", 8), "yuv422p10le": ("yuv422p10le", 10)}
SCALES = [((1080, 1920), (256, 256)), ((2160, 3840), (1080, 1920)), ((1080, 1920), (1080, 1920)), ((540, 960), (1080, 1920))]


def _kernel_case(dev, name, b, src_hw, dst_hw, set_bytes):
    """-> ({case: callable}, bytes read, bytes written) for one format at one scale."""
    kind, bits = FORMATS[name]
    sp, dp = resize.frame_planes(kind, *src_hw), resize.frame_planes(kind, *dst_hw)
    rs, rd = resize.frame_samples(sp), resize.frame_samples(dp)
    item = 1 if bits == 8 else 2
    dtype = torch.uint8 if bits == 8 else torch.int16
    rbytes, wbytes = b * rs * item, b * rd * item
    n_set = max(2, -(-set_bytes // (rbytes + wbytes)))
    g = torch.Generator(device=dev).manual_seed(rs)
    top = 256 if bits == 8 else 1024
    src = [torch.randint(0, top, (b, rs), dtype=dtype, device=dev, generator=g) for _ in range(n_set)]
    dst = [torch.empty((b, rd), dtype=dtype, device=dev) for _ in range(n_set)]
    # the yardstick: B + 1 frames at factor 2, every interval flagged: frames 1, 3, ... become copies of 0, 2, ...
    n_hold = max(2, -(-set_bytes // (2 * wbytes)))
    vid = [torch.randint(0, 256, (2 * b + 1, rd * item), dtype=torch.uint8, device=dev, generator=g) for _ in range(n_hold)]
    flags = torch.ones(b, dtype=torch.uint8, device=dev)
    cases = {
        "hold_a": H.Rotate(lambda k: _native.hold_cut_frames(vid[k], b + 1, 2, flags), n_hold),
        "resize": H.Rotate(lambda k: resize.resize_frames(src[k], sp, dp, bits, out=dst[k]), n_set),
        "hold_b": H.Rotate(lambda k: _native.hold_cut_frames(vid[k], b + 1, 2, flags), n_hold),
    }
    return cases, rbytes, wbytes


def _kernels(dev, a, say):
    out = {}
    for src_hw, dst_hw in SCALES:
        for name in FORMATS:
            label = f"{name} {src_hw[0]}x{src_hw[1]}->{dst_hw[0]}x{dst_hw[1]}"
            cases, rbytes, wbytes = _kernel_case(dev, name, a.batch, src_hw, dst_hw, int(a.set_gb * 1e9))
            ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
            med = {k: H.summary(v)[0] for k, v in ms.items()}
            hold = [wbytes / (med[k] * 1e-3) / 1e9 for k in ("hold_a", "hold_b")]
            written = wbytes / (med["resize"] * 1e-3) / 1e9
            leg = dict(us=round(med["resize"] * 1e3, 1), spread_us=[round(min(ms["resize"]) * 1e3, 1), round(max(ms["resize"]) * 1e3, 1)],
                       gb_per_s=round((rbytes + wbytes) / (med["resize"] * 1e-3) / 1e9, 1), written_gb_per_s=round(written, 1),
                       hold_us=[round(med["hold_a"] * 1e3, 1), round(med["hold_b"] * 1e3, 1)],
                       hold_written_gb_per_s=[round(v, 1) for v in hold],
                       hold_spread=round(H.pair_spread(*hold), 4), vs_hold=round(written / min(hold), 3))
            out[label] = leg
            say(f"{label:38s} {leg['us']:9.1f} us (reps {leg['spread_us'][0]:.1f}-{leg['spread_us'][1]:.1f})  "
                f"{leg['gb_per_s']:7.1f} GB/s r+w  {leg['written_gb_per_s']:7.1f} GB/s written | hold "
                f"{leg['hold_us'][0]:.1f} / {leg['hold_us'][1]:.1f} us, {hold[0]:.1f} / {hold[1]:.1f} GB/s written "
                f"(spread {leg['hold_spread']:.3f}) | written vs hold x{leg['vs_hold']:.3f}")
            del cases
            torch.cuda.empty_cache()
    return out


def _stream(dev, a, say):
    n, (h, w), size = a.stream_frames, (1080, 1920), (256, 256)
    _, fi = H.seeded_model(1, "bf16", dev)
    kind = ("y4m", "420jpeg")
    sp, dp = resize.frame_planes(kind, h, w), resize.frame_planes(kind, size[1], size[0])
    rng = np.random.default_rng(1)
    base = rng.integers(0, 256, resize.frame_samples(sp), dtype=np.uint8)
    rows = np.stack([np.roll(base, 7 * i) for i in range(n)])

    def host_resize(rows):
        out = np.empty((rows.shape[0], resize.frame_samples(dp)), np.uint8)
        for i in range(rows.shape[0]):
            for (_, so, sh, sw, _, _), (_, do, dh, dw, _, _) in zip(sp, dp):
                out[i, do:do + dh * dw] = imageio_lite.resize_linear_u8(rows[i, so:so + sh * sw].reshape(sh, sw), (dw, dh)).ravel()
        return out
    with tempfile.TemporaryDirectory() as d:
        big, small, tmp = (os.path.join(d, f) for f in ("big.y4m", "small.y4m", "host.y4m"))
        with imageio_lite.Y4MWriter(big, w, h, (24, 1), "420jpeg", None, bits=8) as wr:
            wr.write(rows)
        with imageio_lite.Y4MWriter(small, size[0], size[1], (24, 1), "420jpeg", None, bits=8) as wr:
            wr.write(host_resize(rows))

        def run(path, **kw):
            fi.interpolate_video(path, H.NullSink(), 2, chunk_frames=8, **kw)

        def host():
            frames = imageio_lite.read_y4m_packed(big)[0]
            with imageio_lite.Y4MWriter(tmp, size[0], size[1], (24, 1), "420jpeg", None, bits=8) as wr:
                wr.write(host_resize(frames))
            run(tmp)
        runs = {"device": lambda: run(big, resize=size), "pre": lambda: run(small), "host": host}
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
    ap.add_argument("--stream-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(H.ROOT, "profiles", "resize_timing.txt"))
    a = ap.parse_args()
    dev = H.need_gpu("resize_timing")
    report = H.Report(a.out)
    say = report.say
    say(f"# tools/resize_timing.py: B = {a.batch}; "
        f"{H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb, wall_reps=a.stream_reps)}; "
        f"{torch.cuda.get_device_name(0)}")
    report.finish({"kernel": _kernels(dev, a, say), "stream": _stream(dev, a, say)})


if __name__ == "__main__":
    main()
