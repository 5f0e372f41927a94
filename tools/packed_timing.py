"""Time the packed RGB conversions beside the I420 kernels, in one process.

  kernels   unpack (packed -> planar RGB) and pack (planar RGB -> packed) of B frames at 1080p and 2160p:
              i420_a, i420_b     the I420 decode / encode kernels (fiunet_yuv420_to_rgb_u8 ...), the yardstick, measured
                                 as two cases: the difference between them is the run-to-run spread of this job
              rgb24 ... bgra     fiunet_packed_to_rgb_u8 / fiunet_rgb_to_packed_u8 on tight frames (alpha 255)
              ..._pitched        the same with rows W*bpp + 64 bytes apart
              bgra_2alpha        the pack with two packed alpha sources (what forward_rgb_packed launches)
            These kernels do no arithmetic and their frames come from memory, not from a cache: the calls rotate over
            a set of inputs and outputs of at least `--set-gb` GB together for the smallest case (several times the
            256 MB Infinity Cache).  Device time from HIP events around `--iters` back-to-back calls after `--warmup`
            calls; `--reps` repetitions interleaved over the cases; median and spread.  Bytes moved: the packed
            pixels plus three planes of H x W per frame (the I420 cases: one frame of 1.5 H x W plus the planes).
  forward   forward_rgb_packed (rgb24, bgra) beside forward_u8 on already-planar input at B = 8, 1080p, bf16.
One JSON line last.

    python tools/packed_timing.py [--batch 8 --set-gb 1 --iters 200 --reps 7]
"""
import argparse

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native, packed


def _kernel_cases(dev, b, h, w, set_bytes):
    """One set of `n_set` byte buffers wide enough for the widest packed layout, shared by every format and by the I420
    cases (a move's time does not depend on the values), a second one for the alpha sources, and one set of planar RGB
    batches.  -> (cases, bytes moved per case, info)"""
    widest = h * (4 * w + 64)
    n_set = max(2, -(-set_bytes // (b * 6 * h * w)))
    g = torch.Generator(device=dev).manual_seed(h)

    def rnd(shape):
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=dev, generator=g)
    pk = [rnd((b, widest)) for _ in range(n_set)]
    pk2 = [rnd((b, 4 * h * w)) for _ in range(n_set)]
    rgb = [rnd((b, 3, h, w)) for _ in range(n_set)]
    fs = P.i420_frame_bytes(h, w)
    flags = P.colour.colour_flags("mpeg2", "bt709", "limited")
    cases, moved = {}, {}

    def add(name, fn, nbytes):
        cases[name], moved[name] = H.Rotate(fn, n_set), b * nbytes

    def i420(tag):
        add(f"unpack i420_{tag}", lambda k: _native.yuv420_to_rgb(pk[k][:, :fs], rgb[k], h, w, flags, 8), fs + 3 * h * w)
        add(f"pack i420_{tag}", lambda k: _native.rgb_to_yuv420(rgb[k], pk[k][:, :fs], flags, 8), fs + 3 * h * w)
    i420("a")
    for fmt, (code, bpp) in packed.FORMATS.items():
        for tag, lay in (("", packed.resolve_layout(None, fmt, h, w)),
                         ("_pitched", packed.resolve_layout(packed.PackedLayout(w * bpp + 64), fmt, h, w))):
            n = lay.frame_stride
            add(f"unpack {fmt}{tag}",
                lambda k, n=n, lay=lay, code=code: _native.packed_to_rgb(pk[k][:, :n], lay, rgb[k], None, h, w, code),
                (bpp + 3) * h * w)
            add(f"pack {fmt}{tag}",
                lambda k, n=n, lay=lay, code=code: _native.rgb_to_packed(rgb[k], pk[k][:, :n], lay, (), lay, code),
                (bpp + 3) * h * w)
    lay = packed.resolve_layout(None, "bgra", h, w)
    add("pack bgra_2alpha",
        lambda k: _native.rgb_to_packed(rgb[k], pk[k][:, :4 * h * w], lay, (pk2[k], pk2[k - 1]), lay, 3), (4 + 3 + 8) * h * w)
    i420("b")
    return cases, moved, dict(batch=b, set_members=n_set, smallest_case_set_mb=round(n_set * b * 6 * h * w / 2**20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--set-gb", type=float, default=1.0, help="least size of the rotating set of inputs and outputs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--shapes", default="1080x1920,2160x3840")
    ap.add_argument("--out", default=None, help="also write the printed lines to this file")
    a = ap.parse_args()
    dev = H.need_gpu("packed_timing")
    report = H.Report(a.out)
    res = {"kernels": {}, "forward": {},
           "protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb)}
    for shape in a.shapes.split(","):
        h, w = (int(v) for v in shape.split("x"))
        cases, moved, info = _kernel_cases(dev, a.batch, h, w, int(a.set_gb * 1e9))
        ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
        leg = dict(info)
        for k in cases:
            med, lo, hi = H.summary(ms[k])
            leg[k] = dict(ms=round(med, 4), spread_ms=[round(lo, 4), round(hi, 4)],
                          gb_per_s=round(moved[k] / (med * 1e-3) / 1e9, 1))
            report.say(f"{h}x{w} {k:22s} {med:8.4f} ms  (reps {lo:.4f}-{hi:.4f})  {leg[k]['gb_per_s']:7.1f} GB/s")
        for name in ("unpack", "pack"):
            ia, ib = leg[f"{name} i420_a"]["gb_per_s"], leg[f"{name} i420_b"]["gb_per_s"]
            leg[f"{name} i420_spread"] = round(H.pair_spread(ia, ib), 4)
        # the yardstick of every case: the I420 encode's bytes per second
        enc = min(leg["pack i420_a"]["gb_per_s"], leg["pack i420_b"]["gb_per_s"])
        for k in cases:
            if "i420" not in k:
                leg[f"{k} vs_i420_encode"] = round(leg[k]["gb_per_s"] / enc, 3)
        res["kernels"][f"{h}x{w}"] = leg
        del cases
        torch.cuda.empty_cache()

    b, h, w = 8, 1080, 1920
    m, _ = H.seeded_model(3, "bf16", dev, b)
    g = torch.Generator(device=dev).manual_seed(1)
    p1, p2 = (torch.randint(0, 256, (b, 3, h, w), dtype=torch.uint8, device=dev, generator=g) for _ in range(2))
    pout = torch.empty_like(p1)
    runs = {"forward_u8_a": lambda: m.forward_u8(p1, p2, out=pout)}
    keep = []
    for fmt in ("rgb24", "bgra"):
        f1, f2 = (torch.randint(0, 256, (b, packed.frame_bytes(fmt, h, w)), dtype=torch.uint8, device=dev, generator=g)
                  for _ in range(2))
        out = torch.empty_like(f1)
        keep.append((f1, f2, out))
        runs[f"forward_rgb_packed {fmt}"] = (lambda f1=f1, f2=f2, out=out, fmt=fmt:
                                             m.forward_rgb_packed(f1, f2, h, w, format=fmt, out=out))
    runs["forward_u8_b"] = lambda: m.forward_u8(p1, p2, out=pout)
    ms = H.interleaved(runs, warmup=a.warmup, reps=a.reps, iters=5)
    for k in runs:
        med, lo, hi = H.summary(ms[k])
        res["forward"][k] = dict(ms=round(med, 3), spread_ms=[round(lo, 3), round(hi, 3)],
                                 frames_per_s=round(b / (med * 1e-3), 1))
        report.say(f"{b}x{h}x{w} bf16 {k:26s} {med:8.3f} ms  (reps {lo:.3f}-{hi:.3f})  "
                   f"{res['forward'][k]['frames_per_s']:7.1f} frames/s")
    report.finish(res)


if __name__ == "__main__":
    main()
