"""Time the 4:2:2 / 4:4:4 YUV conversions beside the I420 / C420p10 kernels, in one process.

  kernels   decode (YUV -> planar RGB) and encode (planar RGB -> YUV) of B frames, 1080p and 2160p, 8 and 10 bits:
              i420_a, i420_b   the 4:2:0 planar kernels (fiunet_yuv420_to_rgb_u8 ...), measured as two cases: the
                               difference between them is the run-to-run spread of this job
              yuv422p, yuv444p, uyvy422, yuyv422 (8 bits); yuv422p10le, yuv444p10le (10 bits)
                               the new kernels on tight frames (fiunet_yuv_to_rgb_u8 ...)
            The kernels are HBM-bound and a frame comes from memory, not from a cache: the calls rotate over a set of
            inputs and outputs of at least `--set-gb` GB together (several times the 256 MB Infinity Cache).  Device
            time from HIP events around `--iters` back-to-back calls after `--warmup` calls; `--reps` repetitions
            interleaved over the cases; median and spread.  Bytes moved: one frame of the format plus three planes of
            H x W samples per frame.  The yardstick is bytes per second: each new kernel against the slower of the two
            I420 measurements of the same leg.
  forward   forward_yuv beside forward_yuv420 at B = 8, 1080p, bf16, and beside forward_yuv420p10 in fp16 for the
            10-bit formats (the conversions are three of a forward's launches).
One JSON line last.

    python tools/yuv4xx_timing.py [--batch 8 --set-gb 1 --iters 200 --reps 7]
"""
import argparse

import torch

import timing_harness as H  # first: it puts the repository on sys.path for the imports below
import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native
from ai_based_frame_interpolation_amd.colour import YUV_FORMATS, resolve_yuv_layout, yuv_flags, yuv_frame_samples


def _rnd(dev, g, shape, bits):
    # (torch has no uint16 randint: 10-bit codes are drawn as int16, the same bits)
    t = torch.randint(0, 256 if bits == 8 else 1024, shape, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev,
                      generator=g)
    return t.view(torch.uint8 if bits == 8 else torch.uint16)


def _kernel_cases(dev, bits, b, h, w, set_bytes):
    """One set of `n_set` YUV batches wide enough for the largest format (4:4:4) and one set of RGB batches, shared by
    every format (a conversion's time does not depend on the values)."""
    sb = 1 if bits == 8 else 2
    names = [n for n, v in YUV_FORMATS.items() if v[1] == bits]
    widest = 3 * h * w
    n_set = max(2, -(-set_bytes // (b * (widest + 3 * h * w) * sb)))
    g = torch.Generator(device=dev).manual_seed(bits)
    yuv = [_rnd(dev, g, (b, widest), bits) for _ in range(n_set)]
    rgb = [_rnd(dev, g, (b, 3, h, w), bits) for _ in range(n_set)]
    fs420 = P.i420_frame_bytes(h, w)
    flags420 = P.colour.colour_flags("mpeg2", "bt709", "limited", bits=bits)

    def i420(decode):
        if decode:
            return H.Rotate(lambda k: _native.yuv420_to_rgb(yuv[k][:, :fs420], rgb[k], h, w, flags420, bits), n_set)
        return H.Rotate(lambda k: _native.rgb_to_yuv420(rgb[k], yuv[k][:, :fs420], flags420, bits), n_set)

    def new(decode, fmt):
        code = YUV_FORMATS[fmt][0]
        lay = resolve_yuv_layout(None, fmt, h, w)
        n, flags = lay.frame_stride, yuv_flags(fmt, "mpeg2", "bt709", "limited")
        if decode:
            return H.Rotate(lambda k: _native.yuv_to_rgb(yuv[k][:, :n], code, lay, rgb[k], h, w, flags, bits), n_set)
        return H.Rotate(lambda k: _native.rgb_to_yuv(rgb[k], yuv[k][:, :n], code, lay, flags, bits), n_set)
    cases, moved = {}, {}
    for name, decode in (("decode", True), ("encode", False)):
        cases[f"{name} i420_a"] = i420(decode)
        for fmt in names:
            cases[f"{name} {fmt}"] = new(decode, fmt)
            moved[f"{name} {fmt}"] = b * (yuv_frame_samples(fmt, h, w) + 3 * h * w) * sb
        cases[f"{name} i420_b"] = i420(decode)
        moved[f"{name} i420_a"] = moved[f"{name} i420_b"] = b * (fs420 + 3 * h * w) * sb
    return cases, moved, names, dict(batch=b, set_members=n_set, set_mb=round(n_set * b * (widest + 3 * h * w) * sb / 2**20))


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
    dev = H.need_gpu("yuv4xx_timing")
    report = H.Report(a.out)
    res = {"kernels": {}, "forward": {},
           "protocol": H.protocol(warmup=a.warmup, reps=a.reps, iters=a.iters, set_gb=a.set_gb)}
    for shape in a.shapes.split(","):
        h, w = (int(v) for v in shape.split("x"))
        for bits in (8, 10):
            cases, moved, names, info = _kernel_cases(dev, bits, a.batch, h, w, int(a.set_gb * 1e9))
            ms = H.interleaved(cases, warmup=a.warmup, reps=a.reps, iters=a.iters)
            leg = dict(info)
            for k in cases:
                med, lo, hi = H.summary(ms[k])
                leg[k] = dict(ms=round(med, 4), spread_ms=[round(lo, 4), round(hi, 4)],
                              gb_per_s=round(moved[k] / (med * 1e-3) / 1e9, 1))
                report.say(f"{h}x{w} {bits:2d} bit {k:20s} {med:8.4f} ms  (reps {lo:.4f}-{hi:.4f})  "
                           f"{leg[k]['gb_per_s']:7.1f} GB/s")
            for name in ("decode", "encode"):
                ia, ib = leg[f"{name} i420_a"]["gb_per_s"], leg[f"{name} i420_b"]["gb_per_s"]
                leg[f"{name} i420_spread"] = round(H.pair_spread(ia, ib), 4)
                for fmt in names:
                    leg[f"{name} {fmt}_vs_i420"] = round(leg[f"{name} {fmt}"]["gb_per_s"] / min(ia, ib), 3)
                report.say(f"{h}x{w} {bits:2d} bit {name}: i420 spread {leg[f'{name} i420_spread']:.4f}; bytes/s vs i420: "
                           + ", ".join(f"{fmt} {leg[f'{name} {fmt}_vs_i420']:.3f}" for fmt in names))
            res["kernels"][f"{h}x{w}_{bits}bit"] = leg
            del cases
            torch.cuda.empty_cache()

    b, h, w = 8, 1080, 1920
    for bits, prec in ((8, "bf16"), (10, "fp16")):
        m, _ = H.seeded_model(3, prec, dev, b)
        g = torch.Generator(device=dev).manual_seed(1)
        names = [n for n, v in YUV_FORMATS.items() if v[1] == bits]
        opts = dict(siting="mpeg2", matrix="bt709", colour_range="limited")
        f420 = [_rnd(dev, g, (b, P.i420_frame_bytes(h, w)), bits) for _ in range(2)]
        o420 = torch.empty_like(f420[0])
        fwd420 = m.forward_yuv420 if bits == 8 else m.forward_yuv420p10
        base = "forward_yuv420" if bits == 8 else "forward_yuv420p10"
        runs = {f"{base}_a": lambda: fwd420(f420[0], f420[1], h, w, out=o420, **opts)}
        for fmt in names:
            fr = [_rnd(dev, g, (b, yuv_frame_samples(fmt, h, w)), bits) for _ in range(2)]
            runs[f"forward_yuv {fmt}"] = (lambda fr=fr, fmt=fmt, out=torch.empty_like(fr[0]):
                                          m.forward_yuv(fr[0], fr[1], h, w, format=fmt, out=out, **opts))
        runs[f"{base}_b"] = lambda: fwd420(f420[0], f420[1], h, w, out=o420, **opts)
        ms = H.interleaved(runs, warmup=a.warmup, reps=a.reps, iters=5)
        for k in runs:
            med, lo, hi = H.summary(ms[k])
            res["forward"][k] = dict(precision=prec, ms=round(med, 3), spread_ms=[round(lo, 3), round(hi, 3)],
                                     frames_per_s=round(b / (med * 1e-3), 1))
            report.say(f"{b}x{h}x{w} {prec} {k:26s} {med:8.3f} ms  (reps {lo:.3f}-{hi:.3f})  "
                       f"{res['forward'][k]['frames_per_s']:7.1f} frames/s")
        del m, runs
        torch.cuda.empty_cache()
    report.finish(res)


if __name__ == "__main__":
    main()
