#!/usr/bin/env python3
"""Record the bits `metrics.psnr_u8` / `ssim_u8` return on seeded uint8 inputs (GPU).

    FIUNET_LIB=path/to/libfiunet_hip.so python tools/record_metrics_bits.py --commit <hash> [--out FILE]
    python tools/record_metrics_bits.py --verify tests/golden/metrics_u8_bits.npz [--out FILE]

The first form is run with a library built from an EARLIER commit (FIUNET_LIB, the A/B hook of _native.py) and writes
tests/golden/metrics_u8_bits.npz: for every case of tests/metrics_bits_cases.py the shape, the seed, the kind, pred's byte
offset, a SHA-256 of the generated inputs (a drifting generator then shows as a fixture error, not as a metric failure)
and the float64 results as int64 bit patterns (+inf included; an empty array where SSIM refuses the shape), plus the
library's path as given and the commit it was built from.  tests/test_gpu_metrics_bits.py holds today's library to it.

The second form records with whatever library is loaded, carries the path and commit over from FILE, and fails unless
the bytes it writes equal FILE's: the archive is written with fixed time stamps, so equal values are equal bytes.
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLDEN = os.path.join(ROOT, "tests", "golden", "metrics_u8_bits.npz")


def record(library: str, commit: str) -> dict:
    import torch
    import metrics_bits_cases as C
    from ai_based_frame_interpolation_amd import metrics
    dev = torch.device("cuda:0")
    out = {"library": np.array(library), "commit": np.array(commit), "cases": np.array(len(C.CASES), np.int64)}
    for k, (shape, seed, kind, offset) in enumerate(C.CASES):
        pred, target = C.make_inputs(shape, seed, kind)
        p, t = C.to_device(pred, target, offset, dev)
        psnr = C.bits(metrics.psnr_u8(p, t))
        ssim = C.bits(metrics.ssim_u8(p, t)) if C.has_ssim(shape) else np.zeros(0, np.int64)
        out.update({f"c{k}_shape": np.array(shape, np.int64), f"c{k}_seed": np.array(seed, np.int64),
                    f"c{k}_kind": np.array(kind), f"c{k}_offset": np.array(offset, np.int64),
                    f"c{k}_sha256": np.array(C.checksum(pred, target)), f"c{k}_psnr": psnr, f"c{k}_ssim": ssim})
        print(f"case {k} {shape} {kind} +{offset}: psnr {psnr.view(np.float64)!r} ssim {ssim.view(np.float64)!r}")
    return out


def archive(arrays: dict) -> bytes:
    """An .npz (`np.load` reads it) whose bytes depend on the arrays alone: stored, time stamp 1980-01-01."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            member = io.BytesIO()
            np.lib.format.write_array(member, np.asanyarray(a), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), member.getvalue())
    return buf.getvalue()


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--commit", help="the commit the library in FIUNET_LIB was built from")
    ap.add_argument("--verify", metavar="FILE", help="record with the loaded library and compare the bytes with FILE's")
    ap.add_argument("--out", help=f"where to write (default: {os.path.relpath(GOLDEN, ROOT)}; with --verify: nowhere)")
    args = ap.parse_args()
    if args.verify:
        with np.load(args.verify) as z:
            library, commit = str(z["library"]), str(z["commit"])
    else:
        library, commit = os.environ.get("FIUNET_LIB"), args.commit
        if not library or not commit:
            ap.error("set FIUNET_LIB to the earlier commit's library and give --commit (or use --verify)")
    data = archive(record(library, commit))
    out = args.out or (None if args.verify else GOLDEN)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "wb") as f:
            f.write(data)
        print(f"wrote {out}: {len(data)} bytes")
    if args.verify:
        with open(args.verify, "rb") as f:
            same = f.read() == data
        print(f"{args.verify}: {'byte-identical' if same else 'DIFFERENT'} to what the loaded library gives")
        return 0 if same else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
