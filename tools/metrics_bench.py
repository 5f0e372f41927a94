"""Throughput of the device PSNR / SSIM kernels on uint8 frames (HBM roofline: 2 B/pixel read), at 8 x 1080p and at 64
planes of 256x256 (the reference's operating point, what an evaluation run feeds), Python call included.

    python tools/metrics_bench.py [--json] [--no-gauss] [--iters N]

--json: one JSON line {"lib": ..., "us": {"psnr_u8@8x1080x1920": ..., ...}} after the text, for A/B runs in fresh
processes with FIUNET_LIB set to one library or the other."""
import argparse, json, os, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
from ai_based_frame_interpolation_amd import _native, metrics
ap = argparse.ArgumentParser()
ap.add_argument("--json", action="store_true")
ap.add_argument("--no-gauss", action="store_true", help="skip the Gaussian-window SSIM of the training loss")
ap.add_argument("--iters", type=int, default=50, help="timed calls per figure (an A/B wants a window of tenths of a second)")
args = ap.parse_args()
dev = torch.device("cuda:0")
SIZES = ((8, 1080, 1920), (64, 256, 256))


def timed(fn, n=args.iters, warm=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(n): fn()
    torch.cuda.synchronize(); return (time.perf_counter() - t0) / n


us = {}
for b, h, w in SIZES:
    a = torch.randint(0, 256, (b, 1, h, w), dtype=torch.uint8, device=dev)
    c = torch.randint(0, 256, (b, 1, h, w), dtype=torch.uint8, device=dev)
    for name, fn in (("psnr_u8", metrics.psnr_u8), ("ssim_u8", metrics.ssim_u8)):
        dt = timed(lambda: fn(a, c))
        gb = 2 * a.numel() / 1e9
        us[f"{name}@{b}x{h}x{w}"] = dt * 1e6
        print(f"{name}: {dt*1e6:.1f} us per {b} x {h}x{w} frames = {b/dt:.0f} frames/s, {gb/dt:.0f} GB/s algorithmic "
              f"({gb/dt/8000*100:.1f} % of 8 TB/s)")
if not args.no_gauss:
    # Gaussian-window SSIM + MSE of the training loss (train.py:18-87) on fp32 tensors: 8 B/pixel read
    fa = torch.rand(8, 1, 1080, 1920, device=dev)
    fb = (fa + 0.1 * (torch.rand(8, 1, 1080, 1920, device=dev) - 0.5)).clamp(0, 1)
    loss = metrics.CombinedLoss()
    dt = timed(lambda: loss(fa, fb))
    gb = 8 * fa.numel() / 1e9
    us["combined_loss@8x1080x1920"] = dt * 1e6
    print(f"CombinedLoss (ssim_gauss_f32 + mse): {dt*1e6:.1f} us per 8 x 1080p fp32 frames = {8/dt:.0f} frames/s, "
          f"{gb/dt:.0f} GB/s algorithmic ({gb/dt/8000*100:.1f} % of 8 TB/s)")
if args.json:
    print(json.dumps({"lib": _native.LIB_PATH, "us": us}))
