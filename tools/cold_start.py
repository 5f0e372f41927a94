#!/usr/bin/env python
"""Cold start and warm reload, weight_prep "host" against "device" (profiles/cold_start.txt).

Cold start: the reference's CLI flow (model/inference.py:204-251; api/app.py spawns it per request) in a FRESH process
per measurement - load_model -> one 256x256 pair -> postprocess - timed step by step:
  hip_init_ms            first device allocation (runtime + context start-up; the same for both paths)
  torch_load_ms          torch.load of the checkpoint + nn.Module.load_state_dict, on the host
  to_device_ms           model.to(device): ~110 host-to-device copies
  weight_prep_ms         the checkpoint -> kernel buffers step (fiunet_load_weights / fiunet_load_weights_device)
  prepare_precision_ms   the extra weight copies of a precision (bf16x2 / fp16 only; 0 otherwise)
  first_forward_ms       the first forward (workspace allocation, code-object load, LDS attributes)
  second_forward_ms      the same forward again
  postprocess_ms         postprocess_image (device kernel + copy to the host)
Every step ends with a device synchronisation.  Host and device children alternate in one job, so drift hits both.

Warm reload: one child per network holds a live model and alternates `refresh_weights()` + the next `_context()` with
weight_prep "host" and "device"; wall time to a synchronised device, and for the device path also the time between two
events on the stream (what the GPU spends in the kernels).

The parent makes no GPU call; children run one at a time, each under its own timeout, and the first one that fails ends
the job.  Usage: python tools/cold_start.py [--repeats 3] [--out profiles/cold_start.txt]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZE = 256
STEPS = ("hip_init_ms", "torch_load_ms", "to_device_ms", "weight_prep_ms", "prepare_precision_ms", "first_forward_ms",
         "second_forward_ms", "postprocess_ms", "total_ms")


def child_cold(path, fc, precision, prep):
    import torch
    from torch import nn

    from ai_based_frame_interpolation_amd import inference
    dev = torch.device("cuda:0")
    res = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        if torch.cuda.is_initialized():
            torch.cuda.synchronize()
        res[name] = res.get(name, 0.0) + (time.perf_counter() - t0) * 1e3
        return out

    t_all = time.perf_counter()
    timed("hip_init_ms", lambda: torch.zeros(1, device=dev))
    # load_model as it is, with its two phases timed from inside
    real_load, real_to = torch.load, nn.Module.to
    marks = {}

    def load_and_mark(*a, **k):
        marks["load0"] = time.perf_counter()
        return real_load(*a, **k)

    def to_and_mark(self, *a, **k):
        marks["to0"] = time.perf_counter()
        out = real_to(self, *a, **k)
        torch.cuda.synchronize()
        marks["to1"] = time.perf_counter()
        return out

    torch.load, nn.Module.to = load_and_mark, to_and_mark
    try:
        model = inference.load_model(path, dev, precision, frame_channels=fc, weight_prep=prep)
    finally:
        torch.load, nn.Module.to = real_load, real_to
    if not all(k in marks for k in ("load0", "to0", "to1")) or not marks["load0"] <= marks["to0"]:
        raise SystemExit("load_model no longer calls torch.load and then Module.to: torch_load_ms / to_device_ms need new marks")
    res["torch_load_ms"] = (marks["to0"] - marks["load0"]) * 1e3
    res["to_device_ms"] = (marks["to1"] - marks["to0"]) * 1e3
    g = torch.Generator().manual_seed(1)
    f1 = (torch.rand(1, fc, SIZE, SIZE, generator=g) * 2 - 1).to(dev)
    f2 = (torch.rand(1, fc, SIZE, SIZE, generator=g) * 2 - 1).to(dev)
    ctx = timed("weight_prep_ms", lambda: model._context(dev))
    timed("prepare_precision_ms", lambda: ctx.prepare(model._precision_code()))
    out = timed("first_forward_ms", lambda: model(f1, f2))
    out = timed("second_forward_ms", lambda: model(f1, f2))
    img = timed("postprocess_ms", lambda: inference.postprocess_image(out))
    res["total_ms"] = (time.perf_counter() - t_all) * 1e3
    res["checksum"] = int(img.astype("int64").sum())   # host and device children must agree
    return res


def child_reload(path, fc, repeats):
    import torch

    from ai_based_frame_interpolation_amd import inference
    dev = torch.device("cuda:0")
    model = inference.load_model(path, dev, "bf16", frame_channels=fc)
    f = torch.zeros(1, fc, SIZE, SIZE, device=dev)
    model(f, f)
    rows = {"host": [], "device": [], "device_event": []}
    for i in range(2 * (repeats + 1)):
        prep = ("host", "device")[i % 2]
        model.weight_prep = prep
        model.refresh_weights()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        model._context(dev)
        e1.record()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if i >= 2:   # the first of each: its buffers' first use by this path
            rows[prep].append(ms)
            if prep == "device":
                rows["device_event"].append(e0.elapsed_time(e1))
    return rows


def spawn(args, timeout):
    """One child at a time; a child that fails, faults or runs out of time ends the job."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", json.dumps(args)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        raise SystemExit(f"child {args} ended with status {p.returncode}: nothing more is started")
    return json.loads(p.stdout.strip().splitlines()[-1])


def med_spread(v):
    return f"{statistics.median(v):9.2f} [{min(v):8.2f} .. {max(v):8.2f}]"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=3, help="children per (network, precision, weight_prep)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cold_start.txt"))
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds per child")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        c = json.loads(a.child)
        res = child_cold(*c["cold"]) if "cold" in c else child_reload(*c["reload"])
        print(json.dumps(res))
        return 0

    import torch   # (host only: checkpoints for the children)

    from ai_based_frame_interpolation_amd.unet import FrameInterpolationUNet
    lines = [f"cold start and warm reload, weight_prep host vs device; one {SIZE}x{SIZE} pair; ms, median [min .. max] of "
             f"{a.repeats} fresh processes, host and device alternating", ""]
    with tempfile.TemporaryDirectory() as tmp:
        ckpt = {}
        for fc, name in ((1, "gray"), (3, "rgb")):
            torch.manual_seed(fc)
            m = FrameInterpolationUNet(bilinear=True, frame_channels=fc)
            ckpt[name] = os.path.join(tmp, f"{name}.pth")
            torch.save({"model_state_dict": m.state_dict(), "epoch": 0}, ckpt[name])
        for name, fc in (("gray", 1), ("rgb", 3)):
            for precision in ("fp32", "bf16"):
                runs = {"host": [], "device": []}
                for _ in range(a.repeats):
                    for prep in ("host", "device"):
                        runs[prep].append(spawn({"cold": [ckpt[name], fc, precision, prep]}, a.timeout))
                sums = {r["checksum"] for v in runs.values() for r in v}
                assert len(sums) == 1, f"host and device children disagree: {sums}"
                lines.append(f"{name} {precision}: cold start")
                lines.append(f"  {'step':22s} {'host':>33s}   {'device':>33s}")
                for step in STEPS:
                    lines.append(f"  {step:22s} {med_spread([r[step] for r in runs['host']])}   "
                                 f"{med_spread([r[step] for r in runs['device']])}")
                h = statistics.median(r["weight_prep_ms"] for r in runs["host"])
                d = statistics.median(r["weight_prep_ms"] for r in runs["device"])
                th = statistics.median(r["total_ms"] for r in runs["host"])
                td = statistics.median(r["total_ms"] for r in runs["device"])
                lines.append(f"  weight_prep host / device = {h / d:.1f}x; total host / device = {th / td:.3f}x "
                             f"({th - td:+.1f} ms of {th:.0f})")
                lines.append("")
                print("\n".join(lines[-len(STEPS) - 4:]), flush=True)
            rows = spawn({"reload": [ckpt[name], fc, a.repeats]}, a.timeout)
            lines.append(f"{name}: warm reload into a live model (bf16 rounding: error feedback), {a.repeats} each")
            lines.append(f"  host, wall to a synchronised device      {med_spread(rows['host'])}")
            lines.append(f"  device, wall to a synchronised device    {med_spread(rows['device'])}")
            lines.append(f"  device, between events on the stream     {med_spread(rows['device_event'])}")
            lines.append(f"  host / device (wall) = {statistics.median(rows['host']) / statistics.median(rows['device']):.1f}x")
            lines.append("")
            print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
