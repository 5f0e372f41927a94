#!/usr/bin/env python3
"""bench.py -- interpolated frames/s of the MI355X UNet frame-pair forward.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W
Both forms work for N > 1: started WITHOUT a launcher (no WORLD_SIZE in the environment), `--gpus N` makes this
process a launcher itself - it starts N child ranks (one per GPU, RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set,
rendezvous on 127.0.0.1), relays rank 0's JSON line and exits with the worst child status (`launch_ranks`).

A step = one forward of the hot path over one batch of synthetic frame pairs that is already
resident in HBM.  Default workload = BASELINE.json configs[2]: batch 8 of 1920x1080 pairs, bf16
MFMA path, one batch per GPU (weak scaling: frame pairs are independent, ranks exchange
nothing inside the timed region).  Rank 0 prints ONE JSON line; `value` is always this leg, and
`ms_per_step` is the wall time of one of the `--steps` timed steps.  Weights and frames are seeded,
so the same arguments give the same inputs on every run; `--dump-outputs DIR` writes rank 0's
output of the last timed step there (`dump_outputs`), so that two builds can be compared output
for output.

A plain run does only what that line's headline needs: it sets up, warms up, times the steps, dumps if asked and
prints the line, which carries beside the headline fields (and `dumped_outputs`)
  roofline      -- dominant kernel (by time) of the forward: algorithmic FLOPs per launch / its
                   average launch duration, measured live with HIP events recorded on the launch
                   stream between the stages (fiunet_profile_*) of the timed steps themselves, vs the
                   dense MFMA peak.
`--full` adds every other leg below, each measured after the timed steps, never inside them;
`--no-cpu-baseline`, `--no-fp32`, `--no-tile4k`, `--no-power` and `--video-frames` choose among those legs.

Objects that `--full` adds to that line:
  cpu_baseline  -- the PyTorch-CPU oracle (a port of the reference's forward, pinned to reference
                   outputs) timed on this box's host cores: 1080p (1 warm-up + median of 3) and
                   BASELINE configs[0] (one 256x256 pair, 3 warm-up + 10 timed, median), thread
                   count chosen by a short sweep; N=1, rank 0 only.
  parity        -- PSNR of the HIP path and of the CPU oracle against a TRUE middle frame on a
                   checkpoint that interpolates (north_star: within 0.05 dB), and the raw bf16 error
                   of the bench's own random network.
  fp32          -- the reference's own precision (N = 1): BASELINE configs[1] (batch 16 of 256x256 pairs,
                   10 warm-up + 50 timed) and batch 4 of 1080p pairs, HIP-event timed, each with the
                   roofline of its dominant kernel against the fp32 MFMA peak (157.3 TFLOP/s).
  video_sharded -- BASELINE configs[3]: a synthetic 1080p uint8 video held by rank 0, factor 2,
                   end to end through video.interpolate_video_sharded (RCCL send/recv scatter of
                   frame sub-batches, forward_u8, gather), beside the replicas-only `value`.
  tile4k        -- BASELINE configs[4]: N >= 2: one 2160x3840 uint8 pair cut into N row bands + halo through
                   tiling.forward_tiled_distributed (uint8 on the wire); N = 1: the un-tiled pair, the four
                   config-5 bands each and back to back, tiled == un-tiled.
                   video_sharded also carries the HOST-resident (PCIe-inclusive) rate at N = 1.
  rgb_6to3, fp32_contract_on_bf16_pipe, latency_256, power -- N = 1: see rgb_leg, bf16x2_leg,
                   small_frames_leg and power_leg.
The oracle is only the baseline/checker here; the measured path never touches it.
"""
from __future__ import annotations

import argparse
import datetime
import json
import os
import statistics
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import synthetic as S  # noqa: E402

PEAK_TFLOPS = {"bf16": 2500.0, "fp32": 157.3}   # MI355X dense MFMA peaks (MI355X_MICROARCH.md)
PEAK_HBM_GBS = 8000.0
# fused-ideal HBM elements per frame at HxW: 2146.1 M @1080p, scales with pixels
ELEMS_PER_PIXEL = 2146.1e6 / (1080 * 1920)


def conv_flops(h, w):
    """2*MAC over the 18 3x3 convs + the 1x1 head, gray 2->1 network."""
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append(hs[-1] // 2); ws.append(ws[-1] // 2)
    chans = [(2, 64, 64), (64, 128, 128), (128, 256, 256), (256, 512, 512), (512, 512, 512),
             (1024, 512, 256), (512, 256, 128), (256, 128, 64), (128, 64, 64)]
    lv = [0, 1, 2, 3, 4, 3, 2, 1, 0]
    tot = 0.0
    for (ci, cm, co), l in zip(chans, lv):
        tot += 2.0 * hs[l] * ws[l] * 9 * (ci * cm + cm * co)
    return tot + 2.0 * h * w * 64


def make_bench_model(precision: str, seed: int = 0, frame_channels: int = 1,
                     bilinear: bool = True) -> "P.FrameInterpolationUNet":
    """Random-init network of the benchmark: He-scaled conv weights and non-trivial BatchNorm
    statistics so activations stay O(1) through all 19 layers (torch's default init + identity BN
    decays towards zero, and near-zero MFMA operands run at a higher clock than real data: never
    bench on those).  Same weights on every rank."""
    torch.manual_seed(seed)
    model = P.FrameInterpolationUNet(bilinear=bilinear, precision=precision, frame_channels=frame_channels)
    with torch.no_grad():
        for name, prm in model.named_parameters():
            if name.endswith(".up.weight"):     # ConvTranspose2d [in, out, 2, 2] (bilinear=False only)
                prm.normal_(0, (1.0 / prm.shape[0]) ** 0.5)
            elif name.endswith(".up.bias"):
                prm.normal_(0, 0.1)
            elif prm.dim() == 4 and prm.shape[-1] == 3:
                prm.normal_(0, (2.0 / (prm.shape[1] * 9)) ** 0.5)
            elif prm.dim() == 4:
                prm.normal_(0, 0.2 / prm.shape[1] ** 0.5)
            elif name.endswith(".weight"):
                prm.uniform_(0.6, 1.6)
            elif name.endswith(".bias"):
                prm.normal_(0, 0.25 if "double_conv" in name else 0.1)
        for name, buf in model.named_buffers():
            if name.endswith("running_mean"):
                buf.normal_(0, 0.2)
            elif name.endswith("running_var"):
                buf.uniform_(0.5, 1.5)
    return model


class _quiet_native_stdout:
    """RCCL prints a version banner on fd 1 when its communicator is created; bench.py must print
    exactly one JSON line, so native stdout is parked on stderr around that point."""

    def __enter__(self):
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self._saved, 1)
        os.close(self._saved)


def _run_bounded(fn, seconds: float):
    """Run `fn()` on a worker thread and give up after `seconds`: a leg that exercises RCCL
    send/recv for the first time on a new node must not be able to take the headline number down
    with it.  Returns (result, error string or None)."""
    box = {}

    def body():
        try:
            box["r"] = fn()
        except Exception as e:  # noqa: BLE001 -- reported in the JSON, not swallowed
            box["e"] = f"{type(e).__name__}: {e}"

    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(seconds)
    if t.is_alive():
        return None, f"timeout after {seconds:.0f} s"
    return box.get("r"), box.get("e")


# ---------------------------------------------------------------------------------------------
# CPU legs (rank 0, N = 1): the oracle is the timed baseline and the checker, nothing else
# ---------------------------------------------------------------------------------------------
def _cpu_info():
    model = "?"
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else round(int(q) / int(per), 1)
    except (OSError, ValueError):
        pass
    return model, len(os.sched_getaffinity(0)), quota


def _psnr_sweep(O, m, sd_i, dev, precision):
    """|PSNR_hip - PSNR_cpu| against a true middle frame over scenes x sizes x checkpoint seeds."""
    rows, worst = [], 0.0
    for (sh, sw), scenes, ckpts in (((256, 256), (3, 4, 5, 6, 7), (4321, 5321)), ((540, 960), (3, 5, 7), (4321,))):
        for ck in ckpts:
            sd_k = sd_i if ck == 4321 else O.make_interpolating_state_dict(seed=ck)
            mk = m
            if ck != 4321:
                mk = P.FrameInterpolationUNet(bilinear=True)
                mk.load_state_dict(sd_k)
                mk = mk.to(dev).eval()
            mk.precision = precision
            for sc in scenes:
                a8, t8, c8 = S.triplet(sh, sw, device="cpu", seed=sc)
                r8 = O.postprocess_tensor(O.unet_forward(sd_k, O.preprocess_array(a8.numpy()),
                                                         O.preprocess_array(c8.numpy())))
                h8 = mk.forward_u8(a8[None, None].to(dev), c8[None, None].to(dev))[0, 0].cpu().numpy()
                d = O.psnr_u8(t8.numpy(), h8) - O.psnr_u8(t8.numpy(), r8)
                rows.append({"size": f"{sw}x{sh}", "scene": sc, "ckpt": ck, "delta_db": round(d, 4)})
                worst = max(worst, abs(d))
    return rows, worst


def cpu_legs(dev, precision):
    from oracle import unet_oracle as O  # checker / baseline only

    cpu_model, n_aff, quota = _cpu_info()
    # ---- thread count: short sweep on the 256x256 case -----------------------------------
    sd_i = O.make_interpolating_state_dict()
    g1, g2 = O.make_frames(0, 1, 256, 256)  # seed 0
    cands = sorted({t for t in (4, 8, 16, 32, 64, 128) if t <= max(n_aff, 4)})
    sweep = {}
    for t in cands:
        torch.set_num_threads(t)
        O.unet_forward(sd_i, g1, g2)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter(); O.unet_forward(sd_i, g1, g2); ts.append(time.perf_counter() - t0)
        sweep[t] = min(ts)
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    # ---- BASELINE configs[0]: one 256x256 pair, 3 warm-up + 10 timed, median -------------
    for _ in range(3):
        O.unet_forward(sd_i, g1, g2)
    ts = []
    for _ in range(10):
        t0 = time.perf_counter(); O.unet_forward(sd_i, g1, g2); ts.append(time.perf_counter() - t0)
    cfg1_ms = statistics.median(ts) * 1e3
    # the HIP path on the same pair (latency, one pair per call, fp32 and bf16)
    m = P.FrameInterpolationUNet(bilinear=True)
    m.load_state_dict(sd_i)
    m = m.to(dev).eval()
    hip_cfg1 = {}
    for prec in ("fp32", "bf16"):
        m.precision = prec
        d1, d2 = g1.to(dev), g2.to(dev)
        for _ in range(20):
            m(d1, d2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            m(d1, d2)
        torch.cuda.synchronize()
        hip_cfg1[prec] = round((time.perf_counter() - t0) / 200 * 1e3, 3)
        # the same pair through one captured HIP graph (the ~25 launches of a forward replayed as one)
        try:
            gf = P.GraphedForward(m, 1, 256, 256)
            for _ in range(20):
                gf(d1, d2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(200):
                gf(d1, d2)
            torch.cuda.synchronize()
            hip_cfg1[prec + "_graph"] = round((time.perf_counter() - t0) / 200 * 1e3, 3)
            del gf
        except Exception as e:  # noqa: BLE001 -- an extra figure, never the reason to lose the line
            hip_cfg1[prec + "_graph"] = f"{type(e).__name__}: {e}"
    # ---- 1080p: 1 warm-up + 3 timed, median; inputs/outputs stay on the host -------------
    h, w = 1080, 1920
    a_u8, truth_u8, c_u8 = S.triplet(h, w, device="cpu", seed=3)
    fa, fc = O.preprocess_array(a_u8.numpy()), O.preprocess_array(c_u8.numpy())
    ref = O.unet_forward(sd_i, fa, fc)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter(); ref = O.unet_forward(sd_i, fa, fc); ts.append(time.perf_counter() - t0)
    cpu_s = statistics.median(ts)
    cpu_baseline = {
        "value": round(1.0 / cpu_s, 4), "unit": "frames/s", "cores": best, "kind": "port",
        "sample": f"one 1920x1080 frame pair, 1 warm-up + median of 3 runs ({', '.join(f'{t:.2f}' for t in ts)} s), "
                  f"PyTorch-CPU oracle (oracle/unet_oracle.py), fp32, torch {torch.__version__}, "
                  f"{best} threads chosen by a sweep over {cands} on the 256x256 case; CPU: {cpu_model}, "
                  f"{n_aff} logical CPUs visible" + (f", cgroup quota {quota} CPUs" if quota else ""),
        "config1_256x256": {"cpu_ms_median": round(cfg1_ms, 2), "cpu_frames_per_s": round(1e3 / cfg1_ms, 2),
                            "protocol": "1 pair, 3 warm-up + 10 timed, median (SURVEY 8d config 1)",
                            "hip_protocol": "the same pair resident in HBM, 20 warm-up + 200 forwards back to back, wall clock "
                                            "around one synchronize (latency_256 times the same loop with HIP events)",
                            "hip_ms_fp32": hip_cfg1["fp32"], "hip_ms_bf16": hip_cfg1["bf16"],
                            "hip_ms_fp32_hip_graph": hip_cfg1.get("fp32_graph"),
                            "hip_ms_bf16_hip_graph": hip_cfg1.get("bf16_graph")},
        "thread_sweep_256x256_ms": {str(k): round(v * 1e3, 1) for k, v in sweep.items()},
    }
    # ---- PSNR vs a true middle frame, interpolating checkpoint, 1080p --------------------
    ref_u8 = O.postprocess_tensor(ref)
    par = {"checkpoint": "oracle.make_interpolating_state_dict(): 0.5*(f1+f2) carried through the x1 skip "
                         "+ seeded random deep network (~0.04 rms)",
           "psnr_cpu_vs_truth_db": round(O.psnr_u8(truth_u8.numpy(), ref_u8), 4)}
    for prec in ("fp32", "bf16x2", "bf16"):   # (bf16x2: the fast path that meets the fp32 tolerance; stem fused at this size)
        m.precision = prec
        hip_u8 = m.forward_u8(a_u8[None, None].to(dev), c_u8[None, None].to(dev))[0, 0].cpu().numpy()
        par[f"psnr_hip_{prec}_vs_truth_db"] = round(O.psnr_u8(truth_u8.numpy(), hip_u8), 4)
        par[f"psnr_hip_{prec}_vs_cpu_ref_u8_db"] = round(O.psnr_u8(ref_u8, hip_u8), 3)
        out = m(fa.to(dev), fc.to(dev)).cpu()
        par[f"max_abs_{prec}_vs_cpu_ref"] = round(float((out - ref).abs().max()), 8)
    par["psnr_delta_db"] = round(abs(par[f"psnr_hip_{precision}_vs_truth_db"] - par["psnr_cpu_vs_truth_db"]), 4)
    par["psnr_delta_db_bf16x2"] = round(abs(par["psnr_hip_bf16x2_vs_truth_db"] - par["psnr_cpu_vs_truth_db"]), 4)
    # ---- the same criterion over more scenes, sizes and checkpoint seeds (bounded: ~5 s of CPU) ----
    try:
        sweep_rows, worst = _psnr_sweep(O, m, sd_i, dev, precision)
    except Exception as e:  # noqa: BLE001 -- the sweep is an extra: report, do not take the line down
        sweep_rows, worst = [{"error": f"{type(e).__name__}: {e}"}], 0.0
    par["psnr_delta_sweep"] = {"precision": precision, "cases": len(sweep_rows) + 1,
                               "worst_abs_delta_db": round(max(worst, par["psnr_delta_db"]), 4),
                               "bound_db": 0.05, "rows": sweep_rows}
    # ---- raw bf16 error of the bench's own random network (bounded size: 540x960) --------
    bm = make_bench_model(precision).to(dev).eval()
    sd_b = {k: v.detach().cpu() for k, v in bm.state_dict().items()}
    b1, b2 = O.make_frames(2, 1, 540, 960)
    bref = O.unet_forward(sd_b, b1, b2)
    bout = bm(b1.to(dev), b2.to(dev)).cpu()
    par["bench_network_540x960"] = {
        "rel_l2_vs_cpu_ref": round(float((bout - bref).norm() / bref.norm()), 6),
        "max_abs_vs_cpu_ref": round(float((bout - bref).abs().max()), 6),
        "out_absmax": round(float(bref.abs().max()), 4),
        "psnr_u8_vs_cpu_ref_db": round(O.psnr_u8(O.postprocess_tensor(bref), O.postprocess_tensor(bout)), 3),
    }
    return cpu_baseline, par


# ---------------------------------------------------------------------------------------------
# multi-GPU legs
# ---------------------------------------------------------------------------------------------
def video_leg(model, dev, dist, rank, world, n_frames, batch, h, w):
    """BASELINE configs[3]: rank 0 holds the uint8 frames in HBM; scatter -> forward_u8 -> gather."""
    from ai_based_frame_interpolation_amd import video as V

    class _Solo:  # the same code path without a process group (plain `python bench.py`)
        @staticmethod
        def run(frames, n, out=None):
            return P.interpolate_sequence(model, frames, batch=batch)

    torch.cuda.set_device(dev)  # legs run on a worker thread: the current device is per thread

    # [b,H,W] uint8 planes -> [b,H,W] middles, pre/post-processing on device; ragged sub-batches of small
    # frames padded exactly as the single-process loop pads them
    pair_fn = P.sequence_pair_fn(model, batch)

    frames = S.moving_frames(0, n_frames, h, w, device=dev, seed=11) if rank == 0 else None
    out = torch.empty((2 * n_frames - 1, h, w), dtype=torch.uint8, device=dev) if rank == 0 else None
    warm_n = min(n_frames, 2 * world * batch + 1)

    def run(n, o):
        if dist is None:
            return _Solo.run(frames[:n], n)
        return V.interpolate_video_sharded(pair_fn, frames[:n] if rank == 0 else None, n,
                                           (h, w), dev, batch=batch, root=0, out=o)

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    run(warm_n, out[:2 * warm_n - 1] if rank == 0 else None)   # RCCL connections, workspaces
    sync()
    t0 = time.perf_counter()
    res = run(n_frames, out)
    sync()
    dt = time.perf_counter() - t0
    ok = None
    if rank == 0:  # spot-check three pairs against the single-GPU uint8 forward (through the same chunk helper: below
        ok = True  # 1080p a lone pair is padded to the batch at which no layer K-splits, as the loops pad theirs)
        for i in (0, (n_frames - 1) // 2, n_frames - 2):
            mid = pair_fn(frames[i][None], frames[i + 1][None])[0]
            ok = ok and bool(torch.equal(res[2 * i + 1], mid)) and bool(torch.equal(res[2 * i], frames[i]))
    seen = world
    if dist is not None:  # ranks that actually answered on the RCCL communicator, and what each forwarded
        cnt = torch.tensor([V.partition_pairs(n_frames, world)[rank][1]], device=dev, dtype=torch.int64)
        allc = [torch.zeros_like(cnt) for _ in range(world)]
        dist.all_gather(allc, cnt)
        pairs_per_rank = [int(c.item()) for c in allc]
        seen = dist.get_world_size()
    else:
        pairs_per_rank = [n_frames - 1]
    host = None
    if dist is None:
        # PCIe-inclusive rate of the same job (N = 1): the frames start in HOST memory and the result ends there -
        # pinned buffers, chunks double-buffered on a copy stream against the compute stream
        # (inference.interpolate_sequence_host).  Never `value`; reported beside the device-resident number.
        try:
            t0 = time.perf_counter()
            src = frames.cpu().pin_memory()
            obuf = torch.empty((2 * n_frames - 1, h, w), dtype=torch.uint8).pin_memory()
            t_pin = time.perf_counter() - t0
            P.interpolate_sequence_host(model, src[:min(n_frames, 2 * batch + 1)], batch=batch)   # warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hout = P.interpolate_sequence_host(model, src, batch=batch, out=obuf)
            torch.cuda.synchronize()
            th = time.perf_counter() - t0
            same = all(bool(torch.equal(hout[k], res[k].cpu())) for k in (1, n_frames | 1, 2 * n_frames - 3))
            host = {"interpolated_frames_per_s": round((n_frames - 1) / th, 2), "seconds": round(th, 4),
                    "pcie_bytes_per_interpolated_frame": 2 * h * w,
                    "pin_and_stage_seconds_not_timed": round(t_pin, 2),
                    "equal_to_device_resident_result": same,
                    "note": "host uint8 frames -> host uint8 result, pinned, H2D / D2H on a copy stream under the forwards"}
            del src, obuf, hout
        except Exception as e:  # noqa: BLE001 -- an extra: report it, keep the leg
            host = {"error": f"{type(e).__name__}: {e}"}
    return {"frames_in": n_frames, "frames_out": 2 * n_frames - 1, "seconds": round(dt, 4),
            "interpolated_frames_per_s": round((n_frames - 1) / dt, 2),
            "host_resident_frames_per_s": None if host is None else host.get("interpolated_frames_per_s"),
            "host_resident": host, "ranks": seen,
            "pairs_per_rank": pairs_per_rank,
            "backend": ("single process" if dist is None else
                        "rccl (torch.distributed nccl) send/recv" if dist.get_backend() == "nccl" else
                        f"{dist.get_backend()} (REHEARSAL on one card: timings meaningless)"),
            "sub_batch_pairs": batch, "spot_check_equal_to_single_gpu": ok,
            "note": "end to end: frames resident in rank 0's HBM -> interleaved uint8 result in rank 0's HBM"}


def tile4k_single_gpu_leg(model, dev, reps=10):
    """BASELINE configs[4] as far as ONE GPU can measure it: one 2160x3840 pair un-tiled, the four config-5 row
    bands (origins 0 / 544 / 1088 / 1632, + 112-row halo) each on its own - what one of four GPUs would spend on its
    band, the bands being independent forwards - and back to back, and whether tiled == un-tiled."""
    from ai_based_frame_interpolation_amd import tiling as T

    torch.cuda.set_device(dev)
    h, w, n = 2160, 3840, 4
    gen = torch.Generator(device=dev).manual_seed(5)
    f1 = torch.rand((1, 1, h, w), device=dev, generator=gen) * 2 - 1
    f2 = torch.rand((1, 1, h, w), device=dev, generator=gen) * 2 - 1

    def timeit(fn, k=reps, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / k * 1e3

    whole = model(f1, f2)
    t_whole = timeit(lambda: model(f1, f2))
    tiled = T.forward_tiled(model.forward_strip, f1, f2, n)
    equal = bool(torch.equal(tiled, whole))
    t_all = timeit(lambda: T.forward_tiled(model.forward_strip, f1, f2, n), k=max(3, reps // 2))
    bands = []
    for s in T.strip_plan(h, n):
        a = f1[..., s.ext0:s.ext1, :].contiguous()
        b = f2[..., s.ext0:s.ext1, :].contiguous()
        bands.append({"rows": [s.core0, s.core1], "rows_with_halo": [s.ext0, s.ext1],
                      "ms": round(timeit(lambda: model.forward_strip(a, b, s.ext0, h)), 3),
                      "wire_mb_uint8": round((2 * a.numel() + (s.core1 - s.core0) * w) / 1e6, 1)})
    slow = max(bd["ms"] for bd in bands)
    return {"untiled_ms_per_pair": round(t_whole, 3), "untiled_pairs_per_s": round(1e3 / t_whole, 1),
            "bands": bands, "four_bands_back_to_back_ms": round(t_all, 3),
            "recompute_factor": round(t_all / t_whole, 3), "tiled_equals_untiled_bitwise": equal,
            "slowest_band_ms": slow, "latency_bound_if_4_gpus_ms": slow, "precision": model.precision,
            "halo_rows": T.HALO,
            "note": "ONE GPU: band times are what each of four GPUs would compute; no transfer is timed here (N >= 2: "
                    "tiling.forward_tiled_halo_exchange - cores from the root, 112-row input halos from the neighbours; "
                    "DESIGN section 7)"}


def tile4k_leg(model, dev, dist, rank, world, reps):
    """BASELINE configs[4]: one 2160x3840 pair, `world` row bands, 112-row halos exchanged between neighbours;
    uint8 frames, uint8 on the wire."""
    from ai_based_frame_interpolation_amd import tiling as T

    torch.cuda.set_device(dev)
    h, w = 2160, 3840
    shape = (1, 1, h, w)
    f1 = f2 = None
    if rank == 0:
        gen = torch.Generator(device=dev).manual_seed(5)
        f1 = torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8)
        f2 = torch.randint(0, 256, shape, device=dev, generator=gen, dtype=torch.uint8)

    def once():   # cores scattered from the root, 112-row halos fetched from the neighbours (uint8 everywhere)
        return T.forward_tiled_halo_exchange(model.forward_strip, f1, f2, shape, dev, root=0, wire=torch.uint8)

    for _ in range(2):
        out = once()
    dist.barrier(); torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = once()
    dist.barrier(); torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    res = {"ms_per_pair": round(dt * 1e3, 3), "pairs_per_s": round(1.0 / dt, 2), "strips": world,
           "halo_rows": T.HALO, "precision": model.precision, "wire": "uint8: core rows scattered from the root, 112-row input halos exchanged between neighbouring ranks, "
                                                                       "uint8 result gathered (tiling.forward_tiled_halo_exchange)"}
    if rank == 0:
        whole = model.forward_u8(f1, f2)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            whole = model.forward_u8(f1, f2)
        torch.cuda.synchronize()
        res["untiled_one_gpu_ms"] = round((time.perf_counter() - t0) / reps * 1e3, 3)
        res["tiled_equals_untiled_bitwise"] = bool(torch.equal(out, whole))
        res["tiled_vs_untiled_max_abs"] = int((out.int() - whole.int()).abs().max())
    return res


DUMP_BUDGET_BYTES = 64 * 10**6   # --dump-outputs writes at most this much in all
DUMP_SAMPLE = 1 << 22            # values in the sample of an output larger than the budget
DUMP_SAMPLE_SEED = 0


def dump_outputs(out: torch.Tensor, dirpath: str) -> dict:
    """Write what the timed path's last step returned (the interpolated frames, fp32 [B, 1, H, W]) to `dirpath`.
    Within DUMP_BUDGET_BYTES: the whole array as interpolated.npy.  Larger: DUMP_SAMPLE values at flat indices drawn
    by a CPU generator seeded DUMP_SAMPLE_SEED (so the same for every run of the same shape), in ascending order, as
    interpolated_sample.npy (float32), and those indices as interpolated_sample_flat_index.npy (float64, exact)."""
    import numpy as np
    os.makedirs(dirpath, exist_ok=True)
    out = out.detach().float()
    n = out.numel()
    if n * 4 + 4096 <= DUMP_BUDGET_BYTES:   # (+ room for the .npy header)
        np.save(os.path.join(dirpath, "interpolated.npy"), out.cpu().numpy())
        return {"dir": dirpath, "files": {"interpolated": list(out.shape)}, "sampled": False}
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(DUMP_SAMPLE_SEED))[:DUMP_SAMPLE].sort().values
    vals = out.reshape(-1)[idx.to(out.device)].cpu().numpy()
    np.save(os.path.join(dirpath, "interpolated_sample.npy"), vals)
    np.save(os.path.join(dirpath, "interpolated_sample_flat_index.npy"), idx.numpy().astype(np.float64))
    return {"dir": dirpath, "files": {"interpolated_sample": [len(vals)], "interpolated_sample_flat_index": [len(vals)]},
            "sampled": True, "of_shape": list(out.shape), "seed": DUMP_SAMPLE_SEED}


def launch_ranks(n: int) -> int:
    """`python bench.py --gpus N` with no launcher around it: be the launcher.  This process has made NO GPU call
    (importing torch and this package does not initialise HIP; nothing below does either) and never exec()s: it
    starts N CHILD processes, one rank per GPU, with the environment torch.distributed.run would give them, relays
    rank 0's stdout (the one JSON line) and returns the worst child status.  A child that fails or dies takes the
    others down after a grace period (they would wait in a collective for ever), by their exact PIDs."""
    import socket
    import subprocess
    with socket.socket() as sk:   # a free rendezvous port on the loopback interface
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        # rank 0's stdout is the result line; the other ranks' stdout (RCCL banners) goes to stderr
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__), *sys.argv[1:]], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, text=(r == 0)))
    out0 = []
    reader = threading.Thread(target=lambda: out0.extend(procs[0].stdout.readlines()), daemon=True)
    reader.start()
    worst, deadline = 0, None
    while any(p.poll() is None for p in procs):
        time.sleep(0.2)
        bad = [p.returncode for p in procs if p.poll() not in (None, 0)]
        if bad and deadline is None:
            deadline = time.time() + 30.0        # let the others report, then stop them
        if deadline is not None and time.time() > deadline:
            for p in procs:
                if p.poll() is None:
                    p.kill()
    reader.join(10.0)
    for p in procs:
        rc = p.returncode if p.returncode is not None else 1
        worst = max(worst, rc if rc > 0 else (128 - rc if rc < 0 else 0))
    lines = [l for l in out0 if l.strip()]
    for l in lines:
        sys.stdout.write(l)
    sys.stdout.flush()
    if worst == 0 and not any(l.lstrip().startswith("{") for l in lines):
        print("bench.py launcher: rank 0 exited 0 without a result line", file=sys.stderr)
        worst = 1
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--unfused", action="store_true", help="ablation: separate pool/upsample/head kernels")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run every other leg: CPU baseline and parity, fp32 / bf16x2 / "
                         "RGB / 256x256 figures, power, the video and 4K tiling legs (default: the headline only)")
    ap.add_argument("--video-frames", type=int, default=-1,
                    help="frames of the config-4 video leg of --full (default 3000 = BASELINE configs[3]; 0 = skip)")
    ap.add_argument("--no-tile4k", action="store_true")
    ap.add_argument("--no-fp32", action="store_true", help="skip the fp32 legs (A/B runs)")
    ap.add_argument("--no-power", action="store_true", help="skip the rocm-smi power / clock sample")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write rank 0's output of the last timed step to DIR/*.npy (dump_outputs: at most 64 MB, "
                         "a fixed seeded sample of a larger output)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.warmup < 0:
        ap.error("--warmup must not be negative")
    if args.video_frames > 0 and not args.full:
        ap.error("--video-frames sizes a leg of --full: add --full")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(launch_ranks(args.gpus))   # no launcher around us: be one (no GPU call so far, none in there)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: start one rank per GPU "
                         "(`python bench.py --gpus N` does it by itself)")
    dist = None
    # Rehearsals only (never set by the driver).  FIUNET_BENCH_REHEARSE=1 runs the N-rank flow on ONE card -
    # every rank on cuda:0, gloo instead of RCCL (which needs one GPU per rank) - to exercise the multi-rank
    # code paths of this file on a one-GPU box; its numbers mean nothing.  FIUNET_BENCH_REHEARSE=launcher (the
    # CPU test of `launch_ranks`, tests/test_dist.py) stops after the rendezvous: no GPU, no forward, no number.
    rehearse = os.environ.get("FIUNET_BENCH_REHEARSE") == "1"
    if os.environ.get("FIUNET_BENCH_REHEARSE") == "launcher":
        import torch.distributed as dist
        with _quiet_native_stdout():                 # gloo prints its connection banner on fd 1
            dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=120))
            t = torch.tensor([float(rank)], dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)     # the reduction the timed region's maximum takes
            dist.barrier()
        if rank == 0:
            print(json.dumps({"rehearsal": "launcher only: rendezvous + max-reduce over gloo, no forward was run",
                              "value": None, "n_gpus": world, "ranks_seen": dist.get_world_size(),
                              "max_rank_reduced": int(t.item()), "steps": args.steps, "warmup": args.warmup}))
        dist.destroy_process_group()
        return
    if rehearse:
        local_rank = 0
    if world > 1 or "RANK" in os.environ:  # under torch.distributed.run (also with one rank)
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        with _quiet_native_stdout():
            torch.cuda.set_device(local_rank)
            if rehearse:
                dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=600))
            else:
                dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local_rank}"),
                                        timeout=datetime.timedelta(seconds=600))
            dist.barrier()  # creates the RCCL communicator (and prints its banner) here, not later
            torch.cuda.synchronize()
    torch.cuda.set_device(local_rank)
    dev = torch.device(f"cuda:{local_rank}")

    b, h, w = args.batch, args.height, args.width
    model = make_bench_model(args.precision).to(dev).eval()
    model.set_options(unfused=args.unfused)

    gen = torch.Generator(device=dev).manual_seed(1 + rank)
    f1 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
    f2 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # the per-stage events are switched on BEFORE the warm-up, so that the event pool is created there and not inside
    # the timed region (1216 hipEventCreate calls: tens of milliseconds on a busy host - round 4 saw two runs whose
    # step time exceeded the sum of the stage times by 0.8-1.3 ms for that reason); the warm-up's records are discarded
    model._context(dev).profile_enable(True)   # (creates the native context and uploads the weights)
    for _ in range(args.warmup):
        model(f1, f2)
    model._ctx.profile_read()
    # (no garbage-collector pause inside the timed region: a step is 18 asynchronous launches the host must stay ahead of;
    # one run of round 6 lost 19 ms in ONE stage of ONE of its 20 steps - launch starvation, the kernels were not slower)
    import gc
    gc.collect()
    gc.disable()
    barrier()
    out = None
    t0 = time.perf_counter()
    for _ in range(args.steps):
        del out                # the previous step's output goes back to the allocator before the next one is made
        out = model(f1, f2)
    barrier()
    elapsed = time.perf_counter() - t0
    gc.enable()
    nfw, rows = model._ctx.profile_read()
    model._ctx.profile_enable(False)
    if dist is not None:
        t = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    dumped = dump_outputs(out, args.dump_outputs) if args.dump_outputs and rank == 0 else None
    del out
    default_workload = (b, h, w, args.precision, args.unfused) == (8, 1080, 1920, "bf16", False)
    power = None

    # ---- everything below the timed steps runs with --full only: a plain run dumps and prints the headline ----
    # ---- config 4 / config 5 legs (every rank takes part; bounded, failures are reported) ----
    n_video = (args.video_frames if args.video_frames >= 0 else (3000 if default_workload else 0)) if args.full else 0
    video_res = tile_res = None
    if n_video >= 2:
        with _quiet_native_stdout():
            video_res, err = _run_bounded(
                lambda: video_leg(model, dev, dist, rank, world, n_video, b, h, w), 240.0)
        if err:
            video_res = {"error": err, "frames_in": n_video, "ranks": world}
            if "timeout" in err:  # a hung transfer: nothing after it can run on this communicator
                if rank == 0:
                    print(json.dumps(headline(args, world, elapsed, rows, nfw, default_workload,
                                              video_res, None, None, None, dumped=dumped)))
                    sys.stdout.flush()
                os._exit(3)  # the headline is printed, but a hung leg must show in the return code
    if args.full and world == 1 and default_workload and not args.no_tile4k:
        with _quiet_native_stdout():
            tile_res, err = _run_bounded(lambda: tile4k_single_gpu_leg(model, dev), 120.0)
        if err:
            tile_res = {"error": err, "strips": 4}
    if args.full and dist is not None and world >= 2 and default_workload and not args.no_tile4k:
        with _quiet_native_stdout():
            tile_res, err = _run_bounded(lambda: tile4k_leg(model, dev, dist, rank, world, 10), 120.0)
        if err:
            tile_res = {"error": err, "strips": world}
            if "timeout" in err:
                if rank == 0:
                    print(json.dumps(headline(args, world, elapsed, rows, nfw, default_workload,
                                              video_res, tile_res, None, None, dumped=dumped)))
                    sys.stdout.flush()
                os._exit(3)

    # (after the config-4 / config-5 legs since round 6: four seconds of back-to-back forwards right before the 5.7-s video
    # leg heat-soaked the chip it was then compared on - on a warm box the video rate read 3-4 % under `value` while the
    # host-resident variant, which starts after seconds of host-side staging, did not)
    if args.full and world == 1 and default_workload and not args.no_power:
        try:
            power = power_leg(model, f1, f2, dev)
        except Exception as e:  # an extra leg must never cost the headline line
            power = {"error": f"{type(e).__name__}: {e}"}
    del f1, f2

    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    cpu_baseline = parity = fp32 = rgb = x2 = None
    if args.full and world == 1 and default_workload and not args.no_fp32:
        try:
            rgb = rgb_leg(dev, with_oracle=not args.no_cpu_baseline)
        except Exception as e:  # an extra leg must never cost the headline line
            rgb = {"error": f"{type(e).__name__}: {e}"}
        try:
            x2 = bf16x2_leg(dev, with_oracle=not args.no_cpu_baseline)
        except Exception as e:
            x2 = {"error": f"{type(e).__name__}: {e}"}
    if args.full and world == 1 and default_workload and not args.no_fp32:
        try:
            fp32 = fp32_legs(dev)
        except Exception as e:  # an extra leg must never cost the headline line
            fp32 = {"error": f"{type(e).__name__}: {e}"}
    small = None
    if args.full and world == 1 and default_workload and not args.no_fp32:
        try:
            small = small_frames_leg(dev)
        except Exception as e:  # an extra leg must never cost the headline line
            small = {"error": f"{type(e).__name__}: {e}"}
    if args.full and world == 1 and not args.no_cpu_baseline:
        cpu_baseline, parity = cpu_legs(dev, args.precision)
    print(json.dumps(headline(args, world, elapsed, rows, nfw, default_workload, video_res, tile_res,
                              cpu_baseline, parity, fp32, power, rgb, x2, small, dumped)))
    if dist is not None:
        dist.destroy_process_group()


def power_leg(model, f1, f2, dev, seconds=4.0):
    """Socket power and the driver's shader clock while the forward runs back to back (rocm-smi on a thread,
    outside the timed region).  Context only since round 5: the clock the roofline's sustained-clock fraction
    uses is the one measured inside the kernels (profiles/inkernel_clock.json)."""
    import re
    import subprocess

    # Under rocprofv3 the profiler's preloaded library initialises the GPU in every child process; rocm-smi is a
    # `#!/usr/bin/env python3` script, so spawning it would exec from a GPU-initialised process - which this pool
    # forbids (it takes the machine down).  Skip the leg there, and scrub the preload from the child's environment anyway.
    preload = [k for k in os.environ if k.startswith(("ROCP", "ROCPROFILER", "ROCTRACER"))]
    if "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or preload:
        return {"skipped": "a rocprofiler preload is active (LD_PRELOAD / " + ", ".join(sorted(preload)[:3]) + "): "
                           "rocm-smi is not spawned under the profiler"}
    child_env = {k: v for k, v in os.environ.items()
                 if k != "LD_PRELOAD" and not k.startswith(("ROCP", "ROCPROFILER", "ROCTRACER", "HSA_TOOLS"))}

    def num(v):
        m = re.search(r"[-+]?\d+(\.\d+)?", str(v))
        return float(m.group(0)) if m else None

    def smi(*flags):
        out = subprocess.run(["rocm-smi", "-d", str(dev.index or 0), *flags, "--json"], capture_output=True,
                             text=True, timeout=10, env=child_env).stdout
        return next(iter(json.loads(out).values()))

    cap = None
    try:
        cap = num(next(iter(smi("--showmaxpower").values())))
    except Exception:
        pass
    samples, stop = [], threading.Event()

    def sampler():
        while not stop.is_set():
            try:
                c = smi("--showpower", "--showclocks")
                pw = [num(v) for k, v in c.items() if "power" in k.lower()]
                ck = [num(v) for k, v in c.items() if k.lower().startswith("sclk clock speed")]
                if pw and ck:
                    samples.append((pw[0], ck[0]))
            except Exception:
                return

    th = threading.Thread(target=sampler, daemon=True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    model(f1, f2)
    e1.record()
    torch.cuda.synchronize()
    n = max(8, int(seconds * 1e3 / max(e0.elapsed_time(e1), 1e-3)))
    th.start()
    for _ in range(n):      # queued back to back, one synchronisation at the end
        model(f1, f2)
    torch.cuda.synchronize()
    stop.set()
    th.join(12)
    if not samples:
        return {"error": "rocm-smi gave no samples"}
    pw = sorted(s[0] for s in samples)
    ck = sorted(s[1] for s in samples)
    sclk = statistics.median(ck)
    return {"socket_w_median": statistics.median(pw), "socket_w_max": pw[-1], "cap_w": cap, "sclk_mhz_median": sclk,
            "samples": len(samples),
            "note": "rocm-smi while the forward runs back to back, outside the timed region.  Context only: the driver's "
                    "sclk reads ~0.1-0.15 GHz above the clock the kernels measure in-kernel (roofline.inkernel_clock_ghz), "
                    "and socket power below the cap does not mean the clock is free to rise (MI355X_MICROARCH.md, DVFS)"}


def dominant_kernel(rows, precision):
    """Stage rows (kernel name, avg ms, algorithmic FLOPs) grouped by kernel instantiation -> the
    instantiation with the most time and its algorithmic FLOP rate."""
    groups = {}
    for name, ms, fl in rows:
        g = groups.setdefault(name, {"ms": 0.0, "flops": 0.0, "launches": 0})
        g["ms"] += ms; g["flops"] += fl; g["launches"] += 1
    dom_name, dom = max(groups.items(), key=lambda kv: kv[1]["ms"])
    achieved = dom["flops"] / (dom["ms"] * 1e-3) / 1e12 if dom["ms"] > 0 else 0.0
    return dom_name, dom, achieved


def rgb_leg(dev, steps=10, warm=2, with_oracle=True):
    """The 6 -> 3 RGB variant the north star's wording describes (`UNet(n_channels=6, n_classes=3)`, unet.py:66; SURVEY
    section 0: "report both"): batch 8 of 1080p RGB pairs, bf16, same protocol as the headline (inputs resident, HIP
    events around the timed forwards on the launch stream).  +0.38 % FLOPs over the gray network; the stem
    runs as its own kernel here (the fused stem exists for the gray network only), so the 64-channel stem output
    makes one extra round trip through HBM."""
    model = make_bench_model("bf16", frame_channels=3).to(dev).eval()
    b, h, w = 8, 1080, 1920
    gen = torch.Generator(device=dev).manual_seed(3)
    f1 = torch.rand(b, 3, h, w, device=dev, generator=gen) * 2 - 1
    f2 = torch.rand(b, 3, h, w, device=dev, generator=gen) * 2 - 1
    for _ in range(warm):
        model(f1, f2)
    model._ctx.profile_enable(True)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(steps):
        model(f1, f2)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    _, rows = model._ctx.profile_read()
    model._ctx.profile_enable(False)
    fps = b / (ms * 1e-3)
    flops = conv_flops(h, w) + 2.0 * h * w * (4 * 64 * 9 + 2 * 64)   # RGB adds 2 H W (4*64*9 + 2*64)
    # parity of this variant on a small odd-sized pair against the CPU oracle (same weights): the oracle is only the
    # checker, outside every timed region, and only when the CPU legs are enabled
    parity = None
    if with_oracle:
        from oracle import unet_oracle as O
        sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        g = torch.Generator().manual_seed(5)
        s1, s2 = torch.rand(1, 3, 135, 240, generator=g) * 2 - 1, torch.rand(1, 3, 135, 240, generator=g) * 2 - 1
        ref = O.unet_forward(sd, s1, s2)
        out16 = model(s1.to(dev), s2.to(dev)).cpu()
        model.precision = "fp32"
        out32 = model(s1.to(dev), s2.to(dev)).cpu()
        parity = {"fp32_max_abs_vs_cpu_ref": round(float((out32 - ref).abs().max()), 8),
                  "bf16_rel_l2_vs_cpu_ref": round(float((out16 - ref).norm() / ref.norm()), 6),
                  "out_absmax": round(float(ref.abs().max()), 4)}
    return {"value": round(fps, 2), "unit": "frames/s", "ms_per_step": round(ms, 3), "steps": steps, "warmup": warm, "dtype": "bf16",
            "workload": "batch=8 1920x1080 synthetic RGB frame pairs, UNet(6->3, bilinear), bf16 MFMA conv path",
            "whole_forward_tflops": round(fps * flops / 1e12, 1),
            "whole_forward_mfma_frac": round(fps * flops / 1e12 / PEAK_TFLOPS["bf16"], 4),
            "stages_ms": [[n, round(t, 3)] for n, t, _ in rows],
            "parity_135x240": parity}


def bf16x2_leg(dev, with_oracle=True):
    """Round 4: the fp32 CONTRACT (north_star: |d|_inf <= 1e-3 against the reference's PyTorch-CPU forward) met on
    the bf16 matrix cores - precision "bf16x2": activations and weights as two bf16 pieces (16 significant bits),
    wh*xh + wl*xh + wh*xl per product with fp32 accumulation, exact-fp32 stem and head.  Same two workloads and
    protocol as `fp32` (BASELINE configs[1] and batch 4 of 1080p pairs), plus the measured error against the CPU
    oracle on the bench network.  The exact-fp32 figures stay in `fp32`: this is an extra mode, not a substitute."""
    model = make_bench_model("bf16x2").to(dev).eval()
    out = {}
    # (b8_1080p, round 5: the headline's own batch - at batch 4 the deepest level runs 1.125 rounds of workgroups)
    for key, b, h, w, warm, steps in (("config2_b16_256x256", 16, 256, 256, 10, 50), ("b4_1080p", 4, 1080, 1920, 1, 5),
                                      ("b8_1080p", 8, 1080, 1920, 1, 5)):
        gen = torch.Generator(device=dev).manual_seed(1)
        f1 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
        f2 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
        for _ in range(warm):
            model(f1, f2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            model(f1, f2)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        fps = b / (ms * 1e-3)
        out[key] = {"value": round(fps, 2), "unit": "frames/s", "ms_per_step": round(ms, 4), "steps": steps, "warmup": warm,
                    "dtype": "bf16x2 (two-piece bf16 operands, 3 MFMAs per product, fp32 accumulate)",
                    "workload": f"batch={b} {w}x{h} synthetic frame pairs",
                    "algorithmic_tflops": round(fps * conv_flops(h, w) / 1e12, 2),
                    "executed_mfma_frac_of_bf16_peak": round(3 * fps * conv_flops(h, w) / 1e12 / PEAK_TFLOPS["bf16"], 4)}
        del f1, f2
    # the RGB 6 -> 3 network (the north star's wording) in this precision, batch 4 of 1080p pairs
    try:
        rgbm = make_bench_model("bf16x2", frame_channels=3).to(dev).eval()
        gen = torch.Generator(device=dev).manual_seed(1)
        f1 = torch.rand(4, 3, 1080, 1920, device=dev, generator=gen) * 2 - 1
        f2 = torch.rand(4, 3, 1080, 1920, device=dev, generator=gen) * 2 - 1
        rgbm(f1, f2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(5):
            rgbm(f1, f2)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 5
        out["rgb_b4_1080p"] = {"value": round(4 / (ms * 1e-3), 2), "unit": "frames/s", "ms_per_step": round(ms, 4), "steps": 5,
                               "warmup": 1, "workload": "batch=4 1920x1080 synthetic RGB frame pairs, UNet(6->3, bilinear)"}
        del rgbm, f1, f2
    except Exception as e:  # noqa: BLE001 -- an extra entry, never the reason to lose the leg
        out["rgb_b4_1080p"] = {"error": f"{type(e).__name__}: {e}"}
    if not with_oracle:
        return out
    from oracle import unet_oracle as O   # checker only, outside every timed region
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    g = torch.Generator().manual_seed(9)
    s1, s2 = torch.rand(1, 1, 270, 480, generator=g) * 2 - 1, torch.rand(1, 1, 270, 480, generator=g) * 2 - 1
    ref = O.unet_forward(sd, s1, s2)
    got = model(s1.to(dev), s2.to(dev)).cpu()
    model.precision = "fp32"
    got32 = model(s1.to(dev), s2.to(dev)).cpu()
    out["parity_270x480"] = {"max_abs_vs_cpu_ref": round(float((got - ref).abs().max()), 8),
                             "rel_l2_vs_cpu_ref": round(float((got - ref).norm() / ref.norm()), 9),
                             "exact_fp32_max_abs_vs_cpu_ref": round(float((got32 - ref).abs().max()), 8),
                             "out_absmax": round(float(ref.abs().max()), 4), "contract_max_abs": 1e-3}
    return out


def fp32_legs(dev):
    """The reference's own arithmetic (fp32) on the driver-timed line: BASELINE configs[1] (batch 16 of
    256x256 pairs, SURVEY 8d config 2 protocol: 10 warm-up + 50 timed, HIP events around the forwards on
    the launch stream, inputs resident) and batch 4 of 1080p pairs (1 warm-up + 5 timed), each with the
    roofline of its dominant kernel against the fp32 MFMA peak.  ~3 s."""
    model = make_bench_model("fp32").to(dev).eval()
    out = {}
    for key, b, h, w, warm, steps in (("config2_b16_256x256", 16, 256, 256, 10, 50),
                                      ("b4_1080p", 4, 1080, 1920, 1, 5)):
        gen = torch.Generator(device=dev).manual_seed(1)
        f1 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
        f2 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
        for _ in range(warm):
            model(f1, f2)
        model._ctx.profile_enable(True)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(steps):
            model(f1, f2)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / steps
        nfw, rows = model._ctx.profile_read()
        model._ctx.profile_enable(False)
        fps = b / (ms * 1e-3)
        name, dom, ach = dominant_kernel(rows, "fp32")
        peak = PEAK_TFLOPS["fp32"]
        out[key] = {
            "value": round(fps, 2), "unit": "frames/s", "ms_per_step": round(ms, 4), "steps": steps, "warmup": warm,
            "dtype": "fp32", "workload": f"batch={b} {w}x{h} synthetic frame pairs, exact-fp32 MFMA conv path",
            "roofline": {"bound": "mfma", "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s",
                         "frac": round(ach / peak, 4), "kernel": name, "launches_per_step": dom["launches"],
                         "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
                         "algorithmic_flops_per_launch": dom["flops"] / dom["launches"], "traffic": None,
                         "whole_forward_tflops": round(fps * conv_flops(h, w) / 1e12, 2),
                         "whole_forward_mfma_frac": round(fps * conv_flops(h, w) / 1e12 / peak, 4)},
        }
        del f1, f2
    return out


def _concat_stage_launches_upsample(name: str) -> bool:
    """conv3x3_mfma_kernel<T,BN,TH,TW,MODE,EPI>: MODE 2 interpolates the upsampled half inside its gather; every other form
    of a concat stage (direct two-source conv, conv3x3_kwave_kernel) reads it from a tensor an upsample launch wrote."""
    if "conv3x3_mfma_kernel<" not in name:
        return "_kernel<" in name
    args = name.split("<", 1)[1].split(">", 1)[0].split(",")
    return len(args) >= 5 and args[4].strip() != "2"


def small_frames_leg(dev):
    """north_star: "throughput on synthetic 256x256 and 1080p pairs ... as fraction of the roofline".  (a) `latency_256`:
    ONE 256x256 pair - the only size the reference itself ever runs (model/inference.py:29,101-122 resize every input to
    256x256 and forward one pair) - back to back, 20 warm-up + 200 timed forwards between HIP events on the launch stream,
    in every precision, with the fraction of the MFMA peak the 79.9 GFLOP of a forward reach and the launch count (a
    forward of this size is bounded by its ~27-32 dependent dispatches at ~4.5 us each as much as by arithmetic);
    (b) `b16_256x256_bf16`: BASELINE configs[1]'s batch in the headline precision (SURVEY 8d config 2 protocol:
    10 warm-up + 50 timed).  The fp32 / bf16x2 figures of configs[1] are in `fp32` and `fp32_contract_on_bf16_pipe`."""
    out = {"workload": "ONE 256x256 synthetic frame pair per forward (the reference's own operating point), inputs resident, "
                       "20 warm-up + 200 timed forwards back to back, HIP events",
           "flops_per_forward": conv_flops(256, 256)}
    gen = torch.Generator(device=dev).manual_seed(0)
    f1 = torch.rand(1, 1, 256, 256, device=dev, generator=gen) * 2 - 1
    f2 = torch.rand(1, 1, 256, 256, device=dev, generator=gen) * 2 - 1
    for prec in ("bf16", "bf16x2", "fp32"):
        m = make_bench_model(prec).to(dev).eval()
        for _ in range(20):
            m(f1, f2)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(200):
            m(f1, f2)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / 200
        m._ctx.profile_enable(True)
        for _ in range(3):
            m(f1, f2)
        _, rows = m._ctx.profile_read()
        m._ctx.profile_enable(False)
        mult = 3.0 if prec == "bf16x2" else 1.0
        peak = PEAK_TFLOPS["fp32" if prec == "fp32" else "bf16"]
        tf = conv_flops(256, 256) / (ms * 1e-3) / 1e12
        out[prec] = {"ms_per_forward": round(ms, 4), "frames_per_s": round(1e3 / ms, 1), "algorithmic_tflops": round(tf, 1),
                     "roofline": {"bound": "mfma", "achieved": round(tf * mult, 1), "peak": peak, "unit": "TFLOP/s",
                                  "frac": round(tf * mult / peak, 4),
                                  "note": "executed MFMA rate of the whole forward (bf16x2: 3 MFMAs per product)"},
                     # 17 conv launches + one reduce pass per cross-workgroup K cut (it also pools), the stem where it is not
                     # fused, one upsample launch per concat conv (stages 10, 12, 14, 16) that does not interpolate inside its
                     # own gather (gather mode 2 in the kernel's name)
                     "dispatches_per_forward": 17 + sum("+splitk" in r[0] for r in rows) + (0 if "fused" in rows[0][0] else 1)
                                               + sum(_concat_stage_launches_upsample(rows[i][0]) for i in (10, 12, 14, 16)),
                     "cross_workgroup_k_cut_stages": sum("+splitk" in r[0] for r in rows),
                     "in_workgroup_k_cut_stages": sum("+kwave" in r[0] for r in rows),
                     "small_tile_stages": sum(",64,8,32," in r[0] for r in rows)}
        del m
    del f1, f2
    m = make_bench_model("bf16").to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)
    f1 = torch.rand(16, 1, 256, 256, device=dev, generator=gen) * 2 - 1
    f2 = torch.rand(16, 1, 256, 256, device=dev, generator=gen) * 2 - 1
    for _ in range(10):
        m(f1, f2)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(50):
        m(f1, f2)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 50
    fps = 16 / (ms * 1e-3)
    tf = fps * conv_flops(256, 256) / 1e12
    out["b16_256x256_bf16"] = {"value": round(fps, 1), "unit": "frames/s", "ms_per_step": round(ms, 4), "steps": 50, "warmup": 10,
                               "dtype": "bf16", "workload": "batch=16 256x256 synthetic frame pairs (BASELINE configs[1]'s batch, headline precision)",
                               "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": PEAK_TFLOPS["bf16"], "unit": "TFLOP/s",
                                            "frac": round(tf / PEAK_TFLOPS["bf16"], 4)}}
    return out


def headline(args, world, elapsed, rows, nfw, default_workload, video_res, tile_res, cpu_baseline, parity,
             fp32=None, power=None, rgb=None, x2=None, small=None, dumped=None):
    b, h, w = args.batch, args.height, args.width
    fps = world * b * args.steps / elapsed
    ms_step = elapsed / args.steps * 1e3
    flops_frame = conv_flops(h, w)
    es = 2 if args.precision == "bf16" else 4

    # ---- roofline of the dominant kernel (grouped by kernel instantiation) ------------------
    dom_name, dom, achieved = dominant_kernel(rows, args.precision)
    peak = PEAK_TFLOPS[args.precision]
    traffic = traffic_source = rocprof_avg = None
    pmc = os.path.join(ROOT, "profiles", "pmc_summary.json")
    if os.path.exists(pmc) and default_workload:  # the committed PMC pass is of this workload only
        try:
            js = json.load(open(pmc))
            traffic = js.get(dom_name, {}).get("hbm_bytes_per_launch")
            rocprof_avg = js.get(dom_name, {}).get("rocprof_avg_launch_ms")
            meta = js.get("_meta", {})
            traffic_source = ("profiles/pmc_summary.json: separate rocprofv3 --pmc passes (FETCH_SIZE x2 "
                              "corrected + WRITE_SIZE, tools/profile_all.sh) of this command at commit "
                              f"{meta.get('commit', '?')} on {meta.get('date', '?')}; NOT measured by this run")
        except Exception:
            traffic = None
    sum_ms = sum(r[1] for r in rows)
    roofline = {
        "bound": "mfma", "achieved": round(achieved, 2), "peak": peak, "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4), "traffic": traffic, "traffic_source": traffic_source,
        "kernel": dom_name, "launches_per_step": dom["launches"],
        "avg_launch_ms": round(dom["ms"] / dom["launches"], 4),
        # the same kernel's average in the committed `rocprofv3 --kernel-trace --stats` pass (profiles/, same source
        # and commit as `traffic`): NOT measured by this run, quoted so that the two can be compared
        "rocprof_avg_launch_ms_committed_profile": rocprof_avg,
        "algorithmic_flops_per_launch": dom["flops"] / dom["launches"],
        "events_forwards": nfw,
        "whole_forward": {
            "tflops": round(fps / world * flops_frame / 1e12, 2),
            "mfma_frac": round(fps / world * flops_frame / 1e12 / peak, 4),
            "hbm_algorithmic_gbs": round(fps / world * ELEMS_PER_PIXEL * h * w * es / 1e9, 1),
            "hbm_frac": round(fps / world * ELEMS_PER_PIXEL * h * w * es / 1e9 / PEAK_HBM_GBS, 4),
            "sum_stage_ms": round(sum_ms, 3),
        },
        "stages": [{"kernel": n, "ms": round(ms, 4), "tflops": round(fl / (ms * 1e-3) / 1e12, 1) if ms > 0 else 0}
                   for n, ms, fl in rows],
    }
    result = {
        "metric": "interpolated frames/sec at 1080p" if (h, w) == (1080, 1920) else f"interpolated frames/sec at {h}x{w}",
        "value": round(fps, 2), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_step, 3), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None, "dtype": args.precision, "data": "synthetic",
        "config": {"workload": f"batch={b} {w}x{h} synthetic frame pairs per GPU, {args.precision} "
                               f"MFMA conv path, random-init UNet(2->1, bilinear) weights",
                   "batch_per_gpu": b, "height": h, "width": w, "fused": not args.unfused,
                   "parallelism": f"frame-pair shard x{world}, no data-path collective"},
        "roofline": roofline,
    }
    if cpu_baseline is not None:
        result["cpu_baseline"] = cpu_baseline
    if parity is not None:
        result["parity"] = parity
    if fp32 is not None:
        result["fp32"] = fp32
    if rgb is not None:
        result["rgb_6to3"] = rgb
    if x2 is not None:
        result["fp32_contract_on_bf16_pipe"] = x2
    if small is not None:
        result["latency_256"] = small
    if power is not None:
        result["power"] = power   # socket power and the driver's sclk, as reported: NOT what the fractions below rest on
    # The clock the kernels run at is measured IN the kernel (a -DFIUNET_CLOCK diagnostic build: s_memtime / s_memrealtime
    # around the K loop, tools/inkernel_clock.py -> profiles/inkernel_clock.json; rocm-smi's sclk and rocprofv3's
    # GRBM_GUI_ACTIVE quotient both read higher).  Committed measurement of this workload, NOT taken by this run.
    ck = os.path.join(ROOT, "profiles", "inkernel_clock.json")
    if os.path.exists(ck) and default_workload:
        try:
            js = json.load(open(ck))
            mine = [r["ghz_median"] for r in js["stages"] if r["kernel"] == dom_name]
            allc = [r["ghz_median"] for r in js["stages"]]
            if mine:
                ghz = statistics.median(mine)
                pk = 2500.0 * ghz / 2.4
                roofline["inkernel_clock_ghz"] = round(ghz, 3)
                roofline["inkernel_clock_source"] = ("profiles/inkernel_clock.json (" + js["_meta"].get("date", "?") +
                                                     "): committed diagnostic-build measurement, not taken by this run")
                roofline["frac_of_peak_at_sustained_clock"] = round(achieved / pk, 4)
                roofline["whole_forward"]["mfma_frac_at_sustained_clock"] = round(
                    roofline["whole_forward"]["tflops"] / (2500.0 * statistics.median(allc) / 2.4), 4)
        except Exception:  # noqa: BLE001 -- an annotation, never worth the line
            pass
    if video_res is not None:
        result["video_sharded"] = video_res
        # config-4 efficiency at top level: end-to-end video rate / (n_gpus x this run's per-GPU headline rate)
        if isinstance(video_res.get("interpolated_frames_per_s"), (int, float)) and fps > 0:
            result["video_sharded_efficiency"] = round(video_res["interpolated_frames_per_s"] / fps, 4)
            result["video_sharded_efficiency_note"] = ("video_sharded.interpolated_frames_per_s / value (value is already the "
                                                       "whole-job rate over n_gpus): 1.0 = the end-to-end video loop, transfers "
                                                       "included, runs at the rate of the bare forwards")
        if world > 1:   # what the communicator actually did, where a reader of the N > 1 line looks first
            result["rccl_ranks_seen"] = video_res.get("ranks")
            result["pairs_per_rank"] = video_res.get("pairs_per_rank")
            result["collective_backend"] = video_res.get("backend")
    if tile_res is not None:
        result["tile4k"] = tile_res
    if dumped is not None:
        result["dumped_outputs"] = dumped
    return result


if __name__ == "__main__":
    main()
