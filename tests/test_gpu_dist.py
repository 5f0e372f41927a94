"""GPU, two processes on ONE card, gloo backend: the multi-rank CONTROL FLOW of
video.interpolate_video_sharded and tiling.forward_tiled_distributed (partitioning, per-link issue order,
buffer rings, which stream consumes what) with the real HIP forward behind it.  RCCL needs one GPU per
rank, which this build's boxes do not have, so the transport here is NOT the production one: gloo cannot
move device memory in order with a HIP stream (its send/recv hand `data_ptr()` to a host thread), so
`transport.py` stages every device tensor through pinned host memory with an explicit stream
synchronisation on both ends.  What is checked is that the values a rank forwards and the places they
land are right - results equal the single-process ones bit for bit - not stream ordering of RCCL
transfers, and not xGMI.  These are the LAST tests of the GPU tier (tests/conftest.py orders the files):
a failure here cannot mask a parity test.  On a mismatch the workers report WHERE the results differ."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _diff_report(got, want):
    """Where two equally shaped tensors differ: element count, row range, largest difference."""
    if got.shape != want.shape:
        return f"shape {tuple(got.shape)} != {tuple(want.shape)}"
    ne = got != want
    n = int(ne.sum())
    if n == 0:
        return "equal"
    rows = ne.reshape(-1, got.shape[-2], got.shape[-1]).any(0).any(-1).nonzero().flatten()
    lead = ne.reshape(-1, got.shape[-2] * got.shape[-1]).any(-1).nonzero().flatten().tolist()
    d = (got.double() - want.double()).abs().max().item()
    return (f"{n} of {ne.numel()} elements differ; leading indices {lead[:8]}; rows {int(rows[0])}..{int(rows[-1])} "
            f"({rows.numel()} rows); max |d| {d:.3e}")


def _model(prec):
    import ai_based_frame_interpolation_amd as P
    from oracle import unet_oracle as O
    m = P.FrameInterpolationUNet(bilinear=True, precision=prec)
    m.load_state_dict(O.make_seeded_state_dict(1234))
    return m.to("cuda:0").eval()


def _video_worker(rank, world, port, prec, h, w, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import ai_based_frame_interpolation_amd as P
        from ai_based_frame_interpolation_amd import synthetic as S, video
        dev = torch.device("cuda:0")
        m = _model(prec)
        n = 14                             # 13 pairs: 7 + 6, sub-batches of 3 -> 3 pipelined steps, ragged ends
        frames = S.moving_frames(0, n, h, w, device=dev, seed=5) if rank == 0 else None
        pair_fn = P.sequence_pair_fn(m, 3)
        trace = []
        out = video.interpolate_video_sharded(pair_fn, frames, n, (h, w), dev, batch=3, trace=trace)
        torch.cuda.synchronize()
        if rank == 0:
            want = P.interpolate_sequence(m, frames, batch=3)
            q.put(("video", prec, bool(torch.equal(out, want)), len(trace), _diff_report(out, want)))
        else:
            assert out is None
    finally:
        dist.destroy_process_group()


def _tile_worker(rank, world, port, prec, h, w, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from ai_based_frame_interpolation_amd import tiling
        dev = torch.device("cuda:0")
        m = _model(prec)
        shape = (1, 1, h, w)                 # 2160x3840: two bands of 1088 / 1072 rows + 112-row halo: no layer of a band is K-split
        f1 = f2 = None
        if rank == 0:
            g = torch.Generator(device=dev).manual_seed(3)
            f1 = torch.rand(shape, device=dev, generator=g) * 2 - 1
            f2 = torch.rand(shape, device=dev, generator=g) * 2 - 1
        out = tiling.forward_tiled_distributed(m.forward_strip, f1, f2, shape, dev)
        torch.cuda.synchronize()
        # the video form of the same job: uint8 frames, uint8 bands on the wire, pre/post-processing on each rank's band
        u1 = u2 = None
        if rank == 0:
            u1 = torch.randint(0, 256, shape, device=dev, generator=g, dtype=torch.uint8)
            u2 = torch.randint(0, 256, shape, device=dev, generator=g, dtype=torch.uint8)
        out8 = tiling.forward_tiled_distributed(m.forward_strip, u1, u2, shape, dev, wire=torch.uint8)
        # ... and with the halos fetched from the neighbour instead of the root (BASELINE configs[4])
        outx8 = tiling.forward_tiled_halo_exchange(m.forward_strip, u1, u2, shape, dev, wire=torch.uint8)
        torch.cuda.synchronize()
        if rank == 0:
            whole = m(f1, f2)
            local = tiling.forward_tiled(m.forward_strip, f1, f2, world)   # same bands, no transport
            whole8 = m.forward_u8(u1, u2)
            torch.cuda.synchronize()
            ok8 = out8.dtype == torch.uint8 and bool(torch.equal(out8, whole8)) and bool(torch.equal(outx8, whole8))
            q.put(("tile", prec, bool(torch.equal(out, whole)) and ok8, 0,
                   f"2-rank vs un-tiled: {_diff_report(out, whole)} | single-process bands vs un-tiled: "
                   f"{_diff_report(local, whole)} | uint8 wire vs forward_u8 of the whole pair: {_diff_report(out8, whole8)}"))
        else:
            assert out is None and out8 is None and outx8 is None
    finally:
        dist.destroy_process_group()


def _run(worker, prec, h, w):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=worker, args=(r, 2, port, prec, h, w, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(240)
    hung = [p for p in procs if p.is_alive()]
    for p in hung:          # never leave a rank behind on the card
        p.kill()
        p.join(10)
    assert not hung, "a rank did not finish within 240 s"
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return q.get(timeout=5)


@pytest.mark.parametrize("prec,h,w", [("bf16", 1080, 1920), ("fp32", 1080, 1920), ("bf16", 360, 640)])
def test_sharded_video_two_ranks_on_one_gpu(prec, h, w):
    """360x640: the deep layers of a forward are K-split by a rule that depends on the batch, so this case
    holds only because every ragged sub-batch is padded to a full one on both sides (`sequence_pair_fn`)."""
    kind, p, equal, ntrace, where = _run(_video_worker, prec, h, w)
    assert (kind, p) == ("video", prec) and equal, where
    assert ntrace == 4   # root: 2 scatters + 2 gathers to rank 1


def test_tiled_forward_two_ranks_on_one_gpu():
    kind, p, equal, _, where = _run(_tile_worker, "bf16", 2160, 3840)
    assert (kind, p) == ("tile", "bf16") and equal, where


def test_bench_gpus_2_self_launches_on_one_card():
    """`python bench.py --gpus 2` exactly as the driver would type it (no torch.distributed.run around it): the
    process launches its two ranks itself.  One-card REHEARSAL (FIUNET_BENCH_REHEARSE=1: both ranks on cuda:0, gloo
    instead of RCCL, numbers meaningless) with the real forward and the sharded video leg behind it: one JSON line,
    rc 0, both ranks seen, the pairs split 4 + 4, the spot check against the single-GPU result green."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env["FIUNET_BENCH_REHEARSE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--batch", "2", "--height", "360", "--width", "640", "--no-cpu-baseline", "--no-power",
                        "--no-fp32", "--full", "--video-frames", "9"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak"
    assert d["rccl_ranks_seen"] == 2 and d["pairs_per_rank"] == [4, 4], d
    assert d["video_sharded"]["spot_check_equal_to_single_gpu"] is True
    assert "REHEARSAL" in d["collective_backend"]


def test_bench_under_torch_distributed_run_one_rccl_rank():
    """The form the driver uses for N > 1 (`python -m torch.distributed.run ... bench.py --gpus N`), with the one rank a
    one-GPU box has: RCCL communicator creation, the sharded video leg over the nccl backend, one JSON line, rc 0."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                                                            "FIUNET_BENCH_REHEARSE")}
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.join(root, "bench.py"),
                        "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--height", "360", "--width", "640",
                        "--no-cpu-baseline", "--no-power", "--no-fp32", "--full", "--video-frames", "9"],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 1 and d["value"] > 0
    assert "rccl" in d["video_sharded"]["backend"] and d["video_sharded"]["spot_check_equal_to_single_gpu"] is True
