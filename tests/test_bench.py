"""bench.py's measurement contract: `--steps` is the number of timed steps, `ms_per_step` the time of one, and
`--dump-outputs DIR` writes what the last timed step returned (at most 64 MB, a fixed seeded sample beyond that)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_whole_array_or_fixed_sample(tmp_path):
    import bench
    g = torch.Generator().manual_seed(5)
    small = torch.rand(2, 1, 64, 96, generator=g)
    info = bench.dump_outputs(small, str(tmp_path / "small"))
    assert info["sampled"] is False and info["files"] == {"interpolated": [2, 1, 64, 96]}
    got = np.load(tmp_path / "small" / "interpolated.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small.numpy())

    big = torch.rand(8, 1, 1080, 1920, generator=g)   # the default workload's output: 66 MB of fp32
    for d in ("a", "b"):
        info = bench.dump_outputs(big, str(tmp_path / d))
        assert info["sampled"] is True and info["of_shape"] == [8, 1, 1080, 1920]
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= bench.DUMP_BUDGET_BYTES
    vals = np.load(tmp_path / "a" / "interpolated_sample.npy")
    idx = np.load(tmp_path / "a" / "interpolated_sample_flat_index.npy")
    assert vals.dtype == np.float32 and idx.dtype == np.float64 and len(vals) == len(idx) == bench.DUMP_SAMPLE
    assert np.all(np.diff(idx) > 0) and idx[-1] < big.numel()
    assert np.array_equal(big.numpy().reshape(-1)[idx.astype(np.int64)], vals)
    # the sample is fixed: the same indices for every run of the same shape
    assert np.array_equal(idx, np.load(tmp_path / "b" / "interpolated_sample_flat_index.npy"))


@pytest.mark.parametrize("bad", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_rejects_step_counts_it_cannot_time(bad):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *bad], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and not r.stdout.strip(), (r.returncode, r.stdout, r.stderr[-500:])


@pytest.mark.gpu
def test_bench_dumps_what_its_last_timed_step_returned(tmp_path):
    """A small bf16 workload through bench.py in a child process: the result line counts the steps asked for, and the
    dump equals the forward of the same seeded network on the same seeded frames computed here (the forward is
    deterministic, so bit for bit)."""
    import bench
    b, h, w, steps = 2, 64, 96, 3
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--batch", str(b), "--height", str(h), "--width", str(w), "--no-cpu-baseline",
                        "--dump-outputs", str(tmp_path / "dump")], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0
    assert d["dumped_outputs"]["files"] == {"interpolated": [b, 1, h, w]}
    got = np.load(tmp_path / "dump" / "interpolated.npy")

    dev = torch.device("cuda:0")
    model = bench.make_bench_model("bf16").to(dev).eval()
    gen = torch.Generator(device=dev).manual_seed(1)     # rank 0's frames, as bench.main draws them
    f1 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
    f2 = torch.rand(b, 1, h, w, device=dev, generator=gen) * 2 - 1
    want = model(f1, f2).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_bench_video_frames_needs_full():
    """The video leg belongs to --full: sizing it on a plain run is an argument error, not a silent no-op."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--video-frames", "9"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip(), (r.returncode, r.stdout, r.stderr[-500:])


# objects only `--full` puts on the line: a plain run measures nothing beyond its timed steps
FULL_ONLY = ("cpu_baseline", "parity", "fp32", "rgb_6to3", "fp32_contract_on_bf16_pipe", "latency_256", "power",
             "video_sharded", "video_sharded_efficiency", "tile4k")


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_only():
    """The default workload without --full: one JSON line with the headline and the roofline of the timed steps,
    and none of the legs --full adds."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"] == "interpolated frames/sec at 1080p" and d["unit"] == "frames/s" and d["dtype"] == "bf16"
    assert d["higher_is_better"] is True and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 8e3 / d["ms_per_step"]) <= 0.01 * d["value"]   # 8 frame pairs per step
    assert d["roofline"]["events_forwards"] == 2 and len(d["roofline"]["stages"]) > 0
    assert not [k for k in FULL_ONLY if k in d], sorted(d)
