"""GPU (MI355X): hold-out scoring of raw video and scene cuts in it.

A seeded RGB checkpoint, 7 frames of 23x35 (uyvy422 / yuyv422: 23x34), every format of stream.RAW_FORMATS:
  1. unet / linear / repeat: the sse of every plane equals the restatement's (tests/holdout_raw_ref.py) on predictions
     rebuilt with the public forwards on the neighbour frames, exactly; PSNR to 1e-12 relative; SSIM within the 1e-9 of
     tests/test_gpu_holdout.py (one plane per format also against the window-by-window definition)
  2. nv12, bgra, uyvy422 with all five methods: the flow methods' scores are those of optical_flow's warps of the planes
  3. chunk_frames 1, 2, 32 and a pipe give the same result to the last bit, the scene-cut fields included
  4. a tight NV12 clip scores as the same frames in C420mpeg2 Y4M, an rgb24 clip as the same frames in an [N,H,W,3] .npy
  5. a 12-frame clip with one hard cut, as Y4M, .npy and nv12: the cut interval, the excluded targets, per_frame
     untouched, the summary over the kept targets
  6. the `evaluate` command on a raw file and on standard input
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_raw_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import holdout, imageio_lite as IO, metrics, optical_flow as OF, scene  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9   # tests/test_gpu_holdout.py's bound on the device SSIM
H, W, N = 23, 35, 7
PREC = {8: "bf16", 10: "fp16"}
SCENE_KEYS = ("scene_cut", "scene_scores", "cut_intervals", "excluded_frames", "excluded")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rgb_model(dev):
    sd = O.make_interpolating_state_dict(n_channels=6, n_classes=3)
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="bf16")
    m.load_state_dict(sd)
    yield m.to(dev).eval(), sd
    torch.cuda.empty_cache()


def _size(fmt):
    return (H, W - 1) if fmt in R.CAPTURE else (H, W)


def _up(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _raw_file(tmp_path, fmt, rows, name="clip.raw"):
    path = tmp_path / name
    path.write_bytes(rows.astype("<u2" if rows.dtype == np.uint16 else np.uint8).tobytes())
    return str(path)


def _forward(m, fmt, f1, f2, h, w, dev):
    """the public forward of the format's route on host rows [B, row] -> host rows"""
    a, b = _up(f1, dev), _up(f2, dev)
    if fmt == "nv12":
        out = m.forward_nv12(a, b, h, w)
    elif fmt in ("rgb24", "bgr24", "rgba", "bgra"):
        out = m.forward_rgb_packed(a, b, h, w, format=fmt)
    else:
        if f1.dtype == np.uint16:
            a, b = a.view(torch.uint16), b.view(torch.uint16)
        out = m.forward_yuv(a, b, h, w, format=fmt)
        if f1.dtype == np.uint16:
            out = out.view(torch.int16)
    return out.cpu().numpy().view(f1.dtype)


def _same(a, b, keys=("psnr", "ssim", "sse")):
    assert a["methods"] == b["methods"] and a["planes"] == b["planes"] and a["frames"] == b["frames"]
    assert np.array_equal(a["scored_frames"], b["scored_frames"])
    for m in a["methods"]:
        for p in a["planes"]:
            for k in keys:
                assert np.array_equal(a["per_frame"][m][p][k], b["per_frame"][m][p][k], equal_nan=k == "ssim"), (m, p, k)
            assert a["summary"][m][p].keys() == b["summary"][m][p].keys()
            for k, v in a["summary"][m][p].items():
                assert v == b["summary"][m][p][k] or (np.isnan(v) and np.isnan(b["summary"][m][p][k])), (m, p, k)
    for k in SCENE_KEYS:
        assert (k in a) == (k in b)
        if k in a:
            assert np.array_equal(a[k], b[k]), k


# ---- 1. every format against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", sorted(R.FORMATS))
def test_every_raw_format_against_the_restatement(tmp_path, dev, rgb_model, fmt):
    m = rgb_model[0]
    bits, names = R.FORMATS[fmt]
    m.precision = PREC[bits]
    peak = R.peak_of(bits)
    h, w = _size(fmt)
    rows = R.clip(fmt, N, h, w, seed=len(fmt))
    res = holdout.score_video(m, _raw_file(tmp_path, fmt, rows), raw=fmt, width=w, height=h, src_fps=24)
    assert (res["frames"], res["triplets"], res["bits"], res["peak"], res["fps"]) == (N, "sliding", bits, peak, (24, 1))
    assert res["planes"] == list(names) and res["methods"] == ["unet", "linear", "repeat"]
    assert res["scored_frames"].tolist() == list(range(1, N - 1)) and not any(k in res for k in SCENE_KEYS)
    targets = range(1, N - 1)
    preds = {"unet": _forward(m, fmt, rows[:-2], rows[2:], h, w, dev),
             "linear": np.stack([R.predict("linear", rows[t - 1], rows[t + 1], bits) for t in targets]),
             "repeat": np.stack([R.predict("repeat", rows[t - 1], rows[t + 1], bits) for t in targets])}
    brute = 0
    for method, pr in preds.items():
        for j, t in enumerate(targets):
            got_planes, want_planes = R.planes_of(fmt, pr[j], h, w), R.planes_of(fmt, rows[t], h, w)
            for name in names:
                got, p, g = res["per_frame"][method][name], got_planes[name], want_planes[name]
                assert got["sse"].dtype == np.uint64 and int(got["sse"][j]) == R.sse(p, g, peak), (method, t, name)
                assert got["psnr"][j] == pytest.approx(R.psnr(p, g, peak), rel=1e-12), (method, t, name)
                assert got["ssim"][j] == pytest.approx(R.ssim(p, g, peak), abs=TOL), (method, t, name)
                if method == "unet" and j == 0:
                    brute = abs(got["ssim"][j] - R.ssim_bruteforce(p, g, peak))
                    assert brute <= TOL, (name, brute)
    s, a = res["summary"]["unet"][names[0]], res["per_frame"]["unet"][names[0]]
    assert s == holdout._stats(a["psnr"], a["ssim"], a["sse"], h * w, peak)
    order = [res["summary"][k][names[1]]["average_psnr"] for k in ("unet", "linear", "repeat")]
    print(fmt, "average PSNR of", names[1], "unet / linear / repeat:", order, "ssim - brute force:", brute)
    assert order[1] > order[2]


# ---- 2. the flow methods ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["nv12", "bgra", "uyvy422"])
def test_flow_methods_warp_the_planes(tmp_path, dev, rgb_model, fmt):
    m = rgb_model[0]
    m.precision = "bf16"
    h, w = _size(fmt)
    rows = R.clip(fmt, N, h, w, seed=3)
    res = holdout.score_video(m, _raw_file(tmp_path, fmt, rows), raw=fmt, width=w, height=h, methods=holdout.ALL_METHODS,
                              batch=2)
    assert res["methods"] == list(holdout.ALL_METHODS) and "flow_backend" in res
    planes = {name: _up(rows[:, ix], dev) for name, ix in R.plane_indices(fmt, h, w).items()}
    if fmt == "bgra":   # the rounded mean of r, g and b - not alpha
        total = sum(planes[c].to(torch.int32) for c in "rgb")
        lead = ((total * 2 + 3) // 6).to(torch.uint8)
    else:
        lead = planes["y"]
    flow = OF.farneback_flow(lead[:-2], lead[2:], "hip")
    for name, p in planes.items():
        for method, mode in holdout.FLOW_METHODS.items():
            pred = OF.warp(p[:-2], p[2:], flow, mode, "hip")
            ps, sse = metrics.psnr_planes(pred, p[1:-1], 8, return_sse=True)
            got = res["per_frame"][method][name]
            assert np.array_equal(sse.cpu().numpy().view(np.uint64), got["sse"]), (name, method)
            assert np.array_equal(ps.cpu().numpy(), got["psnr"]), (name, method)
            if min(p.shape[1:]) >= 7:
                assert np.array_equal(metrics.ssim_planes(pred, p[1:-1], 8).cpu().numpy(), got["ssim"]), (name, method)
    # the other three are what a run without the flow methods gives
    plain = holdout.score_video(m, _raw_file(tmp_path, fmt, rows), raw=fmt, width=w, height=h)
    for method in plain["methods"]:
        for name in plain["planes"]:
            for k in ("psnr", "ssim", "sse"):
                assert np.array_equal(plain["per_frame"][method][name][k], res["per_frame"][method][name][k])


# ---- 3. chunking --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triplets", ["sliding", "disjoint"])
@pytest.mark.parametrize("fmt", ["nv12", "rgba", "uyvy422", "yuv422p10le"])
def test_chunk_frames_do_not_change_the_result(tmp_path, dev, rgb_model, fmt, triplets):
    m = rgb_model[0]
    bits = R.FORMATS[fmt][0]
    m.precision = PREC[bits]
    h, w = _size(fmt)
    rows = R.clip(fmt, N + 1, h, w, seed=11)   # 8 frames: "disjoint" leaves a trailing frame no triplet uses
    rows[5:] = R.peak_of(bits) - rows[5:]      # a hard cut between frames 4 and 5
    src = _raw_file(tmp_path, fmt, rows)
    kw = dict(raw=fmt, width=w, height=h, triplets=triplets, scene_cut=10, methods=("unet", "linear", "repeat", "motion"))
    ref = holdout.score_video(m, src, chunk_frames=32, **kw)
    assert ref["cut_intervals"].tolist() == [4] and ref["scene_scores"].shape == (N,)
    for c in (1, 2):
        _same(holdout.score_video(m, src, chunk_frames=c, **kw), ref)
    with open(src, "rb") as f:   # a stream of unknown length
        _same(holdout.score_video(m, f, chunk_frames=2, **kw), ref)


# ---- 4. identities with the tested sources --------------------------------------------------------------------------------------
def test_nv12_scores_as_the_same_frames_in_y4m(tmp_path, dev, rgb_model):
    m = rgb_model[0]
    m.precision = "bf16"
    rows = R.clip("nv12", N, H, W, seed=21)
    pl = {name: rows[:, ix] for name, ix in R.plane_indices("nv12", H, W).items()}
    y4m = str(tmp_path / "clip.y4m")
    IO.write_y4m(y4m, pl["y"], (pl["u"], pl["v"]), fps=(24, 1), colourspace="420mpeg2")
    a = holdout.score_video(m, _raw_file(tmp_path, "nv12", rows), raw="nv12", width=W, height=H, src_fps=24)
    b = holdout.score_video(m, y4m)
    _same(a, b)
    assert a["planes"] == ["y", "u", "v"] and a["fps"] == b["fps"]


def test_rgb24_scores_as_the_same_frames_in_npy(tmp_path, dev, rgb_model):
    m = rgb_model[0]
    m.precision = "bf16"
    rows = R.clip("rgb24", N, H, W, seed=22)
    np.save(tmp_path / "clip.npy", rows.reshape(N, H, W, 3))
    a = holdout.score_video(m, _raw_file(tmp_path, "rgb24", rows), raw="rgb24", width=W, height=H)
    b = holdout.score_video(m, str(tmp_path / "clip.npy"))
    assert a["planes"] == ["r", "g", "b"] and b["planes"] == ["c0", "c1", "c2"]
    assert np.array_equal(a["scored_frames"], b["scored_frames"])
    for method in a["methods"]:
        for pa, pb in zip(a["planes"], b["planes"]):
            for k in ("psnr", "ssim", "sse"):
                assert np.array_equal(a["per_frame"][method][pa][k], b["per_frame"][method][pb][k]), (method, pa, k)
            assert a["summary"][method][pa] == b["summary"][method][pb]


# ---- 5. scene cuts ------------------------------------------------------------------------------------------------------------------
def _cut_source(tmp_path, kind):
    """-> (src, keyword arguments, the frames as stored [12, row])"""
    if kind == "npy":
        clip = R.cut_clip("npy", H, W)
        np.save(tmp_path / "cut.npy", clip)
        return str(tmp_path / "cut.npy"), {}, clip.reshape(12, -1)
    if kind == "nv12":
        clip = R.cut_clip("nv12", H, W)
        return _raw_file(tmp_path, "nv12", clip, "cut.raw"), dict(raw="nv12", width=W, height=H), clip
    clip = R.cut_clip("i420", H, W)
    hc, wc = (H + 1) // 2, (W + 1) // 2
    y, u, v = np.split(clip, [H * W, H * W + hc * wc], axis=1)
    IO.write_y4m(str(tmp_path / "cut.y4m"), y.reshape(12, H, W), (u.reshape(12, hc, wc), v.reshape(12, hc, wc)), fps=(24, 1))
    return str(tmp_path / "cut.y4m"), {}, clip


@pytest.mark.parametrize("kind", ["y4m", "npy", "nv12"])
def test_targets_next_to_a_cut_are_left_out_of_the_summary(tmp_path, dev, rgb_model, kind):
    m = rgb_model[0]
    m.precision = "bf16"
    src, kw, stored = _cut_source(tmp_path, kind)
    scores, flags = scene.detect_cuts(_up(stored, dev), 10.0, 8)
    assert flags.cpu().numpy().nonzero()[0].tolist() == [5]
    for triplets, want in (("sliding", [5, 6]), ("disjoint", [5])):
        plain = holdout.score_video(m, src, triplets=triplets, chunk_frames=3, **kw)
        res = holdout.score_video(m, src, triplets=triplets, chunk_frames=3, scene_cut=10, **kw)
        assert not any(k in plain for k in SCENE_KEYS) and list(res)[:len(plain)] == list(plain)
        assert res["scene_cut"] == 10.0 and res["cut_intervals"].tolist() == [5] and res["cut_intervals"].dtype == np.int64
        assert res["scene_scores"].dtype == np.float64 and np.array_equal(res["scene_scores"], scores.cpu().numpy())
        assert res["excluded_frames"].tolist() == want and res["excluded_frames"].dtype == np.int64
        assert res["excluded"].dtype == bool and np.array_equal(res["excluded"], np.isin(res["scored_frames"], want))
        assert np.array_equal(res["excluded"], R.excluded(flags.cpu().numpy(), res["scored_frames"]))
        assert np.array_equal(res["scored_frames"], plain["scored_frames"])
        for method in res["methods"]:   # every target is still predicted and scored: per_frame is bit-identical
            for p in res["planes"]:
                for k in ("psnr", "ssim", "sse"):
                    assert np.array_equal(res["per_frame"][method][p][k], plain["per_frame"][method][p][k]), (method, p, k)
        keep = ~res["excluded"]
        pixels = {"y": H * W, "u": 12 * 18, "v": 12 * 18}
        for method in res["methods"]:
            for p in res["planes"]:
                a = res["per_frame"][method][p]
                want_stats = holdout._stats(a["psnr"][keep], a["ssim"][keep], a["sse"][keep], pixels.get(p, H * W), 255)
                assert res["summary"][method][p] == want_stats, (method, p)
        # the frames across the cut are the worst ones of the blend: leaving them out lifts its minimum
        p0 = res["planes"][0]
        assert res["summary"]["linear"][p0]["min_psnr"] > plain["summary"]["linear"][p0]["min_psnr"]
        lines = list(holdout.csv_lines(res))
        assert lines[0].startswith("frame,time,excluded,unet_") and "left out at 1 scene cut" in holdout.summary_table(res)


def test_every_target_excluded_gives_nan_without_a_warning(tmp_path, dev, rgb_model):
    """The three frames around the cut: the one target has a cut interval on one side."""
    import warnings
    m = rgb_model[0]
    m.precision = "bf16"
    np.save(tmp_path / "three.npy", R.cut_clip("npy", H, W)[4:7])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = holdout.score_video(m, str(tmp_path / "three.npy"), scene_cut=10, methods=("linear",))
    assert res["cut_intervals"].tolist() == [1] and res["excluded"].tolist() == [True] and res["excluded_frames"].tolist() == [1]
    assert np.isfinite(res["per_frame"]["linear"]["c0"]["psnr"]).all()
    s = res["summary"]["linear"]["c0"]
    assert s["identical_frames"] == 0 and all(np.isnan(v) for k, v in s.items() if k != "identical_frames")
    assert "1 left out at 1 scene cut" in holdout.summary_table(res)


# ---- 6. the command line ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stdin", [False, True], ids=["file", "stdin"])
def test_cli_evaluate_raw_in_a_child_process(tmp_path, dev, rgb_model, stdin):
    m, sd = rgb_model
    m.precision = "bf16"
    ck = str(tmp_path / "rgb.pth")
    torch.save(sd, ck)
    src = _raw_file(tmp_path, "rgb24", R.cut_clip("rgb24", H, W))
    want = holdout.score_video(m, src, raw="rgb24", width=W, height=H, src_fps=24, scene_cut=10, chunk_frames=3)
    assert want["cut_intervals"].tolist() == [5]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, "-m", "ai_based_frame_interpolation_amd.cli", "evaluate", "--input",
                          "-" if stdin else src, "--raw", "rgb24", "--size", f"{W}x{H}", "--src-fps", "24", "--scene-cut",
                          "10", "--model", ck, "--precision", "bf16", "--chunk-frames", "3", "--json",
                          str(tmp_path / "o.json"), "--csv", str(tmp_path / "o.csv")],
                         input=open(src, "rb").read() if stdin else None, capture_output=True, cwd=ROOT, env=env, timeout=300)
    assert res.returncode == 0, res.stderr.decode(errors="replace")
    assert not res.stdout and b"2 left out at 1 scene cut" in res.stderr
    assert json.load(open(tmp_path / "o.json")) == json.loads(json.dumps(holdout.to_jsonable(want)))
    assert open(tmp_path / "o.csv").read().splitlines() == list(holdout.csv_lines(want))
