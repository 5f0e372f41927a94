"""CPU: hold-out scoring - the chunk planner, the tests' own numpy restatement, the library's refusals
of the plane metrics (host side, before any pointer is used), the header against the binding, `score_video`'s refusals
before any GPU work, and the `evaluate` command line.  No GPU is touched."""
import ctypes
import io
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import holdout_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, holdout, imageio_lite as IO, metrics  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fiunet_plane_metrics_workspace_bytes", "fiunet_plane_psnr", "fiunet_plane_ssim"]
INVALID = 1   # FIUNET_ERR_INVALID_ARG


# ---- the planner --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("triplets", ["sliding", "disjoint"])
@pytest.mark.parametrize("chunk", [1, 2, 3, 7, 32])
def test_chunk_spans_cover_every_target_once(triplets, chunk):
    bound = chunk + 2 if triplets == "sliding" else 2 * chunk + 1
    for n in range(3, 41):
        spans = holdout.chunk_spans(n, chunk, triplets)
        got = [t for _, _, ts in spans for t in ts]
        assert got == R.targets(n, triplets), (n, got)
        if triplets == "disjoint":
            assert len(got) == (n - 1) // 2
        for first, count, ts in spans:
            assert 1 <= len(ts) <= chunk and 3 <= count <= bound and first >= 0 and first + count <= n
            assert all(first <= t - 1 and t + 1 < first + count for t in ts)
            # the neighbours sit on the chunk's decimation grid: both at an even distance from an input frame
            assert all((t - first) % 2 == 1 for t in ts) or triplets == "sliding"
        # consecutive chunks share the overlap and nothing is read twice beyond it
        for (f0, c0, _), (f1, _, _) in zip(spans[:-1], spans[1:]):
            assert f1 == f0 + chunk * (1 if triplets == "sliding" else 2) and f0 + c0 - f1 == (2 if triplets == "sliding" else 1)


def test_chunk_spans_short_clips_and_arguments():
    for n in (0, 1, 2):
        assert holdout.chunk_spans(n, 4, "sliding") == [] and holdout.chunk_spans(n, 4, "disjoint") == []
    assert holdout.chunk_spans(4, 8, "disjoint") == [(0, 3, [1])]       # the last frame has no use
    assert holdout.chunk_spans(5, 1, "sliding") == [(0, 3, [1]), (1, 3, [2]), (2, 3, [3])]
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="chunk_frames"):
            holdout.chunk_spans(9, bad, "sliding")
    with pytest.raises(ValueError, match="triplets"):
        holdout.chunk_spans(9, 4, "overlapping")
    with pytest.raises(ValueError, match="n_frames"):
        holdout.chunk_spans(-1, 4, "sliding")


# ---- the restatement ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(9, 11), (13, 8)])
@pytest.mark.parametrize("peak", [255, 1023])
def test_reference_ssim_matches_definition(h, w, peak):
    rng = np.random.default_rng(h * 1000 + w + peak)
    a = rng.integers(0, peak + 1, (h, w)).astype(np.uint16 if peak > 255 else np.uint8)
    b = np.clip(a.astype(int) + rng.integers(-peak // 10, peak // 10 + 1, (h, w)), 0, peak).astype(a.dtype)
    assert abs(R.ssim(b, a, peak) - R.ssim_bruteforce(b, a, peak)) < 1e-12
    assert R.ssim(a, a, peak) == pytest.approx(1.0, abs=1e-15)
    assert R.psnr(a, a, peak) == float("inf") and R.psnr(a, b, peak) == R.psnr(b, a, peak)


def test_reference_known_values():
    from oracle import metrics_oracle as M
    rng = np.random.default_rng(3)
    a, b = (rng.integers(0, 256, (12, 15)).astype(np.uint8) for _ in range(2))
    assert R.psnr(a, b, 255) == pytest.approx(M.psnr_u8(a, b), abs=1e-12)     # the restatement the u8 kernels are held to
    assert R.ssim(a, b, 255) == pytest.approx(M.ssim_u8(a, b), abs=1e-12)
    z, f = np.zeros((7, 7), np.uint16), np.full((7, 7), 1023, np.uint16)
    assert R.sse(z, f, 1023) == 49 * 1023 * 1023 and R.psnr(z, f, 1023) == 0.0
    assert R.sse(z, np.full((7, 7), 4000, np.uint16), 1023) == 49 * 1023 * 1023   # above 1023 reads as 1023
    assert R.sse(z, np.full((7, 7), -1, np.int16), 1023) == 49 * 1023 * 1023      # the int16 view of such a word
    assert R.predict("linear", np.array([0, 1, 254], np.uint8), np.array([1, 1, 255], np.uint8), 8).tolist() == [1, 1, 255]
    assert R.predict("linear", np.array([1023, 5], np.uint16), np.array([4000, 6], np.uint16), 10).tolist() == [1023, 6]
    assert R.predict("repeat", np.array([7], np.uint8), np.array([9], np.uint8), 8).tolist() == [7]
    assert R.targets(9, "disjoint") == [1, 3, 5, 7] and R.targets(6, "disjoint") == [1, 3] and R.targets(5, "sliding") == [1, 2, 3]


# ---- the library's host-side checks -------------------------------------------------------------------------------
H, W = 23, 70


def _psnr(lib, p, *, ps=H * W, pp=W, t=None, ts=H * W, tp=W, bits=8, n=1, h=H, w=W, out="p", sse=None, ws="p", wsb=1 << 20):
    t = p if t is None else t
    return lib.fiunet_plane_psnr(p, ps, pp, t, ts, tp, bits, n, h, w, p if out == "p" else out, sse,
                                 p if ws == "p" else ws, wsb, None)


def _ssim(lib, p, *, ps=H * W, pp=W, t=None, ts=H * W, tp=W, bits=8, n=1, h=H, w=W, out="p", ws="p", wsb=1 << 20):
    t = p if t is None else t
    return lib.fiunet_plane_ssim(p, ps, pp, t, ts, tp, bits, n, h, w, p if out == "p" else out,
                                 p if ws == "p" else ws, wsb, None)


@pytest.mark.parametrize("fn", [_psnr, _ssim], ids=["psnr", "ssim"])
def test_plane_metric_refusals(hip_lib_built, fn):
    """Every refusal comes back as FIUNET_ERR_INVALID_ARG from the host, before any launch (no device here: a launch
    would fail with another status) and before the dummy buffer could be dereferenced."""
    lib = _native.lib()
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 255) & ~255   # 256-B aligned, never dereferenced
    msg = lambda: lib.fiunet_last_error_string().decode()   # noqa: E731
    for bits in (0, 9, 12, 16, -8):
        assert fn(lib, p, bits=bits) == INVALID and "bits" in msg()
    assert fn(lib, p, pp=W - 1) == INVALID and "row_pitch" in msg()
    assert fn(lib, p, tp=W - 1) == INVALID and "row_pitch" in msg()
    assert fn(lib, p, n=2, ps=H * W - 1) == INVALID and "image_stride" in msg()
    assert fn(lib, p, n=2, ts=H * W - 1) == INVALID and "image_stride" in msg()
    assert fn(lib, p, n=3, pp=W + 5, ps=(H - 1) * (W + 5) + W - 1) == INVALID and "image_stride" in msg()
    assert fn(lib, p, wsb=0) == INVALID and "workspace" in msg()
    need = lib.fiunet_plane_metrics_workspace_bytes(4, H, W)
    assert need > 0 and fn(lib, p, n=4, wsb=(256 if fn is _psnr else need) - 1) == INVALID and "workspace" in msg()
    assert fn(lib, p, ws=p + 8) == INVALID and "aligned" in msg()
    for kw in (dict(out=None), dict(ws=None), dict(t=0)):
        assert fn(lib, p, **kw) == INVALID and "NULL" in msg()
    assert fn(lib, None) == INVALID and "NULL" in msg()
    for kw in (dict(n=0), dict(h=0), dict(w=0, pp=0), dict(n=65536, ps=1 << 20, ts=1 << 20)):
        assert fn(lib, p, **kw) == INVALID
    assert fn(lib, p + 1, bits=10) == INVALID and "odd address" in msg()


def test_ssim_refuses_planes_below_the_window(hip_lib_built):
    lib = _native.lib()
    buf = ctypes.create_string_buffer(512)
    p = (ctypes.addressof(buf) + 255) & ~255
    for h, w in ((6, 70), (23, 6), (1, 1)):
        assert _ssim(lib, p, h=h, w=w, pp=w, ps=h * w, ts=h * w, tp=w) == INVALID
        assert "7x7" in lib.fiunet_last_error_string().decode()
    assert lib.fiunet_plane_metrics_workspace_bytes(0, H, W) == 0
    assert lib.fiunet_plane_metrics_workspace_bytes(2, H, W) == lib.fiunet_metrics_workspace_bytes(2, H, W)
    assert lib.fiunet_plane_metrics_workspace_bytes(1, 5, 5) >= 256   # PSNR alone needs the sums


def test_python_plane_checks_come_first():
    a = torch.zeros((2, 9, 11), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.psnr_planes(a, a, 8)
    with pytest.raises(ValueError, match="bits"):
        metrics.psnr_planes(a, a, 12)
    with pytest.raises(ValueError, match="8-bit planes"):
        metrics.psnr_planes(a.to(torch.int16), a.to(torch.int16), 8)
    with pytest.raises(ValueError, match="10-bit planes"):
        metrics.ssim_planes(a, a, 10)
    with pytest.raises(ValueError, match="equal shape"):
        metrics.psnr_planes(a, a[:, :, :10], 8)
    assert metrics._plane_layout(a, "a") == (99, 11)
    assert metrics._plane_layout(a[:, 1:8, 2:9], "a") == (99, 11)
    assert metrics._plane_layout(torch.zeros((5, 200), dtype=torch.uint8)[1::2, 7:106].unflatten(1, (9, 11)), "a") == (400, 11)
    assert metrics._plane_layout(torch.zeros((4, 3, 9, 11), dtype=torch.uint8)[:, 1], "a") == (297, 11)
    assert metrics._plane_layout(torch.zeros((4, 3, 9, 11), dtype=torch.uint8), "a") == (99, 11)
    with pytest.raises(ValueError, match="stride 1"):
        metrics._plane_layout(a.transpose(1, 2), "a")
    with pytest.raises(ValueError, match="one stride"):
        metrics._plane_layout(torch.zeros((4, 3, 9, 11), dtype=torch.uint8)[:, :2], "a")


# ---- header and binding -------------------------------------------------------------------------------------------
def test_new_header_names_are_in_the_binding():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"\b(fiunet_plane_[a-z0-9_]*)\s*\(", src)
    assert sorted(declared) == sorted(NEW) and set(NEW) <= set(_native.SYMBOLS)
    assert re.search(r"#define FIUNET_ABI_VERSION 8\b", src) and _native.ABI_VERSION == 8
    assert re.search(r"FIUNET_ERR_INVALID_ARG = 1\b", src)


def test_library_exports_the_new_symbols(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    assert all(hasattr(lib, s) for s in NEW)
    L = _native.lib()
    assert L.fiunet_plane_metrics_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.fiunet_plane_psnr.argtypes) == 15 and len(L.fiunet_plane_ssim.argtypes) == 14


# ---- score_video: refusals before any GPU work ----------------------------------------------------------------------
@pytest.fixture
def no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("GPU work started before the arguments were checked")
    monkeypatch.setattr(holdout, "_score_chunk", boom)
    monkeypatch.setattr(torch.Tensor, "pin_memory", boom)


def _model(cf=1):
    return P.FrameInterpolationUNet(bilinear=True, frame_channels=cf)


def _y4m(path, n, h=16, w=24, chroma=True):
    y = np.zeros((n, h, w), np.uint8)
    c = np.zeros((n, (h + 1) // 2, (w + 1) // 2), np.uint8)
    IO.write_y4m(str(path), y, (c, c) if chroma else None)
    return str(path)


@pytest.mark.parametrize("n", [1, 2])
def test_fewer_than_three_frames(tmp_path, no_gpu, n):
    src = _y4m(tmp_path / "short.y4m", n)
    with pytest.raises(ValueError, match="at least 3 frames"):
        holdout.score_video(_model(), src)
    with open(src, "rb") as f, pytest.raises(ValueError, match="at least 3 frames"):
        holdout.score_video(_model(), io.BytesIO(f.read()))          # a stream: counted as it is read
    np.save(tmp_path / "short.npy", np.zeros((n, 16, 24), np.uint8))
    with pytest.raises(ValueError, match="at least 3 frames"):
        holdout.score_video(_model(), str(tmp_path / "short.npy"))


@pytest.mark.parametrize("kw,match", [
    (dict(methods=("unet", "flow")), "unknown method"),
    (dict(methods=()), "methods"),
    (dict(methods=("unet", "unet")), "methods"),
    (dict(triplets="pairs"), "triplets"),
    (dict(chunk_frames=0), "chunk_frames"),
    (dict(chunk_frames=2.5), "chunk_frames"),
    (dict(chunk_frames=None), "chunk_frames"),
    (dict(batch=0), "batch"),
    (dict(src_fps=29.97), "frame rate"),
    (dict(matrix="bt2020"), None),
], ids=["method", "no-methods", "twice", "triplets", "chunk-0", "chunk-float", "chunk-none", "batch", "fps", "matrix"])
def test_score_video_refusals(tmp_path, no_gpu, kw, match):
    src = _y4m(tmp_path / "clip.y4m", 5)
    if match is None:   # the routes' own refusals apply unchanged: the RGB network's colour options
        with pytest.raises(ValueError):
            holdout.score_video(_model(3), src, **kw)
        return
    with pytest.raises(ValueError, match=match):
        holdout.score_video(_model(), src, **kw)


def test_route_refusals_apply(tmp_path, no_gpu):
    with pytest.raises(ValueError, match="grayscale"):
        holdout.score_video(_Two(), _y4m(tmp_path / "clip.y4m", 5))
    np.save(tmp_path / "f32.npy", np.zeros((5, 16, 24), np.float32))
    with pytest.raises(ValueError, match="uint8 .npy stack"):
        holdout.score_video(_model(), str(tmp_path / "f32.npy"))
    with pytest.raises(ValueError, match="not a YUV4MPEG2 stream"):
        holdout.score_video(_model(), io.BytesIO(b"RIFF....AVI "))


class _Two:
    """A model of neither network: the Y4M route refuses it with its own message."""
    frame_channels = 2


# ---- the result as text -------------------------------------------------------------------------------------------
def test_json_and_csv_forms():
    import json
    res = {"frames": 5, "triplets": "sliding", "bits": 8, "peak": 255, "planes": ["y"], "methods": ["repeat"], "fps": (24, 1),
           "scored_frames": np.array([1, 2, 3], np.int64),
           "per_frame": {"repeat": {"y": {"psnr": np.array([30.5, np.inf, 28.0]), "ssim": np.array([0.9, 1.0, np.nan]),
                                          "sse": np.array([7, 0, 2 ** 40], np.uint64)}}},
           "summary": {"repeat": {"y": holdout._stats(np.array([30.5, np.inf, 28.0]), np.array([0.9, 1.0, np.nan]),
                                                      np.array([7, 0, 2 ** 40], np.uint64), 100, 255)}}}
    back = json.loads(json.dumps(holdout.to_jsonable(res), allow_nan=False))
    a = back["per_frame"]["repeat"]["y"]
    assert a["psnr"] == [30.5, "inf", 28.0] and a["ssim"][:2] == [0.9, 1.0] and a["ssim"][2] == "nan"
    assert a["sse"] == [7, 0, 2 ** 40] and back["scored_frames"] == [1, 2, 3] and float(a["psnr"][1]) == np.inf
    s = res["summary"]["repeat"]["y"]
    assert list(s) == list(holdout.STATS) and s["identical_frames"] == 1
    assert s["average_psnr"] == np.mean([30.5, 28.0]) and s["std_psnr"] == np.std([30.5, 28.0]) and s["max_ssim"] == 1.0
    assert s["psnr_of_mean_mse"] == pytest.approx(10 * np.log10(255.0 ** 2 / ((7 + 2 ** 40) / 3 / 100)), abs=1e-12)
    lines = list(holdout.csv_lines(res))
    assert lines[0] == "frame,time,repeat_y_psnr,repeat_y_ssim,repeat_y_sse" and len(lines) == 1 + 3
    assert lines[2] == "2," + repr(2 / 24) + ",inf,1.0,0"
    assert "repeat" in holdout.summary_table(res)
    empty = holdout._stats(np.array([np.inf]), np.array([np.nan]), np.array([0], np.uint64), 25, 1023)
    assert empty["average_psnr"] == np.inf and np.isnan(empty["average_ssim"]) and empty["psnr_of_mean_mse"] == np.inf


# ---- the CLI ------------------------------------------------------------------------------------------------------
def test_cli_evaluate_arguments():
    a = cli.parse_args(["evaluate", "--input", "-", "--model", "ckpt.pth"])
    assert a.command == "evaluate" and a.triplets == "sliding" and a.methods == ("unet", "linear", "repeat")
    assert a.chunk_frames == 32 and a.batch == 8 and a.json is None and a.csv is None and a.siting is None
    a = cli.parse_args(["evaluate", "--input", "clip.y4m", "--model", "m.pth", "--triplets", "disjoint", "--methods",
                        "unet,repeat", "--precision", "fp16", "--matrix", "bt2020", "--siting", "mpeg2", "--batch", "4",
                        "--chunk-frames", "5", "--src-fps", "30000/1001", "--json", "o.json", "--csv", "o.csv"])
    assert (a.triplets, a.methods, a.precision, a.matrix, a.siting) == ("disjoint", ("unet", "repeat"), "fp16", "bt2020", "mpeg2")
    assert (a.batch, a.chunk_frames, a.json, a.csv) == (4, 5, "o.json", "o.csv")
    assert (a.src_fps.numerator, a.src_fps.denominator) == (30000, 1001)
    for bad in (["--methods", "unet,flow"], ["--methods", ""], ["--triplets", "all"], ["--src-fps", "29.97"], ["--output", "x"]):
        with pytest.raises(SystemExit):
            cli.parse_args(["evaluate", "--input", "-"] + bad)
    with pytest.raises(SystemExit):
        cli.parse_args(["evaluate"])
    # the video command is unchanged
    v = cli.parse_args(["video", "--input", "-", "--output", "-"])
    assert v.command == "video" and v.chunk_frames == 32 and v.raw is None
