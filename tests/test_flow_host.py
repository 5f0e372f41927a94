"""CPU: the host side of the flow baseline - the level arithmetic of the library against the Python
loop, the refusals before any GPU work, the warp weights, the names in the header, the binding, the CLI and hold-out
scoring, and the torch backend of the batched entry points."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import flow_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, cli, evaluation, holdout, optical_flow as OF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["fiunet_flow_workspace_bytes", "fiunet_farneback_flow", "fiunet_flow_warp"]


# ---- the level arithmetic ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(132, 130), (130, 130), (40, 56), (33, 47), (72, 100), (135, 240), (256, 272), (63, 200),
                                 (64, 64), (31, 500), (8, 8), (1, 1), (127, 129), (255, 257), (1080, 1920), (2160, 3840),
                                 (131, 133), (250, 254)])
def test_levels_are_the_python_loops(hip_lib_built, h, w):
    assert _native.debug_flow_plan(h, w) == R.levels_of(h, w)


def test_half_sizes_round_to_even(hip_lib_built):
    plan = _native.debug_flow_plan(132, 130)
    assert plan[2] == (33, 32, 9, 1.5)                   # 32.5 -> 32, not 33
    assert plan[1] == (66, 65, 3, 0.5) and len(plan) == 3
    assert _native.debug_flow_plan(256, 272)[3] == (32, 34, 19, 3.5)
    assert len(_native.debug_flow_plan(63, 200)) == 1    # below min_size 32 at the first halving: level 0 only
    assert [lv[2] for lv in R.levels_of(256, 272)] == [3, 3, 9, 19]


# ---- refusals before any GPU work -----------------------------------------------------------------------------------------
def test_c_abi_refusals(hip_lib_built):
    L = _native.lib()
    p = 0x1000   # never dereferenced: every call below is refused by the argument checks
    need = L.fiunet_flow_workspace_bytes(2, 40, 56)
    assert need == 21 * 2 * 40 * 56 * 4 and need % 256 == 0
    assert L.fiunet_flow_workspace_bytes(0, 40, 56) == 0 and L.fiunet_flow_workspace_bytes(1, 0, 56) == 0
    assert L.fiunet_flow_workspace_bytes(5000, 40, 56) == 0
    fa = dict(prev=p, next=p, bits=8, B=2, H=40, W=56, stride=2240, pitch=56, out=p, ws=p, nbytes=need, stream=None)
    flow = lambda **k: L.fiunet_farneback_flow(*{**fa, **k}.values())
    for null in ("prev", "next", "out", "ws"):
        assert flow(**{null: None}) == 1 and b"NULL" in L.fiunet_last_error_string()
    assert flow(bits=9) == 1 and b"bits" in L.fiunet_last_error_string()
    assert flow(bits=16) == 1
    assert flow(nbytes=need - 1) == 5 and b"workspace too small" in L.fiunet_last_error_string()
    assert flow(pitch=55) == 1 and flow(stride=100) == 1 and flow(B=0) == 1
    assert flow(ws=p + 8) == 1 and b"aligned" in L.fiunet_last_error_string()
    wa = dict(f0=p, f1=p, flow=p, mode=0, bits=8, B=2, H=40, W=56, stride=2240, pitch=56, fh=40, fw=56, out=p,
              ostride=2240, opitch=56, stream=None)
    warp = lambda **k: L.fiunet_flow_warp(*{**wa, **k}.values())
    for null in ("f0", "f1", "flow", "out"):
        assert warp(**{null: None}) == 1
    assert warp(mode=2) == 1 and b"mode" in L.fiunet_last_error_string()
    assert warp(mode=-1) == 1 and warp(bits=12) == 1 and warp(fh=0) == 1 and warp(opitch=10) == 1
    assert warp(bits=10, f0=p + 1) == 1 and b"odd address" in L.fiunet_last_error_string()


def test_python_refusals():
    a = torch.zeros((2, 40, 56), dtype=torch.uint8)
    with pytest.raises(ValueError, match="backend"):
        OF.farneback_flow(a, a, "opencv")
    with pytest.raises(ValueError, match="bits"):
        OF.farneback_flow(a, a, "torch", bits=12)
    with pytest.raises(ValueError, match="equal shape"):
        OF.farneback_flow(a, a[:, :, :50], "torch")
    with pytest.raises(ValueError, match="equal shape"):
        OF.farneback_flow(a[0], a[0], "torch")
    with pytest.raises(ValueError, match="10-bit frames"):
        OF.farneback_flow(a, a, "torch", bits=10)
    with pytest.raises(ValueError, match="mode"):
        OF.interpolate(a, a, "symmetric", "torch")
    with pytest.raises(ValueError, match="flow: expected"):
        OF.warp(a, a, torch.zeros((2, 40, 56), dtype=torch.float32), "motion", "torch")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OF.farneback_flow(a, a, "hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        OF.warp(a, a, torch.zeros((2, 40, 56, 2)), "motion", "hip")
    f = torch.zeros((1, 1, 16, 16), dtype=torch.uint8)
    with pytest.raises(ValueError, match="flow_backend"):
        evaluation.evaluate_triplets(None, f, f, f, methods=("optical_flow",), flow_backend="opencv")
    assert "parity unpinned" in evaluation.optical_flow_backend("hip") and "hip" in evaluation.optical_flow_backend("hip")
    assert "parity unpinned" in holdout.FLOW_BACKEND


# ---- the warp weights: the kernel's closed form is what the Python code rounds to -------------------------------------------
def test_the_1024_weight_cells_need_no_rounding():
    a, b = torch.meshgrid(torch.arange(32), torch.arange(32), indexing="ij")
    mx, my = a.float() / 32, b.float() / 32
    closed = [32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b]
    for k, (y, x) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        probe = torch.zeros((2, 2), dtype=torch.int64)
        probe[y, x] = 1 << 15                  # (w * 2^15 + 2^14) >> 15 == w: the integer weight itself comes out
        assert torch.equal(OF._remap_bilinear(probe, mx, my), closed[k])
    assert torch.equal(sum(closed), torch.full((32, 32), 1 << 15))


# ---- names ------------------------------------------------------------------------------------------------------------
def test_header_binding_and_makefile():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = re.findall(r"\b(fiunet_[a-z0-9_]*flow[a-z0-9_]*)\s*\(", src)
    assert sorted(declared) == sorted(NEW) and set(NEW) <= set(_native.SYMBOLS)
    assert re.search(r"enum fiunet_flow_mode \{ FIUNET_FLOW_REFERENCE = 0, FIUNET_FLOW_MOTION = 1 \}", src)
    assert _native.FLOW_MODES == OF.MODES == ("reference", "motion")
    assert "fiunet_debug_flow_stage" not in src and "fiunet_debug_flow_stage" not in _native.SYMBOLS


def test_library_exports_the_new_symbols(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    assert all(hasattr(lib, s) for s in NEW + ["fiunet_debug_flow_stage", "fiunet_debug_flow_plan"])
    L = _native.lib()
    assert L.fiunet_flow_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.fiunet_farneback_flow.argtypes) == 12 and len(L.fiunet_flow_warp.argtypes) == 16


def test_holdout_and_cli_names():
    assert holdout.METHODS == ("unet", "linear", "repeat")
    assert holdout.ALL_METHODS == holdout.METHODS + ("optical_flow", "motion")
    a = cli.parse_args(["evaluate", "--input", "-", "--methods", "unet,motion,optical_flow"])
    assert a.methods == ("unet", "motion", "optical_flow")
    assert cli.parse_args(["evaluate", "--input", "-"]).methods == holdout.METHODS
    for bad in ("unet,flow", "motion,motion", "farneback"):
        with pytest.raises(SystemExit):
            cli.parse_args(["evaluate", "--input", "-", "--methods", bad])
    with pytest.raises(ValueError, match="unknown method"):
        holdout.score_video(P.FrameInterpolationUNet(bilinear=True, frame_channels=1), "none.y4m", methods=("flow",))
    with pytest.raises(ValueError, match="each once"):
        holdout.score_video(P.FrameInterpolationUNet(bilinear=True, frame_channels=1), "none.y4m",
                            methods=("motion", "motion"))


def _result(methods):
    st = holdout._stats(np.array([30.5]), np.array([0.9]), np.array([7], np.uint64), 100, 255)
    return {"frames": 3, "triplets": "sliding", "bits": 8, "peak": 255, "planes": ["y"], "methods": list(methods),
            "fps": None, "scored_frames": np.array([1], np.int64), "summary": {m: {"y": st} for m in methods}}


def test_summary_table_fits_the_names():
    wide = holdout.summary_table(_result(holdout.ALL_METHODS)).split("\n")
    narrow = holdout.summary_table(_result(holdout.METHODS)).split("\n")
    assert narrow[1].startswith("method  plane ") and narrow[2].startswith("unet    y     ")   # as before
    assert wide[1].startswith("method       plane ") and wide[5].startswith("optical_flow y     ")
    assert len({len(line) for line in wide[1:]}) == 1


# ---- the torch backend of the batched entry points ----------------------------------------------------------------------
def test_torch_backend_is_the_restatement():
    clip = R.texture_clip(40, 56, 1, 2, frames=3)
    f0, mid, f1 = clip[0], clip[1], clip[2]
    ref = OF.interpolate(f0[None], f1[None], "reference", "torch")
    assert torch.equal(ref[0], OF.optical_flow_interpolation_baseline(f0, f1))
    flow = OF.farneback_flow(torch.stack([f0, f1]), torch.stack([f1, f0]), "torch")
    assert flow.shape == (2, 40, 56, 2) and torch.equal(flow[0], OF.calc_optical_flow_farneback(f0, f1))
    motion = OF.warp(f0[None], f1[None], flow[:1], "motion", "torch")[0]
    c = (slice(8, -8), slice(8, -8))
    mse = lambda p: ((p[c].float() - mid[c].float()) ** 2).mean().item()
    linear = ((f0.int() + f1.int() + 1) >> 1).to(torch.uint8)
    assert mse(motion) < mse(linear) < mse(ref[0])    # with the motion; the blend; against the motion
    # a flow of another size is resampled and rescaled per axis; the same size is the field itself
    first = flow[0]
    assert OF.resample_flow(first, 40, 56) is first
    half = OF.resample_flow(torch.ones(40, 56, 2), 20, 28)
    assert half.shape == (20, 28, 2) and torch.equal(half, torch.full((20, 28, 2), 0.5))
    # 10-bit words: codes / 4 enter the flow
    t = R.texture_clip(40, 56, 1, 2, frames=2, peak=1023)
    f10 = OF.farneback_flow(t[:1], t[1:], "torch", bits=10)
    assert torch.equal(f10[0], OF.calc_optical_flow_farneback(t[0].float() / 4, t[1].float() / 4))
    out = OF.warp(t[:1], t[1:], f10, "motion", "torch", bits=10)
    assert out.dtype == torch.int16 and int(out.max()) > 255
