"""CPU: retime "motion"  - the definition `optical_flow._warp_time_torch` and its two identities, what
it buys on translating texture, the plane coverage of every frame layout, the argument checks, the names and the
refusals of fiunet_warp_table_* (which return before any launch, so they need no GPU).

The quality rows are the issue's: a band-limited texture (tests/retime_motion_ref.py) at 64 x 96 moved by (2, 0) and
(3, 1) pixels per bisection step, the frame at wn / den = 1/5, 2/5, 3/5 and 7/16 of the step made by blend and by motion
(flow from the torch backend) and scored against the analytically moved picture.  Motion must be at least 3 dB above
blend: the smallest gap measured when the feature was proposed was 6.3 dB, and the margin allows for another texture
seed and for the flow's own error.  No absolute PSNR is asserted."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import retime_motion_ref as R  # noqa: E402
import retime_motion_stream_rows  # noqa: E402,F401  (adds the new entry points' rows to tests/stream_contract.py)

from ai_based_frame_interpolation_amd import _native, cli, imageio_lite, layout, stream  # noqa: E402
from ai_based_frame_interpolation_amd import optical_flow as OF  # noqa: E402
from ai_based_frame_interpolation_amd import retime as RT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMES = [(1, 5), (2, 5), (3, 5), (7, 16)]


def _frames(h, w, bits, seed):
    g = torch.Generator().manual_seed(seed)
    if bits == 8:
        return [torch.randint(0, 256, (h, w), dtype=torch.uint8, generator=g) for _ in range(2)]
    return [torch.randint(0, 1200, (h, w), generator=g).to(torch.int16) for _ in range(2)]   # (words above 1023 too)


# ---- the definition and its identities ------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("shape,fshape", [((64, 96), (64, 96)), ((96, 128), (96, 128)), ((20, 28), (40, 56))])
def test_half_way_is_the_motion_warp_and_zero_flow_is_the_blend(shape, fshape, bits):
    a, b = _frames(*shape, bits, seed=3)
    g = torch.Generator().manual_seed(4)
    flow = (torch.rand(*fshape, 2, generator=g) - 0.5) * 12
    for wn, den in ((1, 2), (8, 16), (1 << 19, 1 << 20)):
        assert torch.equal(OF._warp_time_torch(a, b, flow, wn, den, bits), OF._warp_torch(a, b, flow, "motion", bits))
    zero = torch.zeros(*fshape, 2)
    for wn, den in TIMES + [(1, 2), (1, 1 << 20), ((1 << 20) - 1, 1 << 20)]:
        got = OF._warp_time_torch(a, b, zero, wn, den, bits)
        assert torch.equal(got, ((den - wn) * R.codes(a, bits) + wn * R.codes(b, bits) + den // 2) // den), (wn, den)
        assert torch.equal(got.to(a.dtype), R.blend_rows(a, b, wn, den, bits))


def test_the_ends_of_the_interval_and_a_nan_flow():
    a, b = _frames(33, 47, 8, seed=5)
    flow = torch.full((33, 47, 2), 2.0)
    near_a = OF._warp_time_torch(a, b, flow, 1, 1 << 20, 8)
    assert (near_a - a.long()).abs().max() <= 1      # s0 ~ 0: A where it is; B weighs 2^-20
    flow[3, 5] = float("nan")
    got = OF._warp_time_torch(a, b, flow, 2, 5, 8)   # a NaN clamps to coordinate 0
    assert int(got[3, 5]) == (3 * int(a[0, 0]) + 2 * int(b[0, 0]) + 2) // 5
    for wn, den in ((0, 5), (5, 5), (6, 5), (1, (1 << 20) + 1)):
        with pytest.raises(ValueError):
            OF._warp_time_torch(a, b, flow, wn, den, 8)


# ---- what it buys -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flows():
    h, w, out = 64, 96, {}
    for step in ((2, 0), (3, 1)):
        a, b = R.texture(h, w, 0, step), R.texture(h, w, 1, step)
        out[step] = (a, b, OF.farneback_flow(a[None], b[None], "torch")[0])
    return out


@pytest.mark.parametrize("step", [(2, 0), (3, 1)])
def test_motion_beats_blend_on_translating_texture(flows, step):
    a, b, flow = flows[step]
    for wn, den in TIMES:
        truth = R.texture(64, 96, wn / den, step)
        blend = R.psnr(R.blend_rows(a, b, wn, den, 8), truth)
        motion = R.psnr(OF._warp_time_torch(a, b, flow, wn, den, 8).to(torch.uint8), truth)
        print(f"step {step} time {wn}/{den}: blend {blend:.1f} dB, motion {motion:.1f} dB")
        assert motion >= blend + 3.0, (step, wn, den, blend, motion)


# ---- every layout's planes cover the frame ------------------------------------------------------------------------------
def _kinds():
    tags = ["mono", "420jpeg", "420mpeg2", "420paldv", "420", "422", "444"] + list(imageio_lite.Y4M_P10_TAGS)
    return list(layout.RAW_FORMATS) + [("y4m", t) for t in tags] + ["npy", ("npy", 3), ("npy", 4)]


@pytest.mark.parametrize("kind", _kinds(), ids=str)
@pytest.mark.parametrize("h,w", [(6, 8), (7, 10), (5, 9)])
def test_the_planes_of_every_layout_cover_the_frame(kind, h, w):
    if kind in ("uyvy422", "yuyv422") and w % 2:
        with pytest.raises(ValueError):
            layout.frame_layout(kind, h, w)
        return
    lay = layout.frame_layout(kind, h, w)
    stream.check_motion_layout(lay, str(kind))
    seen = np.zeros(lay.samples, dtype=int)
    for p in lay.planes:
        R.plane_of(torch.from_numpy(seen), p).add_(1)
    assert (seen == 1).all()


def test_a_layout_with_a_hole_is_refused_by_name():
    lay = layout.frame_layout("nv12", 6, 8)
    with pytest.raises(ValueError, match=r'retime="motion" is not available for nv12 with a hole'):
        stream.check_motion_layout(lay._replace(planes=lay.planes[:2]), "nv12 with a hole")
    with pytest.raises(ValueError, match="more than one"):
        stream.check_motion_layout(lay._replace(planes=lay.planes + lay.planes[:1]), "nv12 twice")


def test_lead_planes():
    assert RT.lead_planes(layout.frame_layout("nv12", 6, 8).planes) == ["y"]
    assert RT.lead_planes(layout.frame_layout("bgra", 6, 8).planes) == ["r", "g", "b"]
    assert RT.lead_planes(layout.frame_layout(("npy", 3), 6, 8).planes) == ["c0", "c1", "c2"]
    assert RT.lead_planes(layout.frame_layout("npy", 6, 8).planes) == ["gray"]
    assert RT.lead_planes(layout.frame_layout("uyvy422", 6, 8).planes) == ["y"]
    row = torch.arange(6 * 8 * 4, dtype=torch.int32).remainder(256).to(torch.uint8)
    planes = layout.frame_layout("bgra", 6, 8).planes
    px = row.reshape(6, 8, 4).to(torch.int32)
    assert torch.equal(R.lead_of(row, planes, 8), ((px[..., :3].sum(-1) * 2 + 3) // 6).to(torch.uint8))


# ---- arguments and names ------------------------------------------------------------------------------------------------
def test_modes():
    assert RT.MODES == ("blend", "nearest") and RT.VIDEO_MODES == ("blend", "nearest", "motion")
    assert RT.check_mode("motion") == "motion"
    with pytest.raises(ValueError):
        RT.check_mode("linear")
    assert stream.check_retime("60", "24", 2, "motion", 2)[3] == "motion"
    assert stream.check_retime(None, None, 2, "motion", 4)[3] == "motion"      # no fps: no effect, as "nearest"
    with pytest.raises(ValueError):
        stream.check_retime("60", "24", 2, "linear", 2)
    # the table's entries under "motion" are blend's: the warp replaces the cross-fade, not the times
    pl = RT.plan(24, 60, 2)
    assert RT.table_entries(pl, [], 0, 0, 11, 4, "motion") == RT.table_entries(pl, [], 0, 0, 11, 4, "blend")


def test_command_line():
    a = cli.parser().parse_args(["video", "--input", "a.y4m", "--output", "b.y4m", "--fps", "60", "--retime", "motion"])
    assert a.retime == "motion"
    assert cli.parser().parse_args(["video", "--input", "a.y4m", "--output", "b.y4m"]).retime == "blend"
    with pytest.raises(SystemExit):
        cli.parser().parse_args(["video", "--input", "a.y4m", "--output", "b.y4m", "--retime", "linear"])


def test_python_refusals():
    grid = torch.zeros((5, 8, 12), dtype=torch.uint8)
    pl = RT.plan(24, 60, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        RT.resample(grid, pl, 0, 0, 3, bits=8, mode="motion")
    with pytest.raises(ValueError, match="retime must be one of"):
        RT.resample_table(grid, [(0, 1, 5)], 8, mode="linear")
    with pytest.raises(ValueError, match="needs the layout"):
        RT._motion_layout(torch.zeros((5, 96), dtype=torch.uint8), None, 8)
    with pytest.raises(ValueError, match="reach sample"):
        RT._motion_layout(torch.zeros((5, 8, 12), dtype=torch.uint8), layout.frame_layout("nv12", 8, 12), 8)
    assert [p[0] for p in RT._motion_layout(torch.zeros((5, 8, 12, 3), dtype=torch.uint8), None, 8)] == ["c0", "c1", "c2"]
    with pytest.raises(ValueError, match="does not fit"):
        _native.warp_entries([(0, 1, 5, 0, 1 << 31)])
    with pytest.raises(ValueError, match="does not fit"):
        _native.warp_entries([(-1, 1, 5, 0, -1)])


def test_header_and_binding(hip_lib_built):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "fiunet.h")).read(), flags=re.S)
    new = ["fiunet_warp_table_u8", "fiunet_warp_table_p10"]
    assert sorted(re.findall(r"\b(fiunet_warp[a-z0-9_]*)\s*\(", src)) == sorted(new) and set(new) <= set(_native.SYMBOLS)
    assert "#define FIUNET_WARP_NO_FLAG (-1)" in src and _native.WARP_NO_FLAG == -1
    import ctypes
    assert ctypes.sizeof(_native.WarpEntry) == 20
    L = _native.lib()
    assert len(L.fiunet_warp_table_u8.argtypes) == len(L.fiunet_warp_table_p10.argtypes) == 14
    import stream_contract as SC
    assert set(new) <= {r.entry for r in SC.ROWS}


@pytest.mark.parametrize("name", ["fiunet_warp_table_u8", "fiunet_warp_table_p10"])
def test_c_abi_refusals(hip_lib_built, name):
    """Every refusal is FIUNET_ERR_INVALID_ARG and comes before a launch and before a pointer is used: the pointers
    here point nowhere."""
    L = _native.lib()
    for what, rc in R.refusals(getattr(L, name)):
        assert rc == 1, (what, rc, L.fiunet_last_error_string())
    if name.endswith("p10"):
        bad = R.refusals(L.fiunet_warp_table_p10, grid=(1 << 20) + 1)
        assert all(rc == 1 for _, rc in bad)
