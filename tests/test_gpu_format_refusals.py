"""GPU (MI355X): every single-fault refusal of the eight frame-format forwards (the seven staged-RGB entry points and
fiunet_forward_p10) returns the status of the table in tests/format_refusals.py, and launches nothing: the workspace and
`out`, filled with a byte pattern before the call, are untouched after it.  One RGB context with seeded weights, B = 1,
32 x 32, bf16, the workspace of the entry point's own query; all of it host-side argument checking."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

import format_refusals as T  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0x7B


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def contexts(dev, seeded_sd):
    """{"rgb": loaded RGB, "gray": loaded grayscale, "unloaded": RGB without weights, "null": None} -> fiunet_ctx handles."""
    models = []
    for sd, cf in ((O.make_seeded_state_dict(77, n_channels=6, n_classes=3), 3), (seeded_sd, 1)):
        m = P.FrameInterpolationUNet(bilinear=True, frame_channels=cf, precision="bf16")
        m.load_state_dict(sd)
        models.append(m.to(dev).eval())
    unloaded = _native.Context(0, 3, True)
    yield {"rgb": models[0]._context(dev)._h, "gray": models[1]._context(dev)._h, "unloaded": unloaded._h, "null": None}
    unloaded.close()


@pytest.fixture(scope="module")
def buffers(dev):
    """Frame buffers large enough for every format of the table, as uint16 (the 8-bit entry points read their bytes)."""
    f1, f2 = (torch.zeros(T.ELEMS, dtype=torch.uint16, device=dev) for _ in range(2))
    return f1, f2, torch.empty(T.ELEMS, dtype=torch.uint16, device=dev)


def _case(contexts, buffers, dev, name, fault):
    """-> (status, untouched) of entry point `name` with `fault`, on a workspace and an `out` filled with FILL."""
    lib = _native.lib()
    f1, f2, out = buffers
    a = valid = T.valid_args(contexts["rgb"], f1.data_ptr(), f2.data_ptr(), out.data_ptr(), None, 0)
    if fault is not None:
        a = T.faulty_args(name, fault, valid)
        if isinstance(T.FAULTS[fault][0], str):
            a["ctx"] = contexts[T.FAULTS[fault][0]]
    # the workspace this call would need; where the fault itself makes the query refuse, the valid call's
    n = (T.workspace_bytes(lib, name, a["ctx"], a) or T.workspace_bytes(lib, name, a["ctx"], valid)
         or T.workspace_bytes(lib, name, contexts["rgb"], valid))
    assert n > 0
    ws = torch.full((n,), FILL, dtype=torch.uint8, device=dev)
    out.view(torch.uint8).fill_(FILL)
    a["ws_bytes"] = n
    if fault != "null-workspace":
        a["ws"] = ws.data_ptr()
    rc = T.call(lib, name, a)
    torch.cuda.synchronize(dev)
    return rc, int((ws != FILL).sum()) == 0 and int((out.view(torch.uint8) != FILL).sum()) == 0


@pytest.mark.parametrize("name", list(T.ENTRIES))
def test_the_valid_call_is_accepted(contexts, buffers, dev, name):
    """(so that each row below is wrong in one way only)"""
    rc, untouched = _case(contexts, buffers, dev, name, None)
    assert rc == 0, _native.lib().fiunet_last_error_string()
    assert not untouched


@pytest.mark.parametrize("name,fault", T.CASES, ids=[
    f"{n[len('fiunet_forward_'):]}-{f}" + ("-tightened" if (n, f) in T.LAUNCHED_BEFORE_REFUSING_ONCE else "") for n, f in T.CASES])
def test_single_fault_is_refused_with_its_status_before_any_launch(contexts, buffers, dev, name, fault):
    rc, untouched = _case(contexts, buffers, dev, name, fault)
    print(f"{name} {fault}: status {rc} ({_native.lib().fiunet_last_error_string().decode()}), "
          f"workspace and out {'untouched' if untouched else 'WRITTEN'}")
    assert rc == T.expected(name, fault), _native.lib().fiunet_last_error_string()
    assert untouched, "something was launched before the refusal"

