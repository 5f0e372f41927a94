"""GPU (MI355X): layouts right at the edge of refusal are accepted and computed right (csrc/plane_check.h).

In one dense buffer the output begins at the sample directly behind the last sample the call reads (tests/
plane_adjacent.py: 2 frames of 5 x 6 samples, step 1 and 2): fiunet_resize_planes_u8, fiunet_warp_table_u8 / _p10,
fiunet_chroma_fill_u8, and fiunet_chroma_pick_u8 with the pick map directly behind M.  The whole buffer is compared byte
for byte with the CPU references of the entry points' own tests - the inputs unchanged, the output exact, a guard behind it
untouched.  One sample earlier the same call is refused (tests/test_plane_check_host.py holds that half without a GPU).
No other GPU test places an output directly behind an input: theirs lie in buffers of their own."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import chroma_ref as CR  # noqa: E402
import plane_adjacent as PA  # noqa: E402
import resize_ref as RR  # noqa: E402
import retime_motion_ref as R  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402
from ai_based_frame_interpolation_amd import chroma as C  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 16


def _want(name, buf, step, bits, flow, pick):
    """The buffer after the call, from the references (CPU tensors; `buf` holds the inputs and the guard pattern)."""
    at, out, _ = PA.spans(name, step)
    want, b = buf.clone(), PA.body(step)
    named = ("p",) + PA.plane(step)[:5]
    if "resize" in name:
        got = RR.resize_planes(buf.numpy(), [PA.plane(step)], buf[out:].numpy(), [PA.plane(step, h=PA.DH, w=PA.DW)], PA.N, bits)
        want[out:] = torch.from_numpy(got)
    elif "warp" in name:
        R.warp_rows(buf[:PA.N * b].view(PA.N, b), [(r, wn, den, flag) for r, wn, den, _, flag in PA.ENTRIES], {0: flow[0]},
                    [named], bits, want[out:out + PA.N * b].view(PA.N, b))
    elif "fill" in name:
        for i in range(PA.N):
            for p in PA.uv(step):
                ca, cb, o = (R.plane_of(want[s + i * p[5]:], ("c",) + p[:5]) for s in (at["a"], at["b"], out))
                o.copy_(C.fill_torch(ca, cb, flow[i], pick[i], bits, (2, 2)).to(want.dtype))
    else:
        for i in range(PA.N):
            ya, yb, ym = (R.plane_of(buf[at[k] + i * b:], named) for k in ("a", "b", "m"))
            want[out + i] = C.pick_torch(ya, yb, ym, flow[i], bits).reshape(())
    return want


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", list(PA.CALLS))
def test_output_directly_behind_the_input(name, step):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    dev = torch.device("cuda:0")
    L = _native.lib()
    item, call = PA.CALLS[name]
    bits = 8 if item == 1 else 10
    rng = np.random.default_rng([len(name), step, item])
    _, out, span = PA.spans(name, step)
    buf = CR.stored(rng, bits, out + span + GUARD)
    fh, fw = (2 * PA.H, 2 * PA.W) if "fill" in name else (PA.H, PA.W)
    flow = torch.from_numpy(rng.uniform(-2.5, 2.5, (PA.N, fh, fw, 2)).astype(np.float32))
    pick = torch.from_numpy(rng.integers(0, 2, (PA.N,) + C.pick_shape(fh, fw)).astype(np.uint8))
    want = _want(name, buf, step, bits, flow, pick)
    assert not torch.equal(want[out:out + span], buf[out:out + span])
    d_buf, d_flow, d_pick = buf.to(dev), flow.to(dev), pick.to(dev)
    # one sample earlier: refused, nothing launched
    assert call(L, d_buf.data_ptr(), item, step, 1, d_flow.data_ptr(), d_pick.data_ptr()) == 1
    assert b"overlap" in L.fiunet_last_error_string()
    torch.cuda.synchronize(dev)
    assert torch.equal(d_buf.cpu(), buf)
    # directly behind: accepted and exact
    rc = call(L, d_buf.data_ptr(), item, step, 0, d_flow.data_ptr(), d_pick.data_ptr())
    assert rc == 0, (rc, L.fiunet_last_error_string())
    torch.cuda.synchronize(dev)
    bad = (d_buf.cpu() != want).nonzero()
    assert bad.numel() == 0, (name, step, bad[:8].tolist(), len(bad))
