"""GPU (MI355X): the stream contract of every entry point of include/fiunet.h - "asynchronous on `stream`; no allocation,
no synchronisation" - which no other GPU test can see, because they all call on the legacy default stream.

  1. every row of tests/stream_contract.py through its instrument: warm up on a side stream, capture one call into a
     graph, replay it twice on other inputs over poisoned outputs and workspaces, and compare bit for bit with an eager
     call on the default stream.  What that proves, and what it cannot, is in that module's docstring.
  2. what capture cannot cover, eagerly on non-blocking side streams: a device-side weight load with the forward behind
     it on one side stream, and one context (and two contexts) on two streams at once.

Every comparison is exact: the eager results at these shapes are tied to the oracles by the entry points' own tests."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_contract as SC  # noqa: E402
import stream_delay as SD  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    e = SC.Env(torch.device("cuda:0"))
    yield e
    e.close()


@pytest.mark.parametrize("row", SC.ROWS, ids=[f"{r.entry}-{r.ident}" for r in SC.ROWS])
def test_captured_replay_equals_the_eager_call(env, row):
    SC.check_row(row, env)


# ---- what capture cannot cover ---------------------------------------------------------------------------------------
def _forward_on(ctx, f1, f2, out, code, ws, stream):
    b, _, h, w = f1.shape
    SC._status("fiunet_forward", _native.lib().fiunet_forward(ctx._h, f1.data_ptr(), f2.data_ptr(), out.data_ptr(), b, h, w, code,
                                                              ws.data_ptr(), ws.numel(), stream))


def _serial(ctx, f1, f2, code):
    """One forward on the default stream, on fresh buffers -> the output."""
    dev = f1.device
    b, _, h, w = f1.shape
    ws = torch.empty(ctx.workspace_bytes(b, h, w, code), dtype=torch.uint8, device=dev)
    out = torch.empty_like(f1)
    _forward_on(ctx, f1, f2, out, code, ws, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return out


#: the delay ahead of the device load: everything behind it is enqueued within a few milliseconds of host time, so work
#: that does not wait for the load has run long before the load starts
LOAD_DELAY_MS = 50.0


def test_device_load_and_forward_on_one_side_stream(env):
    """fiunet_load_weights_device (the second load of a context, new weights) and fiunet_forward behind it on one
    non-blocking side stream with no host synchronisation in between, in fp32 and bf16; then again with
    fiunet_prepare_precision(BF16X2), and FP16, between the load and the forward: "it waits for this load on the device,
    not on the host", also when the load is not on the null stream.  The results are bit for bit those of a context that
    loaded the same weights through the host path.

    What is forced and what is not.  A delay kernel (tests/stream_delay.py, LOAD_DELAY_MS) sits on the side stream behind
    the 2x270x480 forwards and ahead of the load, so the load's kernels cannot start before it has passed, tens of
    milliseconds after the host has enqueued everything.  Work on ANOTHER stream that does not wait for the load - the
    packing of fiunet_prepare_precision, which goes to the null stream and has only the load's event to hold it back - now
    runs before the load every time and packs the previous weights: that race is no longer left to luck.  What is still
    not forced: work that wrongly went to the side stream itself runs behind the delay and the load in stream order and is
    right whatever it waits for, and a wait on the wrong event that happens to complete later than the load looks like the
    right one."""
    dev = env.dev
    sds =[O.make_seeded_state_dict(seed) for seed in (1234, 4321, 999, 31)]
    on_dev = [{k: v.to(device=dev, dtype=torch.float32).contiguous() for k, v in sd.items()
               if not k.endswith("num_batches_tracked")} for sd in sds]
    ctx = _native.Context(0, frame_channels=1, bilinear=True)
    ref = _native.Context(0, frame_channels=1, bilinear=True)
    try:
        ctx.load_state_dict(sds[0])
        big1, big2 = (t.to(dev) for t in O.make_frames(3, 2, 270, 480))
        big_out = torch.empty_like(big1)
        big_ws = torch.empty(ctx.workspace_bytes(2, 270, 480, _native.BF16), dtype=torch.uint8, device=dev)
        f1, f2 = (t.to(dev) for t in O.make_frames(5, 1, 64, 96))
        steps = [(1, (_native.FP32, _native.BF16), None), (2, (_native.BF16X2,), _native.BF16X2), (3, (_native.FP16,), _native.FP16)]
        for which, codes, prepare in steps:
            if prepare is not None:   # the buffers fiunet_prepare_precision packs into exist: the next one allocates nothing
                ctx.prepare(prepare)
            wss = [torch.empty(ctx.workspace_bytes(1, 64, 96, c), dtype=torch.uint8, device=dev) for c in codes]
            outs = [torch.empty_like(f1) for _ in codes]
            for o in outs:
                o.view(torch.uint8).fill_(0xFF)
            torch.cuda.synchronize(dev)
            side = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(side):
                for _ in range(4):
                    _forward_on(ctx, big1, big2, big_out, _native.BF16, big_ws, side.cuda_stream)
                SD.delay(side, LOAD_DELAY_MS)
                ctx.load_state_dict(on_dev[which], prep="device")   # on the current stream: `side`
                if prepare is not None:
                    ctx.prepare(prepare)
                for c, o, ws in zip(codes, outs, wss):
                    _forward_on(ctx, f1, f2, o, c, ws, side.cuda_stream)
            side.synchronize()
            ref.load_state_dict(sds[which])
            for c, o in zip(codes, outs):
                ref.prepare(c)
                SC.same(o, _serial(ref, f1, f2, c), f"load {which}, precision {c}: forward behind a device load on a side "
                                                     "stream against a context loaded through the host path")
    finally:
        ctx.close()
        ref.close()


def _two_streams(env, ctxs, code, b, h, w, rounds=8):
    """ctxs[k] on side stream k: `rounds` forwards each, back to back and alternating, every stream with its own inputs,
    outputs and workspace, no synchronisation before the end.  Every output is bit for bit the serial result."""
    dev = env.dev
    per = []
    for k, ctx in enumerate(ctxs):
        frames = [tuple(t.to(dev) for t in O.make_frames(100 * k + r, b, h, w, c=ctx.frame_channels)) for r in range(rounds)]
        outs = [torch.empty_like(f[0]) for f in frames]
        for o in outs:
            o.view(torch.uint8).fill_(0xFF)
        ws = torch.empty(ctx.workspace_bytes(b, h, w, code), dtype=torch.uint8, device=dev)
        ws.fill_(0x7B)
        per.append((ctx, frames, outs, ws, torch.cuda.Stream(device=dev)))
    torch.cuda.synchronize(dev)
    for r in range(rounds):
        for ctx, frames, outs, ws, side in per:
            _forward_on(ctx, frames[r][0], frames[r][1], outs[r], code, ws, side.cuda_stream)
    for p in per:
        p[4].synchronize()
    for k, (ctx, frames, outs, ws, side) in enumerate(per):
        for r in range(rounds):
            SC.same(outs[r], _serial(ctx, frames[r][0], frames[r][1], code), f"stream {k}, round {r}: against the serial result")


def test_one_context_on_two_streams_at_once(env):
    """Per-call state lives in the workspace only: the gray bf16 forward at 1x256x256 (K cuts, their slab) from one context
    on two side streams at once."""
    ctx = env.ctx("gray")
    ctx.set_options(0)
    ctx.prepare(_native.BF16)
    _two_streams(env, [ctx, ctx], _native.BF16, 1, 256, 256)


def test_two_contexts_on_two_streams_at_once(env):
    """The same with two contexts, gray and RGB."""
    ctxs = [env.ctx("gray"), env.ctx("rgb")]
    for c in ctxs:
        c.set_options(0)
        c.prepare(_native.BF16)
    _two_streams(env, ctxs, _native.BF16, 1, 256, 256)
