"""GPU (MI355X): the package's own multi-stream loops under injected delays (tests/stream_delay.py has the instrument, the
orderings and what is and is not proved).

  1. `stream._run` (every `chunk_frames=` call of the video routes): five cases x six placements.  A delay kernel sits on
     h2d, on the compute stream or on d2h ahead of each chunk's producer (or the source / the sink is slow on the host), and
     the output file is byte for byte what the resident route of the same call (`chunk_frames=None`, `_run_whole`: one
     stream, no threads; tied to the oracles by the routes' own files) writes; so is the frame count, and no thread is left.
     The delay D is 3 x the mean time per chunk of the case's un-delayed streamed run (at least 10 ms, at most 200 ms);
     every run prints it.  One more run stands against ordering 2 with the output ring one slot deeper.
  2. `interpolate_sequence_host`: pageable / pinned source, with / without a caller's pinned `out`, a delay on the copy
     stream before each upload, before each download, on the compute stream before each chunk: bit for bit
     `interpolate_sequence(model, frames.cuda()).cpu()`.
  3. callers on a side stream while the default stream is held busy by a long delay: the video routes (streamed and
     resident), `interpolate_sequence`, `GraphedForward`, `InterpolationService.interpolate` - bit for bit the same call on
     an idle default stream.  Work that strays to the default stream arrives late and the test sees stale bytes.
  4. the sensitivity twins: each of the seven waits of `stream_delay.ORDERINGS` made a no-op under the placement that
     attacks it - the output must DIFFER.  A twin that reports equal bytes means the instrument is blind for that
     ordering: it says so with the streams' identities and is run once more in a fresh child process.

The two `record_stream` obligations have no twin (stream_delay.RECORD_STREAMS).  They are covered from the other side:
under `d2h-first` (a delay before each download) the next chunk allocates on the compute stream while the delayed copy
has not read its source yet, and the bytes must still be right.  This half is proved only as far as the caching allocator
reuses the block, which it does for equal sizes on one stream."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_delay as SD  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    b = SD.Bench("cuda:0", tmp_path_factory.mktemp("stream_delay"))
    cal = SD.calibrate(b.dev)
    print(f"\nstream_delay: {cal['kind']} units per ms = {cal['per_ms']:.1f}")
    return b


def _check_run(res, prep, what):
    assert not res.alive, f"{what}: threads still alive after the run: {res.alive}"
    assert res.n == prep.n_want, f"{what}: {res.n} frames, the resident run wrote {prep.n_want}"
    assert len(res.data) == len(prep.want) and res.data == prep.want, \
        f"{what}: {SD.differing(res.data, prep.want)} of {len(prep.want)} bytes differ from the resident run's"


# ---- 1. stream._run ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", SD.PLACEMENTS)
@pytest.mark.parametrize("case", list(SD.CASES))
def test_delayed_stream_equals_resident(bench, case, placement):
    prep = bench.prepared(case)
    res = bench.run(case, placement=placement, ms=prep.D)
    print(f"\n{case} / {placement}: D = {prep.D:.1f} ms (chunk {prep.chunk_ms:.2f} ms), {res.ins.uploads} chunks, "
          f"{res.ins.delays} delays, {res.wall_ms:.0f} ms, streams {res.ins.identities()}, {res.ins.tries} passed over"
          f"{', BLIND: no stream found that runs beside the others' if res.ins.blind else ''}")
    assert res.ins.uploads >= 5 and res.ins.downloads == res.ins.uploads
    if placement in ("h2d-first", "d2h-first"):
        assert res.ins.delays == res.ins.uploads
    elif placement == "compute-first":   # (a last chunk of one frame has no forward)
        assert res.ins.delays >= 5
    else:
        assert res.ins.delays == 0
    _check_run(res, prep, f"{case} under {placement}")


def test_deeper_output_ring_relies_on_d_free(bench):
    """Ordering 2 where the host-side ring does not already imply it (stream_delay's docstring): with three pinned output
    slots chunk k + 2 is enqueued while chunk k still computes, and `h2d.wait_event(d_free[j])` alone keeps its upload
    out of d_in[j]."""
    o = {r.name: r for r in SD.ORDERINGS}["run-compute-before-reupload"]
    prep = bench.prepared(o.case)
    res = bench.run(o.case, placement=o.placement, ms=prep.D, ring_out=o.ring_out)
    print(f"\n{o.case} / {o.placement} / R_OUT = {o.ring_out}: D = {prep.D:.1f} ms, {res.ins.delays} delays")
    assert res.ins.delays >= 5
    _check_run(res, prep, f"{o.case} under {o.placement} with R_OUT = {o.ring_out}")


# ---- 2. interpolate_sequence_host ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("placement", SD.HOST_PLACEMENTS)
@pytest.mark.parametrize("pinned_src,own_out", [(False, False), (True, False), (False, True), (True, True)])
def test_delayed_host_sequence_equals_device_sequence(bench, pinned_src, own_out, placement):
    model, frames, want, D = bench.host_prepared()
    src = frames.clone().pin_memory() if pinned_src else frames.clone()
    out = torch.empty((2 * frames.shape[0] - 1,) + tuple(frames.shape[1:]), dtype=torch.uint8).pin_memory() if own_out else None
    if out is not None:
        out.fill_(0xFF)
    res = bench.host_run(model, src, out=out, placement=placement, ms=D)
    print(f"\nhost sequence / {placement}: D = {D:.1f} ms, {res.ins.uploads} chunks, {res.ins.delays} delays")
    assert res.ins.uploads == res.ins.downloads == 4
    assert res.ins.delays == (0 if placement == "none" else 4)
    assert out is None or res.data is out
    assert res.data.is_pinned() and torch.equal(res.data, want), \
        f"{int((res.data != want).sum())} of {want.numel()} samples differ from interpolate_sequence on the device"


# ---- 3. callers on a side stream, the default stream busy ----------------------------------------------------------------
def _on_side_stream(bench, ms, fn, setup=None):
    """fn() inside `with torch.cuda.stream(side)` behind a delay of `ms` on the default stream -> its result.  setup: what
    has to run on the side stream before the delay is queued (a graph capture synchronises the device, which would wait
    the delay out and leave the default stream idle for the calls behind it); fn then takes its result."""
    dev = bench.dev
    torch.cuda.synchronize(dev)
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        state = None if setup is None else setup()
        SD.delay(torch.cuda.default_stream(dev), ms)
        got = fn() if setup is None else fn(state)
        side.synchronize()
    busy = not torch.cuda.default_stream(dev).query()
    print(f"\nside stream {side.cuda_stream:#x}: the default stream was {'still busy' if busy else 'idle again'} at the end "
          f"({ms:.0f} ms queued)")
    torch.cuda.synchronize(dev)
    return got


@pytest.mark.parametrize("chunk_frames", [SD.CHUNK, None], ids=["streamed", "resident"])
@pytest.mark.parametrize("case", ["npy-gray", "y4m-420-rgb"])
def test_video_route_on_a_side_stream(bench, case, chunk_frames):
    prep = bench.prepared(case)   # (made on the idle default stream)
    res = _on_side_stream(bench, min(5 * prep.D, SD.MAX_DELAY_MS), lambda: bench.run(case, chunk_frames=chunk_frames))
    _check_run(res, prep, f"{case} on a side stream")


def test_sequence_on_a_side_stream(bench):
    model, frames, want, D = bench.host_prepared()
    d = frames.to(bench.dev)
    got = _on_side_stream(bench, min(5 * D, SD.MAX_DELAY_MS), lambda: P.interpolate_sequence(model, d, batch=SD.BATCH).cpu())
    assert torch.equal(got, want)


def test_graphed_forward_and_service_on_a_side_stream(bench):
    dev = bench.dev
    model = bench.model("gray", "bf16")
    pairs = [tuple(t.to(dev) for t in O.make_frames(seed, 1, 64, 96)) for seed in (41, 42)]
    rng = np.random.default_rng(7)
    a, b = (rng.integers(0, 256, (64, 96), dtype=np.uint8) for _ in range(2))
    with torch.no_grad():
        want = [model(f1, f2).clone() for f1, f2 in pairs]
    svc_want = P.InterpolationService(model=model, device="cuda:0", target_size=None).interpolate(a, b, 2, 30)["frames"]
    torch.cuda.synchronize(dev)

    # the graph is captured on the side stream, then the default stream is held busy, then the two calls replay it
    got = _on_side_stream(bench, SD.MAX_DELAY_MS, lambda g: [g(f1, f2).clone() for f1, f2 in pairs],
                          setup=lambda: P.GraphedForward(model, 1, 64, 96))
    assert not torch.equal(want[0], want[1])
    for g, w in zip(got, want):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))

    svc = P.InterpolationService(model=model, device="cuda:0", target_size=None)
    # (its first request, the other way round, captures the service's graph on the side stream)
    frames = _on_side_stream(bench, SD.MAX_DELAY_MS, lambda _: svc.interpolate(a, b, 2, 30)["frames"],
                             setup=lambda: svc.interpolate(b, a, 2, 30))
    assert len(frames) == len(svc_want) == 4
    for g, w in zip(frames, svc_want):
        assert np.array_equal(g, w)


# ---- 4. the sensitivity twins ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [o.name for o in SD.ORDERINGS])
def test_twin_without_the_wait_differs(bench, name):
    rep = bench.twin(name)
    print(f"\ntwin {name}: {rep}")
    assert not rep["alive"], rep
    # (ordering 2 has no event to wait for in the first two chunks)
    assert rep["skipped"] >= 3 and rep["delays"] >= 4, f"the twin did not take the wait out, or placed no delay: {rep}"
    if rep["differing"] == 0:
        # blind in this process: the streams may share a hardware queue, which runs them in order whatever the code does
        print(f"twin {name}: equal bytes in this process (streams {rep['streams']}, D = {rep['D']} ms): the instrument is "
              "blind here; once more in a fresh child process")
        rep = SD.twin_in_child(name)
        print(f"twin {name} in a fresh process: {rep}")
    assert rep["differing"] > 0, (f"twin {name}: without its wait the output still equals the resident bytes - the "
                                  f"instrument does not see this ordering (streams {rep['streams']}, D = {rep['D']} ms)")
