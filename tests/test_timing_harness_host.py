"""CPU: the measurement protocol of the timing tools (tools/timing_harness.py) with the device taken out:
the order of warm-up and timed calls, what the host-clock loop synchronises and keeps, the arithmetic of a summary, the
in-memory clip, the report file - and every `tools/*_timing.py` imports without a GPU and has a `main`."""
import glob
import importlib
import json
import os
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.insert(0, TOOLS)

import timing_harness as H  # noqa: E402

TIMING_TOOLS = sorted(os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*_timing.py")))


def test_rotate_walks_the_set_in_order():
    seen = []
    fn = H.Rotate(seen.append, 3)
    for _ in range(7):
        fn()
    assert seen == [0, 1, 2, 0, 1, 2, 0]


def _recorded(monkeypatch, **kw):
    """interleaved() over three fake cases with device_ms replaced: -> (the log of events, its result)."""
    log = []

    def fake_device_ms(fn, iters):
        log.append(("timed", fn.name, iters))
        return float(len(log))

    def case(name):
        def fn():
            log.append(("call", name))
        fn.name = name
        return fn
    monkeypatch.setattr(H, "device_ms", fake_device_ms)
    monkeypatch.setattr(H, "synchronize", lambda device=None: log.append(("sync",)))
    ms = H.interleaved({k: case(k) for k in "abc"}, **kw)
    return log, ms


def test_interleaved_warms_every_case_up_then_times_in_rounds(monkeypatch):
    log, ms = _recorded(monkeypatch, warmup=2, reps=4, iters=5)
    first_timed = next(i for i, e in enumerate(log) if e[0] == "timed")
    assert log[:first_timed] == [("call", k) for k in "abc" for _ in range(2)] + [("sync",)]
    assert log[first_timed:] == [("timed", k, 5) for _ in range(4) for k in "abc"]
    assert list(ms) == ["a", "b", "c"] and all(len(v) == 4 for v in ms.values())
    assert ms["a"] == [8.0, 11.0, 14.0, 17.0]   # the recorder's values, untouched, in the order they were taken


def test_interleaved_honours_iters_per_case(monkeypatch):
    log, ms = _recorded(monkeypatch, warmup=1, reps=2, iters={"a": 200, "b": 20, "c": 3})
    assert [e for e in log if e[0] == "timed"] == [("timed", "a", 200), ("timed", "b", 20), ("timed", "c", 3)] * 2
    assert all(len(v) == 2 for v in ms.values())


def test_interleaved_graph_captures_each_case_and_divides_by_its_calls(monkeypatch):
    captured = []

    class FakeGraph:
        def __init__(self, fn, iters):
            self.name, self.iters = fn.name, iters
            self.replay = lambda: log.append(("replay", self.name))
            self.replay.name = fn.name

    def fake_graph_of(fn, iters):
        captured.append((fn.name, iters, len(log)))
        return FakeGraph(fn, iters)
    log = []

    def fake_device_ms(fn, iters):
        log.append(("timed", fn.name, iters))
        return 60.0                                            # ms per replay

    def case(name):
        def fn():
            log.append(("call", name))
        fn.name = name
        return fn
    monkeypatch.setattr(H, "graph_of", fake_graph_of)
    monkeypatch.setattr(H, "device_ms", fake_device_ms)
    monkeypatch.setattr(H, "synchronize", lambda device=None: log.append(("sync",)))
    ms = H.interleaved({k: case(k) for k in "ab"}, warmup=1, reps=3, iters={"a": 20, "b": 5}, graph=True, replays=7)
    warm = [("call", "a"), ("call", "b"), ("sync",)]
    assert captured == [("a", 20, len(warm)), ("b", 5, len(warm))]         # captured after the warm-up, with its own count
    assert log[:len(warm) + 3] == warm + [("replay", "a"), ("replay", "b"), ("sync",)]   # one untimed replay of each
    assert log[len(warm) + 3:] == [("timed", k, 7) for _ in range(3) for k in "ab"]      # `replays` replays per timing
    assert ms == {"a": [3.0] * 3, "b": [12.0] * 3}                         # ms per call: per replay / calls in the graph


def test_protocol_sentence():
    assert H.protocol(warmup=3, reps=7, iters=200, set_gb=1.0) == (
        "HIP events, 3 warm-up calls per case, median of 7 interleaved reps of 200 calls rotating over a set of at least 1.0 GB")
    assert H.protocol(warmup=3, reps=5, iters="10 (1080p) / 200 (256x256)", what="forwards") == (
        "HIP events, 3 warm-up forwards per case, median of 5 interleaved reps of 10 (1080p) / 200 (256x256) forwards")
    assert H.protocol(warmup=2, reps=5, iters=20, replays=10, set_gb=1.0, wall_reps=5) == (
        "HIP events, 2 warm-up calls per case, median of 5 interleaved reps of 10 replays of a graph of 20 calls rotating "
        "over a set of at least 1.0 GB; streamed: host clock behind a device synchronise on either side, one untimed round, "
        "median of 5 interleaved runs")


def test_interleaved_wall_one_untimed_round_then_synchronised_rounds(monkeypatch):
    log, now = [], [0.0]

    def clock():
        log.append("clock")
        return now[0]

    def run(name, cost):
        def fn():
            log.append(name)
            now[0] += cost
            return name.upper()
        return fn
    monkeypatch.setattr(H, "clock", clock)
    monkeypatch.setattr(H, "synchronize", lambda device=None: log.append("sync"))
    results = {}
    secs = H.interleaved_wall({"a": run("a", 2.0), "b": run("b", 0.5)}, reps=3, results=results)
    timed = lambda k: ["sync", "clock", k, "sync", "clock"]  # noqa: E731
    assert log == ["a", "b"] + (timed("a") + timed("b")) * 3
    assert secs == {"a": [2.0, 2.0, 2.0], "b": [0.5, 0.5, 0.5]}
    assert results == {"a": "A", "b": "B"}


def test_summary_and_pair_spread():
    assert H.summary([3.0, 1.0, 2.0, 10.0]) == (2.5, 1.0, 10.0)
    assert H.summary([4.0]) == (4.0, 4.0, 4.0)
    assert H.pair_spread(2.0, 2.0) == 0.0
    assert H.pair_spread(90.0, 100.0) == H.pair_spread(100.0, 90.0) == pytest.approx(0.1)


def test_memory_clip_wraps_its_members_and_ends():
    members, frame_bytes, frames = bytes(range(10)), 5, 5      # two frames held, five served: 25 bytes
    clip = H.MemoryClip(members, frame_bytes, frames)
    buf, got = bytearray(8), []
    while True:
        n = clip.readinto(buf)
        if n == 0:
            break
        assert n <= len(buf)
        got.append(bytes(buf[:n]))
    assert got[1] == bytes([8, 9])                            # a read stops at the wrap of the members ...
    assert got[2] == bytes(range(8))                          # ... and the next one starts at their first byte
    assert b"".join(got) == (members * 3)[:frames * frame_bytes]
    assert clip.readinto(buf) == 0


def test_report_writes_as_it_goes(tmp_path, capsys):
    path = tmp_path / "sub" / "report.txt"
    report = H.Report(str(path))
    report.say("first")
    report.say("second")
    assert path.read_text() == "first\nsecond\n"              # before finish(): a run ended here leaves both lines
    res = {"kernels": {"a": {"ms": 1.5, "spread_ms": [1.0, 2.0]}}, "protocol": H.protocol(warmup=3, reps=7, iters=200)}
    report.finish(res)
    lines = path.read_text().splitlines()
    assert lines[:2] == ["first", "second"] and json.loads(lines[-1]) == res
    assert capsys.readouterr().out.splitlines() == lines


def test_report_appends_to_an_earlier_file_only_when_asked(tmp_path):
    path = tmp_path / "legs.txt"
    H.Report(str(path)).say("leg 1")
    H.Report(str(path), append=True).say("leg 2")
    assert path.read_text() == "leg 1\nleg 2\n"
    H.Report(str(path)).say("alone")
    assert path.read_text() == "alone\n"


def test_report_without_a_path_writes_no_file(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    report = H.Report(None)
    report.say("only printed")
    report.finish({"a": 1})
    assert capsys.readouterr().out == 'only printed\n{"a": 1}\n'
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("tool", TIMING_TOOLS)
def test_timing_tool_imports_without_a_gpu(tool):
    assert callable(importlib.import_module(tool).main)


def test_the_timing_tools_are_found():
    assert len(TIMING_TOOLS) >= 17 and {"wire10_timing", "dedup_timing", "flow_timing", "stream_timing"} <= set(TIMING_TOOLS)
