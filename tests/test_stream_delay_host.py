"""CPU: the tables of tests/stream_delay.py against the source they speak about.  The sensitivity twins select a wait by the
method it goes through and the stream it is called on; a refactor that renames or drops one of the seven waits, or moves
what a placement hangs on, must fail here and not silently in the twins."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stream_delay as SD  # noqa: E402

PKG = os.path.join(SD.ROOT, "ai_based_frame_interpolation_amd")


def _code_lines(name):
    """The lines of a package file without their comments."""
    with open(os.path.join(PKG, name)) as f:
        return [re.sub(r"\s+#.*$", "", line.rstrip("\n")) for line in f]


def _count(name, text):
    return sum(line.count(text) for line in _code_lines(name) if not line.lstrip().startswith("#"))


def test_the_tables_are_complete():
    assert len(SD.ORDERINGS) == 7 and len({o.name for o in SD.ORDERINGS}) == 7
    assert [o.file for o in SD.ORDERINGS].count("stream.py") == 5 and [o.file for o in SD.ORDERINGS].count("inference.py") == 2
    assert len({(o.file, o.kind, o.on) for o in SD.ORDERINGS}) == 7   # what skip_wait selects by names one wait each
    for o in SD.ORDERINGS:
        assert o.kind in ("wait_event", "wait_stream", "event_synchronize")
        assert o.placement in (SD.PLACEMENTS if o.case != "host" else SD.HOST_PLACEMENTS) and o.placement != "none"
        assert o.case == "host" or o.case in SD.CASES
        assert (o.case == "host") == (o.file == "inference.py")
    assert set(SD.HOST_PLACEMENTS) <= set(SD.PLACEMENTS)
    assert set(SD.CASES) == {"npy-gray", "y4m-420-rgb", "y4m-scene", "nv12-resize-area", "npy-fps-dedup"}
    assert SD.MAX_DELAY_MS == 200.0 and SD.FLOOR_MS == 10.0
    assert SD.delay_of(1.0) == 10.0 and SD.delay_of(20.0) == 60.0 and SD.delay_of(500.0) == 200.0


@pytest.mark.parametrize("o", SD.ORDERINGS, ids=[o.name for o in SD.ORDERINGS])
def test_each_wait_stands_once_in_its_file(o):
    assert _count(o.file, o.expr) == 1, f"{o.file}: `{o.expr}` must stand there exactly once"
    # the expression goes through the method the twin patches, on the stream (or in the thread) the twin selects
    if o.kind == "event_synchronize":
        assert o.expr.endswith(".synchronize()")
        lines = _code_lines(o.file)
        at = next(i for i, line in enumerate(lines) if o.expr in line)
        owner, scope = None, len(lines[at]) - len(lines[at].lstrip())
        for line in reversed(lines[:at]):   # outwards, one enclosing block at a time: the function the line stands in
            if line.strip() and len(line) - len(line.lstrip()) < scope:
                scope = len(line) - len(line.lstrip())
                m = re.match(r"\s*def (\w+)\(", line)
                if m:
                    owner = m.group(1)
                    break
        assert owner == {"writer": "writer_main", "main": "_run"}[o.on]
    else:
        assert o.expr.startswith(f"{o.on}.{o.kind}(")


@pytest.mark.parametrize("file,text,n", SD.ANCHORS)
def test_what_the_placements_hang_on(file, text, n):
    assert _count(file, text) == n, f"{file}: `{text}` must stand there {n} time(s)"


@pytest.mark.parametrize("file,text", SD.RECORD_STREAMS)
def test_the_record_stream_obligations_exist(file, text):
    assert _count(file, text) == 1


def test_no_other_wait_goes_through_the_patched_methods():
    """A second wait_event on the same stream, or a second Event.synchronize in the same thread, would be skipped along with
    the named one."""
    for file, kind, n in (("stream.py", ".wait_event(", 2), ("stream.py", ".wait_stream(", 1), ("inference.py", ".wait_event(", 2),
                          ("inference.py", ".wait_stream(", 0)):
        assert _count(file, kind) == n, (file, kind)
    sync = [line.strip() for line in _code_lines("stream.py") if re.search(r"\b(ev|up|d_free\[j\]|\w*event\w*)\.synchronize\(\)", line)]
    assert sync == ["ev.synchronize()", "up.synchronize()"]


def test_the_instrument_restores_what_it_patches():
    """Entering and leaving touches no device in mode "run"."""
    from ai_based_frame_interpolation_amd import stream
    before = (torch.cuda.Stream.__dict__["__new__"], torch.cuda.stream, torch.cuda.Stream.wait_event,
              torch.cuda.Stream.wait_stream, torch.cuda.Event.synchronize, stream._run, stream.R_OUT)
    with SD.Instrument("run", "h2d-first", 5.0, skip=SD.skip_wait("run-upload-before-compute"), ring_out=3) as ins:
        assert stream.R_OUT == 3 and stream._run is not before[5] and torch.cuda.stream is not before[1]
        assert ins.skip == SD.Skip("wait_event", "compute", None)
    after = (torch.cuda.Stream.__dict__["__new__"], torch.cuda.stream, torch.cuda.Stream.wait_event,
             torch.cuda.Stream.wait_stream, torch.cuda.Event.synchronize, stream._run, stream.R_OUT)
    assert all(a is b for a, b in zip(before, after))
