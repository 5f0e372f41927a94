"""Injected delays for the package's own multi-stream loops: the orderings as a table and one instrument
(tests/test_gpu_stream_delay.py runs it on the GPU, tests/test_stream_delay_host.py holds the tables against the source).

tests/stream_contract.py proves the C ABI's stream promise and stops there.  Above it the package runs streams of its own:
`stream._run` (three streams, two host threads, rings of pinned slots and device twins) and
`inference.interpolate_sequence_host` (a copy stream against the compute stream).  On clips of a dozen tiny frames every
producer is done microseconds after it was enqueued, so a missing wait gives the right bytes on every run.  The instrument:

  delay(stream, ms)   a kernel that occupies `stream` for about `ms` (torch.cuda._sleep, calibrated once per process with
                      two events; a chain of fill_ on a private buffer where _sleep proves unusable) and touches no data of
                      the package.  Never above MAX_DELAY_MS.
  Instrument          patches, from the test alone, torch.cuda.stream (the context manager under which stream.py and
                      inference.py enqueue their copies), torch.cuda.Stream.__new__ (the creation order inside `_run` names
                      h2d and d2h; the one stream `interpolate_sequence_host` makes is `copy`), the model's forward_* (the
                      compute stream) and `stream._run` (the reader and the sink).  A PLACEMENT puts the delay ahead of a
                      producer, so that a consumer that does not wait runs first and reads stale data.
  skip (skip_wait)    for the sensitivity twins only: one named wait of ORDERINGS becomes a no-op (Stream.wait_event,
                      Stream.wait_stream or Event.synchronize, selected by the stream - or host thread - it is called on,
                      and a call index).  With its attacking placement the output must DIFFER: that is what shows the delay
                      long enough and the instrument not blind.

What is proved and what is not.  For each row of ORDERINGS: with the attacking placement the output is byte for byte the
resident single-stream result, and without that one wait it is not.  A twin skips only a wait that guards a buffer which
lives for the whole run (d_in, d_out, the pinned slots; dbuf / dmid while they are referenced): what it reads is stale but
live memory of this process.  The two `record_stream` obligations (RECORD_STREAMS) have no twin - a twin would have to
hand live memory back to the allocator.  They are covered from the other side only: under `d2h-first` the next chunk
allocates on the compute stream while the delayed copy has not read its source yet, and the bytes must still be right.
That half is proved ONLY AS FAR AS THE CACHING ALLOCATOR REUSES THE BLOCK, which it does for equal sizes on one stream.

Ordering 2 (`h2d.wait_event(d_free[j])`) is a second line of defence at R_OUT = 2: chunk k + 2, the next user of d_in[j],
is enqueued only after the writer thread has freed chunk k's pinned output slot, that is after chunk k's download, which
waited for chunk k's compute.  The host-side ring therefore implies the ordering and no delay can make the lost wait
visible.  Its twin, and the delayed run that stands against it, run with the output ring one slot deeper (`ring_out=3`,
`stream.R_OUT` patched from the test), where that wait is the only thing that orders the two.

One known way to be blind: two torch streams that land on one hardware queue run in order whatever the code does (a
process has 4 hardware queues by default, and torch hands out its pooled streams in turn).  The instrument therefore probes
every stream the call under test makes (`concurrent`: does work on it start while the compute stream, or a stream made
before it, is held busy, and the other way round?) and passes one that does not over for the next of the pool.  A twin that
still reports equal bytes says so with the streams' identities, and is run once more in a fresh child process (`python
tests/stream_delay.py twin NAME`), where the stream-to-queue assignment starts from scratch.

Importing this module needs no GPU."""
import json
import os
import sys
import tempfile
import threading
import time
from collections import Counter, namedtuple

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MAX_DELAY_MS = 200.0      # one delay is bounded
FLOOR_MS = 10.0           # D = 3 x the mean time per chunk of the un-delayed streamed run, at least this
HOST_SLEEP_S = 0.005      # slow-source: per frame read; slow-sink: per chunk written

PLACEMENTS = ("none", "h2d-first", "compute-first", "d2h-first", "slow-source", "slow-sink")
#: interpolate_sequence_host has one copy stream: "h2d-first" is the delay before each upload on it, "d2h-first" the one
#: before each download
HOST_PLACEMENTS = ("none", "h2d-first", "d2h-first", "compute-first")

#: name: the twin's id; file: where the wait stands (under ai_based_frame_interpolation_amd/); expr: the wait as written
#: there, once; kind / on: how skip_wait selects it (the patched method, and the stream - for Event.synchronize the host
#: thread - it is called on); placement: the one that attacks it; case: the case of CASES (or "host") the twin runs;
#: ring_out: stream.R_OUT for the twin and for its delayed run (None: as it is; see the module docstring)
Ordering = namedtuple("Ordering", "name file expr kind on placement case ring_out what")
ORDERINGS = [
    Ordering("run-upload-before-compute", "stream.py", "compute.wait_event(up)", "wait_event", "compute", "h2d-first",
             "npy-gray", None, "upload -> compute reads d_in[j]"),
    Ordering("run-compute-before-reupload", "stream.py", "h2d.wait_event(d_free[j])", "wait_event", "h2d", "compute-first",
             "npy-gray", 3, "compute's last read of d_in[j] -> the next upload into it"),
    Ordering("run-compute-before-download", "stream.py", "d2h.wait_stream(compute)", "wait_stream", "d2h", "compute-first",
             "npy-fps-dedup", None, "compute -> download (d_out[o], the device twin of the pinned slot)"),
    Ordering("run-download-before-write", "stream.py", "ev.synchronize()", "event_synchronize", "writer", "d2h-first",
             "npy-gray", None, "download -> the writer thread reads the pinned slot"),
    Ordering("run-upload-before-refill", "stream.py", "up.synchronize()", "event_synchronize", "main", "h2d-first",
             "npy-gray", None, "upload done -> the reader refills the pinned slot (a fast source)"),
    Ordering("host-upload-before-compute", "inference.py", "compute.wait_event(up_done[i])", "wait_event", "compute",
             "h2d-first", "host", None, "upload of dbuf[i] -> compute reads it"),
    Ordering("host-compute-before-download", "inference.py", "copy.wait_event(comp_done[i])", "wait_event", "copy",
             "compute-first", "host", None, "compute writes dmid[i] -> download"),
]
#: the lines a placement hangs on: (file, text that must stand there, how often)
ANCHORS = [
    ("stream.py", "compute = torch.cuda.current_stream(dev)", 1),
    ("stream.py", "h2d, d2h = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)", 1),   # the creation order
    ("stream.py", "with torch.cuda.stream(h2d):", 1),
    ("stream.py", "with torch.cuda.stream(d2h):", 1),
    ("stream.py", "R_IN, R_OUT = 3, 2", 1),
    ("stream.py", "for _ in range(R_OUT)", 2),            # the pinned output slots and their device twins
    ("stream.py", "def _run(model, route: _Route, reader, write,", 1),
    ("inference.py", "compute, copy = torch.cuda.current_stream(dev), torch.cuda.Stream(device=dev)", 1),
    ("inference.py", "def upload(i):", 1),               # the caller names tell an upload from a download
    ("inference.py", "def download(i):", 1),
    ("inference.py", "with torch.cuda.stream(copy):", 2),
]
#: the obligations without a twin (file, expression)
RECORD_STREAMS = [
    ("stream.py", "rows.record_stream(d2h)"),
    ("inference.py", "dmid[i].record_stream(copy)"),
    ("inference.py", "fr.record_stream(compute)"),
]

_real_stream_ctx = torch.cuda.stream      # (functions: taking them touches no device)
_real_event_sync = torch.cuda.Event.synchronize
STREAM_TRIES = 8                          # streams tried for one that runs beside the others (the pool hands out the next)


# ---- the delay ---------------------------------------------------------------------------------------------------------
_CAL = {}   # device index -> {"kind": "sleep" | "fill", "per_ms": units per millisecond, "buf": the fill chain's buffer}


def _elapsed_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.current_stream().synchronize()
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _fill_chain(buf, n):
    for k in range(n):
        buf.fill_(k & 0xFF)


def calibrate(dev):
    """Once per process and device -> {"kind", "per_ms"}: cycles of torch.cuda._sleep per millisecond, measured with two
    events on a sleep of about 10 ms and checked on one of 20 ms; fills of a private 16 MiB buffer per millisecond where
    that check fails."""
    dev = torch.device(dev)
    idx = dev.index or 0
    if idx in _CAL:
        return _CAL[idx]
    with torch.cuda.device(idx):
        cal = None
        try:
            torch.cuda._sleep(1000)   # (the first launch loads the kernel)
            n = 1_000_000
            t = _elapsed_ms(lambda: torch.cuda._sleep(n))
            for _ in range(4):
                if t >= 5.0:
                    break
                n = int(n * min(max(10.0 / max(t, 1e-3), 2.0), 1000.0))
                t = _elapsed_ms(lambda: torch.cuda._sleep(n))
            per_ms = n / t
            check = _elapsed_ms(lambda: torch.cuda._sleep(int(20 * per_ms)))
            if t >= 5.0 and 12.0 <= check <= 40.0:
                cal = {"kind": "sleep", "per_ms": per_ms, "check_20ms": check}
        except (RuntimeError, AttributeError):
            cal = None
        if cal is None:
            buf = torch.empty(1 << 24, dtype=torch.uint8, device=dev)
            _fill_chain(buf, 50)
            t = _elapsed_ms(lambda: _fill_chain(buf, 2000))
            cal = {"kind": "fill", "per_ms": 2000 / t, "buf": buf}
    _CAL[idx] = cal
    return cal


def delay(stream, ms):
    """Occupy `stream` for about `ms` milliseconds (at most MAX_DELAY_MS): nothing else on it starts before."""
    ms = min(float(ms), MAX_DELAY_MS)
    if ms <= 0:
        return
    cal = calibrate(stream.device)
    with _real_stream_ctx(stream):
        if cal["kind"] == "sleep":
            torch.cuda._sleep(int(ms * cal["per_ms"]))
        else:
            _fill_chain(cal["buf"], max(int(ms * cal["per_ms"]), 1))


def concurrent(a, b, ms=2.0):
    """Does work on one of the two streams start while the other is held busy?  (Both ways round; both are drained first.)
    Two streams that share a hardware queue do not, whatever the code between them waits for."""
    for x, y in ((a, b), (b, a)):
        x.synchronize()
        y.synchronize()
        delay(x, ms)
        ex, ey = torch.cuda.Event(), torch.cuda.Event()
        ex.record(x)
        ey.record(y)
        _real_event_sync(ey)
        ran = not ex.query()
        x.synchronize()
        if not ran:
            return False
    return True


def delay_of(chunk_ms):
    """D for a run whose un-delayed mean time per chunk is chunk_ms: a consumer that does not wait starts at the latest
    when its own stream has drained the previous chunk, which is one chunk's time."""
    return min(max(3.0 * chunk_ms, FLOOR_MS), MAX_DELAY_MS)


# ---- the instrument --------------------------------------------------------------------------------------------------
Skip = namedtuple("Skip", "kind on index")   # index: None (every call) or a set of call indices


def skip_wait(ordering, index=None):
    """The skip of one row of ORDERINGS (by name or the row itself), for Instrument(skip=...)."""
    o = ordering if isinstance(ordering, Ordering) else {r.name: r for r in ORDERINGS}[ordering]
    return Skip(o.kind, o.on, None if index is None else set(index))


class _SlowReader:
    def __init__(self, reader):
        self._r = reader

    def read_into(self, buf, max_frames):
        k = self._r.read_into(buf, max_frames)
        time.sleep(HOST_SLEEP_S * k)
        return k

    def __getattr__(self, name):
        return getattr(self._r, name)


class Instrument:
    """with Instrument(mode, placement, ms, skip=None, model=None, ring_out=None) as ins: <one call of the package>.

    mode "run": a `chunk_frames=` call of a video route (`stream._run`); "host": `interpolate_sequence_host`.  model: the
    model of the call (for `compute-first`).  Afterwards: ins.uploads / ins.downloads (copy contexts entered), ins.delays
    (delays enqueued), ins.skipped (waits made no-ops), ins.calls (Counter of (kind, on)), ins.identities(); ins.tries /
    ins.blind: every stream the call makes is probed (`concurrent`) against the compute stream and the ones made before
    it, and one that does not run beside them is passed over for the next (tries counts them; blind: none was found)."""

    def __init__(self, mode, placement="none", ms=0.0, skip=None, model=None, ring_out=None):
        assert mode in ("run", "host") and placement in PLACEMENTS
        self.mode, self.placement, self.ms, self.skip, self.model, self.ring_out = mode, placement, ms, skip, model, ring_out
        self.created, self.compute = [], None
        self.uploads = self.downloads = self.delays = self.skipped = 0
        self.calls = Counter()
        self.tries, self.blind, self._rejected = 0, False, []   # streams passed over; True: none found that runs beside
        self.probe_ms = 0.0                                     # host time spent finding them
        self._chunk_open = False
        self._active = mode == "host"   # "run": only between the entry and the exit of stream._run
        self._undo = []

    # -- roles
    def _role(self, s):
        if s is None or not self._active:
            return None
        h = s.cuda_stream
        names = ("h2d", "d2h") if self.mode == "run" else ("copy",)
        for name, c in zip(names, self.created):
            if c.cuda_stream == h:
                return name
        if self.compute is not None and self.compute.cuda_stream == h:
            return "compute"
        return None

    def identities(self):
        names = ("h2d", "d2h") if self.mode == "run" else ("copy",)
        out = {name: f"{c.cuda_stream:#x}" for name, c in zip(names, self.created)}
        out["compute"] = None if self.compute is None else f"{self.compute.cuda_stream:#x}"
        return out

    def _delay(self, s):
        delay(s, self.ms)
        self.delays += 1

    def _skips(self, kind, on):
        idx = self.calls[(kind, on)]
        self.calls[(kind, on)] += 1
        sk = self.skip
        if sk is not None and sk.kind == kind and sk.on == on and (sk.index is None or idx in sk.index):
            self.skipped += 1
            return True
        return False

    # -- patches
    def _patch(self, obj, name, new, raw=None):
        old = obj.__dict__[name] if raw else getattr(obj, name)
        self._undo.append((obj, name, old))
        setattr(obj, name, new)

    def __enter__(self):
        from ai_based_frame_interpolation_amd import stream as pkg_stream
        ins = self
        real_new = torch.cuda.Stream.__dict__["__new__"]
        real_wait_event, real_wait_stream = torch.cuda.Stream.wait_event, torch.cuda.Stream.wait_stream
        real_sync, real_run = torch.cuda.Event.synchronize, pkg_stream._run

        def new(cls, device=None, priority=0, **kw):
            s = real_new.__func__(cls, device, priority, **kw)
            if ins._active and "stream_id" not in kw and "stream_ptr" not in kw:   # a new stream, not a handle's wrapper
                # one that runs beside the compute stream and the streams made before it: on a shared hardware queue
                # no delay can let a consumer overtake its producer, and the run would prove nothing
                others = [ins.compute] + ins.created
                t0 = time.perf_counter()
                ok = all(concurrent(o, s) for o in others)
                while not ok and ins.tries < STREAM_TRIES:
                    ins.tries += 1
                    ins._rejected.append(s)
                    s = real_new.__func__(cls, device, priority, **kw)
                    ok = all(concurrent(o, s) for o in others)
                ins.blind = ins.blind or not ok
                ins.probe_ms += (time.perf_counter() - t0) * 1e3
                ins.created.append(s)
            return s

        def stream_ctx(s):
            role = ins._role(s)
            if role in ("h2d", "d2h"):
                ins._copy_context(s, role)
            elif role == "copy":   # interpolate_sequence_host: told apart by the function that opens the context
                caller = sys._getframe(1).f_code.co_name
                assert caller in ("upload", "download"), caller
                ins._copy_context(s, "h2d" if caller == "upload" else "d2h")
            return _real_stream_ctx(s)

        def wait_event(self, event):
            if not ins._skips("wait_event", ins._role(self)):
                real_wait_event(self, event)

        def wait_stream(self, other):
            if not ins._skips("wait_stream", ins._role(self)):
                real_wait_stream(self, other)

        def synchronize(self):
            on = "main" if threading.current_thread() is threading.main_thread() else "writer"
            if not (ins._active and ins.mode == "run" and ins._skips("event_synchronize", on)):
                real_sync(self)

        def run(model, route, reader, write, *a, **k):
            dev = next(model.parameters()).device
            ins.compute, ins.created, ins._active = torch.cuda.current_stream(dev), [], True
            if ins.placement == "slow-source":
                reader = _SlowReader(reader)
            if ins.placement == "slow-sink":
                inner = write

                def write(rows):
                    time.sleep(HOST_SLEEP_S)
                    inner(rows)
            try:
                return real_run(model, route, reader, write, *a, **k)
            finally:
                ins._active = False

        self._patch(torch.cuda.Stream, "__new__", staticmethod(new), raw=True)
        self._patch(torch.cuda, "stream", stream_ctx)
        self._patch(torch.cuda.Stream, "wait_event", wait_event)
        self._patch(torch.cuda.Stream, "wait_stream", wait_stream)
        self._patch(torch.cuda.Event, "synchronize", synchronize)
        self._patch(pkg_stream, "_run", run)
        if self.ring_out is not None:
            self._patch(pkg_stream, "R_OUT", self.ring_out)
        if self.mode == "host":
            self.compute = torch.cuda.current_stream()
        self._forwards = []
        if self.placement == "compute-first":
            assert self.model is not None
            for name in [n for n in dir(self.model) if n.startswith("forward_") and callable(getattr(self.model, n))]:
                setattr(self.model, name, self._delayed_forward(getattr(self.model, name)))
                self._forwards.append(name)
        return self

    def _copy_context(self, s, which):
        if which == "h2d":
            self.uploads += 1
            self._chunk_open = True
        else:
            self.downloads += 1
        if self.placement == which + "-first":
            self._delay(s)

    def _delayed_forward(self, fwd):
        def forward(*a, **k):
            # "run": once per chunk, ahead of the first forward behind its upload; "host": one forward per chunk
            if self._active and (self.mode == "host" or self._chunk_open):
                self._chunk_open = False
                self._delay(torch.cuda.current_stream())
            return fwd(*a, **k)
        return forward

    def __exit__(self, *exc):
        for name in self._forwards:
            delattr(self.model, name)
        for obj, name, old in reversed(self._undo):
            setattr(obj, name, old)
        self._undo = []
        self._active = False
        return False


# ---- the cases -------------------------------------------------------------------------------------------------------
N_FRAMES, BATCH, CHUNK = 11, 2, 2    # five chunks and a last one: both d_in twins and every pinned slot at least twice
HOST_FRAMES = 9
SCENE_THR = 10.0


def clip(n, row_shape, bits, seed, cuts=(), repeats=()):
    """n frames of `row_shape` samples: a random picture with small frame-to-frame noise, a new picture after each
    interval in `cuts`; a frame in `repeats` is a copy of the one before."""
    rng = np.random.default_rng(seed)
    hi, dt = (256, np.uint8) if bits == 8 else (1024, np.uint16)
    base = rng.integers(0, hi, row_shape)
    out = []
    for i in range(n):
        if i - 1 in cuts:
            base = rng.integers(0, hi, row_shape)
        out.append(out[-1] if i in repeats else np.clip(base + rng.integers(-3, 4, row_shape), 0, hi - 1).astype(dt))
    return np.stack(out)


def _write_y4m(path, n, h, w, tag, bits, seed, cuts=()):
    from ai_based_frame_interpolation_amd import imageio_lite as IO
    hdr = IO._y4m_stream_header(IO._y4m_header_line(w, h, (24, 1), tag, None, bits), bits)
    with IO.Y4MWriter(path, w, h, (24, 1), tag, None, bits=bits) as wr:
        wr.write(clip(n, (hdr["frame_samples"],), bits, seed, cuts))


def _npy_gray(path):
    np.save(path, clip(N_FRAMES, (32, 48), 8, 1))


def _y4m_rgb(path):
    _write_y4m(path, N_FRAMES, 32, 48, "420jpeg", 8, 2)


def _y4m_scene(path):
    # chunks hold intervals 0-1, 2-3, ...: cut 3 is a chunk's last interval (scored with the lookahead frame), 6 a first
    _write_y4m(path, N_FRAMES, 32, 48, "420p10", 10, 3, cuts=(3, 6))


def _nv12(path):
    clip(N_FRAMES, (46 * 70 * 3 // 2,), 8, 4).tofile(path)


def _npy_dedup(path):
    np.save(path, clip(N_FRAMES, (32, 48), 8, 5, repeats=(4, 8, 9)))


def _call_npy(model, src, dst, cf):
    from ai_based_frame_interpolation_amd import stream
    return stream.interpolate_npy_stream(model, src, dst, 2, batch=BATCH, chunk_frames=cf)


def _call_y4m(model, src, dst, cf):
    from ai_based_frame_interpolation_amd import stream
    return stream.interpolate_y4m_stream(model, src, dst, 2, batch=BATCH, chunk_frames=cf)


def _call_scene(model, src, dst, cf):
    from ai_based_frame_interpolation_amd import stream
    return stream.interpolate_y4m_stream(model, src, dst, 2, batch=BATCH, chunk_frames=cf, scene_cut=SCENE_THR)


def _call_nv12(model, src, dst, cf):
    from ai_based_frame_interpolation_amd import stream
    return stream.interpolate_raw_stream(model, src, dst, 2, raw="nv12", width=70, height=46, batch=BATCH, chunk_frames=cf,
                                         src_fps=24, resize=(22, 18), resize_filter="area")


def _call_dedup(model, src, dst, cf):
    from ai_based_frame_interpolation_amd import stream
    # max_gap 2: one lookahead frame, so that 11 frames are five chunks (max_gap 4 reads three ahead: four chunks); the run
    # of two dead intervals 7-8-9 is longer than that and stays as it is, the single one 3-4 is re-timed
    return stream.interpolate_npy_stream(model, src, dst, batch=BATCH, chunk_frames=cf, fps=60, src_fps=24, dedup=0,
                                         max_gap=2)


#: name -> (model variant of stream_contract.VARIANTS, precision, file extensions (in, out), write the source, the call)
Case = namedtuple("Case", "variant precision ext_in ext_out make call")
CASES = {
    "npy-gray": Case("gray", "bf16", ".npy", ".npy", _npy_gray, _call_npy),
    "y4m-420-rgb": Case("rgb", "bf16", ".y4m", ".y4m", _y4m_rgb, _call_y4m),
    "y4m-scene": Case("gray", "fp16", ".y4m", ".y4m", _y4m_scene, _call_scene),
    "nv12-resize-area": Case("rgb", "bf16", ".nv12", ".nv12", _nv12, _call_nv12),
    "npy-fps-dedup": Case("gray", "bf16", ".npy", ".npy", _npy_dedup, _call_dedup),
}

Prepared = namedtuple("Prepared", "src want n_want chunk_ms D")
Result = namedtuple("Result", "n data wall_ms ins alive")


def differing(a, b):
    """How many bytes of two byte strings differ (a length difference counts byte for byte)."""
    k = min(len(a), len(b))
    x, y = np.frombuffer(a, np.uint8, k), np.frombuffer(b, np.uint8, k)
    return int((x != y).sum()) + abs(len(a) - len(b))


class Bench:
    """One process's models, source clips, resident results and measured delays (each made once, on first use)."""

    def __init__(self, dev, tmp):
        self.dev, self.tmp = torch.device(dev), str(tmp)
        self._models, self._prepared, self._host, self._k = {}, {}, None, 0

    def model(self, variant, precision):
        if (variant, precision) not in self._models:
            import ai_based_frame_interpolation_amd as P
            import stream_contract as SC
            from oracle import unet_oracle as O
            seed, cf, bil = SC.VARIANTS[variant]
            m = P.FrameInterpolationUNet(bilinear=bil, frame_channels=cf, precision=precision)
            m.load_state_dict(O.make_seeded_state_dict(seed, n_channels=2 * cf, n_classes=cf, bilinear=bil))
            self._models[(variant, precision)] = m.to(self.dev).eval()
        return self._models[(variant, precision)]

    def case_model(self, name):
        return self.model(CASES[name].variant, CASES[name].precision)

    def _out(self, name):
        self._k += 1
        return os.path.join(self.tmp, f"{name}-{self._k}{CASES[name].ext_out}")

    def run(self, name, chunk_frames=CHUNK, placement="none", ms=0.0, skip=None, ring_out=None):
        """One call of case `name` under the instrument -> Result (data: the output file's bytes; alive: the names of the
        threads it started that a join with a timeout did not end)."""
        case, model, dst = CASES[name], self.case_model(name), self._out(name)
        src = os.path.join(self.tmp, name + case.ext_in)
        if not os.path.exists(src):
            case.make(src)
        before = set(threading.enumerate())
        with Instrument("run", placement, ms, skip, model, ring_out) as ins:
            t0 = time.perf_counter()
            n = case.call(model, src, dst, chunk_frames)
            wall = (time.perf_counter() - t0) * 1e3 - ins.probe_ms
        started = [t for t in threading.enumerate() if t not in before]
        for t in started:
            t.join(timeout=5.0)
        with open(dst, "rb") as f:
            data = f.read()
        os.remove(dst)
        return Result(n, data, wall, ins, [t.name for t in started if t.is_alive()])

    def prepared(self, name):
        """The resident bytes of the case (chunk_frames=None: `_run_whole`, one stream, no threads) and its D, from one
        un-delayed streamed run."""
        if name not in self._prepared:
            calibrate(self.dev)
            ref = self.run(name, chunk_frames=None)
            base = self.run(name)
            chunk_ms = base.wall_ms / max(base.ins.uploads, 1)
            src = os.path.join(self.tmp, name + CASES[name].ext_in)
            self._prepared[name] = Prepared(src, ref.data, ref.n, chunk_ms, delay_of(chunk_ms))
        return self._prepared[name]

    # -- interpolate_sequence_host
    def host_prepared(self):
        """-> (model, frames [9, 32, 48] uint8 on the host, interpolate_sequence(model, frames.cuda()).cpu(), D)."""
        if self._host is None:
            import ai_based_frame_interpolation_amd as P
            calibrate(self.dev)
            model = self.model("gray", "bf16")
            frames = torch.from_numpy(clip(HOST_FRAMES, (32, 48), 8, 6))
            want = P.interpolate_sequence(model, frames.to(self.dev), batch=BATCH).cpu()
            res = self.host_run(model, frames)
            chunk_ms = res.wall_ms / max(res.ins.uploads, 1)
            self._host = (model, frames, want, delay_of(chunk_ms))
        return self._host

    def host_run(self, model, frames, out=None, placement="none", ms=0.0, skip=None):
        import ai_based_frame_interpolation_amd as P
        before = set(threading.enumerate())
        with Instrument("host", placement, ms, skip, model) as ins:
            t0 = time.perf_counter()
            got = P.interpolate_sequence_host(model, frames, batch=BATCH, out=out)
            wall = (time.perf_counter() - t0) * 1e3 - ins.probe_ms
        alive = [t.name for t in threading.enumerate() if t not in before and t.is_alive()]
        return Result(got.shape[0], got, wall, ins, alive)

    # -- the sensitivity twins
    def twin(self, name):
        """The run of ORDERINGS row `name` with its attacking placement and that one wait a no-op -> a dict: "differing"
        (bytes, or elements, that differ from the resident result - must not be 0), "D", "streams", "skipped"."""
        o = {r.name: r for r in ORDERINGS}[name]
        if o.case == "host":
            model, frames, want, D = self.host_prepared()
            res = self.host_run(model, frames, placement=o.placement, ms=D, skip=skip_wait(o))
            diff = int((res.data != want).sum())
        else:
            prep = self.prepared(o.case)
            D = prep.D
            res = self.run(o.case, placement=o.placement, ms=D, skip=skip_wait(o), ring_out=o.ring_out)
            diff = differing(res.data, prep.want)
        return {"twin": name, "differing": diff, "D": round(D, 2), "streams": res.ins.identities(),
                "blind": res.ins.blind, "streams_passed_over": res.ins.tries, "skipped": res.ins.skipped,
                "delays": res.ins.delays, "alive": res.alive}


def twin_in_child(name, timeout=120):
    """`Bench.twin(name)` in a fresh child process (its own stream-to-queue assignment) -> the dict it printed."""
    import subprocess
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "twin", name], capture_output=True, text=True,
                         cwd=ROOT, env=env, timeout=timeout)
    assert res.returncode == 0, res.stderr[-2000:]
    return json.loads(res.stdout.strip().splitlines()[-1])


def _main(argv):
    if len(argv) != 3 or argv[1] != "twin" or argv[2] not in {o.name for o in ORDERINGS}:
        print("usage: stream_delay.py twin " + " | ".join(o.name for o in ORDERINGS), file=sys.stderr)
        return 2
    with tempfile.TemporaryDirectory() as tmp:
        print(json.dumps(Bench("cuda:0", tmp).twin(argv[2])))
    return 0


if __name__ == "__main__":
    sys.exit(_main(sys.argv))
