"""GPU (MI355X): the video routes on combinations of their options, one case per row of tests/video_matrix.py (the full
product of rate x retime x scene_cut x dedup on gray .npy, a pairwise cover of all axes over every source, the pinned
rows).  Every comparison is exact: the bytes written and the returned frame count.  No tolerance anywhere.

  chunk invariance  the row resident (chunk_frames None) and streamed at chunk_frames 1, 3 and 5 (dedup: max_gap + 1 too)
                    writes the same bytes and returns the same count; `scene_log` and `dedup_log`, concatenated over the
                    chunks, are the resident run's (and the host definitions' of tests/scene_ref.py, tests/dedup_ref.py).
                    The first row of each Y4M and raw source reads its chunk_frames 3 run from a pipe (a .npy stack is
                    memory-mapped from a path: it has no pipe).
  reduction         one feature is peeled off at a time - packing, then resize, then chroma "motion", then batch 2 - and
                    the resident result equals the resident result of the row without it, on input prepared as that
                    feature's contract says: the yuv422p10le route on the unpacked clip, packed again on the host
                    (tests/wire10_ref.py); the call without `resize` on the clip resized on the device beforehand
                    (`resize.resize_frames`); for chroma the luma of every frame and every frame that is a copy of a source
                    frame; batch 8.  Each peeled row is the next comparison's base.
  definition        what is left (no packing, resize or chroma "motion"; a row with a plan: fps or dedup) equals the numpy
                    references tests/retime_ref.py, tests/dedup_ref.py and tests/retime_motion_ref.py (`dedup_entries`,
                    `warp_rows` over the device's own flows) applied to the frames that the public factor = G run of the
                    same clip with the same scene_cut writes.  Because every row is peeled down to this, a row with a
                    resize, a packing or chroma "motion" is held to the definition too, through its reductions.

A failure names the row, the chunk size, the first differing output frame and the chunk edge nearest to it.  Models come
from one module-scoped cache, grids (the factor = G runs) from another; all runs are in one process.

measured on an MI355X: the whole file (171 cases) 16 s; the first case 0.7 s (it loads the first model), the cases with a
resize, a packing or retime "motion" 0.1 - 0.35 s, every other case 0.03 - 0.1 s (23 frames of 32 x 32: a run is a few
milliseconds, so all chunk sizes and the full clip stay)
"""
import os
import sys
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as D  # noqa: E402
import retime_motion_ref as RM  # noqa: E402
import retime_ref as RR  # noqa: E402
import test_gpu_dedup_video as DV  # noqa: E402
import video_matrix as M  # noqa: E402
import wire10_ref as W10  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import layout  # noqa: E402
from ai_based_frame_interpolation_amd import optical_flow as OF  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
RS = P.resize
ROWS = M.rows()
#: the first row of each source that can come from a pipe reads its chunk_frames 3 run from one
PIPED = {}
for _r in ROWS:
    if not _r.source.startswith("npy") and _r.clip == "main":
        PIPED.setdefault(_r.source, _r)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    cache = {}

    def get(fc, precision):
        if (fc, precision) not in cache:
            m = P.FrameInterpolationUNet(bilinear=True, frame_channels=fc, precision=precision)
            m.load_state_dict(O.make_seeded_state_dict(1234) if fc == 1 else
                              O.make_seeded_state_dict(77, n_channels=6, n_classes=3))
            cache[(fc, precision)] = m.to(dev).eval()
        return cache[(fc, precision)]
    yield get
    cache.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def grids():
    """{(source, frames' bytes, G, scene_cut, precision): the frames of the public factor = G run}: computed once, shared
    by the rows that need it, never changed."""
    return {}


# ---- one public call ------------------------------------------------------------------------------------------------------
class _Run:
    def __init__(self, n, data, scene_log, dedup_log):
        self.n, self.data, self.scene_log, self.dedup_log = n, data, scene_log, dedup_log


def _fi(dev, models, row):
    return P.FrameInterpolator(model=models(M.SOURCES[row.source][1], row.precision), device=dev, batch=row.batch)


def _call(dev, models, tmp_path, row, frames, chunk, name, pipe=False, size=None, **override):
    """`interpolate_video` of the row on `frames` (of `size`, where that is not the row's source size) -> _Run (the bytes
    of the output file)."""
    src, ext, skw = M.write_source(row, frames, str(tmp_path / f"{name}-in"), size)
    factor, kw = M.call_keywords(row)
    if "factor" in override:
        factor = override.pop("factor")
    kw.update(override)
    dst = str(tmp_path / f"{name}-out{ext}")
    slog, dlog = [], []
    logs = dict(scene_log=slog) if kw.get("scene_cut") is not None else {}
    if kw.get("dedup") is not None:
        logs["dedup_log"] = dlog
    fi = _fi(dev, models, row)
    if not pipe:
        n = fi.interpolate_video(src, dst, factor, chunk_frames=chunk, **skw, **kw, **logs)
    else:
        data = open(src, "rb").read()
        rd, wr = os.pipe()

        def feed():
            with os.fdopen(wr, "wb") as f:
                try:
                    for i in range(0, len(data), 1000):   # (pieces that are no whole frames)
                        f.write(data[i:i + 1000])
                except BrokenPipeError:                   # (the reader failed: its error is the one to report)
                    pass
        t = threading.Thread(target=feed)
        t.start()
        try:
            with os.fdopen(rd, "rb") as f:
                n = fi.interpolate_video(f, dst, factor, chunk_frames=chunk, **skw, **kw, **logs)
        finally:
            t.join()
    assert not os.path.exists(dst + ".part")
    out = _Run(n, open(dst, "rb").read(), slog, dlog)
    os.remove(dst)
    os.remove(src)
    return out


def _decode(row, data, tmp_path, size=None):
    path = str(tmp_path / ("decode" + {"npy": ".npy"}.get(row.source[:3], ".bin")))
    with open(path, "wb") as f:
        f.write(data)
    try:
        return M.read_output(row, path, size)
    finally:
        os.remove(path)


def _first_difference(got, want):
    n = min(got.shape[0], want.shape[0])
    bad = [j for j in range(n) if got[j].shape != want[j].shape or not np.array_equal(got[j], want[j])]
    return bad[0] if bad else (n if got.shape[0] != want.shape[0] else None)


def _where(row, n_frames, chunk, j):
    """Output frame j in input time, and the chunk edge (a first interval of stream._run's chunks) nearest to it."""
    if j is None:
        return "no frame differs (the container's bytes do)"
    t = j * M.RATES[row.rate][3]
    text = f"first differing output frame {j} (input time {float(t):.3f})"
    if chunk is None:
        return text
    edges = DV._edges(n_frames, chunk, M.look_of(row))
    if not edges:
        return text + "; the clip is one chunk"
    e = min(edges, key=lambda s: abs(s - t))
    return text + f"; nearest chunk edge at interval {e} (edges {edges})"


def _same(row, tmp_path, got, want, n_frames, chunk, what, size=None):
    if got.n == want.n and got.data == want.data:
        return
    j = _first_difference(_decode(row, got.data, tmp_path, size), _decode(row, want.data, tmp_path, size))
    raise AssertionError(f"{M.row_id(row)}: {what}, chunk_frames {chunk}: counts {got.n} / {want.n}; "
                         + _where(row, n_frames, chunk, j))


def _cat(log, k):
    return np.concatenate([np.asarray(e[k]) for e in log]) if log else np.zeros(0)


# ---- the definition -------------------------------------------------------------------------------------------------------
def _definition(dev, row, frames, grid, size):
    """The row's output frames from the references, on `grid`: the frames of the factor = G run of `frames` (h, w = size)."""
    _, rkw, rate, step, G = M.RATES[row.rate]
    n, bits = frames.shape[0], M.bits_of(row)
    dead, cuts = M.flags_of(row, frames)
    table_mode = "blend" if row.retime == "motion" else row.retime
    if row.dedup is None:
        want = RR.resample(grid, n, Fraction(*rate), P.retime.parse_fps(rkw["fps"]), rkw["time_depth"], bits,
                           table_mode, cuts)
        dead, gap = [False] * (n - 1), 2
    else:
        gap = row.dedup[1]
        want = D.resample(grid, n, step, G, bits, table_mode, dead, cuts, gap)
    if row.retime != "motion":
        return want
    entries = RM.dedup_entries(want.shape[0], step, G, dead, cuts, gap)
    rows = sorted({r for r, wn, _, _ in entries if wn})
    if not rows:
        return want
    lay = layout.frame_layout(M.SOURCES[row.source][0], *size)
    tg = torch.from_numpy(np.array(grid.view(np.int16) if bits == 10 else grid))   # (a copy: the cached grid is read-only)
    lead = torch.stack([RM.lead_of(tg[r], lay.planes, bits) for r in range(tg.shape[0])]).to(dev)
    idx = torch.tensor(rows, device=dev)
    flow = OF.farneback_flow(lead[idx], lead[idx + 1], "hip", bits=bits).cpu()
    out = torch.from_numpy(want.view(np.int16) if bits == 10 else want)
    RM.warp_rows(tg, entries, {r: flow[i] for i, r in enumerate(rows)}, lay.planes, bits, out)
    return want


def _grid(dev, models, tmp_path, grids, row, frames, size):
    G = M.RATES[row.rate][4]
    key = (row.source, frames.tobytes(), G, row.scene_cut, row.precision)
    if key not in grids:
        plain = M.make(row.clip, source=row.source, precision=row.precision, scene_cut=row.scene_cut)
        run = _call(dev, models, tmp_path, plain, frames, None, "grid", size=size, factor=G)
        g = _decode(plain, run.data, tmp_path, size)
        assert run.n == g.shape[0] == (frames.shape[0] - 1) * G + 1
        g.setflags(write=False)
        grids[key] = g
    return grids[key]


# ---- the case -------------------------------------------------------------------------------------------------------------
def _check_logs(run, row, frames):
    """The resident run's logs against the host definitions on the frames the route saw; the main clips have their one
    cut where the pattern has it."""
    if frames.shape[0] < 2:
        return
    dead, cuts = M.flags_of(row, frames)
    assert len(run.scene_log) == (cuts is not None) and len(run.dedup_log) == (dead is not None), M.row_id(row)
    if cuts is not None:
        assert _cat(run.scene_log, 1).astype(bool).tolist() == cuts, M.row_id(row)
        if row.clip == "main":
            assert np.flatnonzero(cuts).tolist() == [M.pattern_of(row).index("|") - 1], (M.row_id(row), cuts)
    if dead is not None:
        assert _cat(run.dedup_log, 1).astype(bool).tolist() == dead, M.row_id(row)
        assert np.array_equal(_cat(run.dedup_log, 0), D.pair_peak(frames, M.bits_of(row))), M.row_id(row)


@pytest.mark.parametrize("row", ROWS, ids=[M.row_id(r) for r in ROWS])
def test_row(dev, models, grids, tmp_path, row):
    frames = M.frames_of(row)
    n_frames = frames.shape[0]

    # chunk invariance
    res = _call(dev, models, tmp_path, row, frames, None, "resident")
    assert res.n == D.n_out(n_frames, M.RATES[row.rate][3]), (M.row_id(row), res.n)
    if row.resize is None:
        _check_logs(res, row, frames)
    for chunk in M.chunk_sizes(row):
        got = _call(dev, models, tmp_path, row, frames, chunk, f"chunk{chunk}", pipe=chunk == 3 and PIPED.get(row.source) == row)
        _same(row, tmp_path, got, res, n_frames, chunk, "streamed against resident")
        for k in (0, 1):
            for name, a, b in (("scene_log", got.scene_log, res.scene_log), ("dedup_log", got.dedup_log, res.dedup_log)):
                assert np.array_equal(_cat(a, k), _cat(b, k)), (M.row_id(row), name, chunk)

    # reduction: peel one feature at a time; `base` is the resident result of `cur` on `frames` of `size`
    cur, base, size = row, res, M.size_of(row)
    packing = M.SOURCES[cur.source][4]
    if packing is not None:
        nxt = cur._replace(source="yuv422p10le")
        peeled = _call(dev, models, tmp_path, nxt, frames, None, "unpacked")
        oh, ow = M.out_size_of(cur)
        planar = np.frombuffer(peeled.data, "<u2").reshape(peeled.n, -1)
        want = _Run(peeled.n, W10.pack(planar, oh, ow, packing).tobytes(), None, None)
        _same(cur, tmp_path, base, want, n_frames, None, f"packing {packing} against the unpacked route, packed")
        cur, base = nxt, peeled
    if cur.resize is not None:
        kind, bits = M.SOURCES[cur.source][0], M.bits_of(cur)
        sp, dp = RS.frame_planes(kind, *size), RS.frame_planes(kind, *M.out_size_of(cur))
        t = torch.from_numpy(frames.view(np.int16) if bits == 10 else frames).to(dev)
        frames = RS.resize_frames(t, sp, dp, bits, filter=cur.resize).cpu().numpy().view(frames.dtype)
        size, nxt = M.out_size_of(cur), cur._replace(resize=None)
        peeled = _call(dev, models, tmp_path, nxt, frames, None, "pre-resized", size=size)
        _same(cur, tmp_path, base, peeled, n_frames, None, f"resize {cur.resize} against the pre-resized clip")
        _check_logs(peeled, nxt, frames)
        assert all(np.array_equal(_cat(a, k), _cat(b, k)) for k in (0, 1) for a, b in
                   ((base.scene_log, peeled.scene_log), (base.dedup_log, peeled.dedup_log))), (M.row_id(cur), "logs")
        cur, base = nxt, peeled
    if cur.chroma == "motion":
        nxt = cur._replace(chroma="average")
        peeled = _call(dev, models, tmp_path, nxt, frames, None, "average", size=size)
        a, b = _decode(cur, base.data, tmp_path, size), _decode(nxt, peeled.data, tmp_path, size)
        ny = size[0] * size[1]
        assert base.n == peeled.n and a.shape == b.shape, M.row_id(cur)
        bad = [j for j in range(a.shape[0]) if not np.array_equal(a[j, :ny], b[j, :ny])]
        assert not bad, f"{M.row_id(cur)}: chroma motion changes the luma; " + _where(cur, n_frames, None, bad[0])
        source = {f.tobytes() for f in frames}
        bad = [j for j in range(a.shape[0]) if b[j].tobytes() in source and not np.array_equal(a[j], b[j])]
        assert not bad, f"{M.row_id(cur)}: chroma motion changes a source frame; " + _where(cur, n_frames, None, bad[0])
        assert any(b[j].tobytes() in source for j in range(b.shape[0]))
        cur, base = nxt, peeled
    if cur.batch == 2:
        nxt = cur._replace(batch=8)
        peeled = _call(dev, models, tmp_path, nxt, frames, None, "batch8", size=size)
        _same(cur, tmp_path, base, peeled, n_frames, None, "batch 2 against batch 8", size)
        cur, base = nxt, peeled

    # definition
    if M.has_plan(cur):
        grid = _grid(dev, models, tmp_path, grids, cur, frames, size)
        want = _definition(dev, cur, frames, grid, size)
        got = _decode(cur, base.data, tmp_path, size)
        j = _first_difference(got, want)
        assert base.n == want.shape[0] and j is None, \
            f"{M.row_id(cur)}: resident against the definition: counts {base.n} / {want.shape[0]}; " + \
            _where(cur, n_frames, None, j)
