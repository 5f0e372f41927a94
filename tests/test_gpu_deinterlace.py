"""GPU (MI355X): fiunet_deinterlace_u8 / _p10 and `fi.deinterlace` bit for bit against tests/deinterlace_ref.py
(DESIGN.md 3.3w).

  1. planes: every H x W x N of the lists below, both orders, both rates, both methods, the check on and off, at 8 bits,
     10-bit codes and full 16-bit words; each clip runs tight (the per-sample path wherever W is no multiple of the
     vector) and with an aligned pitch (the vector path with its tail)
  2. layouts: steps 2, 3 and 4, every plane of nv12 / uyvy422 / bgra in one call, an unaligned base, a plane more than
     2^32 bytes into its buffer
  3. the window: first / n_frames / n_src at every position of a five-frame clip
  4. guard bands around and between the destination's planes stay untouched
  5. the stream-contract rows: side stream and captured graph
  6. `deinterlace_video`: formats, chunk sizes, file and pipe, the header
  7. the command line, piped into `cli video`
  8. `interpolate_video` writes the same bytes for a clip tagged `It` and the same clip without the token"""
import io
import os
import subprocess
import sys
import threading
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deinterlace_ref as R  # noqa: E402
import deinterlace_stream_rows as RS  # noqa: E402
import large_extent as LE  # noqa: E402
import stream_contract as SC  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import _native, deinterlace as D, imageio_lite as IO, wire10  # noqa: E402
from ai_based_frame_interpolation_amd.layout import frame_layout  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HS = (2, 3, 4, 5, 9, 18)
WS = (1, 2, 5, 6, 7, 8, 16, 37, 64, 67, 131)   # the x < 3 rule, the vector / tail seam (16 or 8 samples), a 64-lane seam
NS = (1, 2, 3, 5)
OPTIONS = [(order, rate, method, check) for order in R.ORDERS for rate in R.RATES
           for method, check in (("adaptive", True), ("adaptive", False), ("bob", True))]
KINDS = {"u8": (8, 256), "p10": (10, 1024), "words16": (10, 65536)}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


def _np_dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def _to_dev(a, dev):
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _to_np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _flags(method, check):
    return D.METHODS[method] | (0 if check else _native.DEINT_NO_SPATIAL_CHECK)


def _run(src, n_src, sp, dst, dp, first, count, order, rate, method, check, bits):
    _native.deinterlace(src, n_src, sp, dst, dp, first, count, D.ORDERS[order], D.RATES[rate], _flags(method, check), bits)


# ---- 1. planes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", HS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_planes_against_the_reference(dev, kind, h):
    bits, top = KINDS[kind]
    dt = _np_dtype(bits)
    vec = 16 // np.dtype(dt).itemsize
    rng = np.random.default_rng(h * 7 + bits + top % 5)
    for w in WS:
        pitch = -(-w // vec) * vec                       # rows 16 bytes apart: the vector path
        fs = h * pitch
        for n in NS:
            clip = rng.integers(0, top, (n, h, w)).astype(dt)
            tight = _to_dev(clip.reshape(n, h * w), dev)
            padded = np.zeros((n, h, pitch), dt)
            padded[:, :, :w] = clip
            pitched = _to_dev(padded.reshape(n, fs), dev)
            for order, rate, method, check in OPTIONS:
                want = R.deinterlace(clip, order, rate, method, check)
                k = want.shape[0]
                out_t = torch.zeros((k, h * w), dtype=tight.dtype, device=dev)
                out_p = torch.zeros((k, fs), dtype=tight.dtype, device=dev)
                _run(tight, n, [(0, h, w, w, 1, h * w)], out_t, [(0, h, w, w, 1, h * w)], 0, n, order, rate, method, check, bits)
                _run(pitched, n, [(0, h, w, pitch, 1, fs)], out_p, [(0, h, w, pitch, 1, fs)], 0, n, order, rate, method, check, bits)
                what = (kind, h, w, n, order, rate, method, check)
                assert np.array_equal(_to_np(out_t).reshape(k, h, w), want), ("tight",) + what
                got_p = _to_np(out_p).reshape(k, h, pitch)
                assert np.array_equal(got_p[:, :, :w], want), ("pitched",) + what
                assert not got_p[:, :, w:].any(), ("pitched: the gap was written",) + what


# ---- 2. layouts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
@pytest.mark.parametrize("step", [2, 3, 4])
def test_stepped_planes(dev, step, bits):
    """`step` planes interleaved sample by sample, all in one call, into a destination of another pitch."""
    n, h, w = 3, 9, 37
    dt = _np_dtype(bits)
    rng = np.random.default_rng(step + bits)
    src = rng.integers(0, 1 << bits, (n, h, w * step)).astype(dt)
    dpitch = w * step + 5
    sp = [(c, h, w, w * step, step, h * w * step) for c in range(step)]
    dp = [(c, h, w, dpitch, step, h * dpitch) for c in range(step)]
    out = torch.zeros((2 * n, h * dpitch), dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
    _run(_to_dev(src.reshape(n, -1), dev), n, sp, out, dp, 0, n, "tff", "field", "adaptive", True, bits)
    got = _to_np(out).reshape(2 * n, h, dpitch)
    for c in range(step):
        assert np.array_equal(got[:, :, c:w * step:step], R.deinterlace(src[:, :, c::step], "tff", "field")), c
    assert not got[:, :, w * step:].any()


@pytest.mark.parametrize("fmt", ["nv12", "uyvy422", "bgra"])
def test_every_plane_of_a_format_in_one_call(dev, fmt):
    h, w, n = 22, 16, 3
    lay = frame_layout(fmt, h, w)
    assert len(lay.planes) == {"nv12": 3, "uyvy422": 3, "bgra": 4}[fmt]
    rows = np.random.default_rng(len(fmt)).integers(0, 256, (n, lay.samples)).astype(np.uint8)
    for order in R.ORDERS:
        got = D.deinterlace(_to_dev(rows, dev), lay, 8, order=order)
        assert np.array_equal(_to_np(got), R.deinterlace_planes(rows, lay.planes, order=order)), order


@pytest.mark.parametrize("bits", [8, 10])
def test_an_unaligned_base_takes_the_per_sample_path(dev, bits):
    n, h, w = 2, 9, 64
    dt = _np_dtype(bits)
    clip = np.random.default_rng(bits).integers(0, 1 << bits, (n, h, w)).astype(dt)
    want = R.deinterlace(clip, "bff", "field")
    plane = [(0, h, w, w, 1, h * w)]
    for shift_src, shift_dst in ((1, 0), (0, 3), (5, 7)):
        buf = torch.zeros(n * h * w + 8, dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
        buf[shift_src:shift_src + n * h * w] = _to_dev(clip.reshape(-1), dev)
        out = torch.zeros(2 * n * h * w + 8, dtype=buf.dtype, device=dev)
        _run(buf[shift_src:], n, plane, out[shift_dst:], plane, 0, n, "bff", "field", "adaptive", True, bits)
        got = _to_np(out)
        assert np.array_equal(got[shift_dst:shift_dst + 2 * n * h * w].reshape(2 * n, h, w), want), (shift_src, shift_dst)
        assert not got[:shift_dst].any() and not got[shift_dst + 2 * n * h * w:].any()


def test_a_plane_more_than_2_to_the_32_bytes_into_its_buffer(dev):
    """Frames 2^31 + 64 samples apart: frame 1 of either buffer starts past byte 2^31, frame 2 past 2^32 (output frames 2
    to 5 all do).  On the vector path (offset 0) and on the per-sample path (offset 1); only the small planes are ever
    touched."""
    n, h, w, pitch, fs = 3, 9, 67, 80, (1 << 31) + 64
    need = (n - 1) * fs + (2 * n - 1) * fs + 3 * h * pitch
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need + LE.HEADROOM:
        pytest.skip(f"plans {need / LE.GIB:.1f} GiB + {LE.HEADROOM / LE.GIB:.0f} GiB headroom, the card has {free / LE.GIB:.1f} GiB free")
    try:
        src = torch.empty((n - 1) * fs + h * pitch + 1, dtype=torch.uint8, device=dev)
        dst = torch.empty((2 * n - 1) * fs + h * pitch + 1, dtype=torch.uint8, device=dev)
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"the allocation failed: {e}")
    clip = np.random.default_rng(32).integers(0, 256, (n, h, w)).astype(np.uint8)
    want = R.deinterlace(clip, "tff", "field")
    padded = np.zeros((n, h, pitch), np.uint8)
    padded[:, :, :w] = clip
    for off in (0, 1):
        for f in range(n):
            src[f * fs + off:f * fs + off + h * pitch] = _to_dev(padded[f].reshape(-1), dev)
        for f in range(2 * n):
            dst[f * fs + off:f * fs + off + h * pitch] = 0
        _run(src, n, [(off, h, w, pitch, 1, fs)], dst, [(off, h, w, pitch, 1, fs)], 0, n, "tff", "field", "adaptive", True, 8)
        got = np.stack([dst[f * fs + off:f * fs + off + h * pitch].cpu().numpy().reshape(h, pitch) for f in range(2 * n)])
        assert np.array_equal(got[:, :, :w], want), off
        assert not got[:, :, w:].any(), off


# ---- 3. the window -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
def test_every_position_of_a_five_frame_window(dev, bits):
    n, h, w = 5, 9, 37
    lay = [(0, h, w, w, 1)]
    clip = np.random.default_rng(50 + bits).integers(0, 1 << bits, (n, h * w)).astype(_np_dtype(bits))
    d = _to_dev(clip, dev)
    for rate, per in (("field", 2), ("frame", 1)):
        whole = _to_np(D.deinterlace(d, lay, bits, "tff", rate))
        assert np.array_equal(whole.reshape(-1, h, w), R.deinterlace(clip.reshape(n, h, w), "tff", rate))
        for first in range(n + 1):
            for count in range(n - first + 1):
                part = _to_np(D.deinterlace(d, lay, bits, "tff", rate, first=first, count=count))
                assert np.array_equal(part, whole[per * first:per * (first + count)]), (rate, first, count)
                if count:   # a window of its own: one context frame either side where the clip has one
                    lo, hi = max(first - 1, 0), min(first + count + 1, n)
                    sub = _to_np(D.deinterlace(d[lo:hi].contiguous(), lay, bits, "tff", rate, first=first - lo, count=count))
                    assert np.array_equal(sub, whole[per * first:per * (first + count)]), (rate, first, count, "sub-window")


# ---- 4. guard bands -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 10])
def test_nothing_outside_the_destination_planes_is_written(dev, bits):
    """Two planes - one on the vector path, one stepped - in frames with room before, between and behind them."""
    n, h, w = 3, 9, 37
    dt = _np_dtype(bits)
    rng = np.random.default_rng(60 + bits)
    a, b = (rng.integers(0, 1 << bits, (n, h, w)).astype(dt) for _ in range(2))
    pa, off_a = 48, 32                     # plane a: step 1, pitch 48, from sample 32 of a frame
    off_b, pb = off_a + h * pa + 16 + 1, 2 * w + 3   # plane b: step 2, behind a gap
    fs = off_b + h * pb + 16
    fs += -fs % 16
    frame = np.zeros((n, fs), dt)
    ia = off_a + np.arange(h)[:, None] * pa + np.arange(w)[None, :]
    ib = off_b + np.arange(h)[:, None] * pb + 2 * np.arange(w)[None, :]
    frame[:, ia], frame[:, ib] = a, b
    guard = 64
    poison = 0xA5 if bits == 8 else 0x5AA5
    out = torch.full((guard + 2 * n * fs + guard,), poison if bits == 8 else poison - 65536 if poison > 32767 else poison,
                     dtype=torch.uint8 if bits == 8 else torch.int16, device=dev)
    planes = [(off_a, h, w, pa, 1, fs), (off_b, h, w, pb, 2, fs)]
    _run(_to_dev(frame, dev), n, planes, out[guard:], planes, 0, n, "bff", "field", "adaptive", True, bits)
    got = _to_np(out)
    body = got[guard:guard + 2 * n * fs].reshape(2 * n, fs)
    assert np.array_equal(body[:, ia], R.deinterlace(a, "bff", "field"))
    assert np.array_equal(body[:, ib], R.deinterlace(b, "bff", "field"))
    untouched = np.ones(fs, bool)
    untouched[ia.reshape(-1)] = untouched[ib.reshape(-1)] = False
    assert (body[:, untouched] == poison).all()
    assert (got[:guard] == poison).all() and (got[guard + 2 * n * fs:] == poison).all()


# ---- 5. the stream contract ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", RS.ROWS, ids=lambda r: f"{r.entry}-{r.ident}")
def test_side_stream_and_captured_graph(dev, row):
    env = SC.Env(dev)
    try:
        SC.check_row(row, env)
    finally:
        env.close()


# ---- 6. deinterlace_video --------------------------------------------------------------------------------------------------
N, VH, VW = 7, 18, 24
CHUNKS = (1, 2, 3, 7, 32)
#: name -> (Y4M tag or None, raw format or None, packing or None)
SOURCES = {"C420jpeg": ("420jpeg", None, None), "C422p10": ("422p10", None, None), "nv12": (None, "nv12", None),
           "uyvy422": (None, "uyvy422", None), "v210": (None, "yuv422p10le", "v210")}


def _source(name, dev):
    """-> (the file's bytes, the layout of a frame, the frames as working rows [N, samples])."""
    tag, raw, packing = SOURCES[name]
    lay = frame_layout(("y4m", tag) if tag else raw, VH, VW)
    rng = np.random.default_rng(sum(name.encode()))
    rows = rng.integers(0, 1 << lay.bits, (N, lay.samples)).astype(_np_dtype(lay.bits))
    if tag:
        f = io.BytesIO()
        head = IO._y4m_header_line(VW, VH, (30000, 1001), tag, None, lay.bits).replace(b" Ip ", b" Ib ")
        f.write(head)
        for r in rows:
            f.write(b"FRAME\n" + r.astype("<u2" if lay.bits == 10 else np.uint8).tobytes())
        return f.getvalue(), lay, rows
    if packing:
        return wire10.pack(_to_dev(rows, dev), VH, VW, packing).cpu().numpy().tobytes(), lay, rows   # (uint8 wire bytes)
    return rows.tobytes(), lay, rows


def _expected(name, rows, lay, dev, order, **kw):
    want = R.deinterlace_planes(rows, lay.planes, order=order, **kw)
    tag, raw, packing = SOURCES[name]
    if packing:
        return wire10.pack(_to_dev(want, dev), VH, VW, packing).cpu().numpy().tobytes(), len(want)
    return want.astype("<u2" if lay.bits == 10 else np.uint8).tobytes(), len(want)


def _payload(data, tag, bits, samples):
    """The frame payloads of a Y4M result, and its header line."""
    line = data[:data.index(b"\n") + 1]
    fsz = samples * (2 if bits == 10 else 1)
    body, pos = [], len(line)
    while pos < len(data):
        assert data[pos:pos + 6] == b"FRAME\n"
        body.append(data[pos + 6:pos + 6 + fsz])
        pos += 6 + fsz
    return line, b"".join(body)


@pytest.mark.parametrize("name", list(SOURCES))
def test_deinterlace_video_is_the_reference_for_every_chunk_size_from_a_file_and_a_pipe(dev, tmp_path, name):
    tag, raw, packing = SOURCES[name]
    data, lay, rows = _source(name, dev)
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    kw = dict(raw=raw, width=VW, height=VH, packing=packing, order="bff") if raw else {}
    want, n_out = _expected(name, rows, lay, dev, "bff")
    assert n_out == 2 * N
    results = set()
    for chunk in CHUNKS:
        dst = tmp_path / f"out{chunk}.bin"
        assert D.deinterlace_video(str(src), str(dst), chunk_frames=chunk, **kw) == 2 * N
        results.add(dst.read_bytes())
    # from a pipe into a pipe, the source written by a thread in pieces that do not end on frames
    rfd, wfd = os.pipe()
    def feed():
        with os.fdopen(wfd, "wb") as f:
            for k in range(0, len(data), 1000):
                f.write(data[k:k + 1000])
    t = threading.Thread(target=feed)
    t.start()
    sink = io.BytesIO()
    sink.close = sink.flush   # (the caller's object stays open)
    with os.fdopen(rfd, "rb") as f:
        assert D.deinterlace_video(f, sink, chunk_frames=3, **kw) == 2 * N
    t.join()
    results.add(sink.getvalue())
    assert len(results) == 1
    got = results.pop()
    if tag:
        line, got = _payload(got, tag, lay.bits, lay.samples)
        assert line == IO._y4m_header_line(VW, VH, (60000, 1001), tag, None, lay.bits) and b" Ip " in line
    assert got == want


def test_deinterlace_video_rates_methods_and_the_auto_order(dev, tmp_path):
    data, lay, rows = _source("C420jpeg", dev)   # tagged Ib
    src = tmp_path / "in.y4m"
    src.write_bytes(data)
    for kw, ref in ((dict(rate="frame"), dict(rate="frame")), (dict(method="bob"), dict(method="bob")),
                    (dict(spatial_check=False), dict(spatial_check=False)), (dict(order="tff"), {})):
        dst = tmp_path / "out.y4m"
        n = D.deinterlace_video(str(src), str(dst), chunk_frames=2, **kw)
        line, got = _payload(dst.read_bytes(), "420jpeg", 8, lay.samples)
        want = R.deinterlace_planes(rows, lay.planes, order=kw.get("order", "bff"), **ref)
        assert n == len(want) and got == want.tobytes(), kw
        fps = (30000, 1001) if kw.get("rate") == "frame" else (60000, 1001)
        assert line == IO._y4m_header_line(VW, VH, fps, "420jpeg", None, 8)
    assert D.deinterlace_video(str(src), str(tmp_path / "o.y4m"), src_fps=(25, 1)) == 2 * N
    assert b" F50:1 " in (tmp_path / "o.y4m").read_bytes()[:80]


# ---- 7., 8. the commands ---------------------------------------------------------------------------------------------------
def _checkpoint(tmp_path):
    path = str(tmp_path / "model.pth")
    torch.save(O.make_seeded_state_dict(1234), path)
    return path


def _y4m(tmp_path, name, token, n=5, h=32, w=32, seed=9):
    rng = np.random.default_rng(seed)
    head = b"YUV4MPEG2 W%d H%d F25:1" % (w, h) + (b" " + token if token else b"") + b" A1:1 C420jpeg\n"
    path = tmp_path / name
    path.write_bytes(head + b"".join(b"FRAME\n" + rng.integers(0, 256, w * h * 3 // 2).astype(np.uint8).tobytes()
                                     for _ in range(n)))
    return str(path)


def test_the_command_line_pipes_into_cli_video(dev, tmp_path):
    n = 5
    src, ckpt, out = _y4m(tmp_path, "in.y4m", b"It", n), _checkpoint(tmp_path), str(tmp_path / "out.y4m")
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cli = [sys.executable, "-m", "ai_based_frame_interpolation_amd.cli"]
    first = subprocess.Popen(cli + ["deinterlace", "--input", src, "--output", "-"], stdout=subprocess.PIPE,
                             stderr=subprocess.PIPE, env=env)
    second = subprocess.Popen(cli + ["video", "--input", "-", "--output", out, "--model", ckpt, "--factor", "2"],
                              stdin=first.stdout, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    first.stdout.close()
    err2 = second.communicate(timeout=300)[1].decode()
    err1 = first.stderr.read().decode()
    assert first.wait(timeout=60) == 0, err1
    assert second.returncode == 0, err2
    assert f"wrote {2 * n} frames" in err1 and f"wrote {4 * n - 1} frames" in err2
    assert "cli deinterlace" not in err2        # the deinterlaced stream says Ip: no warning behind it
    with IO.Y4MReader(out) as r:
        assert r.interlace == "p" and r.header["fps"] == (100, 1)
    assert IO.y4m_frame_count(out) == 4 * n - 1


def test_a_tagged_clip_interpolates_to_the_bytes_of_the_untagged_one(dev, tmp_path):
    model = P.FrameInterpolationUNet(bilinear=True)
    model.load_state_dict(O.make_seeded_state_dict(1234))
    fi = P.FrameInterpolator(model=model.to(dev).eval(), device=dev)
    outs = {}
    for token in (b"It", None):
        src = _y4m(tmp_path, "in.y4m", token)
        dst = str(tmp_path / f"out_{bool(token)}.y4m")
        with warnings.catch_warnings(record=True) as got:
            warnings.simplefilter("always")
            fi.interpolate_video(src, dst, chunk_frames=4)
        assert len([w for w in got if "cli deinterlace" in str(w.message)]) == (1 if token else 0)
        outs[token] = open(dst, "rb").read()
    assert outs[b"It"] == outs[None]
