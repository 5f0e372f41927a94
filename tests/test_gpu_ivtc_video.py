"""GPU (MI355X): `fi.ivtc.ivtc`, `ivtc_video` and `cli ivtc` against the reference pipeline of tests/ivtc_ref.py, byte for
byte.

  1. a telecined clip of the film content of tests/ivtc_content.py in every plane comes back as the film frames' bytes with
     the 24000/1001 header: Y4M 8 bit `It` and `Ib`, `C420p10`, raw nv12, uyvy422, rgb24, yuv422p10le packed as v210; the
     bytes are the same for chunk_frames 1, 2, 3, 7 and 32, from a file and from a pipe
  2. the reference pipeline on a joined clip with an orphan under both fallbacks, without decimation, and on a clip whose
     length is no multiple of 5
  3. `cli ivtc` writes the bytes of the Python call
  4. a progressive clip passes through `ivtc(decimate=False)` unchanged"""
import io
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ivtc_content as C  # noqa: E402
import ivtc_ref as R  # noqa: E402

from ai_based_frame_interpolation_amd import imageio_lite as IO, ivtc as I, wire10  # noqa: E402
from ai_based_frame_interpolation_amd.layout import frame_layout  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (1, 2, 3, 7, 32)
#: name -> (Y4M tag, Y4M interlace token, raw format, packing, order, h, w, pulldown phase)
SOURCES = {"C420jpeg-It": ("420jpeg", b"It", None, None, "tff", 24, 40, 1),
           "C420jpeg-Ib": ("420jpeg", b"Ib", None, None, "bff", 34, 70, 3),
           "C420p10": ("420p10", b"It", None, None, "tff", 24, 40, 4),
           "nv12": (None, None, "nv12", None, "bff", 24, 40, 0),
           "uyvy422": (None, None, "uyvy422", None, "tff", 24, 40, 2),
           "rgb24": (None, None, "rgb24", None, "tff", 24, 40, 1),
           "v210": (None, None, "yuv422p10le", "v210", "bff", 24, 48, 3)}


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


def _planes5(lay):
    return [tuple(p)[-5:] for p in lay.planes]


def film_rows(lay, motion=(3, 1), seed=7):
    """Film frames as rows [16, samples]: every plane of the layout holds the film content at its own size."""
    rows = np.zeros((C.FILM_FRAMES, lay.samples), _np_dtype(lay.bits))
    for i, pl in enumerate(_planes5(lay)):
        rows[:, R.plane_index(pl)] = C.film(pl[1], pl[2], motion, seed=seed + i, bits=lay.bits)
    return rows


def telecine_rows(rows, lay, order, phase):
    out = None
    for pl in _planes5(lay):
        idx = R.plane_index(pl)
        tc, _ = R.telecine(rows[:, idx], order, phase)
        if out is None:
            out = np.zeros((len(tc), rows.shape[1]), rows.dtype)
        out[:, idx] = tc
    return out


def _file_bytes(spec, rows, lay, dev, fps=(30000, 1001)):
    tag, token, raw, packing, order, h, w, _ = spec
    if tag:
        f = io.BytesIO()
        f.write(IO._y4m_header_line(w, h, fps, tag, None, lay.bits).replace(b" Ip ", b" " + token + b" "))
        for r in rows:
            f.write(b"FRAME\n" + r.astype("<u2" if lay.bits == 10 else np.uint8).tobytes())
        return f.getvalue()
    if packing:
        return wire10.pack(_to_dev(rows, dev), h, w, packing).cpu().numpy().tobytes()
    return rows.tobytes()


def _payload(data, bits, samples):
    line = data[:data.index(b"\n") + 1]
    fsz = samples * (2 if bits == 10 else 1)
    body, pos = [], len(line)
    while pos < len(data):
        assert data[pos:pos + 6] == b"FRAME\n"
        body.append(data[pos + 6:pos + 6 + fsz])
        pos += 6 + fsz
    return line, b"".join(body)


def _source(name, dev, n=None):
    tag, token, raw, packing, order, h, w, phase = SOURCES[name]
    lay = frame_layout(("y4m", tag) if tag else raw, h, w)
    film = film_rows(lay)
    tc = telecine_rows(film, lay, order, phase)
    tc = tc[:len(tc) // 5 * 5 if n is None else n]
    kw = dict(raw=raw, width=w, height=h, packing=packing, order=order) if raw else {}
    return lay, film, tc, kw


# ---- 1. ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SOURCES))
def test_ivtc_video_returns_the_film_frames_for_every_chunk_size_from_a_file_and_a_pipe(dev, tmp_path, name):
    tag, token, raw, packing, order, h, w, phase = SOURCES[name]
    lay, film, tc, kw = _source(name, dev)
    n = len(tc)
    want, rep = R.ivtc(tc, _planes5(lay), lay.bits, order)
    # the reference's result is the film: every output frame but a leading orphan is a film frame, in order
    skip = 1 if phase in (2, 3) else 0
    ids = [int(np.flatnonzero((film == f).all(axis=1))[0]) for f in want[skip:]]
    assert ids == sorted(set(ids)) and len(want) == n * 4 // 5 and rep["combed"] == ([0] if skip else [])
    assert phase == 2 or ids == list(range(ids[0], ids[0] + len(ids)))
    data = _file_bytes(SOURCES[name], tc, lay, dev)
    src = tmp_path / "in.bin"
    src.write_bytes(data)
    results = set()
    for chunk in CHUNKS:
        dst = tmp_path / f"out{chunk}.bin"
        got = I.ivtc_video(str(src), str(dst), chunk_frames=chunk, **kw)
        assert got == rep, chunk
        results.add(dst.read_bytes())
    for chunk in (1, 3, 32):   # from a pipe into a pipe, the source written by a thread in pieces that do not end on frames
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
            assert I.ivtc_video(f, sink, chunk_frames=chunk, **kw) == rep, chunk
        t.join()
        results.add(sink.getvalue())
    assert len(results) == 1
    got = results.pop()
    if tag:
        line, got = _payload(got, lay.bits, lay.samples)
        assert line == IO._y4m_header_line(w, h, (24000, 1001), tag, None, lay.bits) and b" Ip " in line
        assert got == want.astype("<u2" if lay.bits == 10 else np.uint8).tobytes()
    elif packing:
        assert got == wire10.pack(_to_dev(want, dev), h, w, packing).cpu().numpy().tobytes()
    else:
        assert got == want.tobytes()


# ---- 2. ------------------------------------------------------------------------------------------------------------------
def _joined(dev):
    lay = frame_layout(("y4m", "420jpeg"), 34, 70)
    a = telecine_rows(film_rows(lay, (3, 1), 7), lay, "tff", 0)
    b = telecine_rows(film_rows(lay, (5, 3), 11), lay, "tff", 0)
    return lay, np.concatenate([a[:8], b[3:15]])      # b's first frame lost its other field to the edit: an orphan at 8


@pytest.mark.parametrize("fallback", ["deinterlace", "keep"])
@pytest.mark.parametrize("decimate", [True, False])
def test_a_joined_clip_equals_the_reference_under_both_fallbacks(dev, tmp_path, fallback, decimate):
    lay, tc = _joined(dev)
    want, rep = R.ivtc(tc, _planes5(lay), 8, "tff", fallback=fallback, decimate=decimate)
    assert rep["combed"] == [8] and rep["frames_out"] == (16 if decimate else 20)
    got, got_rep = I.ivtc(_to_dev(tc, dev), lay, 8, "tff", fallback=fallback, decimate=decimate)
    assert got_rep == rep and np.array_equal(_to_np(got), want)
    src = tmp_path / "in.y4m"
    src.write_bytes(_file_bytes(("420jpeg", b"It", None, None, "tff", 34, 70, 0), tc, lay, dev, fps=(30, 1)))
    for chunk in (4, 7):
        dst = tmp_path / "out.y4m"
        assert I.ivtc_video(str(src), str(dst), fallback=fallback, decimate=decimate, chunk_frames=chunk) == rep
        line, body = _payload(dst.read_bytes(), 8, lay.samples)
        assert body == want.tobytes(), chunk
        assert (b" F24:1 " if decimate else b" F30:1 ") in line


@pytest.mark.parametrize("n", [13, 4, 1])
def test_a_clip_whose_length_is_no_multiple_of_the_cycle(dev, tmp_path, n):
    lay, film, tc, kw = _source("nv12", dev, n=n)
    want, rep = R.ivtc(tc, _planes5(lay), 8, "bff")
    assert rep["frames_out"] == n - n // 5
    got, got_rep = I.ivtc(_to_dev(tc, dev), lay, 8, "bff")
    assert got_rep == rep and np.array_equal(_to_np(got), want)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(tc.tobytes())
    for chunk in (2, 5, 32):
        assert I.ivtc_video(str(src), str(dst), chunk_frames=chunk, **kw) == rep
        assert dst.read_bytes() == want.tobytes(), chunk
    for cycle in (4, 6):
        want, rep = R.ivtc(tc, _planes5(lay), 8, "bff", cycle=cycle)
        assert I.ivtc_video(str(src), str(dst), chunk_frames=3, cycle=cycle, **kw) == rep
        assert dst.read_bytes() == want.tobytes(), cycle


# ---- 3. ------------------------------------------------------------------------------------------------------------------
def test_the_command_line_writes_the_bytes_of_the_python_call(dev, tmp_path):
    lay, film, tc, kw = _source("C420jpeg-It", dev)
    src, a, b = tmp_path / "in.y4m", tmp_path / "a.y4m", tmp_path / "b.y4m"
    src.write_bytes(_file_bytes(SOURCES["C420jpeg-It"], tc, lay, dev))
    rep = I.ivtc_video(str(src), str(a), chunk_frames=4)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    with open(src, "rb") as fin, open(b, "wb") as fout:
        r = subprocess.run([sys.executable, "-m", "ai_based_frame_interpolation_amd.cli", "ivtc", "--input", "-", "--output", "-",
                            "--chunk-frames", "4"], stdin=fin, stdout=fout, stderr=subprocess.PIPE, env=env, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert a.read_bytes() == b.read_bytes()
    m = rep["matches"]
    assert f"wrote {rep['frames_out']} frames" in err and f"p {m['p']}, c {m['c']}, n {m['n']}" in err
    with IO.Y4MReader(str(b)) as rd:
        assert rd.interlace == "p" and rd.header["fps"] == (24000, 1001)


# ---- 4. ------------------------------------------------------------------------------------------------------------------
def test_a_progressive_clip_passes_through_unchanged(dev):
    lay = frame_layout(("y4m", "420jpeg"), 24, 40)
    film = film_rows(lay)
    for order in R.ORDERS:
        got, rep = I.ivtc(_to_dev(film, dev), lay, 8, order, decimate=False)
        assert np.array_equal(_to_np(got), film) and rep["matches"] == {"p": 0, "c": len(film), "n": 0}
        assert rep["combed"] == [] and rep["dropped"] == [] and rep["frames_out"] == len(film)
    tele = I.telecine(_to_dev(film, dev), lay, "tff", 1)
    assert np.array_equal(_to_np(tele), telecine_rows(film, lay, "tff", 1))
