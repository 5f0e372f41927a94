"""GPU (MI355X): NV12 video - the sequence loop and the raw route of `interpolate_video`, byte for byte
against the I420 / Y4M routes on the same frames through a numpy repack (tests/nv12_ref.py).

  5. interpolate_sequence_nv12: 5 frames of 37x53, batch 2 (a ragged last chunk), a planted hard cut, scene_cut 10
  6. interpolate_video(raw="nv12"): 7 frames of 37x53 at factor 2 and at 24 -> 60 fps with scene_cut; chunk_frames 3
     writes the whole-clip run's bytes; a pipe in and out gives the files' bytes
"""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import colour_ref as C  # noqa: E402
import nv12_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import imageio_lite as IO  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

H, W = 37, 53
OPTS = dict(siting="mpeg2", matrix="bt709", colour_range="limited")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def interp(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3)
    m.load_state_dict(O.make_interpolating_state_dict(n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield P.FrameInterpolator(model=m, device="cuda", batch=2)
    torch.cuda.empty_cache()


def _clip(n, cut):
    """Packed I420 frames of a moving texture with a hard cut (another texture) before frame `cut`."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for t in range(n):
        x = xx - 2 * t
        if t < cut:
            r, g, b = (128 + 100 * np.sin(x / 5.0) * np.cos(yy / 7.0), 128 + 90 * np.cos((x + yy) / 6.0),
                       128 + 80 * np.sin((x - 0.5 * yy) / 4.0))
        else:
            r, g, b = (40 + 30 * np.cos(x / 3.0), 200 + 40 * np.sin(yy / 2.0), 60 + 50 * np.sin((x + 2 * yy) / 9.0))
        out.append(np.stack([r, g, b]))
    rgb = np.clip(np.rint(np.stack(out)), 0, 255).astype(np.uint8)
    return C.rgb_to_yuv420(rgb, **OPTS)


# ---- 5. the sequence loop -----------------------------------------------------------------------------------------
def test_interpolate_sequence_nv12_equals_the_repacked_i420_run(dev, interp):
    n, cut = 5, 3
    i420 = _clip(n, cut)
    want = P.interpolate_sequence_yuv420(interp.model, torch.from_numpy(i420).to(dev), H, W, 2, scene_cut=10, **OPTS)
    want = want.cpu().numpy()
    assert np.array_equal(want[2 * cut - 1], want[2 * cut - 2])        # the cut interval is held ...
    assert not np.array_equal(want[1], want[0])                         # ... and the others are interpolated
    nv = torch.from_numpy(R.i420_to_nv12(i420, H, W)).to(dev)
    got = P.interpolate_sequence_nv12(interp.model, nv, H, W, 2, scene_cut=10, **OPTS).cpu().numpy()
    assert got.shape == (2 * n - 1, nv.shape[1])
    assert np.array_equal(got, R.i420_to_nv12(want, H, W))
    # siting None is "mpeg2"
    got_default = P.interpolate_sequence_nv12(interp.model, nv, H, W, 2, scene_cut=10).cpu().numpy()
    assert np.array_equal(got_default, got)


# ---- 6. the raw route ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip_files(tmp_path_factory):
    d = tmp_path_factory.mktemp("nv12")
    i420 = _clip(7, 4)
    hc, wc, ny, nc = R.dims(H, W)
    IO.write_y4m(str(d / "in.y4m"), i420[:, :ny].reshape(-1, H, W),
                 (i420[:, ny:ny + nc].reshape(-1, hc, wc), i420[:, ny + nc:].reshape(-1, hc, wc)),
                 fps=(24, 1), colourspace="420mpeg2")
    (d / "in.nv12").write_bytes(R.i420_to_nv12(i420, H, W).tobytes())
    return d


def _y4m_payload_as_nv12(path):
    out, hdr = IO.read_y4m_packed(str(path))
    return R.i420_to_nv12(out, H, W).tobytes(), hdr, out.shape[0]


RAW = dict(raw="nv12", width=W, height=H, src_fps=24)
RUNS = [("factor2", dict(factor=2, scene_cut=10), 13, (48, 1)), ("fps60", dict(fps=60, scene_cut=10), 16, (60, 1))]


@pytest.mark.parametrize("name,kw,frames,rate", RUNS, ids=[r[0] for r in RUNS])
def test_raw_route_equals_the_repacked_y4m_route(interp, clip_files, name, kw, frames, rate):
    d = clip_files
    n_y4m = interp.interpolate_video(str(d / "in.y4m"), str(d / f"{name}.y4m"), **kw)
    want, hdr, n = _y4m_payload_as_nv12(d / f"{name}.y4m")
    assert n == n_y4m == frames and hdr["fps"] == rate
    got_n = interp.interpolate_video(str(d / "in.nv12"), str(d / f"{name}.nv12"), **kw, **RAW)
    got = (d / f"{name}.nv12").read_bytes()
    assert got_n == frames and len(got) == frames * R.tight(H, W)[3]
    assert got == want
    # streamed three pairs at a time: the same bytes
    assert interp.interpolate_video(str(d / "in.nv12"), str(d / f"{name}_c3.nv12"), chunk_frames=3, **kw, **RAW) == frames
    assert (d / f"{name}_c3.nv12").read_bytes() == want
    assert not [p for p in d.iterdir() if p.name.endswith(".part")]


@pytest.mark.parametrize("chunk", [None, 3], ids=["whole", "chunk3"])
def test_raw_route_through_pipes(interp, clip_files, chunk):
    d = clip_files
    kw = dict(fps=60, scene_cut=10, chunk_frames=chunk)
    interp.interpolate_video(str(d / "in.nv12"), str(d / f"pipe_ref_{chunk}.nv12"), **kw, **RAW)
    want = (d / f"pipe_ref_{chunk}.nv12").read_bytes()
    data = (d / "in.nv12").read_bytes()
    in_r, in_w = os.pipe()
    out_r, out_w = os.pipe()
    got = []

    def feed():
        with os.fdopen(in_w, "wb") as f:
            for s in range(0, len(data), 1000):   # pieces smaller than a frame
                f.write(data[s:s + 1000])
                f.flush()

    def drain():
        with os.fdopen(out_r, "rb") as f:
            got.append(f.read())
    threads = [threading.Thread(target=feed), threading.Thread(target=drain)]
    for t in threads:
        t.start()
    try:
        with os.fdopen(in_r, "rb") as fin, os.fdopen(out_w, "wb") as fout:
            n = interp.interpolate_video(fin, fout, **kw, **RAW)
    finally:
        for t in threads:
            t.join()
    assert n == 16 and got[0] == want


def test_truncated_file_is_refused_and_leaves_no_output(interp, clip_files):
    d = clip_files
    data = (d / "in.nv12").read_bytes()
    (d / "short.nv12").write_bytes(data[:-5])
    with pytest.raises(ValueError, match="whole number"):
        interp.interpolate_video(str(d / "short.nv12"), str(d / "short_out.nv12"), **RAW)
    assert not (d / "short_out.nv12").exists() and not (d / "short_out.nv12.part").exists()
