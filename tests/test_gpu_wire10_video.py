"""GPU (MI355X): v210 / y210le / p210le through the video routes.  The contract is byte identity with the
yuv422p10le route: `interpolate_video(raw="yuv422p10le", packing=p)` on the host-packed clip writes, byte for byte, the
host-packed output (tests/wire10_ref.py) of the existing route on the unpacked clip.

A seeded RGB checkpoint in fp16, 7 frames of 23 x 34 and of 24 x 50 with a hard cut before frame 4 (and, for dedup, frame 3
a repeat of frame 2): factor 2; factor 4 with scene_cut; 24000/1001 -> 60000/1001 fps; dedup 0; resize to 16 x 20 with both
filters; each at chunk_frames 1, 3 and None; a file and a pipe as the source.  `score_video(..., packing=p)` returns the
arrays of the unpacked clip, and `wire10.forward` is its three-step composition."""
import io
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wire10_ref as R  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import holdout, wire10  # noqa: E402
from oracle import unet_oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu

N, CUT = 7, 4
SIZES = [(23, 34), (24, 50)]
SRC = dict(raw="yuv422p10le", src_fps="24000/1001")
VARIANTS = {
    "factor2": dict(factor=2),
    "factor4-scene-cut": dict(factor=4, scene_cut=10),
    "fps-60000-1001": dict(fps="60000/1001"),
    "dedup": dict(dedup=0),
    "resize-linear": dict(resize=(16, 20)),
    "resize-area": dict(resize=(16, 20), resize_filter="area"),
}
CHUNKS = [1, 3, None]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def interp(dev):
    m = P.FrameInterpolationUNet(bilinear=True, frame_channels=3, precision="fp16")
    m.load_state_dict(O.make_interpolating_state_dict(n_channels=6, n_classes=3))
    m = m.to(dev).eval()
    yield P.FrameInterpolator(model=m, device="cuda", batch=2)
    torch.cuda.empty_cache()


def _clip(h, w, repeat=False):
    """uint16 [N, samples] yuv422p10le frames: a moving texture with a hard cut (another texture) before frame CUT; repeat:
    frame 3 is frame 2 again."""
    wc = -(-w // 2)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    cy, cx = np.mgrid[0:h, 0:wc].astype(np.float64)
    out = []
    for t in range(N):
        s = 2 * (t - 1 if repeat and t == 3 else t)
        if t < CUT:
            y, u, v = (500 + 380 * np.sin((xx - s) / 5.0) * np.cos(yy / 7.0), 512 + 300 * np.cos((2 * cx - s + cy) / 6.0),
                       512 + 250 * np.sin((2 * cx - s - 0.5 * cy) / 4.0))
        else:
            y, u, v = (200 + 120 * np.cos((xx - s) / 3.0), 700 + 150 * np.sin(cy / 2.0), 300 + 200 * np.sin((2 * cx - s + 2 * cy) / 9.0))
        out.append(np.concatenate([np.clip(np.rint(p), 0, 1023).astype(np.uint16).reshape(-1) for p in (y, u, v)]))
    return np.stack(out)


def _out_size(h, w, kw):
    return (kw["resize"][1], kw["resize"][0]) if "resize" in kw else (h, w)


def _want(interp, d, clip, h, w, kw):
    """The existing route on the unpacked clip -> its output frames, uint16 [n, samples of the output size]."""
    (d / "in.yuv").write_bytes(clip.astype("<u2").tobytes())
    n = interp.interpolate_video(str(d / "in.yuv"), str(d / "want.yuv"), width=w, height=h, **SRC, **kw)
    return np.frombuffer((d / "want.yuv").read_bytes(), "<u2").reshape(n, -1)


@pytest.mark.parametrize("chunk", CHUNKS, ids=lambda c: f"chunk-{c}")
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("h,w", SIZES)
def test_packed_route_is_the_working_route_packed(interp, tmp_path, h, w, variant, chunk):
    kw = dict(VARIANTS[variant], chunk_frames=chunk)
    clip = _clip(h, w, repeat=variant == "dedup")
    want = _want(interp, tmp_path, clip, h, w, kw)
    oh, ow = _out_size(h, w, kw)
    assert want.shape[1] == R.planar_samples(oh, ow) and want.shape[0] > N
    for p in R.PACKINGS:
        (tmp_path / f"in.{p}").write_bytes(R.pack(clip, h, w, p).tobytes())
        n = interp.interpolate_video(str(tmp_path / f"in.{p}"), str(tmp_path / f"out.{p}"), width=w, height=h, packing=p,
                                     **SRC, **kw)
        got = (tmp_path / f"out.{p}").read_bytes()
        assert n == want.shape[0] and len(got) == n * R.frame_bytes(p, oh, ow), p
        assert got == R.pack(want, oh, ow, p).tobytes(), p
    assert not [f for f in tmp_path.iterdir() if f.name.endswith(".part")]


@pytest.mark.parametrize("chunk", [3, None], ids=lambda c: f"chunk-{c}")
def test_a_pipe_source_and_a_file_object_sink(interp, tmp_path, chunk):
    h, w = SIZES[1]
    kw = dict(factor=2, scene_cut=10, chunk_frames=chunk)
    clip = _clip(h, w)
    want = _want(interp, tmp_path, clip, h, w, kw)
    for p in R.PACKINGS:
        data = R.pack(clip, h, w, p).tobytes()
        rd, wr = os.pipe()

        def feed():
            with os.fdopen(wr, "wb") as f:
                for i in range(0, len(data), 1000):   # (pieces that are no whole frames)
                    f.write(data[i:i + 1000])
        t = threading.Thread(target=feed)
        t.start()
        sink = io.BytesIO()
        with os.fdopen(rd, "rb") as src:
            n = interp.interpolate_video(src, sink, width=w, height=h, packing=p, **SRC, **kw)
        t.join()
        assert n == want.shape[0] and sink.getvalue() == R.pack(want, h, w, p).tobytes(), p


def test_a_truncated_pipe_is_an_error_at_that_point(interp):
    h, w = SIZES[0]
    data = R.pack(_clip(h, w), h, w, "v210").tobytes()[:-10]
    with pytest.raises(ValueError, match="ends inside a frame"):
        interp.interpolate_video(io.BytesIO(data), io.BytesIO(), width=w, height=h, packing="v210", chunk_frames=3, **SRC)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in ("frames", "triplets", "bits", "peak", "planes", "methods", "fps"):
        assert a[k] == b[k], k
    assert np.array_equal(a["scored_frames"], b["scored_frames"])
    for m in a["methods"]:
        for pl in a["planes"]:
            for k in ("psnr", "ssim", "sse"):
                assert np.array_equal(a["per_frame"][m][pl][k], b["per_frame"][m][pl][k], equal_nan=True), (m, pl, k)
            for k, v in a["summary"][m][pl].items():
                assert v == b["summary"][m][pl][k] or (np.isnan(v) and np.isnan(b["summary"][m][pl][k])), (m, pl, k)
    for k in ("scene_scores", "cut_intervals", "excluded_frames", "excluded", "resize", "source_size"):
        if k in a:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("kw", [dict(), dict(scene_cut=10, chunk_frames=2), dict(resize=(16, 20), triplets="disjoint")],
                         ids=["plain", "scene-cut-chunk-2", "resize-disjoint"])
def test_score_video_equals_the_unpacked_clip(interp, tmp_path, kw):
    h, w = SIZES[0]
    clip = _clip(h, w)
    (tmp_path / "in.yuv").write_bytes(clip.astype("<u2").tobytes())
    src = dict(raw="yuv422p10le", width=w, height=h, src_fps=24)
    want = holdout.score_video(interp.model, str(tmp_path / "in.yuv"), **src, **kw)
    assert want["frames"] == N and want["bits"] == 10
    for p in R.PACKINGS:
        (tmp_path / f"in.{p}").write_bytes(R.pack(clip, h, w, p).tobytes())
        _same(holdout.score_video(interp.model, str(tmp_path / f"in.{p}"), packing=p, **src, **kw), want)
        with open(tmp_path / f"in.{p}", "rb") as f:   # a file object: a stream of unknown length
            _same(holdout.score_video(interp.model, f, packing=p, **src, **kw), want)


@pytest.mark.parametrize("h,w", SIZES)
def test_forward_is_its_three_steps(interp, dev, h, w):
    m = interp.model
    clip = _clip(h, w)
    opts = dict(matrix="bt2020", siting="jpeg")
    for p in R.PACKINGS:
        wire = torch.from_numpy(R.pack(clip, h, w, p)).to(dev)
        f1, f2 = wire[:-1][:3], wire[1:][:3]
        got = wire10.forward(m, f1, f2, h, w, p, **opts)
        a, b = wire10.unpack(f1, h, w, p), wire10.unpack(f2, h, w, p)
        assert np.array_equal(a.view(torch.int16).cpu().numpy().view(np.uint16), clip[:3])
        mid = m.forward_yuv(a, b, h, w, format="yuv422p10le", **opts)
        want = wire10.pack(mid, h, w, p)
        assert got.dtype == torch.uint8 and got.shape == (3, R.frame_bytes(p, h, w)) and torch.equal(got, want)
        assert np.array_equal(got.cpu().numpy(), R.pack(mid.view(torch.int16).cpu().numpy().view(np.uint16), h, w, p))
        assert not torch.equal(got, wire[:3])
