"""The table of the video-option matrix (tests/test_video_matrix_host.py holds it to its claims on the CPU,
tests/test_gpu_video_matrix.py runs one case per row on the GPU).  Importing this needs no GPU.

A row names one value on each axis of `AXES` and a clip.  Which rows exist is decided in three steps:

  legal      `legal(row)` asks the product: the public `FrameInterpolator.interpolate_video` is called on a two-frame file of
             the row's source with the engines (`stream._run`, `stream._run_whole`) and `torch.Tensor.pin_memory` replaced
             by a stop (the `no_gpu` stub of tests/test_stream_host.py).  A ValueError before the stop is a refusal, and
             the table never lists a combination as illegal on its own account.
  product    rate x retime x scene_cut x dedup in full on the gray .npy source, every other axis at its neutral value.
             `retime` is documented to have no effect on a run without a plan (no fps, no dedup): `canonical` writes such
             a row with "blend", and the rows that then coincide are one row.
  cover      a greedy pairwise cover of all axes over every source, from a seeded generator (`random.Random(SEED)`, no
             hashes, no set order): the same table on every machine.  `retime` counts as covered by a row only where it
             has an effect (the row has a plan).
  pinned     the rows of `PINNED`, by name.

Clips.  32 x 32 frames (32 wide x 40 high for the "area" rows, which go to 16 wide x 20 high as the "linear" ones do).
The main clip is `PATTERN` of tests/test_gpu_dedup_video.py, made by that file's `_pictures` for every source kind.  The
tolerance-1 rows (dedup 1, max_gap 2) use `NOISE_PATTERN`, whose repeats differ by +-1 per sample and are dead at
tolerance 1 only; its single dead intervals lie where the chunk edges of chunk_frames 3 and 5 fall (with max_gap 2 only a
run of one dead interval makes a span, and PATTERN has none across those edges).  Clips "two" and "one": frames 1-2
and frame 0 of the main clip."""
import atexit
import collections
import itertools
import os
import random
import shutil
import sys
import tempfile
from fractions import Fraction

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (os.path.dirname(HERE), HERE):   # (the package's root too: a job script may import this outside pytest)
    if _p not in sys.path:
        sys.path.insert(0, _p)
import dedup_ref as D  # noqa: E402
import test_gpu_dedup_video as DV  # noqa: E402
import wire10_ref as W10  # noqa: E402

import ai_based_frame_interpolation_amd as P  # noqa: E402
from ai_based_frame_interpolation_amd import imageio_lite as IO  # noqa: E402
from ai_based_frame_interpolation_amd import layout, stream  # noqa: E402

SEED = 20240
THR = 10.0
PATTERN = DV.PATTERN
#             frame     0123456789012345678 9012
NOISE_PATTERN = "ABCCDDEEEEFGGGGGHII|JKKK"
# intervals   2 dead, 3 live: span [2, 4) across edge 3      4 dead, 5 live: span [4, 6) across edge 5
#             6-8 and 11-14 dead: holds (max_gap 2)         17 dead before the cut at 18        20-21 dead: a trailing run
DST = (16, 20)                       # (width, height), as resize= takes it

#: source -> (layout kind, network channels, Y4M tag or None, raw format or None, packing or None)
SOURCES = collections.OrderedDict([
    ("npy-gray", ("npy", 1, None, None, None)),
    ("npy-rgb", (("npy", 3), 3, None, None, None)),
    ("y4m420-gray", (("y4m", "420jpeg"), 1, "420jpeg", None, None)),
    ("y4m420-rgb", (("y4m", "420jpeg"), 3, "420jpeg", None, None)),
    ("y4m422p10-gray", (("y4m", "422p10"), 1, "422p10", None, None)),
    ("nv12", ("nv12", 3, None, "nv12", None)),
    ("rgb24", ("rgb24", 3, None, "rgb24", None)),
    ("yuv422p10le", ("yuv422p10le", 3, None, "yuv422p10le", None)),
    ("v210", ("yuv422p10le", 3, None, "yuv422p10le", "v210")),
    ("p210le", ("yuv422p10le", 3, None, "yuv422p10le", "p210le")),
])
#: rate -> (factor, keywords, source rate, the step of an output frame in input time, G)
RATES = collections.OrderedDict([
    ("x2", (2, {}, (24, 1), Fraction(1, 2), 2)),
    ("x4", (4, {}, (24, 1), Fraction(1, 4), 4)),
    ("24to60-depth2", (2, dict(fps=60, time_depth=2), (24, 1), Fraction(2, 5), 4)),
    ("ntsc-depth3", (2, dict(fps="60000/1001", time_depth=3), (24000, 1001), Fraction(2, 5), 8)),
    ("24to60-depth1", (2, dict(fps=60, time_depth=1), (24, 1), Fraction(2, 5), 2)),
])
AXES = collections.OrderedDict([
    ("source", list(SOURCES)),
    ("rate", list(RATES)),
    ("retime", ["blend", "nearest", "motion"]),
    ("scene_cut", [None, THR]),
    ("dedup", [None, (0, 4), (1, 2), (0, 8)]),          # (tolerance, max_gap)
    ("resize", [None, "linear", "area"]),
    ("chroma", ["average", "motion"]),
    ("precision", ["bf16", "fp16"]),                    # (fp32: the pinned rows)
    ("batch", [2, 8]),
])
NEUTRAL = dict(source="npy-gray", rate="x2", retime="blend", scene_cut=None, dedup=None, resize=None, chroma="average",
               precision="bf16", batch=8)
#: the keyword a refusal's message names when the value on this axis is what the product refuses
KEYWORD = dict(rate=("fps", "factor"), retime=("retime",), scene_cut=("scene_cut",), dedup=("dedup", "max_gap"),
               resize=("resize", "area"), chroma=("chroma",), precision=("precision",), batch=("batch",))
PRODUCT_AXES = ("rate", "retime", "scene_cut", "dedup")

Row = collections.namedtuple("Row", list(AXES) + ["clip"])


def make(clip="main", **values):
    return canonical(Row(clip=clip, **dict(NEUTRAL, **values)))


def has_plan(row) -> bool:
    return "fps" in RATES[row.rate][1] or row.dedup is not None


def canonical(row):
    """`retime` has no effect on a run without a plan (stream._job): such a row is written with "blend"."""
    return row if has_plan(row) or row.retime == "blend" else row._replace(retime="blend")


def row_id(row) -> str:
    def s(v):
        return "none" if v is None else "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
    parts = [row.source, row.rate, row.retime, f"cut-{s(row.scene_cut)}", f"dedup-{s(row.dedup)}", f"resize-{s(row.resize)}",
             f"chroma-{row.chroma}", row.precision, f"b{row.batch}"]
    return "/".join(parts + ([] if row.clip == "main" else [row.clip]))


# ---- clips ----------------------------------------------------------------------------------------------------------------
def size_of(row):
    """(h, w) of a source frame."""
    return (40, 32) if row.resize == "area" else (32, 32)


def out_size_of(row):
    return size_of(row) if row.resize is None else (DST[1], DST[0])


def bits_of(row) -> int:
    return layout.frame_layout(SOURCES[row.source][0], 32, 32).bits


def pattern_of(row) -> str:
    return NOISE_PATTERN if row.dedup is not None and row.dedup[0] == 1 else PATTERN


def _noise_pictures(pattern, samples, bits, seed):
    """`_pictures` of the pattern; the odd repeats of a letter inside a run carry a pattern of -1 / 0 / +1 of their own,
    so that two neighbours of a run differ by at most 1 in every sample (a peak of at most 64: dead at tolerance 1) and
    by 1 in about two thirds of them (not dead at tolerance 0)."""
    hi = 256 if bits == 8 else 1024
    base = np.clip(DV._pictures(pattern, samples, bits, seed), 1, hi - 2)
    rng = np.random.default_rng(seed + 1)
    letters, out, k = [c for c in pattern if c != "|"], [], 0
    for i, ch in enumerate(letters):
        k = k + 1 if i and letters[i - 1] == ch else 0
        out.append(base[i] + (rng.integers(-1, 2, samples) if k % 2 else 0))
    return np.stack(out).astype(base.dtype)


_clips = {}


def frames_of(row) -> np.ndarray:
    """[N, samples] frames of the row's clip as its route stores them (uint8, or uint16 words of 10-bit codes)."""
    h, w = size_of(row)
    kind = SOURCES[row.source][0]
    key = (kind, h, w, pattern_of(row))
    if key not in _clips:
        lay = layout.frame_layout(kind, h, w)
        make_ = _noise_pictures if key[3] == NOISE_PATTERN else DV._pictures
        _clips[key] = make_(key[3], lay.samples, lay.bits, seed=7)
    frames = _clips[key]
    return {"main": frames, "two": frames[1:3], "one": frames[:1]}[row.clip]


def flags_of(row, frames=None):
    """(dead, cuts) of the clip on the host, from the definitions (tests/dedup_ref.py, tests/scene_ref.py): lists with
    one truth value per interval; dead is None without dedup, cuts None without scene_cut.  `frames`: the frames the
    route sees where they are not the source's (a resized clip)."""
    import scene_ref
    frames = frames_of(row) if frames is None else frames
    bits = bits_of(row)
    dead = None if row.dedup is None else D.dead_of(D.pair_peak(frames, bits), row.dedup[0])
    cuts = None
    if row.scene_cut is not None:
        cuts = [bool(v) for v in scene_ref.detect(frames, row.scene_cut, bits)[1]] if frames.shape[0] > 1 else []
    return dead, cuts


def write_source(row, frames, path_stem, size=None):
    """The frames as a file of the row's source kind -> (path, extension, the source's keywords).  size: (h, w) of the
    frames where it is not the row's own source size (a clip resized beforehand)."""
    kind, _, tag, raw, packing = SOURCES[row.source]
    h, w = size_of(row) if size is None else size
    rate = RATES[row.rate][2]
    src_fps = Fraction(*rate)
    if kind == "npy" or (isinstance(kind, tuple) and kind[0] == "npy"):
        path = path_stem + ".npy"
        np.save(path, frames.reshape((-1, h, w) if kind == "npy" else (-1, h, w, kind[1])))
        return path, ".npy", dict(src_fps=src_fps)
    if tag is not None:
        path = path_stem + ".y4m"
        with IO.Y4MWriter(path, w, h, rate, tag, None, bits=bits_of(row)) as wr:
            wr.write(frames)
        return path, ".y4m", {}
    path, kw = path_stem + ".raw", dict(raw=raw, width=w, height=h, src_fps=src_fps)
    if packing is not None:
        frames, kw["packing"] = W10.pack(frames, h, w, packing), packing
    np.ascontiguousarray(frames).tofile(path)
    return path, ".raw", kw


def read_output(row, path, size=None) -> np.ndarray:
    """[n, samples] frames of an output file, as the route stores them (a packed output: unpacked on the host)."""
    kind, _, tag, raw, packing = SOURCES[row.source]
    h, w = out_size_of(row) if size is None else size
    if tag is None and raw is None:
        a = np.load(path)
        return a.reshape(a.shape[0], -1)
    if tag is not None:
        return (IO.read_y4m_packed if bits_of(row) == 8 else IO.read_y4m_packed_p10)(path)[0]
    if packing is not None:
        wire = np.fromfile(path, np.uint8).reshape(-1, W10.frame_bytes(packing, h, w))
        return np.ascontiguousarray(W10.unpack(wire, h, w, packing))
    a = np.fromfile(path, np.uint8 if bits_of(row) == 8 else np.uint16)
    return a.reshape(-1, layout.frame_layout(kind, h, w).samples)


def call_keywords(row):
    """-> (factor, the keywords of `interpolate_video` that the row's options set; the source's come from write_source)."""
    factor, kw = RATES[row.rate][0], dict(RATES[row.rate][1])
    kw.update(retime=row.retime, scene_cut=row.scene_cut)
    if row.dedup is not None:
        kw.update(dedup=row.dedup[0], max_gap=row.dedup[1])
    if row.resize is not None:
        kw.update(resize=DST, resize_filter=row.resize)
    if row.chroma != "average":
        kw.update(chroma=row.chroma)
    return factor, kw


def look_of(row) -> int:
    """The lookahead frames of a streamed chunk (stream._run's `look`)."""
    if row.dedup is None:
        return 1 if row.scene_cut is not None else 0
    return row.dedup[1] if row.scene_cut is not None else row.dedup[1] - 1


def chunk_sizes(row):
    return [1, 3, 5] + ([row.dedup[1] + 1] if row.dedup is not None and row.dedup[1] + 1 not in (1, 3, 5) else [])


# ---- legal: the product's answer --------------------------------------------------------------------------------------------
class _Started(Exception):
    """The stub's stop: every host-side check has passed and the engine was about to run."""


_tmp = None
_legal = {}
_cpu_models = {}


def _tmp_dir():
    global _tmp
    if _tmp is None:
        _tmp = tempfile.mkdtemp(prefix="video_matrix_")
        atexit.register(shutil.rmtree, _tmp, ignore_errors=True)
    return _tmp


def _cpu_interpolator(fc, precision, batch):
    if (fc, precision) not in _cpu_models:
        _cpu_models[(fc, precision)] = P.FrameInterpolationUNet(bilinear=True, frame_channels=fc, precision=precision)
    return P.FrameInterpolator(model=_cpu_models[(fc, precision)], device="cpu", batch=batch)


def legal(row):
    """-> (True, None) where every check of the public entry point passes, or (False, the ValueError) where it refuses
    the row before any device work; the output path must not exist after a refusal.  Both the streamed and the resident
    call are asked, and they must agree."""
    key = row._replace(clip="main")
    if key in _legal:
        return _legal[key]
    h, w = size_of(row)
    lay = layout.frame_layout(SOURCES[row.source][0], h, w)
    stem = os.path.join(_tmp_dir(), f"s{len(_legal)}")
    tiny = np.zeros((2, lay.samples), np.uint8 if lay.bits == 8 else np.uint16)
    src, ext, skw = write_source(row, tiny, stem)
    factor, kw = call_keywords(row)
    fi = _cpu_interpolator(SOURCES[row.source][1], row.precision, row.batch)

    def stop(*a, **k):
        raise _Started()
    saved = (stream._run, stream._run_whole, torch.Tensor.pin_memory)
    stream._run = stream._run_whole = torch.Tensor.pin_memory = stop
    answers = []
    try:
        for cf in (3, None):
            dst = stem + f"-out{cf}" + ext
            try:
                fi.interpolate_video(src, dst, factor, chunk_frames=cf, **skw, **kw)
                raise AssertionError(f"{row_id(row)}: the call returned without reaching an engine")
            except _Started:
                answers.append((True, None))
            except ValueError as e:
                answers.append((False, e))
                assert not os.path.exists(dst) and not os.path.exists(dst + ".part"), (row_id(row), "an output exists")
            for p in (dst, dst + ".part"):
                if os.path.exists(p):
                    os.remove(p)
    finally:
        stream._run, stream._run_whole, torch.Tensor.pin_memory = saved
        os.remove(src)
    assert answers[0][0] == answers[1][0], (row_id(row), "the streamed and the resident call disagree", answers)
    _legal[key] = answers[0]
    return _legal[key]


def is_legal(row) -> bool:
    return legal(row)[0]


def blamed_axes(row):
    """The axes of a refused row whose value, set back to neutral on its own, makes the row legal."""
    return [a for a in AXES if a != "source" and getattr(row, a) != NEUTRAL[a]
            and is_legal(canonical(row._replace(**{a: NEUTRAL[a]})))]


# ---- coverage ---------------------------------------------------------------------------------------------------------------
def pairs_of(row):
    """The (axis, value) pairs a row covers; `retime` only where it has an effect."""
    items = [(a, getattr(row, a)) for a in AXES if a != "retime" or has_plan(row)]
    return set(itertools.combinations(items, 2))


def all_pairs():
    out = []
    for a, b in itertools.combinations(AXES, 2):
        out += [((a, u), (b, v)) for u in AXES[a] for v in AXES[b]]
    return out


def all_triples():
    """Every triple of values of three of PRODUCT_AXES, written canonically (a list without repeats)."""
    out = []
    for axes in itertools.combinations(PRODUCT_AXES, 3):
        for vals in itertools.product(*(AXES[a] for a in axes)):
            out.append(tuple(zip(axes, vals)))
    return out


def triples_of(row):
    items = [(a, getattr(row, a)) for a in PRODUCT_AXES]
    return set(itertools.combinations(items, 3))


def completions(fixed):
    """Rows that hold the (axis, value) items of `fixed` with every other axis neutral, over every source and, for a
    retime value, over a rate with a plan: where none of them is legal the product refuses the combination (a neutral
    value adds no refusal of its own)."""
    fixed = dict(fixed)
    sources = [fixed["source"]] if "source" in fixed else list(SOURCES)
    rates = [fixed["rate"]] if "rate" in fixed else ["x2", "24to60-depth2"]
    dedups = [fixed["dedup"]] if "dedup" in fixed else [None, (0, 4)]
    return [canonical(Row(clip="main", **dict(NEUTRAL, **dict(fixed, source=s, rate=r, dedup=d))))
            for s in sources for r in rates for d in dedups]


def refused(fixed) -> bool:
    return not any(is_legal(r) and set(dict(fixed).items()) <= set(r._asdict().items()) for r in completions(fixed))


# ---- the rows -----------------------------------------------------------------------------------------------------------------
def product_rows():
    out = []
    for vals in itertools.product(*(AXES[a] for a in PRODUCT_AXES)):
        row = make(**dict(zip(PRODUCT_AXES, vals)))
        if row not in out and is_legal(row):
            out.append(row)
    return out


def cover_rows(have):
    """The greedy pass: for the first pair (in `all_pairs` order) that no row has yet, 40 seeded completions of it are
    drawn; the legal one that adds most new pairs becomes a row.  A pair without a legal draw is tried on `completions`;
    if the product refuses those too, the pair is a refusal (`refused`), and the host test checks that it is."""
    rng = random.Random(SEED)
    covered = set()
    for r in have:
        covered |= pairs_of(r)
    out = []
    for pair in all_pairs():
        if pair in covered:
            continue
        fixed = dict(pair)
        draws = []
        for _ in range(40):
            vals = {a: (fixed[a] if a in fixed else rng.choice(AXES[a])) for a in AXES}
            draws.append(canonical(Row(clip="main", **vals)))
        draws += completions(pair)
        best, gain = None, 0
        for r in draws:
            if pair in pairs_of(r) and is_legal(r):
                g = len(pairs_of(r) - covered)
                if g > gain:
                    best, gain = r, g
        if best is not None:
            out.append(best)
            covered |= pairs_of(best)
    return out


#: name -> row.  The rows the issue pins, and under "found-" the smallest rows that exposed a bug, kept.
PINNED = collections.OrderedDict([
    ("motion-dedup8-cuts-y4m420", make(source="y4m420-gray", rate="24to60-depth2", retime="motion", scene_cut=THR,
                                       dedup=(0, 8))),
    ("chroma-motion-dedup-fps", make(source="y4m420-gray", rate="24to60-depth2", dedup=(0, 4), chroma="motion")),
    ("v210-area-dedup-cuts", make(source="v210", rate="x2", scene_cut=THR, dedup=(0, 4), resize="area", precision="fp16")),
    ("rgb-y4m-dedup12-x4", make(source="y4m420-rgb", rate="x4", dedup=(1, 2))),
    ("fp32-fps-dedup-cuts-gray", make(source="npy-gray", rate="24to60-depth2", scene_cut=THR, dedup=(0, 4),
                                      precision="fp32")),
    ("fp32-fps-dedup-cuts-rgb", make(source="rgb24", rate="24to60-depth2", scene_cut=THR, dedup=(0, 4), precision="fp32")),
    ("two-frames-dedup-cuts-fps", make("two", rate="24to60-depth2", scene_cut=THR, dedup=(0, 4))),
    ("one-frame-dedup-cuts-fps", make("one", rate="24to60-depth2", scene_cut=THR, dedup=(0, 4))),
    ("two-frames-y4m-motion-x4", make("two", source="y4m420-gray", rate="x4", retime="motion", scene_cut=THR, dedup=(0, 8),
                                      chroma="motion")),
    ("one-frame-v210-resize", make("one", source="v210", rate="x4", scene_cut=THR, dedup=(1, 2), resize="linear",
                                   precision="fp16")),
])

_rows = None


def rows():
    """Every row of the table, in a fixed order, without repeats: the product, the cover, the pinned rows."""
    global _rows
    if _rows is None:
        out = product_rows()
        out += [r for r in cover_rows(out) if r not in out]
        out += [r for r in PINNED.values() if r not in out]
        _rows = out
    return _rows
