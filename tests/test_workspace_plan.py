"""CPU: the workspace layout of a forward (csrc/fiunet.hip `make_plan`) through the diagnostic entry point
`fiunet_debug_plan` - pure host arithmetic, no device call.  Every activation, pooled tensor, materialised upsampled half,
the ablation path's concat scratch and the split-K slab has a live interval [writer stage, last reader stage]; buffers
whose intervals do not overlap share bytes.  tests/test_stage_plan.py pins how the stages launch; this file pins where
their tensors live.  Everything expected here is recomputed from the tables below (the architecture: unet.py:65-95 of the
reference), never asked of the library:
  * offsets are multiples of 256, every buffer ends inside `total`, and `total` is the largest end;
  * two buffers that are live at the same stage never share a byte (under KEEP_ALL: no two buffers at all);
  * a buffer holds at least the tensor it is for;
  * whatever a conv stage reads - as `fiunet_debug_stage_cfg` reports its form - and what it writes is live at that stage;
  * the slab holds every K cut's partial sums, in the small tile and in whichever tuned tile has more tiles;
  * a stage that is not stored (fused stem, fused head) has no record, every other exactly one;
  * sharing never costs bytes: the default plan is no larger than KEEP_ALL's, and B=8 1080p bf16 fits the figure the
    comment above make_plan states."""
import ctypes

import pytest

from ai_based_frame_interpolation_amd import _native

FP32, BF16, BF16X2, FP16 = _native.FP32, _native.BF16, _native.BF16X2, _native.FP16
KEEP_ALL = _native.OPT_KEEP_ALL
# source forms (csrc/fiunet.hip SrcForm), stage 0's (StemForm) and the epilogues (csrc/conv3x3_mfma.hip.h Epilogue)
DIRECT, POOL, GATHER, UP, CONVT, UPCAT, STEM = range(7)
STEM_FUSED = 0
EPI_PLAIN, EPI_HEAD, EPI_POOL, EPI_HEAD3 = range(4)
# output channels of convs 0..17 (/root/reference/model/unet.py:65-82) and their level
COUT = {True: [64, 64, 128, 128, 256, 256, 512, 512, 512, 512, 512, 256, 256, 128, 128, 64, 64, 64],
        False: [64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024, 512, 512, 256, 256, 128, 128, 64, 64]}
LEVEL = [0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0]
SKIP = {10: 7, 12: 5, 14: 3, 16: 1}   # concat convs: skip source; the low-res source is conv i - 1
POOL_SRC = {2: 1, 4: 3, 6: 5, 8: 7}   # convs that read MaxPool2d(2) of a conv's output: that conv
END = 18                              # "still live after the last conv"
ES = {FP32: 4, BF16: 2, BF16X2: 4, FP16: 2}
SLAB_TILE = {"small": 64 * 8 * 32, "tuned": 32768}   # fp32 partial sums per tile

_FLAGS = {"default": 0, "unfused": _native.OPT_UNFUSED, "keep_all": KEEP_ALL,
          "gather_upsample": _native.OPT_GATHER_UPSAMPLE}
_ARCHS = {"gray": (1, True), "gray_convt": (1, False), "rgb": (3, True)}
_PRECS = {"fp32": FP32, "bf16": BF16, "bf16x2": BF16X2, "fp16": FP16}
_BATCHES = (1, 2, 5, 16)
_SHAPES = ((16, 16), (17, 31), (33, 47), (64, 96), (135, 240), (270, 480), (1080, 1920))
_SWEEP = [pytest.param(_PRECS[p], *_ARCHS[a], _FLAGS[f], id=f"{p}-{a}-{f}") for p in _PRECS for a in _ARCHS for f in _FLAGS]


@pytest.fixture(scope="module")
def stage():
    fn = _native.lib().fiunet_debug_stage_cfg
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]

    def call(prec, b, h, w, i, cf=1, bilinear=True, flags=0):
        out = (ctypes.c_int * 6)()
        assert fn(cf, int(bilinear), flags, prec, b, h, w, i, out) == 0
        return {"small": bool(out[0]), "ksplit": out[1], "kwave": bool(out[2]), "form": out[4], "epi": out[5]}
    return call


def _levels(h, w):
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append(hs[-1] // 2); ws.append(ws[-1] // 2)
    return hs, ws


def _ceil(a, b):
    return (a + b - 1) // b


def _slab_need(c, b, h, w, cout):
    """Bytes of fp32 partial sums a K cut of `c["ksplit"]` slices writes for a b x h x w x cout output."""
    if c["small"]:
        return c["ksplit"] * b * _ceil(h, 8) * _ceil(w, 32) * (cout // 64) * SLAB_TILE["small"] * 4
    shapes, bn = (((16, 32), (32, 16)), 64) if cout == 64 else (((8, 32), (16, 16)), 128)
    tiles = max(b * _ceil(h, th) * _ceil(w, tw) * (cout // bn) for th, tw in shapes)
    return c["ksplit"] * tiles * SLAB_TILE["tuned"] * 4


def _check_plan(stage, prec, cf, bilinear, flags, b, h, w):
    """Every per-plan assertion of the module docstring on one plan; -> total."""
    recs, total = _native.debug_plan(cf, bilinear, flags, prec, b, h, w)
    where = (prec, cf, bilinear, flags, b, h, w)
    cout, es, (hs, ws) = COUT[bilinear], ES[prec], _levels(h, w)
    keep_all = bool(flags & KEEP_ALL)
    st = [stage(prec, b, h, w, i, cf, bilinear, flags) for i in range(18)]

    # ---- the byte ranges
    assert recs and total == max(r["offset"] + r["bytes"] for r in recs), where
    for r in recs:
        assert r["offset"] % 256 == 0 and r["offset"] >= 0 and r["bytes"] > 0, (where, r)
        assert r["offset"] + r["bytes"] <= total, (where, r)
        assert 0 <= r["first"] <= r["last"] <= END, (where, r)
    for k, r in enumerate(recs):
        for q in recs[:k]:
            if keep_all or (r["first"] <= q["last"] and q["first"] <= r["last"]):
                assert r["offset"] + r["bytes"] <= q["offset"] or q["offset"] + q["bytes"] <= r["offset"], (where, r, q)

    # ---- one record per stored tensor, none for a stage that is not stored
    by = {}
    for r in recs:
        key = (r["kind"], r["index"])
        assert key not in by, (where, r)
        by[key] = r
    stored = [not (i == 0 and st[0]["form"] == STEM_FUSED) and
              not (i == 17 and st[17]["epi"] in (EPI_HEAD, EPI_HEAD3) and not keep_all) for i in range(18)]
    ups = [i for i in SKIP if st[i]["form"] in (UP, CONVT)]
    upcat = any(st[i]["form"] == UPCAT for i in SKIP)
    want = ({("act", i) for i in range(18) if stored[i]} | {("pool", k) for k in range(4)} | {("up", i) for i in ups} |
            ({("scratch", 0)} if upcat else set()) | {("slab", 0)})
    assert set(by) == want, (where, sorted(set(by) ^ want))

    # ---- each holds its tensor
    def px(lv):
        return b * hs[lv] * ws[lv]
    for i in range(18):
        if stored[i]:
            assert by["act", i]["bytes"] >= px(LEVEL[i]) * cout[i] * es, (where, i)
    for k in range(4):
        assert by["pool", k]["bytes"] >= px(k + 1) * cout[2 * k + 1] * es, (where, k)
    for i in ups:
        c_up = cout[i - 1] // 2 if st[i]["form"] == CONVT else cout[i - 1]
        assert by["up", i]["bytes"] >= px(LEVEL[i]) * c_up * es, (where, i)
    if upcat:
        assert by["scratch", 0]["bytes"] >= b * h * w * 128 * es, where

    # ---- what stage i reads and writes is live at stage i
    def live(key, i):
        assert key in by, (where, key, i)
        assert by[key]["first"] <= i <= by[key]["last"], (where, i, by[key])
    slab = by["slab", 0]
    for i in range(1, 18):
        f = st[i]["form"]
        if f == DIRECT:
            live(("act", i - 1), i)
        elif f == POOL:
            assert POOL_SRC[i] == i - 1
            live(("pool", LEVEL[i] - 1), i)
            assert by["pool", LEVEL[i] - 1]["first"] <= POOL_SRC[i], (where, i)     # its producer's epilogue may write it
            if st[i - 1]["epi"] != EPI_POOL:   # the ablation path pools right before the conv, from the activation
                live(("act", POOL_SRC[i]), i)
        elif f in (GATHER, UP, CONVT, UPCAT):
            live(("act", SKIP[i]), i)
            live(("act", i - 1), i)
            if f in (UP, CONVT):
                live(("up", i), i)
            if f == UPCAT:
                live(("scratch", 0), i)
        else:
            assert f == STEM and i == 1, (where, i, f)
        if st[i]["epi"] == EPI_POOL:   # it also writes MaxPool2d(2) of its output
            live(("pool", LEVEL[i]), i)
        if stored[i]:
            live(("act", i), i)
            assert by["act", i]["first"] == i, (where, i)
        live(("slab", 0), i)
        if st[i]["ksplit"] > 1:
            assert _slab_need(st[i], b, hs[LEVEL[i]], ws[LEVEL[i]], cout[i]) <= slab["bytes"], (where, i, st[i])
    if stored[17]:   # read after the last conv: the ablation path's 1x1 head, the debug read-back
        assert by["act", 17]["last"] == END, where
    if keep_all:     # the read-back reads every tensor after the forward
        assert all(r["last"] == END for r in recs), where
    return total


@pytest.mark.parametrize("prec,cf,bilinear,flags", _SWEEP)
def test_plan_over_shapes_architectures_and_options(stage, prec, cf, bilinear, flags):
    for b in _BATCHES:
        for h, w in _SHAPES:
            total = _check_plan(stage, prec, cf, bilinear, flags, b, h, w)
            if flags == 0:   # sharing bytes never costs any
                assert total <= _native.debug_plan(cf, bilinear, KEEP_ALL, prec, b, h, w)[1], (b, h, w)


def test_sharing_keeps_batch8_1080p_bf16_within_the_stated_figure(stage):
    """The comment above make_plan: "B=8 1080p bf16 needs 6.2 GB this way instead of the 12.7 GB of one private buffer per
    tensor ... (17.0 GB there)" under KEEP_ALL.  No layout can take less than what is live at once at the fullest stage."""
    total = _check_plan(stage, BF16, 1, True, 0, 8, 1080, 1920)
    assert total <= 6.2e9, total
    recs, _ = _native.debug_plan(1, True, 0, BF16, 8, 1080, 1920)
    private = sum(r["bytes"] for r in recs)
    assert 12.7e9 <= private < 12.8e9, private
    assert total >= max(sum(r["bytes"] for r in recs if r["first"] <= i <= r["last"]) for i in range(18))
    keep = _check_plan(stage, BF16, 1, True, KEEP_ALL, 8, 1080, 1920)
    assert 16.9e9 < keep <= 17.0e9, keep


def test_bad_arguments_are_refused():
    fn = _native.lib().fiunet_debug_plan
    _native.debug_plan(1, True, 0, BF16, 1, 16, 16)   # (sets the argument types)
    recs, n, total = (ctypes.c_longlong * (6 * 64))(), ctypes.c_int(), ctypes.c_ulonglong()
    ok = (1, 1, 0, BF16, 1, 16, 16)
    for bad in ((2, 1, 0, BF16, 1, 16, 16), (1, 1, 0, 4, 1, 16, 16), (1, 1, 0, -1, 1, 16, 16), (1, 1, 0, BF16, 0, 16, 16),
                (1, 1, 0, BF16, 1, 15, 16), (1, 1, 0, BF16, 1, 16, 15)):
        assert fn(*bad, recs, 64, ctypes.byref(n), ctypes.byref(total)) == 1, bad      # FIUNET_ERR_INVALID_ARG
    assert fn(*ok, None, 64, ctypes.byref(n), ctypes.byref(total)) == 1
    assert fn(*ok, recs, 64, None, ctypes.byref(total)) == 1
    assert fn(*ok, recs, 64, ctypes.byref(n), None) == 1
    # too few records: refused, with the count it needs, and nothing written
    recs[0] = -7
    assert fn(*ok, recs, 3, ctypes.byref(n), ctypes.byref(total)) == 1 and n.value > 3 and recs[0] == -7
    assert fn(*ok, recs, n.value, ctypes.byref(n), ctypes.byref(total)) == 0 and recs[0] != -7
    # 2^26 pixels or more: no plan (such frames go band by band)
    assert fn(1, 1, 0, BF16, 1, 8192, 8192, recs, 64, ctypes.byref(n), ctypes.byref(total)) == 2   # FIUNET_ERR_BAD_SHAPE
    with pytest.raises(_native.NativeError):
        _native.debug_plan(1, True, 0, BF16, 1, 8, 16)
