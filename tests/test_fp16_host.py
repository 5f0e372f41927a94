"""CPU: precision "fp16" (include/fiunet.h FIUNET_FP16) at the surfaces that need no GPU - the Python names, the ABI
constants and the launch rule.  fp16 has bf16's element size and MFMA shape, so `choose_conv_cfg` must answer for it
exactly what it answers for bf16 (csrc/fiunet.hip: the 2-byte-element predicate)."""
import ctypes
import os
import re

import pytest

import ai_based_frame_interpolation_amd as P
from ai_based_frame_interpolation_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (Cin, Cout, level, concat stage or 0) of convs 1..17 of UNet(bilinear=True), as tests/test_cfg_rule.py sweeps them
CONVS = [(64, 64, 0, 0), (64, 128, 1, 0), (128, 128, 1, 0), (128, 256, 2, 0), (256, 256, 2, 0), (256, 512, 3, 0), (512, 512, 3, 0),
         (512, 512, 4, 0), (512, 512, 4, 0), (1024, 512, 3, 10), (512, 256, 3, 0), (512, 256, 2, 12), (256, 128, 2, 0),
         (256, 128, 1, 14), (128, 64, 1, 0), (128, 64, 0, 16), (64, 64, 0, 0)]


@pytest.mark.parametrize("name", ["fp16", "float16", "half"])
def test_precision_names_are_accepted(name):
    m = P.FrameInterpolationUNet(bilinear=True, precision=name)
    assert m._precision_code() == _native.FP16


def test_bad_precision_name_still_raises_and_lists_fp16():
    with pytest.raises(ValueError, match="fp16"):
        P.FrameInterpolationUNet(bilinear=True, precision="fp8")
    m = P.FrameInterpolationUNet(bilinear=True)
    m.precision = "float64"
    with pytest.raises(ValueError, match="half"):
        m._precision_code()


def test_env_default(monkeypatch):
    monkeypatch.setenv("FIUNET_PRECISION", "fp16")
    assert P.FrameInterpolationUNet(bilinear=True)._precision_code() == _native.FP16


def test_abi_constants():
    assert _native.FP16 == 3 and _native.ABI_VERSION == 8
    hdr = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    assert re.search(r"\bFIUNET_FP16\s*=\s*3\b", hdr)
    assert int(re.search(r"#define FIUNET_ABI_VERSION (\d+)", hdr).group(1)) == 8
    L = _native.lib()
    L.fiunet_abi_version.restype = ctypes.c_int
    assert L.fiunet_abi_version() == 8


@pytest.fixture(scope="module")
def choose():
    fn = _native.lib().fiunet_debug_choose_cfg
    fn.argtypes = [ctypes.c_int] * 9 + [ctypes.POINTER(ctypes.c_int)]

    def call(prec, b, h, w, cin, cout, splittable=True, concat_stage=0, kwave_ok=True):
        out = (ctypes.c_int * 4)()
        assert fn(prec, b, h, w, cin, cout, int(splittable), concat_stage, int(kwave_ok), out) == 0
        return tuple(out)
    return call


def _levels(h, w):
    hs, ws = [h], [w]
    for _ in range(4):
        hs.append(hs[-1] // 2); ws.append(ws[-1] // 2)
    return hs, ws


def test_launch_rule_is_bf16s(choose):
    n = 0
    shapes = [(1080, 1920, (1, 2, 3, 4, 8, 16)), (256, 256, (1, 2, 4, 8, 16)), (720, 1280, (1, 2, 3, 5, 8)),
              (540, 960, (1, 4)), (135, 240, (1, 3)), (2160, 3840, (1,)), (64, 96, (1, 2, 7))]
    for h, w, batches in shapes:
        hs, ws = _levels(h, w)
        for b in batches:
            for i, (cin, cout, lv, cs) in enumerate(CONVS, start=1):
                for splittable in (True, False):
                    for kwave_ok in (True, False):
                        args = (b, hs[lv], ws[lv], cin, cout, splittable, cs, kwave_ok)
                        assert choose(_native.FP16, *args) == choose(_native.BF16, *args), (h, w, b, i, splittable, kwave_ok)
                        n += 1
    assert n > 1000


def test_stage_plan_is_bf16s():
    fn = _native.lib().fiunet_debug_stage_cfg
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.POINTER(ctypes.c_int)]

    def stage(prec, *a):
        out = (ctypes.c_int * 6)()
        assert fn(a[0], a[1], a[2], prec, *a[3:], out) == 0
        return tuple(out)
    for cf, bil in ((1, 1), (3, 1), (1, 0)):
        for flags in (0, _native.OPT_UNFUSED, _native.OPT_KEEP_ALL, _native.OPT_GATHER_UPSAMPLE):
            for b, h, w in ((1, 256, 256), (8, 1080, 1920), (2, 720, 1280), (1, 33, 47)):
                for s in range(18):
                    a = (cf, bil, flags, b, h, w, s)
                    assert stage(_native.FP16, *a) == stage(_native.BF16, *a), a
