"""CPU: the surface of the device-side weight preparation (fiunet_load_weights_device, weight_prep="host" | "device") -
the header, the binding, the library's exports and host-side argument checks, and the validation of `weight_prep` on
the module, load_model, the service and the CLI.  What the kernels compute is tests/test_gpu_weight_prep.py's."""
import ctypes
import os
import re

import pytest

from ai_based_frame_interpolation_amd import _native, cli
from ai_based_frame_interpolation_amd.inference import load_model
from ai_based_frame_interpolation_amd.serving import InterpolationService
from ai_based_frame_interpolation_amd.unet import FrameInterpolationUNet, GraphedForward  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = "fiunet_load_weights_device"
DIAGNOSTIC = "fiunet_debug_weight_buffer"


def _header():
    src = open(os.path.join(ROOT, "include", "fiunet.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_and_binding_declare_the_device_load():
    src = _header()
    m = re.search(r"int\s+fiunet_load_weights_device\s*\(([^)]*)\)", src)
    assert m, "include/fiunet.h does not declare fiunet_load_weights_device"
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 6 and args[0] == "fiunet_ctx* ctx" and args[-1] == "void* stream"
    assert NEW in _native.SYMBOLS
    # added without a version bump, and not at the tail (older tests read the newest block off it)
    assert re.search(r"#define FIUNET_ABI_VERSION 8\b", src) and _native.ABI_VERSION == 8
    assert _native.SYMBOLS.index(NEW) == _native.SYMBOLS.index("fiunet_load_weights") + 1
    # the diagnostic is no part of the ABI
    assert DIAGNOSTIC not in src and DIAGNOSTIC not in _native.SYMBOLS
    assert _native.WEIGHT_PREPS == ("host", "device")


def test_library_exports_the_device_load_and_its_kernels(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    assert hasattr(lib, NEW) and hasattr(lib, DIAGNOSTIC)
    blob = open(hip_lib_built, "rb").read()
    for kernel in (b"wp_fold_bn_kernel", b"wp_pack_f32_kernel", b"wp_pack_bf16_rne_kernel",
                   b"wp_pack_bf16_feedback_kernel", b"wp_stem_split_kernel"):
        assert kernel in blob, kernel


def test_null_arguments_are_refused_without_a_gpu(hip_lib_built):
    lib = _native.lib()
    lib.fiunet_last_error_string.restype = ctypes.c_char_p
    fake_ctx = ctypes.create_string_buffer(1 << 16)   # never read: the NULL checks come first
    ctx = ctypes.cast(fake_ctx, ctypes.c_void_p)
    names = (ctypes.c_char_p * 1)(b"unet.outc.conv.bias")
    ptrs = (ctypes.c_void_p * 1)(None)
    numels = (ctypes.c_int64 * 1)(1)
    assert lib.fiunet_load_weights_device(None, 1, names, ptrs, numels, None) == 1   # FIUNET_ERR_INVALID_ARG
    assert b"NULL" in lib.fiunet_last_error_string()
    assert lib.fiunet_load_weights_device(ctx, 1, None, ptrs, numels, None) == 1
    assert lib.fiunet_load_weights_device(ctx, 1, names, None, numels, None) == 1
    assert lib.fiunet_load_weights_device(ctx, 1, names, ptrs, None, None) == 1
    assert lib.fiunet_load_weights_device(ctx, -1, names, ptrs, numels, None) == 1
    fn = lib.fiunet_debug_weight_buffer
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                   ctypes.POINTER(ctypes.c_size_t)]
    p, b = ctypes.c_void_p(), ctypes.c_size_t()
    assert fn(None, 0, 0, ctypes.byref(p), ctypes.byref(b)) == 1
    assert fn(ctx, 0, 0, None, ctypes.byref(b)) == 1
    assert fn(ctx, 23, 0, ctypes.byref(p), ctypes.byref(b)) == 1 and fn(ctx, 0, 6, ctypes.byref(p), ctypes.byref(b)) == 1


def test_module_validates_weight_prep_like_precision(monkeypatch):
    monkeypatch.delenv("FIUNET_WEIGHT_PREP", raising=False)
    assert FrameInterpolationUNet(bilinear=True).weight_prep == "host"          # the default does not change
    assert FrameInterpolationUNet(bilinear=True, weight_prep="device").weight_prep == "device"
    with pytest.raises(ValueError, match="weight_prep must be one of"):
        FrameInterpolationUNet(bilinear=True, weight_prep="gpu")
    m = FrameInterpolationUNet(bilinear=True)
    m.weight_prep = "nonsense"          # a plain attribute, validated where it is used
    with pytest.raises(ValueError, match="weight_prep must be one of"):
        m._weight_prep_checked()
    # a changed weight_prep makes the prepared weights stale: the load before was made with another one
    m.weight_prep = "device"
    m._prep_loaded = "host"
    assert m._weight_prep_checked() != m._prep_loaded


def test_env_default_is_honoured(monkeypatch):
    monkeypatch.setenv("FIUNET_WEIGHT_PREP", "device")
    assert FrameInterpolationUNet(bilinear=True).weight_prep == "device"
    assert FrameInterpolationUNet(bilinear=True, weight_prep="host").weight_prep == "host"   # the argument wins
    monkeypatch.setenv("FIUNET_WEIGHT_PREP", "bogus")
    with pytest.raises(ValueError, match="weight_prep must be one of"):
        FrameInterpolationUNet(bilinear=True)


def test_load_model_service_and_binding_validate(monkeypatch, tmp_path):
    monkeypatch.delenv("FIUNET_WEIGHT_PREP", raising=False)
    with pytest.raises(ValueError, match="weight_prep must be one of"):
        load_model(str(tmp_path / "absent.pth"), "cuda", weight_prep="fast")
    with pytest.raises(FileNotFoundError):          # a valid value gets as far as the file
        load_model(str(tmp_path / "absent.pth"), "cuda", weight_prep="device")
    m = FrameInterpolationUNet(bilinear=True).eval()
    assert InterpolationService(model=m).model.weight_prep == "host"
    assert InterpolationService(model=m, weight_prep="device").model.weight_prep == "device"
    with pytest.raises(ValueError, match="weight_prep must be one of"):
        InterpolationService(model=m, weight_prep="both")
    assert m.weight_prep == "device"   # a refused value leaves the caller's model as it was
    ctx = _native.Context.__new__(_native.Context)   # no GPU here: the check precedes every native call
    ctx._h = None
    with pytest.raises(ValueError, match="prep must be one of"):
        ctx.load_state_dict({}, prep="gpu")


@pytest.mark.parametrize("command", ["video", "evaluate"])
def test_cli_takes_weight_prep_where_it_takes_a_model(command, capsys):
    base = [command, "--input", "in.y4m"] + (["--output", "out.y4m"] if command == "video" else [])
    assert cli.parse_args(base).weight_prep is None
    assert cli.parse_args(base + ["--weight-prep", "device"]).weight_prep == "device"
    assert cli.parse_args(base + ["--weight-prep", "host"]).weight_prep == "host"
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--weight-prep", "gpu"])
    assert "--weight-prep" in capsys.readouterr().err
