"""CPU: how the native library is built - csrc/Makefile's dependency rules and _native.build's job count.  Nothing here
compiles: make is only asked (-q, -n) what it would do.

What the rules promise: an edited header makes the library stale, whichever header it is; only the translation units that
include it are recompiled; a library that is up to date is left alone even where its objects are gone (a tree copied
without build/)."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from ai_based_frame_interpolation_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc")
CONV_UNITS = ("conv_f32", "conv_f16", "conv_bf16", "conv_bf16x2")
HEADERS = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.h"))) + ["../../include/fiunet.h"]


def _make(*args):
    return subprocess.run(["make", "-C", CSRC, *args], capture_output=True, text=True)


def _compiled(res):
    """The units whose compile command `make -n` printed."""
    return set(re.findall(r" -c -o \S+ (\w+)\.hip\b", res.stdout))


@pytest.fixture(scope="module")
def units(hip_lib_built):
    res = _make("-pn", "--no-builtin-rules")
    return re.search(r"^UNITS := (.*)$", res.stdout, flags=re.M).group(1).split()


@pytest.fixture(scope="module")
def objdir(hip_lib_built, units, tmp_path_factory):
    """An object directory as a build leaves it, without compiling: every unit's object (empty, as old as the library)
    and its dependency file, written by the preprocessor."""
    d = tmp_path_factory.mktemp("obj")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    jobs = [subprocess.Popen([hipcc, "-std=c++17", "--offload-arch=gfx950", "--offload-host-only", "-MM", "-MP", "-MT",
                              f"{d}/{u}.o", "-MF", f"{d}/{u}.d", f"{u}.hip"], cwd=CSRC, stderr=subprocess.DEVNULL)
            for u in units]
    assert all(j.wait() == 0 for j in jobs)
    when = os.stat(hip_lib_built)
    for u in units:
        open(d / f"{u}.o", "wb").close()
        os.utime(d / f"{u}.o", ns=(when.st_atime_ns, when.st_mtime_ns))
    return f"OBJDIR={d}"


def test_every_source_file_is_a_unit(units):
    assert sorted(units) == sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(CSRC, "*.hip")))
    assert set(CONV_UNITS) <= set(units)


def test_a_built_library_is_up_to_date(hip_lib_built, objdir):
    assert _make("-q").returncode == 0
    assert _make("-q", objdir).returncode == 0


def test_an_edited_header_makes_the_library_stale(hip_lib_built, objdir):
    assert len(HEADERS) >= 15 and {"packed.hip.h", "weights.hip.h", "flow.hip.h", "yuv4xx.hip.h"} <= set(HEADERS)
    for header in HEADERS:
        assert _make("-q", "-W", header).returncode == 1, header
        assert _make("-q", "-W", header, objdir).returncode == 1, header


def test_a_periphery_header_recompiles_its_unit_alone(objdir):
    res = _make("-n", "-W", "resize.hip.h", objdir)
    assert _compiled(res) == {"video"} and "libfiunet_hip.so" in res.stdout


def test_the_layout_rules_recompile_the_units_that_check_layouts(objdir):
    """csrc/plane_check.h is host code of the four periphery units: no conv unit and not the core unit include it."""
    assert _compiled(_make("-n", "-W", "plane_check.h", objdir)) == {"formats", "metrics", "video", "flow"}


def test_the_conv_kernels_recompile_every_conv_unit(objdir, units):
    for header in ("conv3x3_mfma.hip.h", "conv3x3_kwave.hip.h", "conv_launch.hip.h"):
        assert _compiled(_make("-n", "-W", header, objdir)) == set(CONV_UNITS), header
    # what the kernels share with the pointwise kernels reaches the core unit too, and no periphery unit
    assert _compiled(_make("-n", "-W", "conv_common.hip.h", objdir)) == set(CONV_UNITS) | {"fiunet"}
    assert _compiled(_make("-n", "-W", "fiunet_internal.h", objdir)) == set(units)


def test_missing_objects_do_not_rebuild_an_up_to_date_library(hip_lib_built, units, tmp_path):
    empty = f"OBJDIR={tmp_path}"
    assert _make("-q", empty).returncode == 0
    # ... and a stale library without objects or dependency files compiles every unit again
    res = _make("-n", "-W", "resize.hip.h", empty)
    assert _compiled(res) == set(units)


def test_changed_flags_recompile_every_unit(objdir, units):
    d = objdir.split("=", 1)[1]
    flags = _make("-pn", "--no-builtin-rules", objdir)
    now = re.search(r"^FLAGS_NOW := (.*)$", flags.stdout, flags=re.M).group(1)
    try:
        with open(os.path.join(d, "flags.stamp"), "w") as f:
            f.write(now + "\n")
        assert _make("-q", objdir).returncode == 0
        assert _make("-q", objdir, "EXTRA=-DFIUNET_CLOCK").returncode == 1
        assert _compiled(_make("-n", objdir, "EXTRA=-DFIUNET_CLOCK")) == set(units)
    finally:
        os.remove(os.path.join(d, "flags.stamp"))


def test_no_undefined_symbol_is_hidden(hip_lib_built):
    """A hidden symbol cannot come from outside the library, so an undefined one is a weak reference that nothing
    defines - the TLS-init symbol of a thread_local variable named from another unit is one - and position-independent
    code tests it for null by comparing the load address: the call that follows jumps to the library's first byte.
    Such code only runs with a GPU (the launch paths), so it is refused here, where the library is linked."""
    readelf = shutil.which("readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    table = subprocess.run([readelf, "-sW", hip_lib_built], capture_output=True, text=True, check=True).stdout
    assert len(table.splitlines()) > 100
    assert [line for line in table.splitlines() if re.search(r"\bHIDDEN\s+UND\b", line)] == []


def test_build_jobs():
    assert _native.build_jobs({}) == 8
    assert _native.build_jobs({"MAX_JOBS": "4"}) == 4
    assert _native.build_jobs({"MAX_JOBS": "64"}) == 16
    assert _native.build_jobs({"CMAKE_BUILD_PARALLEL_LEVEL": "2"}) == 2
    assert _native.build_jobs({"MAX_JOBS": "3", "CMAKE_BUILD_PARALLEL_LEVEL": "12"}) == 3
    assert _native.build_jobs({"CMAKE_BUILD_PARALLEL_LEVEL": "40"}) == 16
