"""CPU: csrc/plane_check.h, the one place of the C ABI's layout rules.

  1. tests/host_checks/plane_check_main.cpp - the header alone, against a model that enumerates every address of a small
     domain, and at the edges of the address space - built with a plain host compiler and run
  2. an output one sample before the place directly behind its input is refused by every entry point that takes planes
     (tests/plane_adjacent.py; the adjacent place itself is accepted and computed right: tests/test_gpu_plane_adjacent.py)
  3. the header stays host only, and the four units that check layouts include it
"""
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plane_adjacent as PA  # noqa: E402

from ai_based_frame_interpolation_amd import _native  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ai_based_frame_interpolation_amd", "csrc")


def test_the_header_alone_against_the_address_model(tmp_path):
    exe = tmp_path / "plane_check"
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror",
           os.path.join(ROOT, "tests", "host_checks", "plane_check_main.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "plane_check: ok" in r.stdout, r.stdout + r.stderr
    assert "brute force: 247860 cases" in r.stdout


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("name", list(PA.CALLS))
def test_one_sample_before_adjacent_is_refused(hip_lib_built, name, step):
    """(On pointers that are never dereferenced: the refusal comes before a launch.)"""
    L = _native.lib()
    item, call = PA.CALLS[name]
    for shift in (1, 2, PA.body(step)):
        assert call(L, 1 << 24, item, step, shift, 1 << 28, 1 << 30) == 1, shift
        assert b"overlap" in L.fiunet_last_error_string()


def test_the_header_is_host_only_and_the_layout_units_include_it():
    src = open(os.path.join(CSRC, "plane_check.h")).read()
    assert sorted(re.findall(r"#include\s+(\S+)", src)) == ['"../../include/fiunet.h"', "<algorithm>", "<cstddef>", "<cstdint>"]
    assert not re.search(r"\bhip|std::string|\bfail\(", src.split("#pragma once")[1].replace("fail(code, reason)", ""))
    users = {u for u in os.listdir(CSRC) if u != "plane_check.h" and '"plane_check.h"' in open(os.path.join(CSRC, u)).read()}
    assert users == {"formats.hip", "video.hip", "flow.hip", "metrics.hip"}
    # each rule is written once
    units = "".join(open(os.path.join(CSRC, u)).read() for u in sorted(users))
    assert "65535" in src and "B > 65535" not in units
    assert not re.search(r"\w+ < \w+(\[\w\])? && \w+(\[\w\])? < \w+", units)
    for gone in ("resize_check_plane", "warp_check_plane", "resize_extent", "chroma_extent"):
        assert gone not in units
