"""Host side of the refusal table (tests/format_refusals.py): its shape, and the rows that need no device - a NULL context
is refused before any pointer is used, so fake ones will do."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ai_based_frame_interpolation_amd import _native  # noqa: E402

import format_refusals as T  # noqa: E402


def test_the_table_covers_every_entry_point_and_fault():
    assert len(T.ENTRIES) == 8 and {n for n, _ in T.CASES} == set(T.ENTRIES) and {f for _, f in T.CASES} == set(T.FAULTS)
    assert ("fiunet_forward_p10", "gray-ctx") not in T.CASES
    assert T.LAUNCHED_BEFORE_REFUSING_ONCE <= set(T.CASES)
    assert all(T.expected(n, "batch-0") == (T.BAD_SHAPE if T.ENTRIES[n][1] == "yuv" else T.INVALID_ARG) for n in T.ENTRIES)


@pytest.mark.parametrize("name", list(T.ENTRIES))
def test_a_null_context_is_refused_without_a_device(hip_lib_built, name):
    lib = _native.lib()
    fake = ctypes.c_void_p(256)
    a = T.faulty_args(name, "null-ctx", T.valid_args(None, fake, fake, fake, fake, 1 << 30))
    assert T.call(lib, name, a) == T.expected(name, "null-ctx") == T.INVALID_ARG
    assert b"NULL" in lib.fiunet_last_error_string()
