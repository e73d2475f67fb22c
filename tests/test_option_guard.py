"""CPU-only: the library's option table (mlpl_option_info / mlpl_option_accepts need no device) against the test data of
option_guard.py and against the opt_* fields of mlpl_ctx -- one row per field, the defaults and the accepted values as written down."""
import ctypes
import os
import re

import option_guard
from matchinglib_poselib_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = option_guard.option_table()
NAMES = [name for name, _ in TABLE]


def _accepts(name, value):
    return _lib.load_library().mlpl_option_accepts(name.encode(), value)


def test_the_table_names_what_the_test_data_names():
    assert len(NAMES) == 56 and len(set(NAMES)) == 56
    assert set(NAMES) == set(option_guard.SETTABLE) == set(option_guard.DEFAULTS)
    assert set(option_guard.REJECTED) <= set(NAMES)


def test_one_row_per_option_field_of_the_context():
    header = open(os.path.join(ROOT, "matchinglib_poselib_amd", "csrc", "mlpl_internal.h")).read()
    start = header.index("struct mlpl_ctx {")
    struct = re.sub(r"//.*", "", header[start:header.index("\n};", start)])
    fields = re.findall(r"\bopt_(\w+)", struct)
    assert fields == re.findall(r"^\s*int opt_(\w+);", struct, re.M)   # plain ints, one per line
    assert len(fields) == len(set(fields))
    assert set(fields) == set(NAMES)


def test_defaults_are_the_written_ones_and_acceptable():
    for name, default in TABLE:
        assert default == option_guard.DEFAULTS[name], name
        assert _accepts(name, default) == 1, name


def test_settable_values_are_accepted():
    for name, values in option_guard.SETTABLE.items():
        for v in values:
            assert _accepts(name, v) == 1, (name, v)


def test_rejected_values_are_refused():
    for name, values in option_guard.REJECTED.items():
        for v in values:
            assert _accepts(name, v) == 0, (name, v)


def test_every_option_with_a_bounded_value_set_has_refusals():
    """Only an option that takes every non-negative int may go with fewer than one refused value on each side."""
    for name in NAMES:
        below = [v for v in option_guard.REJECTED.get(name, ()) if v < min(option_guard.SETTABLE[name])]
        above = [v for v in option_guard.REJECTED.get(name, ()) if v > max(option_guard.SETTABLE[name])]
        assert below, name
        assert above or _accepts(name, 2**31 - 1) == 1, name


def test_unknown_names_and_indices_are_bad_input():
    lib = _lib.load_library()
    assert _accepts("no_such_option", 0) == _lib.MLPL_E_BAD_INPUT
    assert lib.mlpl_option_accepts(None, 0) == _lib.MLPL_E_BAD_INPUT
    name, default = ctypes.c_char_p(), ctypes.c_int()
    for index in (-1, len(NAMES)):
        assert lib.mlpl_option_info(index, ctypes.byref(name), ctypes.byref(default)) == _lib.MLPL_E_BAD_INPUT
    assert lib.mlpl_option_info(0, None, ctypes.byref(default)) == _lib.MLPL_E_BAD_INPUT
    assert lib.mlpl_option_info(0, ctypes.byref(name), None) == _lib.MLPL_E_BAD_INPUT
