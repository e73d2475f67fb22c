"""CPU-only: the test-side option guard knows every knob the library accepts, so that it restores all of them."""
import os
import re

import option_guard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _capi_function(name):
    text = open(os.path.join(ROOT, "matchinglib_poselib_amd", "csrc", "capi.hip")).read()
    start = text.index(f"int {name}(")
    return text[start:text.index("\n}\n", start)]


def test_guard_names_every_settable_option():
    settable = re.findall(r'!std::strcmp\(name, "(\w+)"\)', _capi_function("mlpl_set_option"))
    assert len(settable) == len(set(settable))
    assert set(settable) == set(option_guard.SETTABLE)
    assert set(option_guard.REJECTED) <= set(option_guard.SETTABLE)


def test_get_option_reads_every_settable_option():
    settable = set(re.findall(r'!std::strcmp\(name, "(\w+)"\)', _capi_function("mlpl_set_option")))
    readable = set(re.findall(r'!std::strcmp\(name, "(\w+)"\)', _capi_function("mlpl_get_option")))
    assert settable == readable
