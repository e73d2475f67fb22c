"""The guard of the C boundary (csrc/mlpl_internal.h: entry_failed behind every entry's function-try-block) without a GPU:
mlpl_debug_entry_guard runs a guarded body that returns, or throws std::bad_alloc, a std::runtime_error or an int.  The exceptions are
thrown and caught inside the library; what comes back is a return code and the text of mlpl_last_error()."""
import pytest

from matchinglib_poselib_amd import _lib


def test_a_body_that_returns_is_left_alone():
    assert _lib.load_library().mlpl_debug_entry_guard(0) == 7


@pytest.mark.parametrize("kind,code,text", [(1, _lib.MLPL_E_NOMEM, "out of host memory"), (2, _lib.MLPL_E_INTERNAL, "entry guard self-test"),
                                            (3, _lib.MLPL_E_INTERNAL, "")])
def test_an_exception_becomes_a_code_and_a_text(kind, code, text):
    lib = _lib.load_library()
    assert lib.mlpl_debug_entry_guard(kind) == code
    err = _lib.last_error()
    assert err.startswith("mlpl_debug_entry_guard: ") and text in err, err
