"""The C ABI of the vertex model's Lagrangian floats on the host (no GPU): include/msomn_floats.h declares eight entry points, both
builds export them, api.NodeQG has the pass-through methods, and a null handle is answered with MSOM_ERR_ARG and a message that names
the call."""
import os
import re

import pytest

from msom_amd import NodeQG, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ["begin", "end", "get", "velocity", "sample", "stage", "record", "track"]


def header_symbols():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msomn_floats.h")).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(msomn?_[a-z0-9_]+)\s*\(", txt)))


@pytest.mark.parametrize("strict", [False, True])
def test_both_builds_export_what_the_header_declares(strict):
    assert header_symbols() == sorted("msomn_floats_" + c for c in CALLS)
    L = api.load_library(strict=strict)
    for n in header_symbols():
        assert hasattr(L, n), n
        assert getattr(L, n).argtypes is not None, n


def test_the_other_headers_do_not_speak_of_floats_and_the_methods_exist():
    for h in ("msom.h", "msom_state.h", "msomn_state.h"):
        assert "floats" not in open(os.path.join(ROOT, "include", h)).read()
    assert "msomn_floats" not in open(os.path.join(ROOT, "include", "msom_floats.h")).read()
    for c in CALLS:
        assert callable(getattr(NodeQG, "floats_" + c))


@pytest.mark.parametrize("strict", [False, True])
def test_a_null_handle_is_an_argument_error_that_names_the_call(strict):
    L = api.load_library(strict=strict)
    for name, args in (("begin", (1, None, None, None)), ("end", ()), ("get", (None, None)), ("velocity", (None, None)), ("sample", (0, None)),
                       ("stage", (1, 0.1)), ("record", (1, 1, -1)), ("track", (0, 1, None, None, None, None))):
        assert getattr(L, "msomn_floats_" + name)(None, *args) == -1
        assert ("msomn_floats_" + name).encode() in L.msom_last_error()
