"""Option floats_tiles of the vertex model on the host (no GPU, so no handle): both builds carry the option keys and the parameter keys
that go with them, include/msomn_floats.h states the contract, a null handle is refused by the option call, by the parameter call and
by every floats call, and api.NodeQG documents the collective calls."""
import os

import numpy as np
import pytest

from msom_amd import NodeQG, api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = [b"floats_tiles", b"floats_msg_cap", b"_resident", b"_unsent", b"_migrated", b"_on_land"]


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_know_the_option_keys(strict):
    L = api.load_library(strict=strict)
    blob = open(L._name, "rb").read()
    for k in KEYS:
        assert k + b"\0" in blob, k
    # the message a tiled handle gives with the option off is the one it always gave
    assert b"%s is not available on a tiled vertex-grid handle (%d x %d tiles)\0" in blob


@pytest.mark.parametrize("strict", [False, True])
def test_a_null_handle_is_refused(strict):
    L = api.load_library(strict=strict)
    assert L.msomn_set_option(None, b"floats_tiles", 1.0) == -1
    assert L.msomn_set_option(None, b"floats_msg_cap", 2.0) == -1
    for k in ("floats_tiles", "floats_msg_cap", "floats_resident", "floats_unsent", "floats_migrated"):
        assert np.isnan(L.msomn_get_param(None, k.encode()))
    for name, args in (("begin", (1, None, None, None)), ("get", (None, None)), ("stage", (1, 0.1)), ("track", (0, 1, None, None, None, None))):
        assert getattr(L, "msomn_floats_" + name)(None, *args) == -1
        assert ("msomn_floats_" + name).encode() in L.msom_last_error()


def test_the_header_states_the_contract_and_the_methods_say_collective():
    txt = open(os.path.join(ROOT, "include", "msomn_floats.h")).read()
    for word in ("floats_tiles", "floats_msg_cap", "collective", "floats_unsent", "floats_migrated", "floats_resident", "MSOM_ERR_CONFIG", "bit for bit"):
        assert word in txt, word
    for m in ("begin", "get", "velocity", "sample", "track"):
        assert "tiles" in getattr(NodeQG, "floats_" + m).__doc__, m
