"""CPU-side checks of the device-side back-and-forth nudging interface (msom_bfn_begin / msom_bfn_steps /
msom_bfn_misfit, the loop of msqg/qg_bfn.py:47-73 moved into the library): both builds export the symbols,
include/msom.h declares them and the five MSOM_BFN_* field ids, the Python field table agrees with the header,
and a null handle is refused.  No GPU, no compute calls."""
import ctypes as C
import os
import re

import pytest

from msom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("msom_bfn_begin", "msom_bfn_steps", "msom_bfn_misfit")
IDS = dict(MSOM_BFN_F1=29, MSOM_BFN_F2=30, MSOM_BFN_F3=31, MSOM_BFN_OBS=32, MSOM_BFN_GAIN=33, MSOM_NFIELDS=34)
MSOM_ERR_ARG = -1


def header():
    txt = open(os.path.join(ROOT, "include", "msom.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_field_ids():
    """the anonymous enum of field ids, evaluated the way the C compiler does (explicit values)"""
    body = re.search(r"enum\s*\{([^}]*MSOM_NFIELDS[^}]*)\}", header()).group(1)
    ids = {}
    for name, val in re.findall(r"\b(MSOM_[A-Z0-9_]+)\s*=\s*(\d+)", body):
        ids[name] = int(val)
    return ids


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_export_the_bfn_symbols(strict):
    path = os.path.join(os.path.dirname(api.__file__), "lib", "libmsomhip_strict.so" if strict else "libmsomhip.so")
    L = C.CDLL(path)
    for fn in FUNCS:
        assert hasattr(L, fn), fn
    L2 = api.load_library(strict=strict)     # the prototypes of api.py resolve too
    for fn in FUNCS:
        assert getattr(L2, fn).restype is C.c_int


def test_header_declares_functions_and_field_ids():
    txt = header()
    assert re.search(r"int\s+msom_bfn_begin\s*\(\s*msom_t\s*\*\s*m\s*\)", txt)
    assert re.search(r"int\s+msom_bfn_steps\s*\(\s*msom_t\s*\*\s*m\s*,\s*int\s+nsteps\s*,\s*double\s+dt\s*,\s*double\s+direction\s*,\s*double\s+k\s*\)", txt)
    assert re.search(r"int\s+msom_bfn_misfit\s*\(\s*msom_t\s*\*\s*m\s*,\s*double\s*\*\s*misfit\s*\)", txt)
    ids = header_field_ids()
    for name, val in IDS.items():
        assert ids.get(name) == val, name
    assert ids["MSOM_PO_MFT"] == 28 and ids["MSOM_PSI"] == 0 and ids["MSOM_Q"] == 1     # the existing ids did not move


def test_python_field_table_agrees_with_the_header():
    ids = header_field_ids()
    n = ids.pop("MSOM_NFIELDS")
    assert len(api.FIELDS) == n == 34
    for name, val in ids.items():
        assert api.FIELDS[name[len("MSOM_"):]] == val, name
    for name in ("BFN_F1", "BFN_F2", "BFN_F3", "BFN_OBS", "BFN_GAIN"):
        assert api.FIELDS[name] == IDS["MSOM_" + name]


@pytest.mark.parametrize("strict", [False, True])
def test_null_handle_is_refused(strict):
    L = api.load_library(strict=strict)
    assert L.msom_bfn_steps(None, 1, 0.1, 1.0, 0.0) == MSOM_ERR_ARG
    assert L.msom_bfn_begin(None) == MSOM_ERR_ARG
    out = C.c_double(7.0)
    assert L.msom_bfn_misfit(None, C.byref(out)) == MSOM_ERR_ARG
