"""CPU-side checks of the running-statistics interface (msom_stats_begin / msom_stats_accumulate / msom_stats_weight /
msom_stats_get / msom_time_filter): both builds export the symbols, include/msom.h declares them and the MSOM_ST_* ids,
api.STATS agrees with the header, the field table is untouched (the accumulators are no field ids), and a null handle is
refused by each call.  No GPU, no compute calls."""
import ctypes as C
import os
import re

import pytest

from msom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("msom_stats_begin", "msom_stats_accumulate", "msom_stats_weight", "msom_stats_get", "msom_time_filter")
IDS = dict(MSOM_ST_PSI=0, MSOM_ST_Q=1, MSOM_ST_PSI2=2, MSOM_ST_Q2=3, MSOM_ST_KE=4, MSOM_ST_UQ=5, MSOM_ST_VQ=6, MSOM_ST_NACC=7,
           MSOM_ST_EKE=16, MSOM_ST_UQ_EDDY=17, MSOM_ST_VQ_EDDY=18, MSOM_ST_QME=32)
MSOM_ERR_ARG = -1


def header():
    txt = open(os.path.join(ROOT, "include", "msom.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_enum(marker):
    """the anonymous enum that holds `marker`, with its explicit values"""
    body = re.search(r"enum\s*\{([^}]*\b%s\b[^}]*)\}" % marker, header()).group(1)
    return {name: int(val) for name, val in re.findall(r"\b(MSOM_[A-Z0-9_]+)\s*=\s*(\d+)", body)}


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_export_the_stats_symbols(strict):
    path = os.path.join(os.path.dirname(api.__file__), "lib", "libmsomhip_strict.so" if strict else "libmsomhip.so")
    L = C.CDLL(path)
    for fn in FUNCS:
        assert hasattr(L, fn), fn
    L2 = api.load_library(strict=strict)     # the prototypes of api.py resolve too
    for fn in FUNCS:
        assert getattr(L2, fn).restype is C.c_int


def test_header_declares_functions_and_ids():
    txt = header()
    m = r"msom_t\s*\*\s*m"
    assert re.search(r"int\s+msom_stats_begin\s*\(\s*%s\s*,\s*unsigned\s+mask\s*\)" % m, txt)
    assert re.search(r"int\s+msom_stats_accumulate\s*\(\s*%s\s*,\s*double\s+w\s*\)" % m, txt)
    assert re.search(r"int\s+msom_stats_weight\s*\(\s*%s\s*,\s*double\s*\*\s*W\s*\)" % m, txt)
    assert re.search(r"int\s+msom_stats_get\s*\(\s*%s\s*,\s*int\s+which\s*,\s*double\s*\*\s*out\s*\)" % m, txt)
    assert re.search(r"int\s+msom_time_filter\s*\(\s*%s\s*,\s*double\s+dt\s*\)" % m, txt)
    assert header_enum("MSOM_ST_NACC") == IDS


def test_python_table_agrees_with_the_header():
    ids = header_enum("MSOM_ST_NACC")
    assert api.STATS == {name[len("MSOM_ST_"):]: val for name, val in ids.items()}


def test_the_accumulators_are_no_field_ids():
    fields = header_enum("MSOM_NFIELDS")
    assert fields.pop("MSOM_NFIELDS") == 34 == len(api.FIELDS)
    assert not any(name.startswith("MSOM_ST_") for name in fields)
    assert not any(name.startswith("ST_") or name in api.STATS for name in api.FIELDS if name not in ("PSI", "Q"))


@pytest.mark.parametrize("strict", [False, True])
def test_null_handle_is_refused(strict):
    L = api.load_library(strict=strict)
    out = C.c_double(7.0)
    assert L.msom_stats_begin(None, 3) == MSOM_ERR_ARG
    assert L.msom_stats_accumulate(None, 1.0) == MSOM_ERR_ARG
    assert L.msom_stats_weight(None, C.byref(out)) == MSOM_ERR_ARG
    assert L.msom_stats_get(None, 0, C.byref(out)) == MSOM_ERR_ARG
    assert L.msom_time_filter(None, 0.1) == MSOM_ERR_ARG
    assert out.value == 7.0
