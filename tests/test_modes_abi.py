"""CPU-side checks of the vertical-mode interface (msom_modes_compute / _layers / _get / _project / _energy / _set_rd): both
builds export the symbols, include/msom.h declares them and the MSOM_MD_* ids in an enum of their own, api.MODES agrees with the
header, the field and statistics tables are untouched (the mode arrays are no field ids), and a null handle is refused by each
call.  No GPU, no compute calls."""
import ctypes as C
import os
import re

import pytest

import msom_amd
from msom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("msom_modes_compute", "msom_modes_layers", "msom_modes_get", "msom_modes_project", "msom_modes_energy", "msom_modes_set_rd")
IDS = dict(MSOM_MD_IBU=0, MSOM_MD_RD=1, MSOM_MD_M2L=2, MSOM_MD_L2M=3, MSOM_MD_N=4)
MSOM_ERR_ARG = -1


def header():
    txt = open(os.path.join(ROOT, "include", "msom.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_enum(marker):
    """the anonymous enum that holds `marker`, with its explicit values"""
    body = re.search(r"enum\s*\{([^}]*\b%s\b[^}]*)\}" % marker, header()).group(1)
    return {name: int(val) for name, val in re.findall(r"\b(MSOM_[A-Z0-9_]+)\s*=\s*(\d+)", body)}


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_export_the_modes_symbols(strict):
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
    assert re.search(r"int\s+msom_modes_compute\s*\(\s*%s\s*\)" % m, txt)
    assert re.search(r"int\s+msom_modes_layers\s*\(\s*%s\s*,\s*int\s+which\s*\)" % m, txt)
    assert re.search(r"int\s+msom_modes_get\s*\(\s*%s\s*,\s*int\s+which\s*,\s*double\s*\*\s*out\s*\)" % m, txt)
    assert re.search(r"int\s+msom_modes_project\s*\(\s*%s\s*,\s*int\s+to_modes\s*,\s*const\s+double\s*\*\s*in\s*,\s*double\s*\*\s*out\s*\)" % m, txt)
    assert re.search(r"int\s+msom_modes_energy\s*\(\s*%s\s*,\s*double\s*\*\s*ke\s*,\s*double\s*\*\s*pe\s*\)" % m, txt)
    assert re.search(r"int\s+msom_modes_set_rd\s*\(\s*%s\s*,\s*int\s+mode\s*\)" % m, txt)
    assert header_enum("MSOM_MD_N") == IDS


def test_python_table_agrees_with_the_header():
    assert api.MODES == {name[len("MSOM_MD_"):]: val for name, val in header_enum("MSOM_MD_N").items()}
    assert msom_amd.MODES is api.MODES and "MODES" in msom_amd.__all__
    for meth in ("modes_compute", "modes_get", "modes_project", "modes_energy", "modes_set_rd"):
        assert callable(getattr(api.QG, meth))


def test_the_mode_arrays_are_no_field_ids():
    fields = header_enum("MSOM_NFIELDS")
    assert fields.pop("MSOM_NFIELDS") == 34 == len(api.FIELDS)
    stats = header_enum("MSOM_ST_NACC")
    assert not any(name.startswith("MSOM_MD_") for name in list(fields) + list(stats))
    assert {name[len("MSOM_ST_"):]: val for name, val in stats.items()} == api.STATS
    assert not any(name.startswith("MD_") for name in list(api.FIELDS) + list(api.STATS))
    assert not any(name.startswith(("MSOM_ST_", "MSOM_")) and not name.startswith("MSOM_MD_") for name in header_enum("MSOM_MD_N"))


@pytest.mark.parametrize("strict", [False, True])
def test_null_handle_is_refused(strict):
    L = api.load_library(strict=strict)
    out, out2 = (C.c_double * 2)(7.0, 7.0), (C.c_double * 2)(7.0, 7.0)
    assert L.msom_modes_compute(None) == MSOM_ERR_ARG
    for which in range(api.MODES["N"]):
        assert L.msom_modes_layers(None, which) == MSOM_ERR_ARG
        assert L.msom_modes_get(None, which, out) == MSOM_ERR_ARG
    for to_modes in (0, 1):
        assert L.msom_modes_project(None, to_modes, out, out2) == MSOM_ERR_ARG
    assert L.msom_modes_energy(None, out, out2) == MSOM_ERR_ARG
    assert L.msom_modes_set_rd(None, 1) == MSOM_ERR_ARG
    assert list(out) == [7.0, 7.0] and list(out2) == [7.0, 7.0]
