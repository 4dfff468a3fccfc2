"""CPU-side checks of the spectrum interface (msom_spec_layout / _bins / _kr / _2d / _cross / _fields / _energy): both builds export the
symbols, include/msom.h declares them, the api.QG methods exist, the field, statistics and mode tables are untouched, a null handle is
refused by each call, and msom_spec_layout -- host arithmetic, no handle -- is run for real against tests/spec_ref.py.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import msom_amd
import spec_ref as R
from msom_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("msom_spec_layout", "msom_spec_bins", "msom_spec_kr", "msom_spec_2d", "msom_spec_cross", "msom_spec_fields", "msom_spec_energy")
MSOM_ERR_ARG, MSOM_ERR_CONFIG = -1, -3


def header():
    txt = open(os.path.join(ROOT, "include", "msom.h")).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def header_enum(marker):
    body = re.search(r"enum\s*\{([^}]*\b%s\b[^}]*)\}" % marker, header()).group(1)
    return {name: int(val) for name, val in re.findall(r"\b(MSOM_[A-Z0-9_]+)\s*=\s*(\d+)", body)}


def test_error_codes_of_the_header():
    txt = header()
    assert re.search(r"#define\s+MSOM_ERR_ARG\s+\(-1\)", txt) and re.search(r"#define\s+MSOM_ERR_CONFIG\s+\(-3\)", txt)


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_export_the_spec_symbols(strict):
    path = os.path.join(os.path.dirname(api.__file__), "lib", "libmsomhip_strict.so" if strict else "libmsomhip.so")
    L = C.CDLL(path)
    for fn in FUNCS:
        assert hasattr(L, fn), fn
    L2 = api.load_library(strict=strict)     # the prototypes of api.py resolve too
    for fn in FUNCS:
        assert getattr(L2, fn).restype is C.c_int


def test_header_declares_the_functions():
    txt = header()
    m = r"msom_t\s*\*\s*m"
    cd, d = r"const\s+double\s*\*\s*", r"double\s*\*\s*"
    assert re.search(r"int\s+msom_spec_layout\s*\(\s*int\s+nx\s*,\s*int\s+ny\s*,\s*int\s*\*\s*nbins\s*,\s*long\s*\*\s*count\s*\)", txt)
    assert re.search(r"int\s+msom_spec_bins\s*\(\s*%s\s*\)" % m, txt)
    assert re.search(r"int\s+msom_spec_kr\s*\(\s*%s\s*,\s*%skr\s*\)" % (m, d), txt)
    assert re.search(r"int\s+msom_spec_2d\s*\(\s*%s\s*,\s*%sa\s*,\s*%sb\s*,\s*int\s+layers\s*,\s*%sout\s*\)" % (m, cd, cd, d), txt)
    assert re.search(r"int\s+msom_spec_cross\s*\(\s*%s\s*,\s*%sa\s*,\s*%sb\s*,\s*int\s+layers\s*,\s*%sspec\s*,\s*%sflux\s*\)" % (m, cd, cd, d, d), txt)
    assert re.search(r"int\s+msom_spec_fields\s*\(\s*%s\s*,\s*int\s+field_a\s*,\s*int\s+field_b\s*,\s*%sspec\s*,\s*%sflux\s*\)" % (m, d, d), txt)
    assert re.search(r"int\s+msom_spec_energy\s*\(\s*%s\s*,\s*%ske\s*,\s*%spe\s*\)" % (m, d, d), txt)


def test_python_surface_and_untouched_tables():
    for meth in ("spec_bins", "spec_kr", "spec_2d", "spec_cross", "spec_fields", "spec_energy"):
        assert callable(getattr(api.QG, meth))
    assert msom_amd.spec_layout is api.spec_layout and "spec_layout" in msom_amd.__all__
    fields = header_enum("MSOM_NFIELDS")
    assert fields.pop("MSOM_NFIELDS") == 34 == len(api.FIELDS)
    assert {name[len("MSOM_"):]: val for name, val in fields.items()} == api.FIELDS
    stats = header_enum("MSOM_ST_NACC")
    assert {name[len("MSOM_ST_"):]: val for name, val in stats.items()} == api.STATS
    assert {name[len("MSOM_MD_"):]: val for name, val in header_enum("MSOM_MD_N").items()} == api.MODES
    assert not any("SPEC" in name for name in list(fields) + list(stats) + list(api.FIELDS) + list(api.STATS) + list(api.MODES))


@pytest.mark.parametrize("strict", [False, True])
def test_null_handle_is_refused(strict):
    L = api.load_library(strict=strict)
    x, y = (C.c_double * 64)(*([7.0] * 64)), (C.c_double * 64)(*([7.0] * 64))
    assert L.msom_spec_bins(None) == MSOM_ERR_ARG
    assert L.msom_spec_kr(None, x) == MSOM_ERR_ARG
    assert L.msom_spec_2d(None, C.addressof(x), C.addressof(x), 1, C.addressof(y)) == MSOM_ERR_ARG
    assert L.msom_spec_cross(None, C.addressof(x), C.addressof(x), 1, x, y) == MSOM_ERR_ARG
    assert L.msom_spec_fields(None, 0, 1, x, y) == MSOM_ERR_ARG
    assert L.msom_spec_energy(None, x, y) == MSOM_ERR_ARG
    assert list(x) == [7.0] * 64 and list(y) == [7.0] * 64


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("nx,ny", [(8, 8), (16, 16), (64, 32), (32, 128), (256, 256)])
def test_layout_equals_the_reference_rule(strict, nx, ny):
    nb, cnt = api.spec_layout(nx, ny, strict=strict)
    assert nb == R.nbins(nx, ny) == max(nx, ny) // 2 - 2
    assert np.array_equal(cnt, R.count(nx, ny))
    # nbins alone, without the counts
    L = api.load_library(strict=strict)
    n = C.c_int(-5)
    assert L.msom_spec_layout(nx, ny, C.byref(n), None) == 0 and n.value == nb


def test_layout_counts_by_brute_force():
    """the rule itself, point by point: r^2 <= R2 <= (r + 1)^2 with both ends inclusive"""
    nx, ny = 16, 8
    nb, cnt = api.spec_layout(nx, ny)
    want = np.zeros(nb, dtype=int)
    for i in range(-nx // 2, nx // 2):
        for j in range(-ny // 2, ny // 2):
            R2 = i * i + (2 * j) ** 2
            for r in range(nb):
                want[r] += r * r <= R2 <= (r + 1) ** 2
    assert np.array_equal(cnt, want) and np.array_equal(R.count(nx, ny), want)


@pytest.mark.parametrize("nx,ny", [(12, 12), (4, 8), (0, 0), (16, 12), (8, 4), (-8, 8)])
def test_layout_refuses_bad_sides(nx, ny):
    L = api.load_library()
    n = C.c_int(-5)
    assert L.msom_spec_layout(nx, ny, C.byref(n), None) == MSOM_ERR_CONFIG
    assert n.value == -5
    with pytest.raises(api.MsomError):
        api.spec_layout(nx, ny)
