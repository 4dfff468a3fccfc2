"""The running statistics of the vertex model (msomn_stats_*, include/msom.h) on the host: no GPU.

The header declares the four entry points with the signatures of their msom_stats_* twins and no second enum, both libraries export
them and refuse a null handle, msom_amd.api declares their ctypes signatures, and the state-file names of a handle with statistics
(msom_amd.state.NODE_STATS_RECORDS / NODE_STATS_KEYS) go through the pure-Python writer and reader and the C checker."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from msom_amd import api
from msom_amd.state import NODE_STATS_KEYS, NODE_STATS_RECORDS, StateFormatError, read_state, write_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ("msomn_stats_begin", "msomn_stats_accumulate", "msomn_stats_weight", "msomn_stats_get")
ACC = ("PSI", "Q", "PSI2", "Q2", "KE", "UQ", "VQ")
MSOM_ERR_ARG = -1


def header_text():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msom.h")).read(), flags=re.S)


def test_header_declares_the_four_calls_and_no_second_enum():
    txt, m = header_text(), r"msomn_t\s*\*\s*m"
    assert re.search(r"int\s+msomn_stats_begin\s*\(\s*%s\s*,\s*unsigned\s+mask\s*\)" % m, txt)
    assert re.search(r"int\s+msomn_stats_accumulate\s*\(\s*%s\s*,\s*double\s+w\s*\)" % m, txt)
    assert re.search(r"int\s+msomn_stats_weight\s*\(\s*%s\s*,\s*double\s*\*\s*W\s*\)" % m, txt)
    assert re.search(r"int\s+msomn_stats_get\s*\(\s*%s\s*,\s*int\s+which\s*,\s*double\s*\*\s*out\s*\)" % m, txt)
    assert "MSOMN_ST_" not in txt                       # the ids are MSOM_ST_*
    assert [api.STATS[n] for n in ACC] == list(range(api.STATS["NACC"]))


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_export_the_calls_and_refuse_a_null_handle(strict):
    raw = C.CDLL(os.path.join(ROOT, "msom_amd", "lib", "libmsomhip_strict.so" if strict else "libmsomhip.so"))
    for n in FUNCS:
        assert hasattr(raw, n), n
    L = api.load_library(strict=strict)
    for n in FUNCS:
        assert getattr(L, n).argtypes is not None, n
    out = C.c_double()
    assert L.msomn_stats_begin(None, 3) == MSOM_ERR_ARG
    assert L.msomn_stats_accumulate(None, 1.0) == MSOM_ERR_ARG
    assert L.msomn_stats_weight(None, C.byref(out)) == MSOM_ERR_ARG
    assert L.msomn_stats_get(None, 0, C.byref(out)) == MSOM_ERR_ARG
    for n in ("stats_begin", "stats_accumulate", "stats_weight", "stats_get"):
        assert callable(getattr(api.NodeQG, n)), n


def test_state_names_of_a_handle_with_statistics(tmp_path):
    assert NODE_STATS_RECORDS == tuple("st_" + n.lower() for n in ACC)          # record k holds accumulator MSOM_ST_k
    assert NODE_STATS_KEYS == ("mask", "count", "every", "on", "W", "samples")
    assert all(len(n) <= 16 for n in NODE_STATS_RECORDS)
    rng = np.random.default_rng(9)
    N, nl = 8, 2
    sel = ("st_psi", "st_ke")                           # mask PSI | KE
    rec = {"node": np.arange(9.0), "stats": np.array([1 << 0 | 1 << 4, 3, 1, 1, 0.125, 3], dtype=np.float64),
           "psi": rng.standard_normal((nl, N + 1, N + 1)), "q": rng.standard_normal((nl, N + 1, N + 1))}
    rec.update({n: rng.standard_normal((nl, N + 1, N + 1)) for n in sel})
    rec["mask"] = np.ones((1, N + 1, N + 1))
    p = tmp_path / "s.msom"
    write_state(p, rec, N + 1, N + 1, nl, params="N = 8\nnl = 2\n", dialect=2, t=0.5, iter=3)
    d = read_state(p)
    names = ["time", "node", "stats", "psi", "q", "st_psi", "st_ke", "mask"]
    assert list(d["records"]) == names
    assert dict(zip(NODE_STATS_KEYS, d["records"]["stats"])) == dict(mask=17, count=3, every=1, on=1, W=0.125, samples=3)
    for n in sel:
        assert np.array_equal(d["records"][n], rec[n]), n
    # the C checker walks the new names, and refuses a flipped byte in an accumulator
    assert api.state_check(p) == len(names)
    i = api.state_info(p)
    assert (i["dialect"], i["nx"], i["nl"], i["iter"], i["names"]) == (2, N + 1, nl, 3, names)
    b = bytearray(p.read_bytes())
    b[bytes(b).index(b"st_ke\0") + 64 + 8 * 7 + 1] ^= 0x10
    p.write_bytes(bytes(b))
    with pytest.raises(StateFormatError):
        read_state(p)
    with pytest.raises(api.MsomError) as e:
        api.state_check(p)
    assert e.value.code == -2
