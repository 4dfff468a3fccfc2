"""The state file of the vertex model (include/msomn_state.h) on the host: no GPU.

The four entry points are declared by the new header alone and exported by both libraries; include/msom_state.h declares what it
declared; msom_amd.state writes and reads a dialect-2 file with a record on the cell grid, and the C checker accepts it.

tests/golden/state_node_32x3.msom was written by
    PYTHONPATH=.:tests python tests/test_node_state_host.py --make-golden
which is make_golden_node() below: write_state of what the CPU oracle orn holds after 3 steps of orn.node_params(32, 3, bc_fac=1)
with an island mask, constants included (mask, S2 as set_const left it).  The oracle does not hand out the dt limiter's `previous`:
it is what the step's second update returns, so the third step is also made call by call on a second oracle, which must end on the
stepped oracle's bits (as golden_content() of test_state_host.py does for the cell model).
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from msom_amd import api
from msom_amd.state import StateFormatError, digest, read_state, write_state

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_NODE = os.path.join(ROOT, "tests", "golden", "state_node_32x3.msom")
GN, GNL = 32, 3
NODE_SCALARS = ("seed", "noise_draw", "corrector_step", "nbar", "pg_set", "topo_set", "forcing_3d", "sqg", "DT")   # record `node`


def golden_mask(N):
    """an island and a ragged coast (land_mask of test_gpu_node_parity.py, restated: that module needs no GPU to import, but this
    file should not depend on a GPU test file)"""
    m = np.ones((1, N + 1, N + 1))
    m[0, N // 4: N // 4 + N // 8 + 1, N // 2: N // 2 + N // 8] = 0
    m[0, : N // 6, : N // 5] = 0
    m[0, 0, :] = m[0, -1, :] = m[0, :, 0] = m[0, :, -1] = 0
    return m


def golden_oracle():
    import orn
    txt = orn.node_params(GN, GNL, bc_fac=1.0)
    o = orn.NodeOracle(txt, smoother=orn.GS_RB, quiet=1)
    mk = golden_mask(GN)
    o.set(orn.MASK, mk)
    o.set(orn.PSI, orn.node_psi(GNL, GN) * mk)
    o.set_const()
    return txt, o


def golden_node_content():
    import orn
    txt, a = golden_oracle()
    _, b = golden_oracle()
    for o in (a, b):
        o.step(True)
        o.step(True)
    a.step(True)
    # b: the third step call by call (event forcing, update, dtnext with no event ahead, advance dt / 2, update, advance dt)
    b.forcing()
    dt = b.update(orn.Q, orn.DQ, b.param("DT"))
    b.advance(orn.QPRED, orn.Q, orn.DQ, dt / 2)
    previous = b.update(orn.QPRED, orn.DQ, dt)
    b.advance(orn.Q, orn.Q, orn.DQ, dt)
    assert dt == a.dt and np.array_equal(a.get(orn.Q), b.get(orn.Q)) and np.array_equal(a.get(orn.PSI), b.get(orn.PSI))
    st = a.mgstats()
    rec = {"mgstats": np.array([st.i, st.resb, st.resa, st.nrelax], dtype=np.float64),
           "node": np.array([1, 0, 0, 0, 0, 0, 0, 0, a.param("DT")], dtype=np.float64),
           "psi": a.get(orn.PSI), "q": a.get(orn.Q), "q_forcing": a.get(orn.QFORC), "mask": a.get(orn.MASK), "S2": a.get(orn.S2)}
    return dict(records=rec, nx=GN + 1, ny=GN + 1, nl=GNL, params=txt, dialect=2, t=a.t, dt=a.dt, previous=previous, iter=3)


def make_golden_node(path=GOLDEN_NODE):
    write_state(path, **golden_node_content())


# ------------------------------------------------------------------ the headers and the libraries

def header_symbols(name):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(msomn?_[a-z0-9_]+)\s*\(", txt)))


def test_the_new_header_declares_exactly_the_four_symbols():
    assert header_symbols("msomn_state.h") == ["msomn_create_from_state", "msomn_state_dbg_flip", "msomn_state_load", "msomn_state_save"]
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msomn_state.h")).read(), flags=re.S)
    for n in ("msomn_state_save", "msomn_state_load", "msomn_state_dbg_flip"):
        assert re.search(r"\bint\s+" + n + r"\s*\(\s*msomn_t\s*\*", txt), n
    assert re.search(r"msomn_t\s*\*\s*msomn_create_from_state\s*\(\s*const char\s*\*", txt)


def test_msom_state_h_declares_what_it_declared():
    assert header_symbols("msom_state.h") == ["msom_create_from_state", "msom_state_check", "msom_state_dbg_flip", "msom_state_info",
                                             "msom_state_load", "msom_state_save"]


def test_msom_h_names_the_new_header_without_declaring_it():
    txt = open(os.path.join(ROOT, "include", "msom.h")).read()
    assert "msomn_state.h" in txt
    assert not [n for n in header_symbols("msom.h") if n.startswith("msomn_state") or n == "msomn_create_from_state"]


@pytest.mark.parametrize("strict", [False, True])
def test_both_libraries_export_the_four_symbols(strict):
    """through ctypes alone: no handle is created"""
    L = ctypes.CDLL(os.path.join(ROOT, "msom_amd", "lib", "libmsomhip_strict.so" if strict else "libmsomhip.so"))
    for n in header_symbols("msomn_state.h"):
        assert hasattr(L, n), n
    assert api.load_library(strict=strict).msomn_state_save.argtypes is not None


# ------------------------------------------------------------------ the format: a dialect-2 file with a cell record

def test_dialect_2_round_trip_with_a_cell_record(tmp_path):
    rng = np.random.default_rng(4)
    N, nl = 8, 2
    rec = {"node": np.arange(9.0), "psi": rng.standard_normal((nl, N + 1, N + 1)), "noise": rng.standard_normal((1, N, N)),
           "mask": np.ones((1, N + 1, N + 1))}
    p = tmp_path / "n.msom"
    write_state(p, rec, N + 1, N + 1, nl, params="N = 8\nnl = 2\n", dialect=2, stochastic=1, noise_mode=1, cells=("noise",), t=0.5, iter=7)
    d = read_state(p)
    assert (d["version"], d["dialect"], d["nx"], d["ny"], d["nl"], d["nptr"], d["stochastic"], d["noise_mode"]) == (1, 2, N + 1, N + 1, nl, 0, 1, 1)
    assert list(d["records"]) == ["time", "node", "psi", "noise", "mask"]
    for k, a in rec.items():
        assert d["records"][k].shape == a.shape and np.array_equal(d["records"][k], a), k
    assert d["digests"]["noise"] == digest(rec["noise"])
    # the C checker walks it: the record's own (ny, nx) differ from the header's
    assert api.state_check(p) == 5
    i = api.state_info(p)
    assert (i["dialect"], i["nx"], i["ny"], i["nl"], i["iter"], i["names"]) == (2, N + 1, N + 1, nl, 7, ["time", "node", "psi", "noise", "mask"])
    # default behaviour unchanged: without the keyword the cell-shaped array is refused, and a vertex-shaped one under the keyword too
    with pytest.raises(StateFormatError):
        write_state(p, rec, N + 1, N + 1, nl, dialect=2)
    with pytest.raises(StateFormatError):
        write_state(p, rec, N + 1, N + 1, nl, dialect=2, cells=("noise", "psi"))
    # a flipped byte in the cell record is refused by both readers
    write_state(p, rec, N + 1, N + 1, nl, dialect=2, cells=("noise",))
    b = bytearray(p.read_bytes())
    at = bytes(b).index(b"noise\0") + 64 + 8 * 5 + 2
    b[at] ^= 0x04
    p.write_bytes(bytes(b))
    with pytest.raises(StateFormatError):
        read_state(p)
    with pytest.raises(api.MsomError) as e:
        api.state_check(p)
    assert e.value.code == -2


def test_the_checker_names_the_dialect(tmp_path):
    import subprocess
    exe = os.path.join(ROOT, "msom_amd", "lib", "msom_state_check")
    r = subprocess.run([exe, GOLDEN_NODE, os.path.join(ROOT, "tests", "golden", "state_32x32x3.msom")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "dialect 2 (vertex), 33 x 33 x 3" in lines[0] and "dialect 0 (msqg), 32 x 32 x 3" in lines[1]


# ------------------------------------------------------------------ msom_nc_truncate (msomn_run resuming from a checkpoint)

def test_nc_truncate_sets_a_file_back(tmp_path):
    L = api.load_library()
    cs, ci, cd = ctypes.c_char_p, ctypes.c_int, ctypes.c_double
    names = (cs * 2)(b"psi", b"q")
    L.msom_nc_create2.argtypes = [cs, ci, ci, ci, cd, ci, ctypes.POINTER(cs), ci]
    L.msom_nc_append.argtypes = [cs, ci, ci, ci, ci, ctypes.POINTER(cs), cd, ctypes.POINTER(ctypes.POINTER(cd))]
    L.msom_nc_truncate.argtypes = [cs, ctypes.c_long]
    nl, n1 = 2, 9
    p = str(tmp_path / "v.nc").encode()
    assert L.msom_nc_create2(p, nl, n1, n1, 100.0, 2, names, 1) == 0
    rng = np.random.default_rng(6)
    kept = []
    for k in range(4):
        a, b = rng.standard_normal(nl * n1 * n1), rng.standard_normal(nl * n1 * n1)
        ptrs = (ctypes.POINTER(cd) * 2)(a.ctypes.data_as(ctypes.POINTER(cd)), b.ctypes.data_as(ctypes.POINTER(cd)))
        assert L.msom_nc_append(p, nl, n1, n1, 2, names, 0.1 * k, ptrs) == k
        kept.append(open(p, "rb").read())
    assert L.msom_nc_truncate(p, 5) != 0 and open(p, "rb").read() == kept[3]   # more than it holds: refused, untouched
    for nrec in (4, 2, 1):
        assert L.msom_nc_truncate(p, nrec) == 0
        assert open(p, "rb").read() == kept[nrec - 1], nrec
    from scipy.io import netcdf_file
    with netcdf_file(p.decode(), "r", mmap=False) as nc:
        assert nc.variables["psi"].shape == (1, nl, n1, n1) and np.allclose(nc.variables["time"][:], [0.0])
    (tmp_path / "junk").write_bytes(b"not a file of this kind")
    assert L.msom_nc_truncate(str(tmp_path / "junk").encode(), 0) != 0


# ------------------------------------------------------------------ the golden file

def test_golden_node_file_is_what_the_oracle_gives(tmp_path):
    assert os.path.getsize(GOLDEN_NODE) < 1 << 20
    assert api.state_check(GOLDEN_NODE) == 8
    i = api.state_info(GOLDEN_NODE)
    assert (i["version"], i["dialect"], i["nx"], i["ny"], i["nl"], i["iter"]) == (1, 2, GN + 1, GN + 1, GNL, 3)
    assert i["names"] == ["time", "mgstats", "node", "psi", "q", "q_forcing", "mask", "S2"]
    d = read_state(GOLDEN_NODE)
    assert d["t"] > 0 and d["previous"] > 0 and np.abs(d["records"]["q"]).max() > 0
    assert np.array_equal(d["records"]["mask"], golden_mask(GN))
    assert dict(zip(NODE_SCALARS, d["records"]["node"]))["DT"] < 5e-2   # the clamped DT, not the params text's
    # byte for byte: the writer and the oracle of today make the file of the day it was committed
    make_golden_node(tmp_path / "g.msom")
    assert (tmp_path / "g.msom").read_bytes() == open(GOLDEN_NODE, "rb").read()


if __name__ == "__main__":
    if sys.argv[1:] == ["--make-golden"]:
        make_golden_node()
        print("wrote", GOLDEN_NODE)
