"""The fused visit on the marched levels below the finest (option march_visit_levels): prolongation + 4 half-sweeps and 4 more
half-sweeps in one launch on the interior chunks, the trailing wave storing the level's correction where the finest level's applies
it to psi.  Same lean bodies, same expression order => bit-identical to the two passes (option 0) in both builds.  The dispatch is
asserted through msom_get_param("march_visit_<k>"), which asks the schedule function the dispatch runs on (march_next), and through
the launch count of the profile slot march_visit_coarse, so that an ignored option cannot compare a path with itself.  All cases
run with march = 2: the levels here are far below the size where marching gains."""
import functools

import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F
from test_gpu_parity import make_pair, rel

pytestmark = pytest.mark.gpu

# shape -> the levels below the finest that take the fused visit.  1024 x 128: level 1 is 512 x 64, the smallest level that holds a
# fused chunk (3 chunk rows of 14, 4 strips, everything else ring); 2048 x 128 x 4: level 1 is 1024 x 64 (the library takes
# power-of-two sides only, so neither the chunk height of 14 nor the strip width of 48 half-columns divides a level of any
# shape here: partial and wall chunks run the ring passes beside the fused ones in every case); 2048 x 256: levels 1 and 2
SHAPES = {(1024, 128, 2): (1,), (1024, 128, 3): (1,), (1024, 128, 5): (1,), (1024, 512, 6): (1,), (2048, 128, 4): (1,), (2048, 256, 3): (1, 2)}


@functools.lru_cache(maxsize=None)
def run(nx, ny, nl, strict, levels, fine, steps=3, tol=None, opts=()):
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    if tol is not None:
        g.option("TOLERANCE", tol)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    if strict:
        g.option("uniform_S", 1)   # the chained smoother exists for the uniform-S column solver (opt-in in the strict build)
    g.option("march", 2)
    for k, v in opts:
        g.option(k, v)
    g.option("march_visit", fine)
    g.option("march_visit_levels", levels)
    assert g.param("march_visit") == float(fine != 0)
    want = SHAPES[(nx, ny, nl)] if levels else ()
    for k in range(1, int(g.param("nlevels"))):
        assert g.param(f"march_visit_{k}") == float(k in want), k
    g.option("profile", 1)
    g.profile_reset()
    g.set_tnext(float("inf"))
    out = dict(dts=[])
    for i in range(steps):
        out["dts"].append(g.step())
        if i == 0:
            out["psi1"], out["q1"] = g.get(F["PSI"]), g.get(F["Q"])
    out["psi"], out["q"] = g.get(F["PSI"]), g.get(F["Q"])
    st = g.mgstats()
    out["st"] = (st.i, st.resa, st.resb)
    out["visits"] = g.profile_read("march_visit_coarse")[1]
    g.close()
    return out


def same(a, b, nlevels_fused):
    assert b["visits"] == 0
    assert a["visits"] > 0 and a["visits"] % nlevels_fused == 0
    assert a["dts"] == b["dts"] and a["st"] == b["st"]
    for k in ("psi1", "q1", "psi", "q"):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("fine", [2, 0])
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,nl", sorted(SHAPES))
def test_level_visit_equals_two_passes(nx, ny, nl, strict, fine):
    """psi and q after one RK2 step and after three, every dt, the last solve's (i, resa, resb): bit for bit, with the finest level's
    own visit on and off"""
    a = run(nx, ny, nl, strict, 1, fine)
    b = run(nx, ny, nl, strict, 0, fine)
    same(a, b, len(SHAPES[(nx, ny, nl)]))


@pytest.mark.parametrize("ring", [0, 1, 2])
@pytest.mark.parametrize("pairs", [1, 2])
@pytest.mark.parametrize("rows", [14, 20, 42])
def test_level_visit_chunk_shapes(rows, pairs, ring):
    """chunk height, wave pairs per workgroup and the way the wall-ring chunks run change no bit (2048 x 256 x 3: level 1 holds
    chunks of every height, level 2 -- 64 rows -- one to three chunk rows)"""
    shape = (2048, 256, 3)
    o = (("march_visit_rows", rows), ("march_visit_pairs", pairs), ("march_visit_ring", ring))
    a = run(*shape, True, 1, 2, steps=2, opts=o)
    b = run(*shape, True, 0, 2, steps=2)
    same(a, b, 2)


@pytest.mark.parametrize("nx,ny,nl,fine,rows,pairs,ring", [(1024, 512, 6, 2, 20, 1, 1), (1024, 512, 6, 0, 14, 2, 0), (1024, 128, 5, 0, 42, 2, 2),
                                                          (2048, 128, 4, 2, 20, 2, 2), (1024, 128, 2, 2, 14, 1, 2)])
def test_level_visit_chunk_shapes_product_build(nx, ny, nl, fine, rows, pairs, ring):
    """the same in the product build on the other shapes, with the finest visit on and off: the general-body ring forms of every way
    the ring runs, contracted arithmetic"""
    o = (("march_visit_rows", rows), ("march_visit_pairs", pairs), ("march_visit_ring", ring))
    a = run(nx, ny, nl, False, 1, fine, steps=2, opts=o)
    b = run(nx, ny, nl, False, 0, fine, steps=2)
    same(a, b, 1)


@pytest.mark.parametrize("nx,ny,nl,strict,fine", [(1024, 512, 6, False, 2), (2048, 256, 3, True, 0)])
@pytest.mark.parametrize("split", [-1, 2])
def test_level_visit_launch_split(split, nx, ny, nl, strict, fine):
    """all fused chunk rows in the second of the two mixed launches, or two of them in the first: no bit changes"""
    a = run(nx, ny, nl, strict, 1, fine, steps=2, opts=(("march_visit_split", split),))
    b = run(nx, ny, nl, strict, 0, fine, steps=2)
    same(a, b, len(SHAPES[(nx, ny, nl)]))


@pytest.mark.parametrize("strict", [True, False])
def test_level_visit_fallback_with_adapted_nrelax(strict):
    """a tight tolerance: several cycles per solve, nrelax adapts, and visits that do not relax exactly 4 + 4 half-sweeps take the
    two passes -- the same bits as option 0"""
    shape = (1024, 512, 6)
    a = run(*shape, strict, 1, 2, steps=2, tol=1e-9)
    b = run(*shape, strict, 0, 2, steps=2, tol=1e-9)
    assert a["st"][0] > 1   # the solve did take more than one cycle
    same(a, b, 1)


def test_level_visit_against_oracle():
    """product build, the visit on every marched level, against the CPU oracle (general column solver): 3 steps at TOLERANCE 1e-12,
    <= 1e-10 relative on psi and q -- the bound of tests/test_gpu_march_visit.py::test_visit_against_oracle"""
    nx, ny, nl = 1024, 512, 3
    o, g = make_pair(nx, ny, nl, strict=False, TOLERANCE=1e-12)
    g.option("march", 2)
    g.option("march_visit", 2)
    g.option("march_visit_levels", 1)
    assert g.param("march_visit") == 1.0 and g.param("march_visit_1") == 1.0
    g.option("profile", 1)
    for _ in range(3):
        o.step(); g.step()
    assert g.profile_read("march_visit_coarse")[1] > 0
    assert g.t == pytest.approx(o.t, rel=1e-12)
    assert rel(g.get(F["Q"]), o.get(orc.Q)) <= 1e-10
    assert rel(g.get(F["PSI"]), o.get(orc.PSI)) <= 1e-10
