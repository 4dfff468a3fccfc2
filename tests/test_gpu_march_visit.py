"""The finest level's fused visit (k_relax_visit, option march_visit): prolongation + 4 half-sweeps and 4 half-sweeps +
correction in one launch on the interior chunks, the two passes on the chunks around them.  Same lean bodies, same
expression order => bit-identical to the two passes (option 0) in both builds; the dispatch is asserted through
msom_get_param("march_visit"), which asks the schedule function the dispatch runs on (march_next), and the profile slot of the
same name."""
import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F
from test_gpu_parity import make_pair, rel

pytestmark = pytest.mark.gpu


def run(nx, ny, nl, strict, visit, steps, tol=None, **opts):
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    if tol is not None:
        g.option("TOLERANCE", tol)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    if strict:
        g.option("uniform_S", 1)   # the chained smoother exists for the uniform-S column solver (opt-in in the strict build)
    for k, v in opts.items():
        g.option(k, v)
    g.option("march_visit", 2 * visit)   # 2: also below the size where it gains (march_visit_min)
    assert g.param("march_visit") == float(visit)   # an ignored option would compare a path with itself
    g.option("profile", 2)
    g.profile_reset()
    g.set_tnext(float("inf"))
    out = dict(psi1=None, dts=[])
    for i in range(steps):
        out["dts"].append(g.step())
        if i == 0:
            out["psi1"], out["q1"] = g.get(F["PSI"]), g.get(F["Q"])
    out["psi"], out["q"] = g.get(F["PSI"]), g.get(F["Q"])
    st = g.mgstats()
    out["st"] = (st.i, st.resa, st.resb)
    out["visits"] = g.profile_read("march_visit")[1]
    g.close()
    return out


def same(a, b):
    assert a["dts"] == b["dts"] and a["st"] == b["st"]
    for k in ("psi1", "q1", "psi", "q"):
        assert np.array_equal(a[k], b[k]), k


CASES = [(4096, 4096, 6), (2048, 2048, 3), (2048, 2048, 2), (2048, 2048, 4), (2048, 2048, 5), (1024, 512, 6)]


@pytest.mark.parametrize("nx,ny,nl", CASES)
@pytest.mark.parametrize("strict", [True, False])
def test_visit_equals_two_passes(nx, ny, nl, strict):
    """one RK2 step (two solves) and three: psi, q, dt, cycle count and residuals bit for bit.  1024 x 512: neither side is
    a multiple of the visit's chunk height (28 rows) or strip width (96 cells), so partial and wall chunks run the two passes beside it"""
    opts = dict(march=2) if nx * ny * nl < 2 ** 23 else {}
    a = run(nx, ny, nl, strict, 1, 3, **opts)
    b = run(nx, ny, nl, strict, 0, 3, **opts)
    assert a["visits"] > 0 and b["visits"] == 0
    same(a, b)


@pytest.mark.parametrize("rows,pairs", [(14, 1), (42, 2), (20, 2)])
def test_visit_chunk_shapes(rows, pairs):
    """chunk height and wave pairs per workgroup change no bit"""
    nx, ny, nl = 1024, 512, 4
    a = run(nx, ny, nl, True, 1, 2, march=2, march_visit_rows=rows, march_visit_pairs=pairs)
    b = run(nx, ny, nl, True, 0, 2, march=2)
    assert a["visits"] > 0
    same(a, b)


@pytest.mark.parametrize("strict", [True, False])
def test_visit_fallback_with_adapted_nrelax(strict):
    """a tight tolerance: several cycles per solve, nrelax adapts, and visits that do not relax exactly 4 + 4 half-sweeps take
    the two passes -- the same bits as option 0"""
    a = run(2048, 2048, 3, strict, 1, 2, tol=1e-9)
    b = run(2048, 2048, 3, strict, 0, 2, tol=1e-9)
    same(a, b)


@pytest.mark.parametrize("block_small", [0, 1024])
@pytest.mark.parametrize("strict", [True, False])
def test_visit_parameter_follows_the_dispatch_without_fused_prolongation(strict, block_small):
    """prolong_fused = 0: the level is prolongated by its own kernel, the visit has no coarse level to interpolate and takes
    neither k_relax_visit nor the PL pass -- the parameter says so (0, ring -1) and the profile slots count no launch; the
    result is that of march_visit = 0 under the same option, bit for bit.  block_small = 1024 would admit block2 on every
    level here, but only where neither march nor block8 applies: the marched finest level stays marched (path 3) and follows
    prolong_fused like any marched level"""
    nx, ny, nl = 1024, 512, 4

    def one(visit):
        txt = orc.double_gyre_params(nx, nl, extra=f"Ny = {ny}\n")
        g = QG(txt, strict=strict)
        g.option("quiet", 1)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
        g.set_const()
        if strict:
            g.option("uniform_S", 1)
        for k, v in dict(march=2, march_visit=visit, prolong_fused=0, block_small=block_small).items():
            g.option(k, v)
        assert g.param("march_levels") >= 1 and g.param("relax_path_0") == 3.0
        assert g.param("march_visit") == 0.0 and g.param("march_visit_ring") == -1.0
        g.option("profile", 2)
        g.profile_reset()
        g.set_tnext(float("inf"))
        out = dict(dts=[g.step() for _ in range(2)], psi=g.get(F["PSI"]), q=g.get(F["Q"]))
        assert g.profile_read("march_visit")[1] == 0 and g.profile_read("march_pl")[1] == 0
        assert g.profile_read("march_corr")[1] > 0     # the marched passes themselves ran
        g.close()
        return out
    a, b = one(2), one(0)
    assert a["dts"] == b["dts"]
    assert np.array_equal(a["psi"], b["psi"]) and np.array_equal(a["q"], b["q"])


def test_visit_against_oracle():
    """product build, the visit on, against the CPU oracle (general column solver): 3 steps at TOLERANCE 1e-12, <= 1e-10
    relative on psi and q -- the bound of tests/test_gpu_march.py::test_march_against_oracle"""
    nx, ny, nl = 1024, 512, 3
    o, g = make_pair(nx, ny, nl, strict=False, TOLERANCE=1e-12)
    g.option("march", 2)
    g.option("march_visit", 2)
    assert g.param("march_visit") == 1.0
    g.option("profile", 2)
    for _ in range(3):
        o.step(); g.step()
    assert g.profile_read("march_visit")[1] > 0
    assert g.t == pytest.approx(o.t, rel=1e-12)
    assert rel(g.get(F["Q"]), o.get(orc.Q)) <= 1e-10
    assert rel(g.get(F["PSI"]), o.get(orc.PSI)) <= 1e-10
