"""The wall-ring chunks around the fused finest-level visit (option march_visit_ring): 0 two passes over the whole chunk grid
with a skip rectangle, 1 two passes over the ring chunks only, 2 ring chunks as workgroups of two k_relax_visit launches.  The
same chunks run the same bodies on the same cells in all three, so psi, q, dt, the cycle count and the residuals are identical
bit for bit, in both builds.  The path is asserted through msom_get_param("march_visit_ring") (an ignored option would compare a
path with itself) and the profile slot march_visit, which counts once per visit."""
import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F

pytestmark = pytest.mark.gpu


def run(nx, ny, nl, strict, ring, steps=3, **opts):
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    if strict:
        g.option("uniform_S", 1)   # the chained smoother exists for the uniform-S column solver (opt-in in the strict build)
    for k, v in opts.items():
        g.option(k, v)
    g.option("march_visit", 2)     # also below the size where the fused visit gains (march_visit_min)
    g.option("march_visit_ring", ring)
    assert g.param("march_visit") == 1.0
    assert g.param("march_visit_ring") == float(ring)
    g.option("profile", 2)
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
    out["visits"] = g.profile_read("march_visit")[1]
    g.close()
    return out


def same(a, b):
    assert a["dts"] == b["dts"] and a["st"] == b["st"] and a["visits"] == b["visits"] > 0
    for k in ("psi1", "q1", "psi", "q"):
        assert np.all(np.isfinite(a[k])), k
        assert np.array_equal(a[k], b[k]), k


CASES = [(4096, 4096, 6), (2048, 2048, 2), (2048, 2048, 3), (2048, 2048, 5), (1024, 512, 6)]


@pytest.mark.parametrize("nx,ny,nl", CASES)
@pytest.mark.parametrize("strict", [True, False])
def test_ring_paths_give_the_same_bits(nx, ny, nl, strict):
    """after one RK2 step and after three.  1024 x 512: neither side is a multiple of a chunk height or strip width"""
    opts = dict(march=2) if nx * ny * nl < 2 ** 23 else {}
    ref = run(nx, ny, nl, strict, 0, **opts)
    for ring in (1, 2):
        same(run(nx, ny, nl, strict, ring, **opts), ref)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("opts", [dict(march_visit_rows=14), dict(march_visit_rows=42), dict(march_visit_pairs=1), dict(march_rows=8),
                                  dict(march_visit_rows=14, march_visit_split=2), dict(march_visit_rows=14, march_visit_split=1000)],
                         ids=lambda o: ",".join(f"{k}={v}" for k, v in o.items()))
def test_ring_paths_under_chunk_shapes(opts, strict):
    """fused chunk height, wave pairs per workgroup, ring chunk height and where the two launches of path 2 divide the fused
    chunk rows (2: nearly all in the second launch; beyond their number: all in the first) change no bit"""
    nx, ny, nl = 1024, 512, 4
    ref = run(nx, ny, nl, strict, 0, 2, march=2, **opts)
    for ring in (1, 2):
        same(run(nx, ny, nl, strict, ring, 2, march=2, **opts), ref)


def test_ring_parameter_without_a_fused_visit():
    """no fused visit on the handle: the parameter says so instead of echoing the option"""
    g = QG(orc.double_gyre_params(64, 3))
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(3, 64, 64))
    g.set_const()
    g.option("march_visit_ring", 2)
    assert g.param("march_visit") == 0.0 and g.param("march_visit_ring") == -1.0
    g.close()
