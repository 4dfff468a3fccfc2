"""Option rhs_close: the speculative tendency pass (k_rhs_lpw, RES instantiation with CLS = 1 / 2) also closes the solve in front of it --
max|b - (lap + Gamma) psi|, and in the second RK stage max|u| per layer -- instead of a launch of k_resmax_march on the same psi.  In the
first stage dt comes from max|u|, which stays in front of the pass as the psi-only form of k_resmax_march.

The by-products repeat k_resmax_march's operations one for one (in the product build: its fused multiply-add pattern), so a run with the
option at 1 or 2 equals the run with 0 BIT FOR BIT in both builds: psi, q, every dt and (i, resb, resa, nrelax) of the last solve.
mgstats().sum is held to rel = 1e-12, the margin tests/test_gpu_rhs_resid.py gives it (the option does not touch it).

Every handle is forced onto the marched finest level (options march = 2 and uniform_S = 1, as tests/test_gpu_march.py does), so that the
smoother's last pass applies the correction, and every test asserts what msom_get_param("rhs_close") reports: a silent fallback would pass
everything else.  The chained smoother takes levels of at least 512 x 64 cells (sweep_path), so the grids whose by-product must run are the
smallest of that kind: 512 columns are 9 strips of 58, the last one ragged, and with nl = 5 (two strips per workgroup) the last workgroup's
second strip lies past the right edge.  One layer has no uniform S in this library and stays on the parent's path.  The narrower grids of tests/test_gpu_rhs_resid.py (64 x 64 x 1 ... 128 x 16 x 3, the last with fewer
rows than one chunk) cannot be marched: there the correction is applied by the residual pass, the option must report 0 and the runs are held
equal all the same (SMALL)."""
import gc

import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F

pytestmark = pytest.mark.gpu

# nl = 2: top and bottom layers only; 5: idle wavefronts and a strip past the right edge; 6: the benchmark's layers, two chunks;
# nl = 3, 4, 7, 8: every NL is a register allocation of its own in k_resmax_march
GRIDS = [(512, 64, 2), (512, 64, 5), (512, 128, 6), (512, 64, 3), (512, 64, 4), (512, 64, 7), (512, 64, 8)]
# not marched: the option resolves to 0.  So does one layer at any size: S counts as uniform from two layers on (build_coefs), the max-only
# pass of a one-layer handle is not k_resmax_march and the tendency kernel's is not the UNI instantiation
SMALL = [(64, 64, 1), (128, 64, 2), (256, 64, 5), (256, 128, 6), (128, 16, 3), (512, 64, 1)]
BUILDS = [True, False]


def params(nx, ny, nl, extra=""):
    return orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)


def fr_field(g, nx, ny, nl):
    """bench.py's spatially varying Froude field"""
    x, y = (np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny
    shape = 1.0 + 0.3 * np.outer(np.sin(2 * np.pi * y), np.cos(2 * np.pi * x))
    g.set(F["FR"], np.stack([g.param(f"Fr_{l}") * shape for l in range(nl - 1)]))


def qforc_field(g, nx, ny, nl):
    g.set(F["QFORC"], 1e-4 * np.random.default_rng(5).standard_normal((nl, ny, nx)))


def handle(nx, ny, nl, strict, close, extra="", pre=None, tol=1e-7, psi_scale=1.0, **opts):
    g = QG(params(nx, ny, nl, extra), strict=strict)
    g.option("quiet", 1)
    g.option("TOLERANCE", tol)
    g.option("march", 2)
    g.option("uniform_S", opts.pop("uniform_S", 1))
    g.option("rhs_resid", opts.pop("rhs_resid", 1))
    if close is not None:
        g.option("rhs_close", close)
    for k, v in opts.items():
        g.option(k, v)
    if pre:
        pre(g, nx, ny, nl)
    g.set(F["PSI"], psi_scale * orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    return g


def snap(g, dts):
    st = g.mgstats()
    return g.get(F["PSI"]), g.get(F["Q"]), list(dts), (st.i, st.resb, st.resa, st.nrelax), st.sum


def run(nx, ny, nl, strict, close, expect=None, **kw):
    """3 steps, snapshots after the first and the last; expect: what the handle must report for rhs_close (default: what was asked)"""
    g = handle(nx, ny, nl, strict, close, **kw)
    assert g.param("rhs_close") == (close if expect is None else expect)
    dts, out = [], []
    for n in range(3):
        dts.append(g.step())
        if n in (0, 2):
            out.append(snap(g, dts))
    assert g.param("rhs_close") == (close if expect is None else expect)
    g.close()
    return out


def same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]), "psi"
        assert np.array_equal(x[1], y[1]), "q"
        assert x[2] == y[2], "dt"
        assert x[3] == y[3], f"(i, resb, resa, nrelax): {x[3]} / {y[3]}"
        assert x[4] == pytest.approx(y[4], rel=1e-12), "sum"
    assert len(a) == len(b)


def both_against_off(nx, ny, nl, strict, **kw):
    ref = run(nx, ny, nl, strict, 0, **kw)
    for close in (1, 2):
        same(run(nx, ny, nl, strict, close, **kw), ref)
    return ref


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("tol", [1e-7, 1e-3])   # several cycles per solve: the speculative pass is discarded; one: it is accepted
@pytest.mark.parametrize("nx,ny,nl", GRIDS)
def test_steps_equal_option_off(nx, ny, nl, tol, strict):
    both_against_off(nx, ny, nl, strict, tol=tol)


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("nx,ny,nl", SMALL)
def test_small_grids_resolve_to_off(nx, ny, nl, strict):
    ref = run(nx, ny, nl, strict, 0, tol=1e-3)
    for close in (1, 2):
        same(run(nx, ny, nl, strict, close, expect=0, tol=1e-3), ref)


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("tol", [1e-7, 1e-3])
def test_speculative_pass(tol, strict):
    """async_solve = 0: no speculative pass, the option resolves to 0; every run equals the plain one"""
    nx, ny, nl = 512, 64, 5
    ref = both_against_off(nx, ny, nl, strict, tol=tol, async_solve=1)
    for close in (1, 2):
        same(run(nx, ny, nl, strict, close, expect=0, tol=tol, async_solve=0), ref)
    cycles = ref[-1][3][0]
    assert cycles == 1 if tol == 1e-3 else cycles > 1   # accepted / discarded, as the case is meant


# chunk heights (rhs_dbg = rows << 8) that are odd (made even for the by-products) or do not divide ny, the ghost-line body everywhere,
# partial and free slip walls, a 3-D forcing (the QF instantiations)
VARIANTS = {
    "rows9_odd": dict(rhs_dbg=9 << 8),
    "rows10": dict(rhs_dbg=10 << 8),
    "rows13_odd": dict(rhs_dbg=13 << 8),
    "edge_body": dict(lpw_dbg=4),
    "partial_slip": dict(extra="sbc = 2.0\n"),
    "free_slip": dict(extra="sbc = 0\n"),
    "qforc": dict(pre=qforc_field),
}


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("nx,ny,nl", [(512, 64, 5), (512, 128, 6)])
def test_variants_equal_option_off(nx, ny, nl, variant, strict):
    both_against_off(nx, ny, nl, strict, tol=1e-3, **VARIANTS[variant])


def cfl_scale(nx, ny, nl, frac=0.25):
    """factor on synthetic_psi that puts CFL D / max|u| at about frac DT.  The viscous clamp of set_const may halve DT (0.05 -> 0.025):
    the smaller one is taken, so the CFL limit binds by a factor of two at least"""
    D, CFL, DT = 80.0 / nx, 0.6, 0.025
    psi = orc.synthetic_psi(nl, ny, nx)
    gy, gx = np.gradient(psi, D, axis=(1, 2))
    return CFL * D / (frac * DT * max(np.abs(gx).max(), np.abs(gy).max()))


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("nx,ny,nl", [(512, 64, 5), (512, 64, 2)])
def test_max_u_sets_dt(nx, ny, nl, strict):
    """psi scaled until CFL D / max|u| < DT: every dt then comes from max|u|, the first stage's from the psi-only pass and the limiter's
    `previous` of the next step from the second stage's by-product.  Without this case the max|u| bits reach no compared number"""
    scale = cfl_scale(nx, ny, nl)
    kw = dict(tol=1e-3 * scale, psi_scale=scale)   # the solve is linear in psi: the tolerance that gives one cycle scales with it
    ref = both_against_off(nx, ny, nl, strict, **kw)
    g = handle(nx, ny, nl, strict, 0, **kw)
    DT = g.param("DT")
    g.close()
    dts = ref[-1][2]
    assert len(dts) == 3 and all(0 < dt < DT for dt in dts), (dts, DT)
    assert dts[0] != dts[1] and dts[1] != dts[2], dts
    assert ref[-1][3][0] == 1   # one cycle per solve: the speculative passes counted


# what turns the by-product off: a spatially varying Froude field (general S), the doubly periodic box, no residual by-product to ride
# beside, more layers than the fast kernels take
OFF = {
    "fr": dict(pre=fr_field, uniform_S=0),
    "periodic": dict(extra="sbc = -1\ntau0 = 0\n"),
    "rhs_resid_0": dict(rhs_resid=0),
    "nl16": dict(),
}


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("why", sorted(OFF))
def test_conditions_that_turn_it_off(why, strict):
    nx, ny, nl = (512, 64, 16) if why == "nl16" else (512, 64, 5)
    ref = run(nx, ny, nl, strict, 0, tol=1e-3, **OFF[why])
    for close in (1, 2):
        same(run(nx, ny, nl, strict, close, expect=0, tol=1e-3, **OFF[why]), ref)


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("tol", [1e-7, 1e-3])
def test_option_toggled_between_steps(tol, strict):
    nx, ny, nl = 512, 64, 2
    out = []
    for toggle in (True, False):
        g = handle(nx, ny, nl, strict, 0, tol=tol)
        dts = [g.step()]
        if toggle:
            g.option("rhs_close", 2)
            assert g.param("rhs_close") == 2
        dts.append(g.step())
        dts.append(g.step())
        if toggle:
            g.option("rhs_close", 0)
        assert g.param("rhs_close") == 0
        dts.append(g.step())
        out.append([snap(g, dts)])
        g.close()
    same(*out)


def test_option_values():
    g = handle(512, 64, 2, False, None)
    assert g.param("rhs_close") == 0       # far below the size from which the default turns it on
    for v in (1, 2, 0, -1):
        g.option("rhs_close", v)
        assert g.param("rhs_close") == max(v, 0)
    with pytest.raises(Exception):
        g.option("rhs_close", 3)
    g.option("rhs_close", 2)
    g.option("mg_fused", 0)                # no fused solve: no speculative pass to ride in
    assert g.param("rhs_close") == 0
    g.close()


# what the default resolves to at the two benchmark sizes that turn the residual by-product on
FULL = [(4096, 6, 2), (2048, 3, 2)]


@pytest.mark.parametrize("n,nl,default", FULL)
def test_full_size_default_equals_option_off(n, nl, default):
    """the metric size and the next one down, product build, default options against rhs_close = 0, after 1 and 3 steps (hazards of this
    kernel family have shown only at full size)"""
    psi0 = orc.synthetic_psi(nl, n, n)
    ref = []
    for close in (0, None):
        g = QG(params(n, n, nl), strict=False)
        g.option("quiet", 1)
        if close is not None:
            g.option("rhs_close", close)
        g.set(F["PSI"], psi0)
        g.set_const()
        # the default must have resolved to on here: otherwise both handles run the same path and the comparison says nothing
        assert g.param("rhs_close") == (0 if close == 0 else default)
        dts = []
        for k in range(3):
            dts.append(g.step())
            if k in (0, 2):
                st = g.mgstats()
                cur = (g.get(F["PSI"]), g.get(F["Q"]), list(dts), (st.i, st.resb, st.resa, st.nrelax), st.sum)
                if close == 0:
                    ref.append(cur)
                else:
                    same([cur], [ref[k // 2]])
                    ref[k // 2] = None
                del cur
        g.close()
        gc.collect()
