"""Vertical normal modes on the device (msom_modes_compute / _get / _project / _energy / _set_rd) against the numpy restatement of
msqg/eigmode.h in tests/modes_ref.py and against numpy in the expression order include/msom.h documents.

Stratifications: the table of workloads.LAYERS with MSOM_FR = table * (1 + 0.3 (2 rand - 1)) per cell and interface (fixed seed),
one case with varRo = 1, and the untouched uniform table (the compact form).  eps = 2^-52.

1. spectrum and vectors per column against modes_ref.modes_dgeev (S and dh taken from the handle):
     |iBu - ref| <= 8 nl eps max_m |iBu_ref|,   |M2L - ref|, |L2M - ref| <= 4 nl eps / gap * max|ref|,
   gap = the column's smallest eigenvalue gap over its largest eigenvalue, from the reference.  The two CPU routes of modes_ref
   differ among themselves by up to 3.2 nl eps and 0.72 nl eps / gap, so the bounds are 2.5x and 5.5x the reference's own noise.
   Every column must have gap >= 1e-4 and |vr[0][m]| / max|vr| >= 1e-6 (asserted on the reference); none is skipped.
2. structure of the device's own output, 3. projections, 4. compact against per-column form, 5. modal energies, 6. tiles,
7. the Rd hook of the wavelet filter, 8. state and errors."""
import ctypes as C
import functools

import numpy as np
import pytest

import modes_ref as R
import orc
from msom_amd import FIELDS as F
from msom_amd import MODES as MD
from msom_amd import QG, workloads
from test_gpu_bfn import TOL_PRODUCT
from test_gpu_hooks import DevBuf
from test_gpu_parity import rand_field, rel
from test_gpu_stats import ghosted, velocities
from test_gpu_tiled import assemble, run_tiled

pytestmark = pytest.mark.gpu

MSOM_ERR_ARG, MSOM_ERR_CONFIG, MSOM_ERR_STATE = -1, -3, -6
EPS = R.EPS
#        nx  ny  nl  extra                      stratification
CASES = [(64, 64, 3, "", "fr"),
         (128, 32, 6, "", "fr"),
         (32, 32, 1, "", "fr"),
         (32, 32, 2, "", "fr"),
         (32, 32, 8, "", "fr"),
         (32, 32, 9, "", "fr"),                 # above MSOM_FASTNL: the vector matrix in LDS
         (32, 32, 16, "", "fr"),
         (32, 32, 3, "varRo = 1\n", "varRo"),
         (32, 32, 6, "", "uniform"),            # compact form
         (32, 32, 16, "", "uniform"),
         (64, 64, 2, "sbc = -1\ntau0 = 0\n", "fr")]     # doubly periodic: the ghosts of the energy pass
IDS = [f"{c[0]}x{c[1]}x{c[2]}-{c[4]}" + ("-periodic" if "sbc = -1" in c[3] else "") for c in CASES]
BOTH = pytest.mark.parametrize("strict", [True, False], ids=["strict", "product"])
ALL = pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)


def params(nx, ny, nl, extra=""):
    return orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)


def random_fr(nl, ny, nx, seed=16):
    """the table value times 1 + 0.3 (2 rand - 1) per cell and interface.  The seed is one whose columns meet the condition test 1
    asserts on the reference (nl = 16, 32 x 32: smallest surface entry 2.5e-6 of the largest; seeds 11, 14, 18 fall below 1e-6)"""
    table = np.array(eval(workloads.LAYERS[nl][0]), dtype=np.float64)[:max(nl - 1, 1)]
    r = np.random.default_rng(seed).random((table.size, ny, nx))
    return table[:, None, None] * (1 + 0.3 * (2 * r - 1))


def make(nx, ny, nl, extra, strat, strict, compact=None):
    g = QG(params(nx, ny, nl, extra), strict=strict)
    g.option("quiet", 1)
    if compact is not None:
        g.option("modes_compact", compact)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    if strat == "fr":
        g.set(F["FR"], random_fr(nl, ny, nx))
    g.set_const()
    g.set_tnext(float("inf"))
    return g


class Dec:
    """one handle with its decomposition fetched, and the reference of the same inputs"""

    def __init__(self, case, strict):
        nx, ny, nl, extra, strat = CASES[case]
        self.nx, self.ny, self.nl, self.periodic = nx, ny, nl, "sbc = -1" in extra
        self.g = g = make(nx, ny, nl, extra, strat, strict)
        assert g.param("modes_ready") == 0
        g.modes_compute()
        assert g.param("modes_ready") == 1 and g.param("modes_compact") == (strat == "uniform")
        self.ibu, self.rd, self.m2l, self.l2m = (g.modes_get(MD[n]) for n in ("IBU", "RD", "M2L", "L2M"))
        self.dh = np.array([g.param(f"dh_{l}") for l in range(nl)])
        self.S = g.get(F["S"])
        self.ref = R.modes_dgeev(self.S, self.dh)       # (iBu, M2L, L2M, lambda)


@functools.lru_cache(maxsize=None)
def dec(case, strict):
    return Dec(case, strict)


def project_np(coef, x, nl, to_modes):
    """the documented order: acc = 0; acc = acc + c * x, inner index ascending.  coef: L2M (array m*nl + k) or M2L (array k*nl + m)"""
    out = np.empty_like(x)
    for o in range(nl):
        acc = np.zeros(x.shape[1:])
        for i in range(nl):
            acc = acc + coef[o * nl + i] * x[i]
        out[o] = acc
    return out


# ------------------------------------------------------------------ 1. against the reference

@BOTH
@ALL
def test_spectrum_and_vectors_against_reference(case, strict):
    d = dec(case, strict)
    nl = d.nl
    ibu, m2l, l2m, lam = d.ref
    gap = R.rel_gap(lam)
    assert gap.min() >= 1e-4 and R.surface_ratio(m2l, nl).min() >= 1e-6       # sorting and the surface sign are well defined
    bound_l = 8 * nl * EPS * np.abs(ibu).max(axis=0)
    r_l = np.abs(d.ibu - ibu).max(axis=0) / np.where(bound_l > 0, bound_l, 1)
    r_v = [np.abs(got - want).max(axis=0) / (4 * nl * EPS / gap * np.abs(want).max(axis=0)) for got, want in ((d.m2l, m2l), (d.l2m, l2m))]
    print(f"{IDS[case]} {'strict' if strict else 'product'}: min gap {gap.min():.2e}; worst error over its bound: iBu {r_l.max():.3f} "
          f"(= {8 * r_l.max():.2f} nl eps), M2L {r_v[0].max():.3f}, L2M {r_v[1].max():.3f} (= {4 * max(r_v[0].max(), r_v[1].max()):.2f} nl eps / gap)")
    assert np.all(np.abs(d.ibu - ibu) <= bound_l)
    assert r_v[0].max() <= 1 and r_v[1].max() <= 1


# ------------------------------------------------------------------ 2. structure of the device's own output

@BOTH
@ALL
def test_structure(case, strict):
    d = dec(case, strict)
    nl = d.nl
    assert d.g.L.msom_modes_layers(d.g.h, MD["IBU"]) == nl == d.g.L.msom_modes_layers(d.g.h, MD["RD"])
    assert d.g.L.msom_modes_layers(d.g.h, MD["M2L"]) == nl * nl == d.g.L.msom_modes_layers(d.g.h, MD["L2M"])
    assert np.all(d.ibu[0] == 0) and np.all(d.ibu[1:] < 0) and np.all(np.diff(d.ibu, axis=0) < 0)      # strictly descending
    assert np.all(d.m2l[:nl] > 0)                                                                       # vr[0][m]: positive at the surface
    assert np.all(d.rd[0] == 0)
    with np.errstate(divide="ignore"):
        assert np.array_equal(d.rd[1:], np.sqrt(-1.0 / d.ibu[1:]))
    M = d.m2l.reshape(nl, nl, d.ny, d.nx)                # [k][m]
    L = d.l2m.reshape(nl, nl, d.ny, d.nx)                # [m][k]
    want = d.dh[None, :, None, None] * np.swapaxes(M, 0, 1)
    if strict:
        assert np.array_equal(L, want)
    else:
        assert rel(L, want) <= TOL_PRODUCT
    orth = np.abs(np.einsum("mkyx,knyx->mnyx", L, M) - np.eye(nl)[:, :, None, None]).max()
    print(f"{IDS[case]}: max|L2M @ M2L - I| = {orth / (nl * EPS):.2f} nl eps")
    assert orth <= 8 * nl * EPS


# ------------------------------------------------------------------ 3. projections

@BOTH
@ALL
def test_projection_against_numpy(case, strict):
    d = dec(case, strict)
    g, nl = d.g, d.nl
    x = rand_field(70 + case, (nl, d.ny, d.nx))
    for to_modes, coef in ((1, d.l2m), (0, d.m2l)):
        want = project_np(coef, x, nl, to_modes)
        host = g.modes_project(x, to_modes)
        inplace = x.copy()
        g.modes_project(inplace, to_modes, out=inplace)                        # in == out, host
        a, b = DevBuf(x), DevBuf(np.zeros_like(x))
        assert g.L.msom_modes_project(g.h, to_modes, a.ptr, b.ptr) == 0          # device -> device: queued, not waited for
        assert g.L.msom_modes_project(g.h, to_modes, a.ptr, a.ptr) == 0          # in == out, device
        assert g.L.msom_sync(g.h) == 0
        dev, dev_inplace = b.host(), a.host()
        a.free(); b.free()
        for got in (host, inplace, dev, dev_inplace):
            if strict:
                assert np.array_equal(got, want), to_modes
            else:
                assert rel(got, want) <= TOL_PRODUCT, to_modes
            assert np.array_equal(got, host)                                    # every route runs the same kernel
    back = g.modes_project(g.modes_project(x, 1), 0)
    print(f"{IDS[case]}: round trip {np.abs(back - x).max() / (nl * EPS * np.abs(x).max()):.2f} nl eps max|x|")
    assert np.abs(back - x).max() <= 16 * nl * EPS * np.abs(x).max()


# ------------------------------------------------------------------ 4. compact against per-column form

@BOTH
@pytest.mark.parametrize("nl", [1, 3, 8, 12])
def test_compact_equals_per_column_form(nl, strict):
    nx = ny = 32
    a = make(nx, ny, nl, "", "uniform", strict)
    b = make(nx, ny, nl, "", "uniform", strict, compact=0)
    assert a.param("modes_compact") == 1 and b.param("modes_compact") == 0 and a.param("modes_bytes") == 0 == b.param("modes_bytes")
    a.modes_compute()
    b.modes_compute()
    assert a.param("modes_compact") == 1 and b.param("modes_compact") == 0
    assert a.param("modes_bytes") == 0 and b.param("modes_bytes") == (nl * nl + nl) * 8 * ny * nx
    for n in ("IBU", "RD", "M2L", "L2M"):
        ga, gb = a.modes_get(MD[n]), b.modes_get(MD[n])
        assert np.array_equal(ga, gb), n                                        # the same kernel on the same numbers
        assert np.all(ga == ga[:, :1, :1])                                      # broadcast
    x = rand_field(5, (nl, ny, nx))
    for to_modes in (1, 0):
        assert np.array_equal(a.modes_project(x, to_modes), b.modes_project(x, to_modes))
    for ea, eb in zip(a.modes_energy(), b.modes_energy()):
        assert np.allclose(ea, eb, rtol=2 * nx * ny * EPS, atol=0)
    a.close()
    b.close()


# ------------------------------------------------------------------ 5. energy

def energy_np(d):
    """(ke[m], pe[m]) from the fetched matrices, and the layer-space totals of the two identities"""
    g, nl = d.g, d.nl
    psi = g.get(F["PSI"])
    D = g.param("L0") / g.param("N")
    u, v = velocities(psi, d.periodic, 2.0 * D)
    um, vm, pm = (np.einsum("mkyx,kyx->myx", d.l2m.reshape(nl, nl, d.ny, d.nx), x) for x in (u, v, psi))
    ke = np.sum(0.5 * (um * um + vm * vm) * D ** 2, axis=(1, 2))
    pe = np.sum(0.5 * (-d.ibu) * pm * pm * D ** 2, axis=(1, 2))
    ke_layers = np.sum(0.5 * d.dh[:, None, None] * (u * u + v * v) * D ** 2)
    dhc = 0.5 * (d.dh[:-1] + d.dh[1:])
    pe_layers = np.sum(0.5 * d.S[:nl - 1] * (psi[:-1] - psi[1:]) ** 2 / dhc[:, None, None] * D ** 2)
    return ke, pe, ke_layers, pe_layers


@BOTH
@ALL
def test_modal_energy(case, strict):
    d = dec(case, strict)
    g, nl = d.g, d.nl
    tol = 2 * d.nx * d.ny * EPS      # any summation order of non-negative terms, plus the round-off of the summands
    ke, pe = g.modes_energy()
    ke_np, pe_np, ke_layers, pe_layers = energy_np(d)
    print(f"{IDS[case]}: ke {np.abs(ke / ke_np - 1).max():.2e}, pe {np.abs(pe[1:] / pe_np[1:] - 1).max() if nl > 1 else 0:.2e}, "
          f"sum ke {abs(ke.sum() / ke_layers - 1):.2e}, sum pe {abs(pe.sum() / pe_layers - 1) if nl > 1 else 0:.2e} (bound {tol:.2e})")
    assert pe[0] == 0 and np.all(ke > 0) and np.all(pe[1:] > 0)
    assert np.all(np.abs(ke - ke_np) <= tol * ke_np) and np.all(np.abs(pe - pe_np) <= tol * pe_np)
    assert abs(ke.sum() - ke_layers) <= tol * ke_layers               # l2m^T l2m = D
    assert abs(pe.sum() - pe_layers) <= tol * pe_layers               # l2m^T Lambda l2m = D amat
    only_ke, only_pe = np.full(nl, -1.0), np.full(nl, -1.0)
    dp = C.POINTER(C.c_double)
    assert g.L.msom_modes_energy(g.h, only_ke.ctypes.data_as(dp), None) == 0
    assert g.L.msom_modes_energy(g.h, None, only_pe.ctypes.data_as(dp)) == 0
    assert np.array_equal(only_ke, ke) and np.array_equal(only_pe, pe)
    assert g.L.msom_modes_energy(g.h, None, None) == MSOM_ERR_ARG


# ------------------------------------------------------------------ 6. tiles

@pytest.mark.parametrize("strat", ["fr", "uniform"])
def test_tiles_equal_single_tile(strat):
    """2 x 2 tiles in one process, strict build: the decomposition and the projections are pointwise, so bit for bit; the energies
    are summed per tile and then over the tiles, an order the single tile does not have, so they are held to the bound of 5."""
    nx = ny = 64
    nl, px, py = 3, 2, 2
    par = params(nx, ny, nl, "MGLEVELS = 5\n")
    psi = orc.synthetic_psi(nl, ny, nx)
    fr = random_fr(nl, ny, nx)
    x = rand_field(9, (nl, ny, nx))
    tx, ty = nx // px, ny // py

    def pre(g, rank):
        ix, iy = g.tile[2], g.tile[3]
        if strat == "fr":
            g.set(F["FR"], fr[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx])
            g.set_const()
        g.modes_compute()

    def fn(g, rank):
        ix, iy = g.tile[2], g.tile[3]
        xt = np.ascontiguousarray(x[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx])
        res = {n: g.modes_get(MD[n]) for n in ("IBU", "RD", "M2L", "L2M")}
        res.update(to_modes=g.modes_project(xt, 1), to_layers=g.modes_project(xt, 0), energy=g.modes_energy(), compact=g.param("modes_compact"))
        return res

    out = run_tiled(par, px, py, psi, nsteps=0, strict=True, fn=fn, pre=pre)
    g = QG(par, strict=True)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    if strat == "fr":
        g.set(F["FR"], fr)
    g.set_const()
    g.modes_compute()
    for o in out:
        o.update(o["extra"])
        assert o["compact"] == (strat == "uniform") == g.param("modes_compact")
    for n in ("IBU", "RD", "M2L", "L2M"):
        assert np.array_equal(assemble(out, n, px, py), g.modes_get(MD[n])), n
    assert np.array_equal(assemble(out, "to_modes", px, py), g.modes_project(x, 1))
    assert np.array_equal(assemble(out, "to_layers", px, py), g.modes_project(x, 0))
    ke, pe = g.modes_energy()
    tol = 2 * nx * ny * EPS
    for o in out:
        assert np.array_equal(o["energy"][0], out[0]["energy"][0]) and np.array_equal(o["energy"][1], out[0]["energy"][1])   # collective
        assert np.all(np.abs(o["energy"][0] - ke) <= tol * ke) and np.all(np.abs(o["energy"][1] - pe) <= tol * pe)
    g.close()


# ------------------------------------------------------------------ 7. the Rd hook

@BOTH
@pytest.mark.parametrize("case", [0, 8], ids=[IDS[0], IDS[8]])
def test_set_rd_feeds_the_wavelet_filter(case, strict):
    d = dec(case, strict)
    g = d.g
    nx, ny, nl, extra, strat = CASES[case]
    g.modes_set_rd(1)
    assert np.array_equal(g.get(F["RD"])[0], d.rd[1])
    other = make(nx, ny, nl, extra, strat, strict)
    other.set(F["RD"], d.rd[1:2])
    assert g.wavelet_levels() == other.wavelet_levels() > 1
    for k in range(g.wavelet_levels()):
        assert np.array_equal(g.siglev(k), other.siglev(k)), k
    if nl > 2:
        g.modes_set_rd(2)
        assert np.array_equal(g.get(F["RD"])[0], d.rd[2])
    for bad in (0, nl, -1):
        assert g.L.msom_modes_set_rd(g.h, bad) == MSOM_ERR_ARG
    other.close()


def test_set_rd_one_layer_is_an_argument_error():
    d = dec(2, True)
    assert d.nl == 1
    for mode in (0, 1):
        assert d.g.L.msom_modes_set_rd(d.g.h, mode) == MSOM_ERR_ARG


# ------------------------------------------------------------------ 8. state and errors

def test_call_order_and_errors():
    nx = ny = 32
    nl = 3
    g = QG(params(nx, ny, nl), strict=True)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    g.set_tnext(float("inf"))
    L, h = g.L, g.h
    big, x = np.full((nl * nl, ny, nx), 7.0), np.full((nl, ny, nx), 7.0)
    e = (C.c_double * nl)(*([7.0] * nl))

    def refused(code):
        for which in range(MD["N"]):
            assert L.msom_modes_layers(h, which) == code
            assert L.msom_modes_get(h, which, big.ctypes.data) == code
        assert L.msom_modes_project(h, 1, x.ctypes.data, x.ctypes.data) == code
        assert L.msom_modes_energy(h, e, e) == code
        assert L.msom_modes_set_rd(h, 1) == code
        assert np.all(big == 7.0) and np.all(x == 7.0) and list(e) == [7.0] * nl

    refused(MSOM_ERR_STATE)                                  # before msom_modes_compute
    assert g.param("modes_ready") == 0 and g.param("modes_bytes") == 0
    g.modes_compute()
    assert g.param("modes_ready") == 1
    for which in (-1, MD["N"]):
        assert L.msom_modes_layers(h, which) == MSOM_ERR_ARG and L.msom_modes_get(h, which, big.ctypes.data) == MSOM_ERR_ARG
    assert L.msom_modes_get(h, MD["IBU"], None) == MSOM_ERR_ARG
    assert L.msom_modes_project(h, 1, None, x.ctypes.data) == MSOM_ERR_ARG and L.msom_modes_project(h, 1, x.ctypes.data, None) == MSOM_ERR_ARG
    assert np.all(big == 7.0) and np.all(x == 7.0)
    g.set_const()                                            # drops the modes
    refused(MSOM_ERR_STATE)
    # one interface without stratification: the spectrum is degenerate
    fr = random_fr(nl, ny, nx)
    fr[1] = 0.0
    g.set(F["FR"], fr)
    g.set_const()
    assert L.msom_modes_compute(h) == MSOM_ERR_CONFIG and b"not positive" in L.msom_last_error()
    refused(MSOM_ERR_STATE)
    assert g.param("modes_ready") == 0 and g.param("modes_bytes") == 0
    assert g.step() > 0                                      # the handle stays usable
    g.set(F["FR"], random_fr(nl, ny, nx))
    g.set_const()
    g.modes_compute()                                        # and a sound stratification computes again
    assert g.param("modes_ready") == 1 and g.param("modes_bytes") == (nl * nl + nl) * 8 * ny * nx
    for bad in ("modes_compact",):
        assert L.msom_set_option(h, bad.encode(), 2.0) == MSOM_ERR_ARG
    g.close()


@BOTH
def test_bench_kernel_names(strict):
    d = dec(0, strict)
    ms = C.c_double(-1.0)
    for name in (b"modes_project", b"modes_energy"):
        assert d.g.L.msom_bench_kernel(d.g.h, name, 2, C.byref(ms)) == 0 and ms.value > 0
    assert d.g.L.msom_bench_kernel(d.g.h, b"modes_nothing", 2, C.byref(ms)) == MSOM_ERR_ARG
