"""Known answers for tests/newqg_ref.py, the numpy restatement the GPU tests hold the newqg dialect to (no GPU here)."""
import os

import numpy as np
import pytest

import newqg_ref as nq
import orc

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = np.finfo(np.float64).eps
C_MG = 0.0737   # |psi error| <= resa * C_MG * L0^2 on the square with the wall on the face


def eigenfunction(par, k, l):
    nx, ny = par.nx, par.ny
    x = (np.arange(nx) + 0.5) * par.D
    y = (np.arange(ny) + 0.5) * par.D
    Ly = par.L0 * ny / nx
    psi = np.sin(l * np.pi * y / Ly)[:, None] * np.sin(k * np.pi * x / par.L0)[None, :]
    lam = -(4 / par.D**2) * (np.sin(k * np.pi * par.D / (2 * par.L0)) ** 2 + np.sin(l * np.pi * par.D / (2 * Ly)) ** 2)
    return psi, lam


@pytest.mark.parametrize("gp_low", [0.0, 2500.0])
def test_comp_q_of_the_discrete_eigenfunction(gp_low):
    par = nq.sample_par(32, gp_low=gp_low)
    psi, lam = eigenfunction(par, 3, 2)
    q = nq.comp_q(psi, par)
    want = (lam + par.iRd2_low) * psi
    # round-off of the five-point sum: a few eps of the largest term 4 |psi| / D^2
    assert np.abs(q - want).max() <= 16 * EPS * 4 / par.D**2


@pytest.mark.parametrize("gp_low", [0.0, 2500.0])
def test_solve_returns_the_eigenfunction(gp_low):
    par = nq.sample_par(32, gp_low=gp_low)
    psi, lam = eigenfunction(par, 3, 2)
    q = (lam + par.iRd2_low) * psi
    got, st = nq.invert(np.zeros_like(psi), q, par, tol=1e-12)
    assert st.resa <= 1e-12
    # the Helmholtz term only makes the operator more definite: the Poisson bound holds
    err = np.abs(got - psi).max()
    print(f"gp_low {gp_low}: cycles {st.i} resa {st.resa:.3e} err {err:.3e} bound {st.resa * C_MG * par.L0**2:.3e}")
    assert err <= st.resa * C_MG * par.L0**2


def test_arakawa_invariants_on_the_periodic_domain():
    par = nq.sample_par(32, sbc=-1.0)
    rng = np.random.default_rng(5)
    psi = rng.standard_normal((32, 32))
    pp = nq.pad_psi(psi, True)
    zeta = nq.lap(pp, par.D)
    zp = nq.pad_zq(zeta, pp, par.bc_fac, True)
    J = nq.jacobian(pp, zp, par.D)
    for w in (np.ones_like(psi), psi, zeta):
        assert abs((w * J).sum()) <= 64 * EPS * np.abs(w * J).sum()


def test_ghost_rules_and_the_corner():
    par = nq.sample_par(16, sbc=100.0)
    rng = np.random.default_rng(2)
    psi = rng.standard_normal((16, 16))
    pp = nq.pad_psi(psi, False)
    assert np.array_equal(pp[1:-1, 0], -psi[:, 0]) and np.array_equal(pp[-1, 1:-1], -psi[-1, :])
    assert pp[0, 0] == psi[0, 0] and pp[-1, 0] == psi[-1, 0] and pp[0, -1] == psi[0, -1] and pp[-1, -1] == psi[-1, -1]
    z = nq.pad_zq(np.zeros_like(psi), pp, par.bc_fac, False)
    assert par.bc_fac == 100.0 / ((0.5 * 100.0 + 1) * par.D * par.D)
    assert np.array_equal(z[1:-1, 0], par.bc_fac * (psi[:, 0] - pp[1:-1, 0]))       # = 2 bc_fac psi
    assert np.array_equal(z[0, 1:-1], par.bc_fac * (psi[0, :] - pp[0, 1:-1]))
    # the corner: the y rule on the x-ghost column, bc_fac * (psi[x-ghost, interior row] - psi[corner ghost]) = -2 bc_fac psi
    assert z[0, 0] == par.bc_fac * (pp[1, 0] - pp[0, 0]) == par.bc_fac * (-psi[0, 0] - psi[0, 0])
    assert z[-1, -1] == par.bc_fac * (pp[-2, -1] - pp[-1, -1])
    # free slip: every ghost is a zero
    z0 = nq.pad_zq(np.zeros_like(psi), pp, 0.0, False)
    assert not z0[0, :].any() and not z0[:, 0].any() and not z0[-1, :].any() and not z0[:, -1].any()


def test_limiter_recurrence():
    par = nq.sample_par(32)   # D = 3.125, CFL = 0.2
    lim = nq.Limiter()
    D, CFL = par.D, par.CFL
    # previous = 0: the first value is damped towards 0
    d1 = lim(10.0, 1.0, par)
    assert d1 == (0.0 + 0.1 * (D / 10.0 * CFL)) / 1.1
    # growing: damped again from d1
    d2 = lim(10.0, 1.0, par)
    assert d2 == (d1 + 0.1 * (D / 10.0 * CFL)) / 1.1
    # a large velocity: the limit drops below previous and is taken as it is
    d3 = lim(1e4, 1.0, par)
    assert d3 == D / 1e4 * CFL and lim.previous == d3
    # no flow: dtmax / CFL * CFL, damped
    d4 = lim(0.0, 1.0, par)
    assert d4 == (d3 + 0.1 * (1.0 / CFL * CFL)) / 1.1


def test_psi_of_the_ref_and_of_the_layered_oracle_agree():
    """independent pin: with gp_low = 0 the layered oracle at nl = 1 solves the same Poisson problem by its own code"""
    N, L0, tol = 32, 100.0, 1e-12
    par = nq.sample_par(N, gp_low=0.0)
    rng = np.random.default_rng(11)
    q = rng.standard_normal((N, N))
    psi_r, st = nq.invert(np.zeros((N, N)), q, par, tol=tol)
    o = orc.Oracle(orc.double_gyre_params(N, 1, L0=L0), TOLERANCE=tol, quiet=1)
    o.set_const()
    o.set(orc.Q, q[None])
    so = o.invertq()
    psi_o = o.get(orc.PSI)[0]
    assert st.resa <= tol and so.resa <= tol
    assert np.abs(psi_r - psi_o).max() <= (st.resa + so.resa) * C_MG * L0**2


@pytest.mark.parametrize("case", ["sbc0", "sbc100"])
def test_golden_file_is_reproduced_bit_for_bit(case):
    g = np.load(os.path.join(HERE, "golden", "newqg_32.npz"))
    par = nq.sample_par(32, sbc=float(g[f"{case}_in_sbc"]))
    m = nq.Model(par, g[f"{case}_in_psi"])
    dts, stats = [], []
    for _ in range(3):
        dts.append(m.step())
        stats.append((m.stats.i, m.stats.nrelax, m.stats.resb, m.stats.resa))
    assert np.array_equal(m.psi, g[f"{case}_psi"]) and np.array_equal(m.q, g[f"{case}_q"]) and np.array_equal(m.dq, g[f"{case}_dq"])
    assert np.array_equal(np.array(dts), g[f"{case}_dt"])
    assert np.array_equal(np.array(stats, dtype=np.float64), g[f"{case}_mgstats"])
