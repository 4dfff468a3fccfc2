"""The newqg dialect (msom_create_newqg) on the device against tests/newqg_ref.py: the tendency kernel k_nq_rhs and its validation chain,
the Helmholtz solve, three steps, the golden file, known answers, guards, NetCDF and the energy diagnostic.  Strict build: the
reference's bits; product build: the project's bounds (1e-13 per kernel as tests/test_gpu_parity.rel measures it, 1e-10 for solves and
steps)."""
import ctypes as C
import os

import numpy as np
import pytest

import newqg_ref as nq
import orc
from msom_amd import FIELDS as F
from msom_amd import MGStats, NewQG, QG
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -52
C_MG = 0.0737
# the smallest shapes at which these kernels can go wrong (nx, ny, sbc, nq_rows): rows narrower than a wavefront and levels 4 -> 1;
# one strip plus its 4 halo lanes; tall; three strips of 60 output columns with seams inside the grid; doubly periodic; >= 4 chunks
SHAPES = [(16, 16, 0.0, 0), (16, 16, 100.0, 0), (64, 32, 0.0, 0), (64, 32, 100.0, 0), (64, 32, -1.0, 0), (32, 128, 100.0, 0), (32, 128, -1.0, 0),
          (128, 128, 0.0, 0), (128, 128, 100.0, 0), (128, 128, -1.0, 0), (64, 64, -1.0, 0), (32, 128, 100.0, 8), (32, 128, 0.0, 8)]
ALL_ON = dict(beta=0.5, nu=0.5, hEkb=0.3, gp_low=2500.0)


def make(par, strict, **opts):
    g = NewQG(par.text(), strict=strict)
    g.option("quiet", 1)
    for k, v in opts.items():
        g.option(k, v)
    return g


def field(seed, ny, nx, zero_mean=False):
    a = np.random.default_rng(seed).standard_normal((ny, nx))
    return a - a.mean() if zero_mean else a


def same(got, want, strict, bound, what):
    """strict: the bits; product: rel <= bound.  The ghost-dependent cells -- corners, then the first and last two rows and columns --
    are asserted on their own, so that a wrong corner or edge rule is named"""
    parts = {"corners": (np.array([0, 0, -1, -1]), np.array([0, -1, 0, -1]))}
    edge = np.zeros(want.shape, dtype=bool)
    edge[:2, :] = edge[-2:, :] = edge[:, :2] = edge[:, -2:] = True
    parts["edges"] = np.nonzero(edge)
    parts["interior"] = np.nonzero(~edge)
    scale = max(np.abs(want).max(), 1e-300)
    for name, idx in parts.items():
        if want[idx].size == 0:
            continue
        d = np.abs(got[idx] - want[idx]).max() / scale
        print(f"{what} {name}: rel {d:.3g}")
        if strict:
            assert np.array_equal(got[idx], want[idx]), (what, name, d)
        else:
            assert d <= bound, (what, name, d)


def frozen_step_ref(par, psi, qforc):
    """one step with NITERMAX = 0 -- both solves leave psi alone -- by the reference: (zeta, dq, q_out, dt)"""
    q0 = nq.comp_q(psi, par)
    zeta, dq = nq.tendency(psi, par, qforc)
    lim = nq.Limiter()
    dt, _ = nq.dtnext(0.0, np.inf, lim(nq.umax(psi, par), par.DT, par))
    return zeta, dq, q0 + dq * dt, dt


# ---------------------------------------------------------------- 1. k_nq_rhs against the reference

def run_rhs_case(par, strict, rows, use_qforc, seed=3):
    nx, ny = par.nx, par.ny
    psi = 100.0 * field(seed, ny, nx)   # max|u| large enough for the limiter to take D / max|u| (above D CFL / DT = 25)
    qforc = field(seed + 1, ny, nx) if use_qforc else None
    zeta_r, dq_r, qout_r, dt_r = frozen_step_ref(par, psi, qforc)
    for adv in (0, 1):
        g = make(par, strict, NITERMAX=0, nq_rows=rows, nq_adv_fused=adv)
        g.set(F["PSI"], psi[None])
        if use_qforc:
            g.set(F["QFORC"], qforc[None])
        g.set_const()
        if adv == 0:   # msom_update: zeta and dq of the psi the (skipped) solve leaves
            dq, _ = g.update()
            same(dq[0], dq_r, strict, 1e-13, "update dq")
            same(g.get(F["ZETA"])[0], zeta_r, strict, 1e-13, "update zeta")
            g.set_const()   # previous = 0 again
        dt = g.step()
        assert dt == dt_r if strict else abs(dt - dt_r) <= 1e-12 * dt_r
        same(g.get(F["ZETA"])[0], zeta_r, strict, 1e-13, f"adv_fused {adv} zeta")
        same(g.get(F["Q"])[0], qout_r, strict, 1e-13, f"adv_fused {adv} q_out")
        if adv == 0:
            same(g.get(F["DQ"])[0], dq_r, strict, 1e-13, "step dq")
        g.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,sbc,rows", SHAPES)
def test_rhs_kernel_against_ref_every_shape(nx, ny, sbc, rows, strict):
    run_rhs_case(nq.sample_par(nx, ny, sbc=sbc, **ALL_ON), strict, rows, True)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("off", ["beta", "nu", "hEkb", "gp_low", "QFORC", "all"])
@pytest.mark.parametrize("sbc", [100.0, -1.0])
def test_rhs_kernel_against_ref_every_term_off(off, sbc, strict):
    terms = dict(ALL_ON)
    for k in terms:
        if off in (k, "all"):
            terms[k] = 0.0
    run_rhs_case(nq.sample_par(64, 32, sbc=sbc, **terms), strict, 0, off not in ("QFORC", "all"), seed=5)


# ---------------------------------------------------------------- 2. fused against the validation chain

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,sbc,rows", SHAPES + [(1024, 512, 100.0, 0), (1024, 512, -1.0, 0)])
def test_fused_equals_chain(nx, ny, sbc, rows, strict):
    par = nq.sample_par(nx, ny, sbc=sbc, **ALL_ON)
    psi, qforc = 100.0 * field(21, ny, nx), field(22, ny, nx)
    out = {}
    for fused in (1, 0):
        for adv in (1, 0):
            g = make(par, strict, NITERMAX=0, nq_rows=rows, nq_fused=fused, nq_adv_fused=adv)
            g.set(F["PSI"], psi[None])
            g.set(F["QFORC"], qforc[None])
            g.set_const()
            dt = g.step()
            out[fused, adv] = (dt, g.get(F["ZETA"])[0], g.get(F["Q"])[0], g.get(F["DQ"])[0] if not (fused and adv) else None)
            g.close()
    dt0, z0, q0, dq0 = out[0, 0]
    for key, (dt, z, q, dq) in out.items():
        assert dt == dt0
        same(z, z0, strict, 1e-13, f"{key} zeta")
        same(q, q0, strict, 1e-13, f"{key} q")
        if dq is not None:
            same(dq, dq0, strict, 1e-13, f"{key} dq")


# ---------------------------------------------------------------- 3. msom_invertq against helm_ref.solve

SOLVE_SHAPES = [(16, 16, 0.0, 2500.0), (64, 32, 0.0, 2500.0), (32, 128, 0.0, 2500.0), (128, 128, 0.0, 2500.0), (64, 64, -1.0, 2500.0), (32, 32, 0.0, 0.0)]
_solve_ref = {}


def solve_ref(nx, ny, sbc, gp_low, tol, warm):
    """computed once per case, shared by the builds, never modified"""
    key = (nx, ny, sbc, gp_low, tol, warm)
    if key not in _solve_ref:
        par = nq.sample_par(nx, ny, sbc=sbc, gp_low=gp_low)
        q = field(7, ny, nx)
        psi0 = np.zeros((ny, nx))
        if warm:
            psi0 = 0.5 * solve_ref(nx, ny, sbc, gp_low, tol, False)[3] + 1e-3 * field(8, ny, nx)
        psi, st = nq.invert(psi0, q, par, tol=tol)
        for a in (q, psi0, psi):
            a.setflags(write=False)
        _solve_ref[key] = (par, q, psi0, psi, st)
    return _solve_ref[key]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("tol", [1e-9, 1e-5])
@pytest.mark.parametrize("nx,ny,sbc,gp_low", SOLVE_SHAPES)
def test_invertq_against_helm_ref(nx, ny, sbc, gp_low, tol, warm, strict):
    par, q, psi0, psi_r, st_r = solve_ref(nx, ny, sbc, gp_low, tol, warm)
    print(f"reference: cycles {st_r.i} nrelax {st_r.nrelax} resb {st_r.resb:.3g} resa {st_r.resa:.3g}")
    if tol == 1e-9 and not warm:   # the reference itself: a solve of several cycles in which the 1.2 / 10 rule has acted
        if (nx, ny) == (16, 16):
            assert (st_r.i, st_r.nrelax) == (2, 3)
        else:
            assert st_r.i >= 3 and st_r.nrelax == 2
    g = make(par, strict, TOLERANCE=tol)
    g.set_const()
    psi, st = g.invertq(q[None], psi0[None])
    psi = psi[0]
    assert np.array_equal(psi, g.get(F["PSI"])[0])
    assert (st.i, st.nrelax) == (st_r.i, st_r.nrelax)
    last = g.mgstats()
    assert (last.i, last.nrelax, last.resb, last.resa, last.sum) == (st.i, st.nrelax, st.resb, st.resa, st.sum)
    assert abs(st.sum - st_r.sum) <= nx * ny * EPS * np.abs(q).sum()
    if strict:
        assert np.array_equal(psi, psi_r) and st.resb == st_r.resb and st.resa == st_r.resa
    else:
        print("psi rel", rel(psi, psi_r))
        assert rel(psi, psi_r) <= 1e-10
        # the round-off floor of a residual (tests/test_gpu_modal_invert.py, one problem): (16 + 1) eps of the terms it is a difference of
        floor = 17 * EPS * (np.abs(q).max() + (abs(par.iRd2_low) + 8 / par.D**2) * np.abs(psi_r).max())
        for got, want in ((st.resa, st_r.resa), (st.resb, st_r.resb)):
            print(f"|diff| {abs(got - want):.3g} of {want:.3g}, floor {floor:.3g}")
            assert abs(got - want) <= 1e-9 * want + floor
    g.close()


# ---------------------------------------------------------------- 4. three steps

_steps_ref = {}


def steps_ref(nx, ny, sbc, tol):
    key = (nx, ny, sbc, tol)
    if key not in _steps_ref:
        par = nq.sample_par(nx, ny, sbc=sbc, TOLERANCE=tol)
        psi0 = orc.synthetic_psi(1, ny, nx, amp=500.0)[0]   # the limiter takes D / max|u|, which moves between the two updates of a step
        m = nq.Model(par, psi0)
        dts, stats = [], []
        for _ in range(3):
            dts.append(m.step())
            stats.append((m.stats.i, m.stats.nrelax, m.stats.resb, m.stats.resa))
        _steps_ref[key] = (par, psi0, m.psi.copy(), m.q.copy(), dts, stats)
    return _steps_ref[key]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,sbc", [(32, 32, 0.0), (32, 32, 100.0), (64, 32, 0.0), (64, 32, -1.0)])
def test_three_steps(nx, ny, sbc, strict):
    tol = 1e-5 if strict else 1e-12
    par, psi0, psi_r, q_r, dts_r, stats_r = steps_ref(nx, ny, sbc, tol)
    g = make(par, strict)
    g.set(F["PSI"], psi0[None])
    g.set_const()
    dts, stats = [], []
    for _ in range(3):
        dts.append(g.step())
        s = g.mgstats()
        stats.append((s.i, s.nrelax, s.resb, s.resa))
    # the dt sequence shows how often `previous` moved: once per update, in both updates of a step
    print("dt", dts, "reference", dts_r)
    assert g.iter == 3 and g.t == (dts[0] + dts[1]) + dts[2]
    q, psi = g.get(F["Q"])[0], g.get(F["PSI"])[0]
    if strict:
        assert dts == dts_r and stats == stats_r
        assert np.array_equal(q, q_r) and np.array_equal(psi, psi_r)
    else:
        assert all(abs(a - b) <= 1e-12 * b for a, b in zip(dts, dts_r))
        print("q rel", rel(q, q_r), "psi rel", rel(psi, psi_r))
        assert rel(q, q_r) <= 1e-10 and rel(psi, psi_r) <= 1e-10
    g.close()


@pytest.mark.parametrize("strict", [True, False])
def test_steps_to_a_scheduled_time(strict):
    """msom_set_tnext: dtnext() shortens the steps so that the event time is hit exactly (n == 0, dt1 < dt and the plain branch)"""
    tol = 1e-5 if strict else 1e-12
    par = nq.sample_par(32, TOLERANCE=tol)
    psi0 = orc.synthetic_psi(1, 32, 32, amp=500.0)[0]
    m = nq.Model(par, psi0)
    g = make(par, strict)
    g.set(F["PSI"], psi0[None])
    g.set_const()
    for tnext in (0.003, 0.0031, 0.02, np.inf):
        m.tnext = tnext
        g.set_tnext(tnext)
        for _ in range(2):
            dt_r, dt = m.step(), g.step()
            print("tnext", tnext, "dt", dt, "reference", dt_r, "t", g.t)
            if strict:
                assert dt == dt_r and g.t == m.t
            else:
                assert abs(dt - dt_r) <= 1e-12 * dt_r and abs(g.t - m.t) <= 1e-12 * m.t
    assert m.t >= 0.0031 and g.iter == 8
    q = g.get(F["Q"])[0]
    assert np.array_equal(q, m.q) if strict else rel(q, m.q) <= 1e-10
    g.close()


@pytest.mark.parametrize("strict", [True, False])
def test_create_from_the_sample_file(tmp_path, strict):
    path = tmp_path / "params.in"
    path.write_text(nq.SAMPLE)
    g = NewQG(path=str(path), strict=strict)
    par = nq.sample_par(128)
    for k, v in dict(model=1, N=128, ny=128, L0=100.0, DT=par.DT, CFL=0.2, TOLERANCE=1e-5, f0=46.5, nu=0.5, gp_low=2500.0, bc_fac=0.0,
                     iRd2_low=par.iRd2_low, nlevels=7).items():
        assert g.param(k) == v, k
    psi = field(6, 128, 128)
    g.set(F["PSI"], psi[None])
    g.set_const()
    q, want = g.get(F["Q"])[0], nq.comp_q(psi, par)
    assert np.array_equal(q, want) if strict else rel(q, want) <= 1e-13
    g.close()


@pytest.mark.parametrize("case", ["sbc0", "sbc100"])
def test_strict_build_reproduces_the_golden_file(case):
    gold = np.load(os.path.join(HERE, "golden", "newqg_32.npz"))
    par = nq.sample_par(32, sbc=float(gold[f"{case}_in_sbc"]))
    out = {}
    for adv in (1, 0):
        g = make(par, True, nq_adv_fused=adv)
        g.set(F["PSI"], gold[f"{case}_in_psi"][None])
        g.set_const()
        dts, stats = [], []
        for _ in range(3):
            dts.append(g.step())
            s = g.mgstats()
            stats.append((s.i, s.nrelax, s.resb, s.resa))
        assert np.array_equal(np.array(dts), gold[f"{case}_dt"])
        assert np.array_equal(np.array(stats, dtype=np.float64), gold[f"{case}_mgstats"])
        assert np.array_equal(g.get(F["PSI"])[0], gold[f"{case}_psi"]) and np.array_equal(g.get(F["Q"])[0], gold[f"{case}_q"])
        if not adv:
            assert np.array_equal(g.get(F["DQ"])[0], gold[f"{case}_dq"])
        g.close()


# ---------------------------------------------------------------- 5. known answer on the device

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("gp_low", [0.0, 2500.0])
def test_eigenfunction_through_comp_q_and_invertq(gp_low, strict):
    par = nq.sample_par(32, gp_low=gp_low, TOLERANCE=1e-12)
    x = (np.arange(32) + 0.5) * par.D
    psi = np.sin(2 * np.pi * x / par.L0)[:, None] * np.sin(3 * np.pi * x / par.L0)[None, :]
    lam = -(4 / par.D**2) * (np.sin(3 * np.pi * par.D / (2 * par.L0)) ** 2 + np.sin(2 * np.pi * par.D / (2 * par.L0)) ** 2)
    g = make(par, strict)
    g.set_const()
    q = g.comp_q(psi[None])[0]
    assert np.abs(q - (lam + par.iRd2_low) * psi).max() <= 16 * EPS * 4 / par.D**2
    got, st = g.invertq(((lam + par.iRd2_low) * psi)[None])
    err = np.abs(got[0] - psi).max()
    print(f"cycles {st.i} resa {st.resa:.3g} err {err:.3g} bound {st.resa * C_MG * par.L0**2:.3g}")
    assert st.resa <= 1e-12 and err <= st.resa * C_MG * par.L0**2
    g.close()


# ---------------------------------------------------------------- 6. state and guards

def refused_calls(g):
    """every entry point of msom.h that is an msqg operator, called on the handle g; yields (name, return code)"""
    L, h = g.L, g.h
    a = np.zeros((1, g.ny, g.nx))
    p = a.ctypes.data
    d, st, ci = C.c_double(), MGStats(), [C.c_int() for _ in range(6)]
    yield "msom_remove_mean", L.msom_remove_mean(h, F["PSI"])
    yield "msom_read_inputs", L.msom_read_inputs(h, b".")
    yield "pystep_bfn", L.pystep_bfn(h, p, 1, g.ny, g.nx, p, 1, g.ny, g.nx, 1.0, 1)
    yield "pyq2p", L.pyq2p(h, p, 1, g.ny, g.nx, p, 1, g.ny, g.nx)
    yield "pyp2q", L.pyp2q(h, p, 1, g.ny, g.nx, p, 1, g.ny, g.nx)
    yield "msom_bfn_begin", L.msom_bfn_begin(h)
    yield "msom_bfn_steps", L.msom_bfn_steps(h, 1, 0.1, 1.0, 0.0)
    yield "msom_bfn_misfit", L.msom_bfn_misfit(h, C.byref(d))
    yield "msom_stats_begin", L.msom_stats_begin(h, 1)
    yield "msom_stats_accumulate", L.msom_stats_accumulate(h, 1.0)
    yield "msom_stats_weight", L.msom_stats_weight(h, C.byref(d))
    yield "msom_stats_get", L.msom_stats_get(h, 0, p)
    yield "msom_time_filter", L.msom_time_filter(h, 0.1)
    yield "msom_modes_compute", L.msom_modes_compute(h)
    yield "msom_modes_layers", L.msom_modes_layers(h, 0)
    yield "msom_modes_get", L.msom_modes_get(h, 0, p)
    yield "msom_modes_project", L.msom_modes_project(h, 1, p, p)
    yield "msom_modes_energy", L.msom_modes_energy(h, C.byref(d), None)
    yield "msom_modes_set_rd", L.msom_modes_set_rd(h, 1)
    yield "msom_modes_mgstats", L.msom_modes_mgstats(h, 0, C.byref(st))
    yield "msom_run", L.msom_run(h, b".", 1)
    yield "msom_write_bas", L.msom_write_bas(h, F["PSI"], b"/nonexistent/x.bas")
    yield "msom_read_bas", L.msom_read_bas(h, F["PSI"], b"/nonexistent/x.bas")
    yield "msom_wavelet_filter", L.msom_wavelet_filter(h, 1.0)
    yield "msom_energy_tend", L.msom_energy_tend(h, 0.1)
    yield "msom_filter_de", L.msom_filter_de(h, F["PSI"], 1.0)
    yield "msom_reset_de", L.msom_reset_de(h)
    yield "pystep_de", L.pystep_de(h, *([p, 1, g.ny, g.nx] * 7), 0)
    yield "msom_dbg_wavelet_levels", L.msom_dbg_wavelet_levels(h)
    yield "msom_dbg_siglev", L.msom_dbg_siglev(h, 0, p)
    yield "msom_dbg_wavelet_apply", L.msom_dbg_wavelet_apply(h, F["PSI"])
    yield "msom_tile_info", L.msom_tile_info(h, *(C.byref(v) for v in ci))
    yield "msom_dbg_relax", L.msom_dbg_relax(h, 0, p, p, 1)
    yield "msom_dbg_residual", L.msom_dbg_residual(h, p, p, p, C.byref(d))
    yield "msom_dbg_helm_relax", L.msom_dbg_helm_relax(h, 0, p, p, 2, None)
    yield "msom_dbg_helm_residual", L.msom_dbg_helm_residual(h, p, p, p, C.byref(d))
    yield "msom_dbg_restrict", L.msom_dbg_restrict(h, 0, p, p)
    yield "msom_dbg_prolong", L.msom_dbg_prolong(h, 1, p, p)
    yield "msom_dbg_op", L.msom_dbg_op(h, b"del2", F["PSI"], F["ZETA"], 0.0, 1.0)


@pytest.mark.parametrize("strict", [True, False])
def test_state_and_guards(strict):
    par = nq.sample_par(32)
    g = make(par, strict)
    assert g.param("model") == 1
    for k, v in dict(N=32, nx=32, ny=32, nl=1, L0=100.0, DT=par.DT, CFL=0.2, tend=200.0, dtout=0.1, f0=46.5, beta=0.5, nu=0.5, hEkb=0.0, tau0=1e-3,
                     gp_low=2500.0, sbc=0.0, bc_fac=0.0, iRd2_low=par.iRd2_low, dh_0=1.0, nlevels=5).items():
        assert g.param(k) == v, k
    # call order: nothing that needs q = comp_q(psi) runs before msom_set_const
    assert g.L.msom_update(g.h, None, None, 1.0) == -6
    dt = C.c_double()
    assert g.L.msom_step(g.h, C.byref(dt)) == -6
    psi = field(1, 32, 32)
    g.set(F["PSI"], psi[None])
    g.set_const()
    q0, p0 = g.get(F["Q"]), g.get(F["PSI"])
    # msqg operators: MSOM_ERR_CONFIG, a message naming the call, psi and q untouched
    n = 0
    for name, rc in refused_calls(g):
        assert rc == -3, (name, rc)
        assert name in g.L.msom_last_error().decode(), name
        n += 1
    assert n == 39
    assert np.array_equal(g.get(F["Q"]), q0) and np.array_equal(g.get(F["PSI"]), p0)
    # fields and options of the other dialect
    a = np.zeros((1, 32, 32))
    for fid in range(34):
        if fid in NewQG.FIELD_IDS:
            assert g.L.msom_field_layers(g.h, fid) == 1
        else:
            assert g.L.msom_field_layers(g.h, fid) == 0
            assert g.L.msom_set_field(g.h, fid, a.ctypes.data) == -1 and g.L.msom_get_field(g.h, fid, a.ctypes.data) == -1
    for key in ("fused", "march", "mode_pv_invert", "stochastic", "rhs_variant", "bogus"):
        assert g.L.msom_set_option(g.h, key.encode(), 1.0) == -1, key
    for key in ("TOLERANCE", "NITERMAX", "NITERMIN", "DT", "quiet", "profile", "nq_fused", "nq_adv_fused", "nq_rows"):
        assert g.L.msom_set_option(g.h, key.encode(), g.param(key) if key in ("TOLERANCE", "DT") else 1.0) == 0, key
    g.close()


@pytest.mark.parametrize("strict", [True, False])
def test_msqg_handle_beside_a_newqg_handle(strict):
    txt = orc.double_gyre_params(32, 2)
    psi0 = orc.synthetic_psi(2, 32, 32)

    def three_steps(with_newqg):
        n = None
        if with_newqg:
            n = make(nq.sample_par(32), strict)
            n.set(F["PSI"], field(4, 32, 32)[None])
            n.set_const()
        g = QG(txt, strict=strict)
        assert g.param("model") == 0
        g.set(F["PSI"], psi0)
        g.set_const()
        dts = []
        for _ in range(3):
            dts.append(g.step())
            if n is not None:
                n.step()
        out = (dts, g.get(F["Q"]), g.get(F["PSI"]))
        g.close()
        if n is not None:
            n.close()
        return out

    a, b = three_steps(False), three_steps(True)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ---------------------------------------------------------------- 7. NetCDF, 8. energy

@pytest.mark.parametrize("strict", [True, False])
def test_write_nc_then_read_nc(tmp_path, strict):
    par = nq.sample_par(32)
    g = make(par, strict)
    psi = field(9, 32, 32)
    g.set(F["PSI"], psi[None])
    g.set_const()
    path = str(tmp_path / "vars.nc")
    g.write_nc(path)
    g.set(F["PSI"], np.zeros((1, 32, 32)))
    g.read_nc(F["PSI"], path, "psi")
    assert np.array_equal(g.get(F["PSI"])[0], psi.astype(np.float32).astype(np.float64))
    g.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,sbc", [(64, 32, 0.0), (64, 64, -1.0)])
def test_ke_against_ref(nx, ny, sbc, strict):
    par = nq.sample_par(nx, ny, sbc=sbc)
    psi = field(12, ny, nx)
    m = nq.Model(par, psi)
    terms = m.ke_terms()
    g = make(par, strict)
    g.set(F["PSI"], psi[None])
    g.set_const()
    ke = g.ke()
    print("ke", ke, "reference", terms.sum())
    assert abs(ke - terms.sum()) <= nx * ny * EPS * np.abs(terms).sum()
    g.close()
