"""GPU parity tests (run with -m gpu on the MI355X box): the HIP path, called through the
C ABI (include/msom.h via msom_amd.api), against the CPU oracle on the same seeded inputs.

Two builds of the same kernels are checked:
  * strict (libmsomhip_strict.so: -ffp-contract=off, reference expression order, true
    divisions): BIT-EXACT against the oracle with red-black ordering on both sides;
  * fast (libmsomhip.so, the product: FMA contraction, reciprocal multiplies, uniform-S
    column solver): within the fp64 tolerances stated next to each assertion.
"""
import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F

pytestmark = pytest.mark.gpu

CASES = [(32, 32, 3), (64, 64, 2), (64, 32, 3), (32, 64, 6), (32, 32, 1), (16, 16, 4)]


def make_pair(nx, ny, nl, strict, extra="", psi=None, **opts):
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)
    o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1)
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    for k, v in opts.items():
        o.option(k, v)
        g.option(k, v)
    p0 = orc.synthetic_psi(nl, ny, nx) if psi is None else psi
    o.set(orc.PSI, p0)
    g.set(F["PSI"], p0)
    o.set_const()
    g.set_const()
    return o, g


def rel(a, b):
    d = np.abs(a - b).max()
    s = max(np.abs(b).max(), 1e-300)
    return d / s


def rand_field(seed, shape, scale=1.0):
    return scale * np.random.default_rng(seed).standard_normal(shape)


# ------------------------------------------------------------------ strict build: bit-exact

@pytest.mark.parametrize("nx,ny,nl", CASES)
def test_strict_operators_bit_exact(nx, ny, nl):
    o, g = make_pair(nx, ny, nl, strict=True)
    assert np.array_equal(g.get(F["Q"]), o.get(orc.Q))          # comp_q in set_const
    assert np.array_equal(g.get(F["S"]), o.get(orc.S))
    psi = rand_field(1, (nl, ny, nx))
    # pyp2q = comp_del2 + comp_stretch
    q_g = np.empty_like(psi)
    g.pyp2q(psi, q_g)
    assert np.array_equal(q_g, o.pyp2q(psi))
    # comp_del2 with add != 0 and comp_stretch alone
    o.set(orc.ZETA, psi[::-1].copy()); g.set(F["ZETA"], psi[::-1].copy())
    o.comp_del2(orc.PSI, orc.ZETA, 0.5, -2.0); g.op("del2", F["PSI"], F["ZETA"], 0.5, -2.0)
    assert np.array_equal(g.get(F["ZETA"]), o.get(orc.ZETA))
    o.comp_stretch(orc.PSI, orc.ZETA, 1.0, 0.3); g.op("stretch", F["PSI"], F["ZETA"], 1.0, 0.3)
    assert np.array_equal(g.get(F["ZETA"]), o.get(orc.ZETA))


@pytest.mark.parametrize("nx,ny,nl", CASES)
def test_strict_advection_bit_exact(nx, ny, nl):
    o, g = make_pair(nx, ny, nl, strict=True)
    psi, zeta = rand_field(2, (nl, ny, nx)), rand_field(3, (nl, ny, nx))
    for m, P, Z, D in ((o, orc.PSI, orc.ZETA, orc.DQ), (g, F["PSI"], F["ZETA"], F["DQ"])):
        m.set(P, psi); m.set(Z, zeta); m.set(D, 0.1 * psi)
    o.advection_pv(orc.ZETA, orc.Q, orc.PSI, orc.DQ, 1.0)
    g.op("advection", F["ZETA"], F["DQ"])
    assert np.array_equal(g.get(F["DQ"]), o.get(orc.DQ))


def test_strict_advection_with_background_flow_bit_exact():
    nx = ny = 32; nl = 3
    o, g = make_pair(nx, ny, nl, strict=True, extra="upg = [0.3,0.1,0.0]\nvpg = [0.0,-0.2,0.05]\nflsrv = 1\n")
    assert np.array_equal(g.get(F["PSIPG"]), o.get(orc.PSIPG))
    assert np.array_equal(g.get(F["ZETAPG"]), o.get(orc.ZETAPG))
    psi, zeta = rand_field(4, (nl, ny, nx)), rand_field(5, (nl, ny, nx))
    for m, P, Z, D in ((o, orc.PSI, orc.ZETA, orc.DQ), (g, F["PSI"], F["ZETA"], F["DQ"])):
        m.set(P, psi); m.set(Z, zeta); m.set(D, np.zeros_like(psi))
    o.reset_limiter()
    dt_o = o.advection_pv(orc.ZETA, orc.Q, orc.PSI, orc.DQ, 1e10)
    g.op("advection", F["ZETA"], F["DQ"])
    assert np.array_equal(g.get(F["DQ"]), o.get(orc.DQ))
    # full update incl. the 2*nl limiter calls with the cached background-flow velocity
    o2, g2 = make_pair(nx, ny, nl, strict=True, extra="upg = [0.3,0.1,0.0]\nvpg = [0.0,-0.2,0.05]\nflsrv = 1\n", TOLERANCE=1e-9)
    d_o = o2.update()
    dq_g, d_g = g2.update(want=True)
    assert d_g == d_o
    assert np.array_equal(dq_g, o2.get(orc.DQ))


@pytest.mark.parametrize("nx,ny,nl", CASES)
def test_strict_multigrid_pieces_bit_exact(nx, ny, nl):
    o, g = make_pair(nx, ny, nl, strict=True)
    assert g.nlevels() == o.nlevels()
    a, b = rand_field(6, (nl, ny, nx)), rand_field(7, (nl, ny, nx))
    r_o, m_o = o.residual(a, b)
    r_g, m_g = g.residual(a, b)
    assert np.array_equal(r_g, r_o) and m_g == m_o
    for lev in range(g.nlevels()):
        lx, ly = g.level_dims(lev)
        assert (lx, ly) == o.level_dims(lev)
        da, res = rand_field(8 + lev, (nl, ly, lx)), rand_field(20 + lev, (nl, ly, lx))
        for ns in (1, 3):
            assert np.array_equal(g.relax(lev, da, res, ns), o.relax(lev, da, res, ns)), (lev, ns)
        if lev + 1 < g.nlevels():
            assert np.array_equal(g.restrict(lev, res), o.restrict(lev, res))
        if lev >= 1:
            assert np.array_equal(g.prolong(lev, da), o.prolong(lev, da))


@pytest.mark.parametrize("nx,ny,nl", CASES)
@pytest.mark.parametrize("tol", [1e-3, 1e-11])
def test_strict_invertq_bit_exact(nx, ny, nl, tol):
    o, g = make_pair(nx, ny, nl, strict=True, TOLERANCE=tol)
    q = o.get(orc.Q) + rand_field(9, (nl, ny, nx), 1e-6)
    p_o = o.pyq2p(q)
    p_g = np.empty_like(q)
    g.pyq2p(p_g, q)
    so, sg = o.mgstats(), g.mgstats()
    assert (sg.i, sg.nrelax) == (so.i, so.nrelax)
    assert sg.resb == so.resb and sg.resa == so.resa
    assert sg.sum == pytest.approx(so.sum, rel=1e-12, abs=1e-18)   # summation order differs
    assert np.array_equal(p_g, p_o)


@pytest.mark.parametrize("nx,ny,nl", [(32, 32, 3), (64, 32, 2), (32, 32, 6), (32, 32, 1)])
def test_strict_ten_steps_bit_exact(nx, ny, nl):
    o, g = make_pair(nx, ny, nl, strict=True)
    o.set_tnext(1.0); g.set_tnext(1.0)
    for k in range(10):
        o.step()
        dt = g.step()
        assert dt == o.dt, k
        assert g.t == o.t
    assert np.array_equal(g.get(F["Q"]), o.get(orc.Q))
    assert np.array_equal(g.get(F["PSI"]), o.get(orc.PSI))
    # KE line of msqg/qg.c:108: summation order differs between CPU and GPU -> 1e-13 relative
    assert g.ke() == pytest.approx(o.ke(), rel=1e-13)


def test_strict_topography_qforcing_and_slip():
    nx = ny = 32; nl = 3
    o, g = make_pair(nx, ny, nl, strict=True, extra="sbc = 2.0\nEks = 0.001\nRe = 500\n", TOLERANCE=1e-9)
    x = (np.arange(nx) + 0.5) / nx
    topo = 0.01 * np.exp(-((x[None, :] - 0.5) ** 2 + (x[:, None] - 0.5) ** 2) * 30)[None]
    qf = rand_field(11, (nl, ny, nx), 1e-7)
    o.set(orc.TOPO, topo); g.set(F["TOPO"], topo)
    o.option("flag_topo", 1)
    o.set(orc.QFORC, qf); g.set(F["QFORC"], qf)
    d_o = o.update()
    dq_g, d_g = g.update()
    assert d_g == d_o
    assert np.array_equal(dq_g, o.get(orc.DQ))


def test_strict_pystep_bfn_both_directions():
    nx = ny = 32; nl = 3
    o, g = make_pair(nx, ny, nl, strict=True, TOLERANCE=1e-9)
    q = o.get(orc.Q)
    for direction in (1.0, -1.0, 1.0):
        tend = np.empty_like(q)
        g.pystep_bfn(q, tend, direction, 1)
        assert np.array_equal(tend, o.pystep_bfn(q, direction))


def test_strict_stochastic_variant_bit_exact():
    """-D_STOCHASTIC path (msqg/qg_stochastic.h) with the reference-exact serial rand() noise."""
    nx = ny = 16; nl = 3
    o, g = make_pair(nx, ny, nl, strict=True, extra="tr_stoch = 50\namp_stoch = 1e-5\n", stochastic=1)
    sig = np.abs(rand_field(12, (nl, ny, nx)))
    o.set(orc.SIGMA, sig); g.set(F["SIGMA"], sig)
    import ctypes
    libc = ctypes.CDLL(None)
    for m in (o, g):
        libc.srand(7)
        m.set_tnext(float('inf'))
        for _ in range(3):
            m.step()
        m.q_end = m.get(orc.Q if m is o else F["Q"])
    assert np.array_equal(g.q_end, o.q_end)


# ------------------------------------------------------------------ fast (product) build: tolerances

@pytest.mark.parametrize("nx,ny,nl,extra", [(64, 64, 3, ""), (128, 64, 6, ""), (64, 64, 2, "sbc = 0.5\n")])
def test_fast_stochastic_rides_in_the_tendency_pass(nx, ny, nl, extra):
    """Product build, -D_STOCHASTIC (msqg/qg_stochastic.h:36-63, 128-149): relaxation and noise are folded into q_in by
    a pre-pass and the advance rides in the tendency kernel (stoch_fused = 1); against the separate kernels
    (stoch_fused = 0) and against the oracle on the same serial rand() stream."""
    import ctypes
    libc = ctypes.CDLL(None)
    ex = extra + "tr_stoch = 50\namp_stoch = 1e-5\n"
    sig = np.abs(rand_field(12, (nl, ny, nx)))
    res = []
    for which in ("oracle", 1, 0):
        o, g = make_pair(nx, ny, nl, strict=False, extra=ex, stochastic=1, TOLERANCE=1e-12)
        m = o if which == "oracle" else g
        if which != "oracle":
            g.option("stoch_fused", which)
        m.set(orc.SIGMA if m is o else F["SIGMA"], sig)
        libc.srand(7)
        m.set_tnext(float("inf"))
        for _ in range(4):
            m.step()
        res.append(m.get(orc.Q if m is o else F["Q"]))
    assert rel(res[1], res[0]) <= 1e-9 and rel(res[2], res[0]) <= 1e-9
    assert rel(res[1], res[2]) <= 1e-10 and not np.array_equal(res[1], res[2])   # the two paths are different code


@pytest.mark.parametrize("nx,ny,nl", CASES)
def test_fast_operators_within_tolerance(nx, ny, nl):
    o, g = make_pair(nx, ny, nl, strict=False)
    assert g.param("uniform_S") == (1.0 if nl > 1 else 0.0)
    psi, zeta = rand_field(2, (nl, ny, nx)), rand_field(3, (nl, ny, nx))
    q_g = np.empty_like(psi)
    g.pyp2q(psi, q_g)
    assert rel(q_g, o.pyp2q(psi)) <= 1e-13     # per-kernel parity gate of SURVEY 8d
    for m, P, Z, D in ((o, orc.PSI, orc.ZETA, orc.DQ), (g, F["PSI"], F["ZETA"], F["DQ"])):
        m.set(P, psi); m.set(Z, zeta); m.set(D, np.zeros_like(psi))
    o.advection_pv(orc.ZETA, orc.Q, orc.PSI, orc.DQ, 1.0)
    g.op("advection", F["ZETA"], F["DQ"])
    assert rel(g.get(F["DQ"]), o.get(orc.DQ)) <= 1e-13
    a, b = rand_field(6, (nl, ny, nx)), rand_field(7, (nl, ny, nx))
    r_o, m_o = o.residual(a, b)
    r_g, m_g = g.residual(a, b)
    assert rel(r_g, r_o) <= 1e-13 and m_g == pytest.approx(m_o, rel=1e-13)
    for lev in range(g.nlevels()):
        lx, ly = g.level_dims(lev)
        da, res = rand_field(8 + lev, (nl, ly, lx)), rand_field(20 + lev, (nl, ly, lx))
        assert rel(g.relax(lev, da, res, 2), o.relax(lev, da, res, 2)) <= 1e-13, lev
        if lev >= 1:
            assert rel(g.prolong(lev, da), o.prolong(lev, da)) <= 1e-15


@pytest.mark.parametrize("uniform", [0, 1])
def test_fast_general_S_field_path(uniform):
    """Spatially varying Froude number (frpg file in the reference) uses the S-field kernels."""
    nx = ny = 32; nl = 3
    o, g = make_pair(nx, ny, nl, strict=False)
    x = (np.arange(nx) + 0.5) / nx
    fr = np.stack([0.0023669 * (1 + 0.3 * np.sin(2 * np.pi * x[None, :]) * np.ones((ny, 1))),
                   0.0076173 * (1 + 0.2 * np.cos(2 * np.pi * x[:, None]) * np.ones((1, nx)))])
    if uniform == 0:
        o.set(orc.FR, fr); g.set(F["FR"], fr)
    o.set_const(); g.set_const()
    assert g.param("uniform_S") == float(uniform)
    lx, ly = g.level_dims(1)
    da, res = rand_field(1, (nl, ly, lx)), rand_field(2, (nl, ly, lx))
    assert rel(g.relax(1, da, res, 2), o.relax(1, da, res, 2)) <= 1e-13
    q = o.get(orc.Q)
    o.option("TOLERANCE", 1e-11); g.option("TOLERANCE", 1e-11)
    p_g = np.empty_like(q)
    g.pyq2p(p_g, q)
    assert rel(p_g, o.pyq2p(q)) <= 1e-9


@pytest.mark.parametrize("nx,ny,nl", [(64, 64, 3), (64, 32, 6), (32, 32, 1)])
def test_fast_ten_steps_tight_tolerance(nx, ny, nl):
    """10-step run with TOLERANCE = 1e-12: <= 1e-10 relative on psi and q."""
    o, g = make_pair(nx, ny, nl, strict=False, TOLERANCE=1e-12)
    o.set_tnext(1.0); g.set_tnext(1.0)
    for _ in range(10):
        o.step()
        g.step()
    assert g.t == pytest.approx(o.t, rel=1e-12)
    assert rel(g.get(F["Q"]), o.get(orc.Q)) <= 1e-10
    assert rel(g.get(F["PSI"]), o.get(orc.PSI)) <= 1e-10
    assert g.ke() == pytest.approx(o.ke(), rel=1e-9)


def test_fast_hundred_steps_reference_tolerance_ke():
    """At the reference TOLERANCE = 1e-3 (1 cycle per solve): ke_1 within 1e-4 after 100 steps."""
    nx = ny = 64; nl = 3
    o, g = make_pair(nx, ny, nl, strict=False)
    o.set_tnext(float('inf')); g.set_tnext(float('inf'))
    for _ in range(100):
        o.step()
        g.step()
    assert g.ke() == pytest.approx(o.ke(), rel=1e-4)
    assert g.mgstats().i == o.mgstats().i


def test_lex_reference_ordering_vs_gpu_red_black():
    """Reference-faithful lexicographic GS (CPU) vs red-black (GPU): same discrete solution
    once both are converged (TOLERANCE 1e-12), SURVEY section 7 hard part 2(b)."""
    nx = ny = 64; nl = 3
    txt = orc.double_gyre_params(nx, nl)
    o = orc.Oracle(txt, smoother=orc.GS_LEX, quiet=1, TOLERANCE=1e-12)
    o.set(orc.PSI, orc.synthetic_psi(nl, ny, nx)); o.set_const()
    g = QG(txt); g.option("quiet", 1); g.option("TOLERANCE", 1e-12)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); g.set_const()
    q = o.get(orc.Q)
    p_g = np.empty_like(q)
    g.pyq2p(p_g, q)
    p_o = o.pyq2p(q)
    # bound derived from the two runs themselves: each side stops with max|res| = resa, and an iterate with residual r is
    # within |A^-1|_inf * r of the discrete solution; |A^-1|_inf <= max of the solution of -lap(w) = 1 on the square with
    # w = 0 on the walls = 0.0737 L0^2 (the stretching term only makes the operator more definite; its barotropic mode
    # has eigenvalue 0, so the Poisson bound is attained).  Measured: 8.7e-8 relative at 32^2 x 3 (tests/golden), 3.9e-8
    # at 64^2 x 3 (round 1) against a bound of ~4e-7.
    resa = g.mgstats().resa + o.mgstats().resa
    bound = resa * 0.0737 * 80.0 ** 2 / np.abs(p_o).max()
    assert resa < 2e-12 and bound < 1e-6
    assert rel(p_g, p_o) <= bound


def test_bas_files_byte_identical(tmp_path):
    nx = ny = 32; nl = 3
    o, g = make_pair(nx, ny, nl, strict=True)
    po, pg = str(tmp_path / "o.bas"), str(tmp_path / "g.bas")
    o.write_bas(orc.Q, po)
    g.write_bas(F["Q"], pg)
    assert open(po, "rb").read() == open(pg, "rb").read()
    g2 = QG(orc.double_gyre_params(nx, nl), strict=True)
    g2.read_bas(F["PSI"], pg)
    assert np.array_equal(g2.get(F["PSI"]), g.get(F["Q"]).astype(np.float32).astype(np.float64))


def test_error_convention():
    from msom_amd import MsomError
    with pytest.raises(MsomError):
        QG("N = 48\nnl = 2\n")            # not a power of two
    with pytest.raises(MsomError):
        QG("N = 32\nnl = 17\n")           # more layers than the column solver supports
    g = QG("N = 32\nnl = 2\nFr = [0.1]\ndh = [0.5,0.0]\nRom = 0.1\n")
    with pytest.raises(MsomError, match="thickness"):
        g.set_const()                      # reference: "thickness = 0: aborting", qg.h:990-996
    g = QG("N = 32\nnl = 2\nFr = [0.1]\ndh = [0.5,0.5]\n")
    with pytest.raises(MsomError, match="Rom"):
        g.set_const()                      # reference: "Rom <= 0: aborting", qg.h:1009-1012
    with pytest.raises(MsomError):
        QG(path="/nonexistent/params.in")


# ------------------------------------------------------------------ full-size properties (BASELINE config)

@pytest.mark.parametrize("N,nl", [(2048, 3), (4096, 6)])
def test_full_size_properties(N, nl):
    """Size-independent properties at BASELINE.json's sizes (the oracle comparison at these sizes is
    tests/test_gpu_oracle_fullsize.py): analytic eigenfunction of lap + Gamma (closed-form q and closed-form inverse), linearity
    of comp_q, and self-consistency of the reported residual."""
    txt = orc.double_gyre_params(N, nl)
    g = QG(txt)
    g.option("quiet", 1)
    g.set_const()
    S = [(g.param(f"Fr_{l}") / g.param("Rom")) ** 2 for l in range(nl - 1)]
    G = np.zeros((nl, nl))
    for l in range(nl):
        if l > 0:
            c = S[l - 1] * g.param(f"idh0_{l}"); G[l, l - 1] += c; G[l, l] -= c
        if l < nl - 1:
            c = S[l] * g.param(f"idh1_{l}"); G[l, l + 1] += c; G[l, l] -= c
    gam, vec = np.linalg.eig(G)
    D = 80.0 / N
    x = (np.arange(N) + 0.5) / N
    k, m_, iv = 3, 5, 1
    h = np.outer(np.sin(m_ * np.pi * x), np.sin(k * np.pi * x))
    psi = 1e-3 * vec[:, iv].real[:, None, None] * h[None]
    lam = -(4 / D**2) * (np.sin(k * np.pi / (2 * N)) ** 2 + np.sin(m_ * np.pi / (2 * N)) ** 2)
    q_exact = (lam + gam[iv].real) * psi
    q = np.empty_like(psi)
    g.pyp2q(psi, q)
    # conditioning of the 5-point stencil on a smooth field: eps * |psi| * 8/D^2
    assert np.abs(q - q_exact).max() <= 4e-16 * np.abs(psi).max() * 8 / D**2 * 4
    # linearity
    psi2 = np.roll(psi, 1, axis=0)
    qa, qb = np.empty_like(psi), np.empty_like(psi)
    g.pyp2q(psi2, qa)
    g.pyp2q(psi + 2 * psi2, qb)
    assert np.abs(qb - (q + 2 * qa)).max() <= 1e-12 * np.abs(qb).max() + 4e-16 * np.abs(psi).max() * 8 / D**2 * 8
    del qa, qb, psi2
    # inverse: tight tolerance recovers psi
    g.option("TOLERANCE", 1e-7 * np.abs(q_exact).max())
    p = np.empty_like(psi)
    g.pyq2p(p, q_exact)
    st = g.mgstats()
    assert st.resa <= 1e-7 * np.abs(q_exact).max() and st.i < 30
    assert np.abs(p - psi).max() <= 1e-5 * np.abs(psi).max()
    # reported residual == recomputed residual
    _, mres = g.residual(p, q_exact)
    assert mres == pytest.approx(st.resa, rel=1e-12)


@pytest.mark.parametrize("nx,ny,nl", [(64, 64, 3), (128, 32, 6), (32, 32, 1), (16, 16, 2), (256, 128, 4)])
@pytest.mark.parametrize("extra", ["", "sbc = 1.5\nRe = 300\nEks = 0.001\n"])
def test_fused_tendency_equals_unfused_chain(nx, ny, nl, extra):
    """kernels_fused.hip (one pass over psi) against the kernel-per-reference-loop chain:
    bit-exact in the strict build, and both bit-exact against the oracle."""
    o, g = make_pair(nx, ny, nl, strict=True, extra=extra, TOLERANCE=1e-9)
    qf = rand_field(31, (nl, ny, nx), 1e-7)
    o.set(orc.QFORC, qf); g.set(F["QFORC"], qf)
    q = o.get(orc.Q)
    d_o = o.update()
    g.option("fused", 1)
    dq1, d1 = g.update()
    g.option("fused", 0)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); 
    g2 = make_pair(nx, ny, nl, strict=True, extra=extra, TOLERANCE=1e-9)[1]
    g2.set(F["QFORC"], qf)
    g2.option("fused", 0)
    dq0, d0 = g2.update()
    assert d1 == d0 == d_o
    assert np.array_equal(dq1, dq0)
    assert np.array_equal(dq1, o.get(orc.DQ))


@pytest.mark.parametrize("nx,ny,nl,uniform", [(512, 64, 3, 1), (256, 128, 6, 0), (256, 64, 1, 1), (1024, 32, 2, 1)])
def test_wide_level_two_point_relax_kernel(nx, ny, nl, uniform):
    """k_relax_color_x2 (two same-colour points per thread, 16-byte accesses) is used when a
    half row is >= 128 wide: bit-exact in the strict build, 1e-13 in the product build."""
    for strict in (True, False):
        o, g = make_pair(nx, ny, nl, strict=strict)
        if not uniform:
            x = (np.arange(nx) + 0.5) / nx
            fr = np.stack([o.param(f"Fr_{l}") * (1 + 0.3 * np.sin(2 * np.pi * (l + 1) * x))[None, :] * np.ones((ny, 1)) for l in range(nl - 1)])
            o.set(orc.FR, fr); g.set(F["FR"], fr)
            o.set_const(); g.set_const()
        for lev in (0, 1):
            lx, ly = g.level_dims(lev)
            da, res = rand_field(40 + lev, (nl, ly, lx)), rand_field(50 + lev, (nl, ly, lx))
            got, ref = g.relax(lev, da, res, 2), o.relax(lev, da, res, 2)
            if strict:
                assert np.array_equal(got, ref), (lev, strict)
            else:
                assert rel(got, ref) <= 1e-13, (lev, strict)
        # and through the whole solver
        q = o.get(orc.Q) + rand_field(9, (nl, ny, nx), 1e-6)
        p_g = np.empty_like(q)
        g.pyq2p(p_g, q)
        p_o = o.pyq2p(q)
        if strict:
            assert np.array_equal(p_g, p_o)
        else:
            assert rel(p_g, p_o) <= 1e-9


@pytest.mark.parametrize("nx,ny,nl,extra", [(256, 128, 6, ""), (128, 16, 3, "sbc = -1\n"), (512, 32, 1, ""), (256, 256, 4, "varRo = 1\n")])
@pytest.mark.parametrize("strict", [True, False])
def test_lds_correct_residual_equals_plain(nx, ny, nl, extra, strict):
    """k_correct_residual (correction + residual + face velocities through an LDS tile) against
    k_residual2<CORRECT> (rhs_dbg bit 128 selects the plain kernel; bit 256 the plain red-prolong kernel): psi, q, dt and the multigrid statistics
    of a few steps are identical bit for bit in both builds."""
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)
    out = {}
    for dbg in (0, 128 + 256):      # 256: one-parity-per-thread form of the fused red half-sweep + prolongation
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("rhs_dbg", dbg); g.option("TOLERANCE", 1e-7)
        g.option("rhs_resid", 0 if dbg else 1)        # first residual of a solve: from the tendency pass (option) / from k_residual2
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
        g.set_const()
        dts = [g.step() for _ in range(3)]
        st = g.mgstats()
        out[dbg] = (g.get(F["PSI"]), g.get(F["Q"]), dts, (st.i, st.resb, st.resa))
        g.close()
    if strict:
        assert np.array_equal(out[0][0], out[384][0]) and np.array_equal(out[0][1], out[384][1])
        assert out[0][2] == out[384][2] and out[0][3] == out[384][3]
    else:  # the product build's tendency pass forms the residual with a different association (one carried number)
        assert rel(out[0][0], out[384][0]) <= 1e-9 and rel(out[0][1], out[384][1]) <= 1e-11
        assert out[0][2] == pytest.approx(out[384][2], rel=1e-9) and out[0][3][0] == out[384][3][0]


@pytest.mark.parametrize("nx,ny,nl", [(256, 128, 6), (64, 64, 3), (32, 32, 1), (512, 64, 2), (128, 128, 8), (128, 64, 7), (64, 64, 5), (256, 256, 4)])
@pytest.mark.parametrize("strict", [True, False])
def test_one_launch_coarse_levels_equal_per_kernel_path(nx, ny, nl, strict):
    """option mg_coarse: the levels of at most 32 cells a side (option mg_coarse_dim) solved by ONE workgroup (k_mg_coarse) give the
    same psi as the kernel-per-half-sweep path (bit for bit in the strict build)"""
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    out = {}
    for opt in (0, 1, 2, 3):   # 1: the levels through global memory, 2: resident in LDS, 3: the same with the pool pre-filled with NaN
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("TOLERANCE", 1e-8)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
        g.set_const()
        g.option("mg_coarse", opt)
        for _ in range(2):
            g.step()
        st = g.mgstats()
        out[opt] = (g.get(F["PSI"]), (st.i, st.resa))
        g.close()
    for opt in (1, 2, 3):
        if strict:
            assert np.array_equal(out[0][0], out[opt][0]) and out[0][1] == out[opt][1], opt
        else:
            assert rel(out[opt][0], out[0][0]) <= 1e-10 and out[0][1][0] == out[opt][1][0], opt
    # the one-launch variants run the same per-point code: identical among themselves in both builds; NaN anywhere in the LDS
    # pool would surface here if a cell were read before the launch wrote it
    assert np.array_equal(out[1][0], out[2][0]) and np.array_equal(out[2][0], out[3][0]) and np.isfinite(out[3][0]).all()


@pytest.mark.parametrize("nx,ny,nl", [(128, 64, 3), (64, 64, 6), (256, 128, 2), (192, 80, 4), (64, 32, 1)])
@pytest.mark.parametrize("strict", [True, False])
def test_blocked_smoother_equals_plain_sweeps(nx, ny, nl, strict):
    """k_relax_block (two red-black sweeps per pass through LDS, optional on-the-fly
    prolongation) must reproduce the plain colour-by-colour sweeps bit for bit."""
    if nx == 192:
        pytest.skip("non power-of-two grids are rejected at create time")
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    res = {}
    for blk in (1, 0):
        g = QG(txt, strict=strict)
        g.option("quiet", 1)
        g.option("uniform_S", 1)
        g.option("block_sweeps", blk)
        g.option("block8", 0)       # blk = 0: one launch per colour (the 8-half-sweep form of the kernel has its test in test_gpu_march.py)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
        g.set_const()
        assert g.param("uniform_S") == (1.0 if nl > 1 else 0.0)
        da, rr = rand_field(60, (nl, ny, nx)), rand_field(61, (nl, ny, nx))
        out = [g.relax(0, da, rr, n) for n in (2, 3, 4)]
        g.option("TOLERANCE", 1e-10)
        q = g.get(F["Q"]) + rand_field(9, (nl, ny, nx), 1e-6)
        p = np.empty_like(q)
        g.pyq2p(p, q)
        st = g.mgstats()
        for _ in range(3):
            g.step()
        res[blk] = (out, p, (st.i, st.resa, st.nrelax), g.get(F["Q"]))
    if nl > 1:
        for a, b in zip(res[1][0], res[0][0]):
            assert np.array_equal(a, b)          # same column arithmetic, same inputs
        if strict:
            assert res[1][2] == res[0][2]
            assert np.array_equal(res[1][1], res[0][1])
            assert np.array_equal(res[1][3], res[0][3])
        else:
            # product build: the two kernels that interpolate from the coarse level contract the
            # bilinear formula to FMA differently -> rounding-level differences only
            assert res[1][2][0] == res[0][2][0] and res[1][2][2] == res[0][2][2]
            assert rel(res[1][1], res[0][1]) <= 1e-11 and rel(res[1][3], res[0][3]) <= 1e-11


# ------------------------------------------------------------------ doubly periodic domain (sbc = -1)

PER = "sbc = -1\n"


@pytest.mark.parametrize("nx,ny,nl", [(32, 32, 3), (64, 32, 2), (16, 16, 6), (256, 64, 3)])
def test_periodic_strict_bit_exact(nx, ny, nl):
    """periodic(right); periodic(top) (msqg/qg.h:842-846): operators, multigrid pieces, solver
    and time steps against the oracle, strict build bit for bit."""
    o, g = make_pair(nx, ny, nl, strict=True, extra=PER)
    o.remove_mean(orc.PSI); g.remove_mean(F["PSI"])            # msqg/qg.c:65-70
    assert np.allclose(g.get(F["PSI"]), o.get(orc.PSI), rtol=0, atol=1e-18)
    psi = rand_field(1, (nl, ny, nx))
    q_g = np.empty_like(psi)
    g.pyp2q(psi, q_g)
    assert np.array_equal(q_g, o.pyp2q(psi))
    zeta = rand_field(3, (nl, ny, nx))
    for m, P, Z, D in ((o, orc.PSI, orc.ZETA, orc.DQ), (g, F["PSI"], F["ZETA"], F["DQ"])):
        m.set(P, psi); m.set(Z, zeta); m.set(D, np.zeros_like(psi))
    o.advection_pv(orc.ZETA, orc.Q, orc.PSI, orc.DQ, 1.0)
    g.op("advection", F["ZETA"], F["DQ"])
    J = g.get(F["DQ"])
    assert np.array_equal(J, o.get(orc.DQ))
    a, b = rand_field(6, (nl, ny, nx)), rand_field(7, (nl, ny, nx))
    r_o, m_o = o.residual(a, b)
    r_g, m_g = g.residual(a, b)
    assert np.array_equal(r_g, r_o) and m_g == m_o
    for lev in range(g.nlevels()):
        lx, ly = g.level_dims(lev)
        da, res = rand_field(8 + lev, (nl, ly, lx)), rand_field(20 + lev, (nl, ly, lx))
        assert np.array_equal(g.relax(lev, da, res, 2), o.relax(lev, da, res, 2)), lev
        if lev >= 1:
            assert np.array_equal(g.prolong(lev, da), o.prolong(lev, da)), lev
    # solver + time steps from a smooth state
    o, g = make_pair(nx, ny, nl, strict=True, extra=PER)
    o.remove_mean(orc.PSI)
    g.set(F["PSI"], o.get(orc.PSI))     # identical start (the mean is a sum: order differs on the GPU)
    o.set_const(); g.set_const()
    o.set_tnext(float("inf")); g.set_tnext(float("inf"))
    for k in range(4):
        o.step()
        assert g.step() == o.dt, k
    assert (g.mgstats().i, g.mgstats().resa) == (o.mgstats().i, o.mgstats().resa)
    assert np.array_equal(g.get(F["Q"]), o.get(orc.Q))
    assert np.array_equal(g.get(F["PSI"]), o.get(orc.PSI))


def test_periodic_background_flow_and_fast_build():
    nx = ny = 32; nl = 3
    extra = PER + "upg = [0.3,0.1,0.0]\nvpg = [0.0,-0.2,0.05]\n"
    o, g = make_pair(nx, ny, nl, strict=True, extra=extra)
    assert np.array_equal(g.get(F["PSIPG"]), o.get(orc.PSIPG))
    d_o = o.update()
    dq, d_g = g.update()
    assert d_g == d_o and np.array_equal(dq, o.get(orc.DQ))     # linear-Dirichlet ghosts of psipg, qg.h:1105-1114
    o, g = make_pair(nx, ny, nl, strict=False, extra=PER)
    o.set_tnext(float("inf")); g.set_tnext(float("inf"))
    for _ in range(5):
        o.step(); g.step()
    assert rel(g.get(F["Q"]), o.get(orc.Q)) <= 1e-9


def test_periodic_arakawa_identities_on_gpu():
    """sum J = sum psi J = sum zeta J = 0 (Arakawa 1966) for the HIP Jacobian on a periodic box."""
    N, nl = 64, 2
    txt = f"N = {N}\nnl = {nl}\nL0 = 1\nRom = 1\nbeta = 0\nsbc = -1\nFr = [0]\ndh = [0.5,0.5]\n"
    for strict in (True, False):
        g = QG(txt, strict=strict)
        g.set_const()
        psi, zeta = rand_field(4, (nl, N, N)), rand_field(5, (nl, N, N))
        g.set(F["PSI"], psi); g.set(F["ZETA"], zeta); g.set(F["DQ"], np.zeros_like(psi))
        g.op("advection", F["ZETA"], F["DQ"])
        J = g.get(F["DQ"])
        scale = np.abs(J).sum()
        assert abs(J.sum()) <= 1e-13 * scale
        assert abs((J * psi).sum()) <= 1e-13 * scale * np.abs(psi).max()
        assert abs((J * zeta).sum()) <= 1e-13 * scale * np.abs(zeta).max()


def test_device_noise_statistics_and_tiling_independence():
    """noise_mode = 1: counter-based N(0,1) on the device (the reference's serial rand() stream
    cannot be reproduced in parallel: parity is statistical)."""
    nx = ny = 256; nl = 3
    txt = orc.double_gyre_params(nx, nl, extra="tr_stoch = 50\namp_stoch = 2.0\n")
    fields = []
    for seed in (11, 11, 12):
        g = QG(txt)
        g.option("quiet", 1); g.option("stochastic", 1); g.option("noise_mode", 1); g.option("seed", seed)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); g.set_const()
        sig = np.full((nl, ny, nx), 0.5)
        g.set(F["SIGMA"], sig)
        g.set_tnext(float("inf"))
        g.step()
        fields.append(g.get(F["NOISE"]))
    assert np.array_equal(fields[0], fields[1]) and not np.array_equal(fields[0], fields[2])
    n = fields[0] / (2.0 * 0.5)                      # amp * sigma
    N = n.size
    assert abs(n.mean()) < 5 / np.sqrt(N) and abs(n.var() - 1) < 5 * np.sqrt(2 / N)
    assert abs(np.mean(n**3)) < 5 * np.sqrt(15 / N) and abs(np.mean(n**4) - 3) < 5 * np.sqrt(96 / N)
    # neighbours and layers uncorrelated
    for a, b in ((n[:, :, 1:], n[:, :, :-1]), (n[:, 1:], n[:, :-1]), (n[1:], n[:-1])):
        assert abs(np.mean(a * b)) < 5 / np.sqrt(a.size)
    # the same field comes out of a 2 x 2 tiling (counter = global cell index)
    from test_gpu_tiled import run_tiled, assemble
    txt_t = orc.double_gyre_params(nx, nl, extra="tr_stoch = 50\namp_stoch = 2.0\nMGLEVELS = 7\n")
    out = run_tiled(txt_t, 2, 2, orc.synthetic_psi(nl, ny, nx), nsteps=1, strict=False,
                    opts={"stochastic": 1, "noise_mode": 1, "seed": 11},
                    fn=lambda g, r: g.get(F["NOISE"]), pre=lambda g, r: g.set(F["SIGMA"], np.full((nl, ny // 2, nx // 2), 0.5)))
    got = np.concatenate([np.concatenate([out[iy * 2 + ix]["extra"] for ix in range(2)], axis=2) for iy in range(2)], axis=1)
    assert np.array_equal(got, fields[0])


@pytest.mark.parametrize("nx,ny,nl,nptr,extra", [(32, 32, 3, 2, ""), (64, 32, 2, 1, PER), (32, 32, 1, 3, "")])
def test_passive_tracers_bit_exact(nx, ny, nl, nptr, extra):
    """nptr > 0 (msqg/qg.h:574-588, 634-647): tracer tendency -J(psi, c) + c-diffusion +
    relaxation and the tracer part of advance_qg, strict build against the oracle."""
    ex = extra + f"nptr = {nptr}\nptr_r = [{','.join(['10', '0', '3.5'][:nptr])}]\nPe = [{','.join(['200', '50', '0'][:nptr])}]\n"
    o, g = make_pair(nx, ny, nl, strict=True, extra=ex)
    assert g.param("nptr") == nptr == o.param("nptr")
    c0, rel_ = rand_field(70, (nl * nptr, ny, nx), 1e-3), rand_field(71, (nl * nptr, ny, nx), 1e-3)
    o.set(orc.PTR, c0); g.set(F["PTR"], c0)
    o.set(orc.PTR_RELAX, rel_); g.set(F["PTR_RELAX"], rel_)
    d_o = o.update()
    dq, d_g = g.update()
    assert d_g == d_o and np.array_equal(dq, o.get(orc.DQ))
    assert np.array_equal(g.get(F["DPTR"]), o.get(orc.DPTR))
    o.set_tnext(float("inf")); g.set_tnext(float("inf"))
    for _ in range(4):
        o.step(); g.step()
    assert np.array_equal(g.get(F["PTR"]), o.get(orc.PTR))
    assert np.array_equal(g.get(F["Q"]), o.get(orc.Q))
    assert np.abs(g.get(F["PTR"]) - c0).max() > 0


@pytest.mark.parametrize("nl", list(range(1, 17)))
def test_every_supported_layer_count(nl):
    """nl = 1 ... MSOM_MAXNL: three RK2 steps at 256 x 128 (wide-level kernels, LDS-tiled correction, fused
    tendency + advance, one-launch coarse levels; from nl = 9 on the generic column solver, one kernel per reference loop:
    msqg/poisson_layer.h:77 sizes its column arrays by nl), strict build bit-exact against the oracle, product build
    within 1e-9."""
    nx, ny = 256, 128
    for strict in (True, False):
        o, g = make_pair(nx, ny, nl, strict=strict, TOLERANCE=1e-9)
        for _ in range(3):
            o.step(); g.step()
        if strict:
            assert np.array_equal(g.get(F["PSI"]), o.get(orc.PSI)) and np.array_equal(g.get(F["Q"]), o.get(orc.Q))
            assert g.t == o.t
        else:
            assert rel(g.get(F["PSI"]), o.get(orc.PSI)) <= 1e-9 and rel(g.get(F["Q"]), o.get(orc.Q)) <= 1e-9


def test_more_layers_than_supported_is_rejected():
    from msom_amd import MsomError
    txt = orc.double_gyre_params(32, 16).replace("nl = 16", "nl = 17")
    with pytest.raises(MsomError, match="supported range"):
        QG(txt)


@pytest.mark.parametrize("seed", range(12))
def test_randomised_configurations_strict_vs_oracle(seed):
    """differential test over random parameter combinations (layers, aspect ratio, slip, both viscosities, drag,
    variable Rossby number, background flow, topography, 3-D forcing, non-uniform Froude field): three RK2 steps,
    strict build bit-exact against the oracle"""
    rng = np.random.default_rng(1000 + seed)
    nl = int(rng.choice([1, 2, 3, 4, 6]))
    nx = int(rng.choice([32, 64, 128, 256]))
    ny = int(rng.choice([nx, max(16, nx // 2), min(256, nx * 2)]))
    extra = ""
    if rng.random() < 0.5:
        extra += f"sbc = {rng.choice([0.5, 2.0, 100.0])}\n"
    if rng.random() < 0.5:
        extra += f"Re = {rng.choice([200.0, 1500.0])}\n"
    if rng.random() < 0.3:
        extra += "Re4 = 0\n"
    if rng.random() < 0.5:
        extra += f"Eks = {rng.choice([0.001, 0.01])}\n"
    if rng.random() < 0.3:
        extra += "varRo = 1\n"
    pg = rng.random() < 0.4 and nl > 1
    if pg:
        extra += "upg = [" + ",".join(f"{v:.2f}" for v in rng.uniform(-0.3, 0.3, nl)) + "]\nvpg = [" + ",".join(f"{v:.2f}" for v in rng.uniform(-0.3, 0.3, nl)) + "]\n"
        if rng.random() < 0.5:
            extra += "flsrv = 1\n"
    o, g = make_pair(nx, ny, nl, strict=True, extra=extra, TOLERANCE=float(rng.choice([1e-3, 1e-8])))
    redo = False
    if rng.random() < 0.4:
        tp = 0.05 * rand_field(seed + 50, (1, ny, nx))
        o.set(orc.TOPO, tp); g.set(F["TOPO"], tp)
        o.option("flag_topo", 1); g.option("flag_topo", 1)
    if rng.random() < 0.4:
        qf = rand_field(seed + 60, (nl, ny, nx), 1e-6)
        o.set(orc.QFORC, qf); g.set(F["QFORC"], qf)
    if nl > 1 and rng.random() < 0.4:
        x = (np.arange(nx) + 0.5) / nx
        fr = np.stack([o.param(f"Fr_{l}") * (1 + 0.3 * np.sin(2 * np.pi * (l + 1) * x))[None, :] * np.ones((ny, 1)) for l in range(nl - 1)])
        o.set(orc.FR, fr); g.set(F["FR"], fr)
        redo = True
    if redo:
        o.set_const(); g.set_const()
    for _ in range(3):
        o.step(); g.step()
    desc = f"nl={nl} {nx}x{ny} {extra!r}"
    assert g.t == o.t, desc
    assert np.array_equal(g.get(F["PSI"]), o.get(orc.PSI)), desc
    assert np.array_equal(g.get(F["Q"]), o.get(orc.Q)), desc


@pytest.mark.parametrize("nx,nl", [(128, 1), (512, 3)])
def test_graph_replay_of_the_cycle_equals_eager_launches(nx, nl):
    """option graph: the launches of one multigrid cycle captured into a hipGraph per (nrelax, first restriction) and replayed
    (launch-bound grids only: no marching level).  Strict build: psi, q and mgstats equal the eager cycle step by step; the
    captured kernels hold pointers and coefficients by value, so an option or TOLERANCE change in between must drop the
    captured graphs (set_option -> clear_graphs) -- exercised by toggling TOLERANCE between the steps"""
    outs = []
    for graph in (0, 1):
        txt = orc.double_gyre_params(nx, nl)
        g = QG(txt, strict=True)
        g.option("quiet", 1); g.option("graph", graph)
        g.set(F["PSI"], orc.synthetic_psi(nl, nx, nx)); g.set_const(); g.set_tnext(float("inf"))
        rec = []
        for k in range(4):
            g.option("TOLERANCE", [1e-3, 1e-9, 1e-6, 1e-9][k])   # several cycles per solve, nrelax adapts: more than one captured graph
            g.step()
            st = g.mgstats()
            rec.append((g.get(F["PSI"]), g.get(F["Q"]), (st.i, st.resb, st.resa, st.nrelax)))
        outs.append(rec)
        g.close()
    for a, b in zip(*outs):
        assert a[2] == b[2]
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,nl,extra,tol", [(64, 64, 3, "", 1e-3), (256, 128, 6, "sbc = 1.5\nRe = 300\nEks = 0.001\n", 1e-3), (128, 128, 2, "sbc = -1\ntau0 = 0\n", 1e-3),
                                               (64, 64, 3, "", 1e-9), (512, 512, 3, "", 1e-3), (32, 32, 1, "", 1e-3)])
def test_speculative_tendency_pass_changes_nothing(nx, ny, nl, extra, tol, strict):
    """option async_solve (round 3): after the first multigrid cycle of a solve the tendency kernel is queued before the host has
    read max|res| and max|u| -- dt from k_step_dt on the device in the first RK stage, a spare q buffer in the second -- and run
    again the ordinary way if the solve needs more cycles (tol 1e-9: always).  Same numbers as with the option off, step by
    step, in both builds; with output times ahead (dtnext() shortens dt) and with none"""
    outs = []
    for async_solve, step_sync in ((0, 1), (1, 1), (1, 0)):     # step_sync = 0: msom_step returns with its last tendency pass still running
        txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("TOLERANCE", tol); g.option("async_solve", async_solve); g.option("step_sync", step_sync)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); g.set_const()
        rec = []
        for k in range(6):
            g.set_tnext(float("inf") if k < 3 else g.t + 0.0371)      # an output event ahead: dtnext() cuts dt to land on it
            dt = g.step()
            if step_sync == 0 and k % 2:
                g.step(); dt2 = g.step()          # steps queued back to back, nothing read in between
                g.sync()
            st = g.mgstats()
            rec.append((dt, g.t, g.get(F["Q"]), g.get(F["PSI"]), (st.i, st.resa)))
        outs.append(rec)
        g.close()
    for a, b in zip(outs[0], outs[1]):
        assert a[0] == b[0] and a[1] == b[1] and a[4] == b[4]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    # the lazily synchronised run took extra steps after the odd ones: compare the steps before the first of them, then run the
    # synchronous variant through the same sequence
    assert outs[2][0][0] == outs[0][0][0] and np.array_equal(outs[2][0][2], outs[0][0][2]) and np.array_equal(outs[2][0][3], outs[0][0][3])
    g = QG(orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra), strict=strict)
    g.option("quiet", 1); g.option("TOLERANCE", tol)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); g.set_const()
    for k in range(6):
        g.set_tnext(float("inf") if k < 3 else g.t + 0.0371)
        g.step()
        if k % 2:
            g.step(); g.step()
        assert g.t == outs[2][k][1]
        assert np.array_equal(g.get(F["Q"]), outs[2][k][2]) and np.array_equal(g.get(F["PSI"]), outs[2][k][3])
    g.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,nl", [(64, 64, 3), (256, 128, 6), (128, 256, 1), (512, 512, 2), (1024, 64, 4)])
def test_residual_pass_that_restricts_two_levels(nx, ny, nl, strict):
    """option restrict2 (default on, round 3): the pre-cycle residual pass writes the level-2 residual as well (k_residual2, res_c2) and
    the restriction chain starts one level lower.  Same sums in the same order as k_restrict: q, psi, cycle counts and residuals equal
    to the run with the option off, bit for bit in both builds; several cycles per solve (the pass runs before every cycle)"""
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    out = []
    for on in (1, 0):
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("TOLERANCE", 1e-9); g.option("restrict2", on)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); g.set_const()
        for _ in range(2):
            g.step()
        st = g.mgstats()
        out.append((g.get(F["PSI"]), g.get(F["Q"]), (st.i, st.resb, st.resa, st.nrelax)))
        g.close()
    assert out[0][2] == out[1][2] and out[0][2][0] >= 2
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("nx,ny,nl,extra", [(256, 128, 6, ""), (64, 64, 3, ""), (32, 32, 1, ""), (512, 64, 2, ""), (64, 64, 5, ""), (256, 256, 4, ""),
                                            (128, 128, 3, "sbc = -1\ntau0 = 0\n"), (64, 128, 6, "sbc = -1\ntau0 = 0\n"), (128, 128, 3, "sbc = 1.5\nRe = 300\n")])
@pytest.mark.parametrize("strict", [True, False])
def test_lean_coarse_kernel_equals_per_kernel_path(nx, ny, nl, extra, strict):
    """mg_coarse = 4 (default, round 3): k_mg_coarse_lean -- the levels of <= 32 cells a side as plain arrays in LDS, the phases spelled out
    with the expressions of the stand-alone kernels -- against one launch per half-sweep on every level (mg_coarse = 0, block8 = 0) and
    against the older one-launch form (mg_coarse = 2); uniform S (validation build: on request); walls, partial slip, doubly periodic;
    TOLERANCE 1e-8: several cycles per solve, nrelax adapts"""
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)
    out = {}
    for opt in (0, 2, 4):
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("TOLERANCE", 1e-8); g.option("uniform_S", 1)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
        g.set_const()
        g.option("mg_coarse", opt)
        if opt == 0:
            g.option("block8", 0)
        assert g.param("mg_coarse_lean") == (1.0 if opt == 4 else 0.0)
        for _ in range(2):
            g.step()
        st = g.mgstats()
        out[opt] = (g.get(F["PSI"]), g.get(F["Q"]), (st.i, st.resa, st.nrelax))
        g.close()
    for opt in (2, 4):
        if strict:
            assert np.array_equal(out[0][0], out[opt][0]) and np.array_equal(out[0][1], out[opt][1]) and out[0][2] == out[opt][2], opt
        else:
            assert rel(out[opt][0], out[0][0]) <= 1e-10 and out[0][2][0] == out[opt][2][0], opt


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nx,ny,nl,coarse", [(256, 256, 3, 4), (1024, 128, 2, 4), (128, 512, 6, 4), (512, 512, 1, 4), (256, 256, 4, 0), (2048, 64, 3, 0)])
def test_restriction_chain_in_one_launch(nx, ny, nl, coarse, strict):
    """option restrict_pyr (default on, round 3): the restrictions below the level the residual pass reaches in launches of up to five levels
    (k_restrict_pyramid: a tile of 2^n x 2^n cells and its means on n levels through LDS) against one launch per level; with the one-launch
    coarse group (mg_coarse = 4: the chain ends at 32 cells a side) and without (mg_coarse = 0: down to the coarsest level, two pyramid
    launches on the larger grids); bit for bit in both builds"""
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else ""))
    out = []
    for on in (1, 0):
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("TOLERANCE", 1e-9); g.option("restrict_pyr", on); g.option("mg_coarse", coarse)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx)); g.set_const()
        for _ in range(2):
            g.step()
        st = g.mgstats()
        out.append((g.get(F["PSI"]), g.get(F["Q"]), (st.i, st.resb, st.resa, st.nrelax)))
        g.close()
    assert out[0][2] == out[1][2]
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


# the kernel-selection options of msom_set_option and their defaults
KERNEL_OPTIONS = dict(march_rows=0, march_xcd=1, march_flip=1, march_dbg=0, march_lean=2, march_dma=2, march_visit_rows=0,
                      march_visit_pairs=2, resmax_rows=0, block_variant=0, rhs_dbg=0, lpw_dbg=0)


def test_kernel_options_belong_to_the_handle():
    """an option set on one handle reaches no other: handles created before and after it report the defaults (a distinct value per
    key, so two keys that shared one field would show); the same for the vertex model's node_march_rows"""
    from msom_amd import NodeQG
    import orn

    txt = orc.double_gyre_params(32, 3)
    a = QG(txt)
    b = QG(txt)
    for i, k in enumerate(KERNEL_OPTIONS):
        b.option(k, 10 + i)
    c = QG(txt)
    for i, (k, v) in enumerate(KERNEL_OPTIONS.items()):
        assert (a.param(k), b.param(k), c.param(k)) == (v, 10 + i, v), k
    for g in (a, b, c):
        g.close()

    par = orn.node_params(32, 2)
    a = NodeQG(par)
    b = NodeQG(par)
    b.set_option("node_march_rows", 20)
    c = NodeQG(par)
    assert (a.param("node_march_rows"), b.param("node_march_rows"), c.param("node_march_rows")) == (0, 20, 0)
    for g in (a, b, c):
        g.close()
