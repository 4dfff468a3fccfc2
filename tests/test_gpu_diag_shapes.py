"""The wavelet scale filter (msom_wavelet_filter, kernels_wavelet.hip, wavelet_setup / wavelet_apply) and the energy / PV
budgets (msom_energy_tend, msom_filter_de, pystep_de; k_advection_de / k_dissip_de / k_ekman_de) against the CPU oracle
beyond 32^2 squares: non-square grids whose pyramid ends at 2 x 1, 1 x 4 or 16 x 1 cells (a root level of several cells,
one-row levels whose bilinear stencil reads their own ghost rows, the level spacing L0 / (nx >> k) taken from x alone),
partial slip and the single-tile periodic wrap, 2 - 16 layers, a stratification S that differs from column to column
(MSOM_FR perturbed, varRo) and the large-scale flow (PSIPG field, upg / vpg).  The oracle itself is pinned on these shapes
by tests/test_oracle_wavelet_kat.py and tests/test_oracle_energy_kat.py.

strict build: np.array_equal.  product build: relative to max|reference|, starting from the constants of
test_gpu_wavelet.py / test_gpu_energy.py for the same quantity -- transform 1e-14, filter event 1e-8, steps after it 1e-7,
budgets 1e-7, filter_de / pystep_de 1e-8.  A case that exceeds its constant while its strict build is bit-exact differs by
rounding only (FMA contraction, reciprocal multiplies); it would get 4 x the deviation measured on an MI355X in BOUNDS below,
never more than 10 x the constant.  None does.  Measured (max over the compared fields) / bound:

  wavelet case          transform        filter event     two steps later
  64x32x2               1.2e-16 / 1e-14  1.2e-14 / 1e-8   6.6e-15 / 1e-7
  32x128x9-slip         2.3e-16 / 1e-14  6.7e-15 / 1e-8   5.2e-15 / 1e-7
  128x64x16-periodic    2.0e-16 / 1e-14  7.6e-15 / 1e-8   7.5e-15 / 1e-7
  16x64x5-slip          1.4e-16 / 1e-14  6.9e-15 / 1e-8   3.0e-15 / 1e-7
  256x16x3              1.2e-16 / 1e-14  5.9e-15 / 1e-8   5.7e-15 / 1e-7

  budget case           three steps      filter_de
  64x32x4-periodic      4.8e-15 / 1e-7   4.8e-15 / 1e-8
  32x64x9-slip-fr-pg    2.9e-15 / 1e-7   3.8e-15 / 1e-8
  64x64x16-varRo        4.1e-13 / 1e-7   4.1e-13 / 1e-8
  128x32x7-slip-fr-upg  9.8e-15 / 1e-7   9.8e-15 / 1e-8
  16x16x2-fr            3.6e-15 / 1e-7   3.6e-15 / 1e-8

  pystep_de 64x32x9     2.1e-13 / 1e-8
  S = (Fr / Ro)^2       0 / 1e-15 (one division, one multiplication, each correctly rounded or within an ulp)"""
import functools

import numpy as np
import pytest

import orc
from msom_amd import FIELDS as F
from msom_amd import QG
from test_gpu_tiled import assemble, run_tiled

pytestmark = pytest.mark.gpu
DE = ("DE_BF", "DE_VD", "DE_J1", "DE_J2", "DE_J3", "DE_FT", "PO_MFT")

# product-build bounds per quantity; BOUNDS[(quantity, case id)] overrides the starting constant for one case
START = {"transform": 1e-14, "event": 1e-8, "steps": 1e-7, "budget": 1e-7, "filter_de": 1e-8, "pystep_de": 1e-8}
BOUNDS = {}


def bound(quantity, case):
    b = BOUNDS.get((quantity, case), START[quantity])
    assert b <= 10 * START[quantity]
    return b


def same(a, b, strict, rtol, name=""):
    d, s = np.abs(a - b).max(), max(np.abs(b).max(), 1e-300)
    print(f"{name}: max|gpu - oracle| / max|oracle| = {d / s:.3g} (bound {'exact' if strict else rtol})")
    if strict:
        assert np.array_equal(a, b), f"{name}: max diff {d:g}"
    else:
        assert d <= rtol * s, f"{name}: {d / s:g} > {rtol:g}"


def params(nx, ny, nl, extra):
    return orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)


# On 16 x 64 with afilt = 4 (Delta_0 = 5, sig_filt = 4 Rd in [2, 12]) level 1 has a coefficient other than 0 only where four
# neighbouring cells all have Rd > 2.5; with this seed two cells of level 1 do, so that a second level is mixed there as well
RD_SEED = 18


def random_rd(nx, ny):
    return 0.5 + 2.5 * np.random.default_rng(RD_SEED).random((1, ny, nx))


def perturbed(fr, seed):
    """every column its own Fr (hence S), all positive"""
    return fr * (1 + 0.3 * np.random.default_rng(seed).random(fr.shape))


# ------------------------------------------------------------------ wavelet filter
# id: (nx, ny, nl, extra, afilt, levels, root (nx, ny))
WAVELET = {
    "64x32x2": (64, 32, 2, "", 3, 6, (2, 1)),
    "32x128x9-slip": (32, 128, 9, "sbc = 0.5\n", 7, 6, (1, 4)),
    "128x64x16-periodic": (128, 64, 16, "sbc = -1\ntau0 = 0\n", 3, 7, (2, 1)),
    "16x64x5-slip": (16, 64, 5, "sbc = 1.5\n", 4, 5, (1, 4)),
    "256x16x3": (256, 16, 3, "", 1, 5, (16, 1)),
}
WV_TOL = 1e-11


def wavelet_oracle(case, psi):
    nx, ny, nl, extra, afilt, K, root = WAVELET[case]
    txt = params(nx, ny, nl, extra + f"afilt = {afilt}\n")
    o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1, TOLERANCE=WV_TOL)
    o.set(orc.RD, random_rd(nx, ny))
    o.set(orc.PSI, psi)
    o.set_const()
    return txt, o


def wavelet_gpu(case, txt, psi, strict):
    nx, ny = WAVELET[case][:2]
    g = QG(txt, strict=strict)
    g.option("quiet", 1); g.option("TOLERANCE", WV_TOL)
    g.set(F["RD"], random_rd(nx, ny))
    g.set(F["PSI"], psi)
    g.set_const()
    return g


@functools.lru_cache(maxsize=None)
def transform_reference(case):
    nx, ny, nl, extra, afilt, K, root = WAVELET[case]
    psi = np.random.default_rng(nx).standard_normal((nl, ny, nx))
    txt, o = wavelet_oracle(case, psi)
    levels = o.wavelet_levels()
    sig = [o.siglev(k) for k in range(levels)]
    o.wavelet_apply(orc.PSI)
    return txt, psi, levels, sig, o.get(orc.PSI)


@functools.lru_cache(maxsize=None)
def event_reference(case, dtflt):
    nx, ny, nl = WAVELET[case][:3]
    psi = orc.synthetic_psi(nl, ny, nx)
    txt, o = wavelet_oracle(case, psi)
    o.wavelet_filter(dtflt)
    event = {k: o.get(getattr(orc, k)) for k in ("PSI", "Q", "QOF", "TMP")}
    for _ in range(2):
        o.step()
    return txt, psi, event, o.get(orc.Q)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", list(WAVELET))
def test_siglev_and_transform(case, strict):
    nx, ny, nl, extra, afilt, K, root = WAVELET[case]
    txt, psi, levels, sig, ref = transform_reference(case)
    g = wavelet_gpu(case, txt, psi, strict)
    assert g.wavelet_levels() == levels == K
    assert sig[K - 1].shape == (1, root[1], root[0])
    # neither all-pass nor all-stop: at least two levels with coefficients strictly between 0 and 1 in the mean
    means = [float(s.mean()) for s in sig]
    assert sum(0 < m < 1 for m in means) >= 2, means
    for k in range(K):                                   # host arithmetic: equal in both builds
        assert np.array_equal(g.siglev(k), sig[k]), k
    g.wavelet_apply(F["PSI"])
    assert np.abs(ref - psi).max() > 1e-3 * np.abs(psi).max()
    same(g.get(F["PSI"]), ref, strict, bound("transform", case), "transform " + case)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("dtflt", [0.5, -0.5])
@pytest.mark.parametrize("case", list(WAVELET))
def test_wavelet_filter(case, dtflt, strict):
    txt, psi, event, q2 = event_reference(case, dtflt)
    g = wavelet_gpu(case, txt, psi, strict)
    q0g = g.get(F["Q"])
    g.wavelet_filter(dtflt)
    assert np.abs(event["QOF"]).max() > 0 and np.abs(event["PSI"] - psi).max() > 0
    for k, ref in event.items():
        same(g.get(F[k]), ref, strict, bound("event", case), f"{k} after the event, {case}")
    if dtflt < 0:
        assert np.array_equal(g.get(F["Q"]), q0g)
    else:
        assert np.abs(g.get(F["Q"]) - q0g).max() > 0
    # the model keeps running on the filtered state
    for _ in range(2):
        g.step()
    assert all(np.isfinite(v).all() for v in (q2, g.get(F["Q"])))
    same(g.get(F["Q"]), q2, strict, bound("steps", case), "q two steps later, " + case)


# ------------------------------------------------------------------ energy / PV budgets
# id: (nx, ny, nl, extra, perturbed FR, PSIPG field, background flow (DE_J2 != 0))
BUDGET = {
    "64x32x4-periodic": (64, 32, 4, "sbc = -1\ntau0 = 0\nediag = 0\nRe = 500\n", False, False, False),
    "32x64x9-slip-fr-pg": (32, 64, 9, "sbc = 0.5\nediag = 1\nRe = 800\nEks = 0.003\nflsrv = 1\n", True, True, True),
    "64x64x16-varRo": (64, 64, 16, "varRo = 1\nediag = 0\nEks = 0.001\n", False, False, False),
    "128x32x7-slip-fr-upg": (128, 32, 7, "sbc = 1.5\nediag = 0\nflsrv = 1\nupg = [0.3,0.1,0,0,0,0,0]\nvpg = [0,-0.2,0.05,0,0,0,0]\n", True, False, True),
    "16x16x2-fr": (16, 16, 2, "ediag = 1\n", True, False, False),
}
DE_TOL = 1e-9
DE_EXTRA = "afilt = 4\ndtflt = 0.25\n"


def budget_setup(m, fid, case, fr0=None):
    """the same inputs on either side: m = Oracle or QG, fid(name) = its field id; returns the Fr field the handle held"""
    nx, ny, nl, extra, fr, pg, flow = BUDGET[case]
    psi = orc.synthetic_psi(nl, ny, nx)
    m.option("quiet", 1); m.option("TOLERANCE", DE_TOL)
    held = m.get(fid("FR"))
    if fr:
        m.set(fid("FR"), perturbed(held if fr0 is None else fr0, nx + nl))
    if pg:
        m.set(fid("PSIPG"), 0.3 * psi[::-1].copy())
    m.set(fid("RD"), random_rd(nx, ny))
    m.set(fid("PSI"), psi)
    m.set_const()
    return held


def budget_run(m, fid, dts=None):
    """the loop of test_energy_tend_through_time_steps (event comp_diag with the oracle's step size, then the step), the
    seven fields; filter_de, the seven fields again; reset_de.  dts = None: the oracle, which records its step sizes"""
    cycles, used = [], []
    for it in range(3):
        used.append(m.dt if dts is None else dts[it])
        m.energy_tend(used[-1])
        m.step()
        cycles.append(m.mgstats().i)
    before = {k: m.get(fid(k)) for k in DE}
    q0 = m.get(fid("Q"))
    m.filter_de(fid("PO_MFT"), 0.25)
    cycles.append(m.mgstats().i)
    after = {k: m.get(fid(k)) for k in DE}
    q1 = m.get(fid("Q"))
    m.reset_de()
    return used, cycles, before, after, q0, q1, {k: m.get(fid(k)) for k in DE}


@functools.lru_cache(maxsize=None)
def budget_reference(case):
    nx, ny, nl, extra = BUDGET[case][:4]
    txt = params(nx, ny, nl, extra + DE_EXTRA)
    o = orc.Oracle(txt, smoother=orc.GS_RB)
    fr0 = budget_setup(o, lambda k: getattr(orc, k), case)
    S = o.get(orc.S)
    return txt, fr0, S, budget_run(o, lambda k: getattr(orc, k))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", list(BUDGET))
def test_energy_budgets(case, strict):
    nx, ny, nl, extra, fr, pg, flow = BUDGET[case]
    txt, fr0, S, (dts, cycles, before, after, q0, q1, cleared) = budget_reference(case)
    # what the oracle did is worth comparing with: every solve converged, nothing overflowed, no array is trivially zero
    assert max(cycles) <= 5, cycles
    assert all(np.isfinite(v).all() for v in list(before.values()) + list(after.values()))
    for k in ("DE_BF", "DE_VD", "DE_J1", "DE_J3"):
        assert np.abs(before[k]).max() > 0, k
    assert (np.abs(before["DE_J2"]).max() > 0) == flow
    assert np.all(before["DE_FT"] == 0) and np.abs(after["DE_FT"]).max() > 0
    assert np.abs(before["PO_MFT"]).max() > 0 and np.all(after["PO_MFT"] == 0)
    g = QG(txt, strict=strict)
    held = budget_setup(g, lambda k: F[k], case, fr0=fr0)
    assert np.array_equal(held, fr0)
    if fr or "varRo" in extra:                              # the general-S path, S of the thread's own column
        assert g.param("uniform_S") == 0
        assert np.ptp(S, axis=2).min() > 0 if fr else np.ptp(S, axis=1).min() > 0
    if strict:
        assert np.array_equal(g.get(F["S"]), S)
    else:
        same(g.get(F["S"]), S, strict, 1e-15, "S " + case)   # one division, one multiplication
    _, gcycles, gb, ga, gq0, gq1, gc = budget_run(g, lambda k: F[k], dts)
    assert max(gcycles) <= 5, gcycles
    for k in DE:
        same(gb[k], before[k], strict, bound("budget", case), f"{k} after three steps, {case}")
    for k in DE:
        same(ga[k], after[k], strict, bound("filter_de", case), f"{k} after filter_de, {case}")
    assert np.array_equal(gq0, gq1) and np.array_equal(q0, q1)      # filter_de restores q
    assert all(np.all(gc[k] == 0) and np.all(cleared[k] == 0) for k in DE[:6])
    same(gc["PO_MFT"], cleared["PO_MFT"], strict, bound("filter_de", case), "PO_MFT after reset_de, " + case)


@functools.lru_cache(maxsize=None)
def pystep_reference():
    nx, ny, nl = 64, 32, 9
    txt = params(nx, ny, nl, "afilt = 4\ndtflt = 0.25\nRe = 800\n")
    o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1, TOLERANCE=WV_TOL)
    fr0 = o.get(orc.FR)
    o.set(orc.FR, perturbed(fr0, 5))
    o.set(orc.PSI, orc.synthetic_psi(nl, ny, nx))
    o.set_const()
    S = o.get(orc.S)
    psi = 1.3 * orc.synthetic_psi(nl, ny, nx)
    full = o.pystep_de(psi, 0)
    ke = o.pystep_de(psi, 1)
    assert np.all(o.get(orc.S) == 0) and np.all(o.get(orc.PSI) == 0)
    o.set_const()
    return txt, fr0, S, psi, full, ke, o.get(orc.S)


@pytest.mark.parametrize("strict", [True, False])
def test_pystep_de(strict):
    """64 x 32 x 9 with a per-column S: onlyKE = 0, then onlyKE = 1 (S = 0 until the next set_const) on the same handle"""
    nx, ny, nl = 64, 32, 9
    txt, fr0, S, psi, full, ke, S_restored = pystep_reference()
    assert np.array_equal(S, S_restored) and S.min() > 0 and np.ptp(S, axis=2).min() > 0
    assert np.all(full[3] == 0) and all(np.abs(full[k]).max() > 0 for k in (0, 1, 2, 4, 5))
    assert np.abs(full[2] - ke[2]).max() > 0               # the stretching part of DE_J1 is gone with S = 0
    g = QG(txt, strict=strict)
    g.option("quiet", 1); g.option("TOLERANCE", WV_TOL)
    assert np.array_equal(g.get(F["FR"]), fr0)
    g.set(F["FR"], perturbed(fr0, 5))
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    assert g.param("uniform_S") == 0
    for onlyKE, ref in ((0, full), (1, ke)):
        outs = [np.empty((nl, ny, nx)) for _ in range(6)]
        g.pystep_de(psi, *outs, onlyKE)
        for name, a, b in zip(DE, outs, ref):
            same(a, b, strict, bound("pystep_de", "64x32x9"), f"{name} onlyKE = {onlyKE}")
        assert np.all(g.get(F["PSI"]) == 0)
    assert np.all(g.get(F["S"]) == 0)
    g.set_const()                                          # restores the per-column S = (Fr / Ro)^2
    if strict:
        assert np.array_equal(g.get(F["S"]), S_restored)
    else:
        same(g.get(F["S"]), S_restored, strict, 1e-15, "S restored")


# ------------------------------------------------------------------ tiles
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("sbc", ["", "sbc = -1\ntau0 = 0\n"], ids=["walls", "periodic"])
def test_filter_and_budgets_on_non_square_tiles(sbc, strict):
    """2 x 2 tiles of 32 x 16 (global 64 x 32 x 3, MGLEVELS = 4): the tile's own pyramid ends at 2 x 1, the gathered top
    grid goes 4 x 2 -> 2 x 1 on the host (WvTop with a one-row level).  Filter event and budget run equal to the single
    tile bit for bit; strict build: the single tile equal to the oracle on the same number of multigrid levels."""
    px = py = 2
    tx, ty, nl = 32, 16, 3
    gnx, gny = tx * px, ty * py
    txt = params(gnx, gny, nl, "MGLEVELS = 4\nediag = 0\nafilt = 4\ndtflt = 0.25\n" + sbc)
    psi = orc.synthetic_psi(nl, gny, gnx)
    Rd = random_rd(gnx, gny)
    opts = {"TOLERANCE": 1e-10}

    def pre(g, rank):
        ix, iy = rank % px, rank // px
        g.set(F["RD"], Rd[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx])
        g.set_const()

    def event(m, fid):
        m.wavelet_filter(0.5)
        res = [m.get(fid("PSI")), m.get(fid("Q")), m.get(fid("QOF"))]
        m.step()
        return res + [m.get(fid("Q"))]

    def budgets(m, fid):
        for _ in range(3):
            m.energy_tend(0.02)
            m.step()
        res = [m.get(fid(k)) for k in DE]
        m.filter_de(fid("PO_MFT"), 0.25)
        return res + [m.get(fid(k)) for k in DE]

    def single(run):
        g = QG(txt, strict=strict)
        g.option("quiet", 1); g.option("TOLERANCE", 1e-10)
        g.set(F["RD"], Rd); g.set(F["PSI"], psi)
        g.set_const()
        g.set_tnext(float("inf"))
        assert g.nlevels() == 4
        if run is event:
            assert g.wavelet_levels() == 6 and g.siglev(5).shape == (1, 1, 2)
        return run(g, lambda k: F[k])

    def oracle(run):
        o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1, TOLERANCE=1e-10)
        o.set(orc.RD, Rd); o.set(orc.PSI, psi)
        o.set_const()
        assert o.nlevels() == 4 and o.wavelet_levels() == 6
        return run(o, lambda k: getattr(orc, k))

    for run in (event, budgets):
        out = run_tiled(txt, px, py, psi, nsteps=0, strict=strict, opts=opts, pre=pre, fn=lambda g, rank: run(g, lambda k: F[k]))
        ref = single(run)
        assert len(ref) == len(out[0]["extra"])
        for k, r in enumerate(ref):
            got = assemble([{"v": t["extra"][k]} for t in out], "v", px, py)
            assert np.array_equal(got, r), (run.__name__, k, np.abs(got - r).max())
        assert all(np.abs(r).max() > 0 for k, r in enumerate(ref) if not (run is budgets and k in (3, 5, 7 + 3, 7 + 6)))   # DE_J2, DE_FT before, DE_J2, PO_MFT after
        if strict:
            for k, (r, orf) in enumerate(zip(ref, oracle(run))):
                assert np.array_equal(r, orf), (run.__name__, k, np.abs(r - orf).max())
