"""The vertical-mode eigen solver on the device (k_modes_eig through msom_modes_compute / _get) on the stratifications where an eigen
solver goes wrong, which the +-30 % table of tests/test_gpu_modes.py keeps out by construction: graded stratification, a nearly
unstratified interface (near-degenerate pairs, relative gaps down to 4e-11), thin layers (modes that all but vanish at the surface), and
the columns msom_modes_compute must refuse (MODES_WEAK).  tools/modes_host_check.cpp runs the same columns through the host build.

Handles: 64 x 32, nl = 2, 3, 6, 8 (vector matrix in registers), 9, 16 (in LDS), strict and product build, set_const and modes_compute
only.  S0 = 5000, t = i / 63 along x, thickness sets "eq" (1 / nl each) and "thin" (geometric, bottom = 1e3 * top, sum 1):
  eq handle:   rows 0 .. 15 graded S_l = S0 10^(-8 t l / max(nl - 2, 1)); rows 16 .. 31 weak middle S_mid = S0 10^(-8 t), mid = (nl - 1) // 2;
               before MSOM_FR is set, the untouched uniform column (compact form), held to its closed form as well
  thin handle: weak middle in every row
The reference side is built from the S and dh_l read back from the handle.  Every column must have a longdouble reference
lambda_1 >= 16 * 8 nl eps lambda_max (asserted; none skipped), every refused column lambda_1 <= 8 nl eps lambda_max / 16.

Criteria per column, none of which needs a gap (T = D^1/2 A D^-1/2 in numpy.longdouble, modes_ref.hard_criteria), eps = 2^-52:
 (a) all finite; iBu_0 == 0, iBu[1:] < 0, iBu non-increasing (a computed tie in a near-degenerate pair is legitimate),
     Rd[1:] == sqrt(-1 / iBu[1:])
 (b) Sturm counts: #{eig T < lam_m - tol} <= m and #{eig T < lam_m + tol} >= m + 1 for lam_m = -iBu_m, tol = 8 nl eps lambda_max
 (c) |T y_m - lam_m y_m|_2 <= 8 nl eps |T|_F |y_m|_2 with y_m = D^1/2 M2L[:, m] (lam_0 = 0)
 (d) |M2L^T D M2L - I| <= 8 nl eps
 (e) M2L[0][m] >= 0
 (f) L2M == dh[k] * M2L[k][m], bit for bit in the strict build, within TOL_PRODUCT in the product build
and where the reference gap is >= 1e-4 and the surface ratio >= 1e-6 (the low-t end) the vector bound of test_gpu_modes part 1,
4 nl eps / gap * max|ref|, against modes_ref.modes_eigh.

Negative controls, run once.  (1) The library built with the MODES_WEAK rule alone reverted, on the refused columns on the MI355X: every
msom_modes_compute returns 0, so every case of test_too_weak_an_interface_is_refused fails; nl = 9 thin comes back with
iBu_1 = +4.19e-11 (strict) / +4.55e-11 (product) > 0 and Rd_1 = NaN in all 2048 cells, the others with an iBu_1 of -6e-13 ... -2e-8 that
is rounding noise (reference lambda_1: 1e-17 ... 1e-24 of lambda_max).  The host build of the issue's column, nl = 6,
dh = [0.05, 0.08, 0.12, 0.2, 0.25, 0.3], S = [1e4, 1e4, 1e-14, 1e4, 1e4], gives lambda = -1.10e-10, -2.47e-11, 1.59e5, ...
(2) tools/modes_host_check.cpp on a scratch copy of modes_inl.h with one rotation of ModesMemV::rotate scaled by 1 + 1e-9: (c) and (d)
fail for nl = 9 and 16 (residual 2.6e3 .. 2.8e4, orthonormality 1.2e5 .. 7.3e5 times the bound) and for no nl <= 8.

First measured on MI355X, worst ratio over its bound ("a / b": strict / product where they differ); easy columns: those of the 2048
with reference gap >= 1e-4 and surface ratio >= 1e-6; surface ratio: smallest min_m |vr[0][m]| / max|vr| of a column:
  nl set   eigenvalue (b)  residual (c)   orthonorm. (d)  surface ratio  easy columns  vectors there   closed form: eigenvalue, vector
   2 eq    0.000           0.016          0.031           1.00e+00        2048         0.063           0.000          0.063
   2 thin  0.070           0.070          0.116 / 0.022   3.16e-02        2048         0.012 / 0.125
   3 eq    0.061           0.081          0.064 / 0.052   5.00e-01         992         0.052 / 0.046   0.043          0.025
   3 thin  0.045           0.045          0.076 / 0.065   3.16e-02         256         0.002
   6 eq    0.042 / 0.044   0.043          0.039 / 0.043   2.02e-01         864         0.162           0.038          0.011 / 0.009
   6 thin  0.030           0.030          0.036           1.21e-08           0         -
   8 eq    0.028 / 0.029   0.039 / 0.031  0.035 / 0.036   1.50e-01         800         0.076 / 0.071   0.008          0.007 / 0.005
   8 thin  0.013           0.024          0.031 / 0.034   4.67e-09           0         -
   9 eq    0.027           0.028          0.042 / 0.050   1.21e-09         848         0.017           0.008 / 0.017  0.008 / 0.004
   9 thin  0.012           0.018          0.032 / 0.029   2.73e-09           0         -
  16 eq    0.014 / 0.013   0.022          0.027 / 0.029   8.03e-02         624         0.051 / 0.046   0.010 / 0.009  0.005 / 0.003
  16 thin  0.011           0.020 / 0.015  0.020 / 0.019   1.74e-09           0         -
No computed ties.  Reference lambda_1 over the threshold 8 nl eps lambda_max: >= 117 (nl = 16), 255 (9), 870 (8), 2.3e3 (6), 1.8e3 (3),
2.8e14 (2) on the columns that must succeed; <= 1.4e-3 (nl = 3, eq) on the refused ones."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import modes_ref as R
import orc
from msom_amd import FIELDS as F
from msom_amd import MODES as MD
from msom_amd import QG, workloads
from test_gpu_bfn import TOL_PRODUCT
from test_gpu_modes import MSOM_ERR_CONFIG, MSOM_ERR_STATE, params
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

EPS = R.EPS
NX, NY = 64, 32
T = np.arange(NX) / (NX - 1.0)
ROM = float(re.search(r"^Rom\s*=\s*(\S+)", workloads.DOUBLE_GYRE, re.M).group(1))
NLS = (2, 3, 6, 8, 9, 16)
REFUSED_NLS = (3, 6, 9, 16)
WEAK = {"eq": 1e-17, "thin": 1e-20}          # S_mid / S0 of the columns that must be refused

BOTH = pytest.mark.parametrize("strict", [True, False], ids=["strict", "product"])
SETS = pytest.mark.parametrize("dhset", ["eq", "thin"])
ALL_NL = pytest.mark.parametrize("nl", NLS)


def thickness(dhset, nl):
    return R.dh_eq(nl) if dhset == "eq" else R.dh_thin(nl)


def hard_params(nl, dhset, S):
    """the double gyre with its Fr and dh tables overridden by later lines (the parser keeps the last one; a line holds < 300 characters).
    Equal layers are written to round-trip, so that dh is 1 / nl rounded once and the closed form applies"""
    dh = thickness(dhset, nl)
    dh_txt = ",".join(repr(float(v)) if dhset == "eq" else f"{v:.10g}" for v in dh)
    fr_txt = ",".join(f"{ROM * np.sqrt(s):.10g}" for s in S)
    lines = f"Fr = [{fr_txt}]\ndh = [{dh_txt}]\n"
    assert max(len(l) for l in lines.split("\n")) < 290
    return params(NX, NY, nl, lines)


def fr_field(S_cols, rows=NY):
    """MSOM_FR [nl - 1][rows][nx] that makes S = (FR / Ro)^2 the columns S_cols [nl - 1][nx] in every row"""
    return np.repeat((ROM * np.sqrt(S_cols))[:, None, :], rows, axis=1)


def family_fr(nl, dhset):
    if dhset == "thin":
        return fr_field(R.hard_S("weak", nl, T))
    return np.concatenate([fr_field(R.hard_S("graded", nl, T), NY // 2), fr_field(R.hard_S("weak", nl, T), NY - NY // 2)], axis=1)


def handle(nl, dhset, S_uniform, strict):
    g = QG(hard_params(nl, dhset, S_uniform), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(nl, NY, NX))
    g.set_const()
    g.set_tnext(float("inf"))
    return g


class Fetched:
    """one decomposition fetched from a handle, with the criteria of its columns"""

    def __init__(self, g, nl, one_column=False):
        a = [g.modes_get(MD[n]) for n in ("IBU", "RD", "M2L", "L2M")] + [g.get(F["S"])[:nl - 1]]
        if one_column:                                       # the compact form: every cell holds the same numbers
            assert all(np.all(x == x[:, :1, :1]) for x in a)
            a = [x[:, :1, :1] for x in a]
        self.ibu, self.rd, self.m2l, self.l2m, self.S = a
        self.dh = np.array([g.param(f"dh_{l}") for l in range(nl)])
        self.crit = R.hard_criteria(self.S, self.dh, self.ibu, self.m2l)


class Hard:
    def __init__(self, nl, dhset, strict):
        self.nl, self.dhset, self.strict = nl, dhset, strict
        self.g = g = handle(nl, dhset, np.full(nl - 1, R.S0), strict)
        self.uniform = None
        if dhset == "eq":                                    # the untouched uniform column: one eigenproblem, compact form
            assert g.param("modes_compact") == 1
            assert g.L.msom_modes_compute(g.h) == 0
            self.uniform = Fetched(g, nl, one_column=True)
        g.set(F["FR"], family_fr(nl, dhset))
        g.set_const()
        self.status = g.L.msom_modes_compute(g.h)
        self.ready, self.compact = g.param("modes_ready"), g.param("modes_compact")
        self.f = Fetched(g, nl) if self.status == 0 else None
        self.tag = f"nl = {nl} {dhset} {'strict' if strict else 'product'}"


@functools.lru_cache(maxsize=None)
def hard(nl, dhset, strict):
    return Hard(nl, dhset, strict)


def decompositions(h):
    return [("families", h.f)] + ([("uniform", h.uniform)] if h.uniform is not None else [])


# ------------------------------------------------------------------ the columns that must succeed

@BOTH
@SETS
@ALL_NL
def test_every_column_is_a_fair_case_and_is_accepted(nl, dhset, strict):
    h = hard(nl, dhset, strict)
    assert h.status == 0 and h.ready == 1 and h.compact == 0
    for name, f in decompositions(h):
        ratio = f.crit["lam1"] / f.crit["thr"]
        print(f"{h.tag} {name}: reference lambda_1 / (8 nl eps lambda_max) >= {float(ratio.min()):.3g}")
        assert np.all(ratio >= 16) and ratio.shape == ((NY, NX) if name == "families" else (1, 1))      # every column, none skipped


@BOTH
@SETS
@ALL_NL
def test_signs_order_and_left_vectors(nl, dhset, strict):
    """(a), (e), (f)"""
    h = hard(nl, dhset, strict)
    for name, f in decompositions(h):
        for x in (f.ibu, f.rd, f.m2l, f.l2m):
            assert np.all(np.isfinite(x)), name
        assert np.all(f.ibu[0] == 0) and np.all(f.ibu[1:] < 0) and np.all(np.diff(f.ibu, axis=0) <= 0), name
        assert np.all(f.rd[0] == 0) and np.array_equal(f.rd[1:], np.sqrt(-1.0 / f.ibu[1:])), name
        assert np.all(f.m2l[:nl] >= 0), name
        M = f.m2l.reshape((nl, nl) + f.ibu.shape[1:])        # [k][m]
        L = f.l2m.reshape((nl, nl) + f.ibu.shape[1:])        # [m][k]
        want = f.dh[None, :, None, None] * np.swapaxes(M, 0, 1)
        if strict:
            assert np.array_equal(L, want), name
        else:
            assert rel(L, want) <= TOL_PRODUCT, name
        print(f"{h.tag} {name}: ties among the eigenvalues {int(np.sum(np.diff(f.ibu[1:], axis=0) == 0))}, smallest surface entry over the "
              f"largest entry {R.surface_ratio(f.m2l, nl).min():.2e}")


@BOTH
@SETS
@ALL_NL
def test_eigenvalues_by_sturm_counts(nl, dhset, strict):
    """(b)"""
    h = hard(nl, dhset, strict)
    for name, f in decompositions(h):
        print(f"{h.tag} {name}: worst |lambda - reference| over 8 nl eps lambda_max: {float(f.crit['lam_err'].max()):.3f}")
        assert np.all(f.crit["sturm_ok"]), name


@BOTH
@SETS
@ALL_NL
def test_residual_and_orthonormality(nl, dhset, strict):
    """(c), (d)"""
    h = hard(nl, dhset, strict)
    for name, f in decompositions(h):
        print(f"{h.tag} {name}: worst over its bound (8 nl eps): residual {float(f.crit['res'].max()):.3f}, M2L^T D M2L - I {float(f.crit['orth'].max()):.3f}")
        assert f.crit["res"].max() <= 1, name
        assert f.crit["orth"].max() <= 1, name


@BOTH
@SETS
@ALL_NL
def test_vectors_where_the_gap_allows(nl, dhset, strict):
    """the sub-columns part 1 of test_gpu_modes would accept, at its bound"""
    h = hard(nl, dhset, strict)
    f = h.f
    ibu, m2l, l2m, lam = R.modes_eigh(f.S, f.dh)
    gap = R.rel_gap(lam)
    ok = (gap >= 1e-4) & (R.surface_ratio(m2l, nl) >= 1e-6)
    if dhset == "eq":
        assert np.all(ok[:, 0])                              # t = 0 is the uniform column
    worst = 0.0
    for got, want in ((f.m2l, m2l), (f.l2m, l2m)):
        r = np.abs(got - want).max(axis=0) / (4 * nl * EPS / gap * np.abs(want).max(axis=0))
        worst = max(worst, r[ok].max()) if ok.any() else worst
        assert np.all(r[ok] <= 1)
    print(f"{h.tag}: {int(ok.sum())} of {ok.size} columns with gap >= 1e-4 and surface ratio >= 1e-6; worst vector error over 4 nl eps / gap: {worst:.3f}")


@BOTH
@ALL_NL
def test_uniform_column_against_the_closed_form(nl, strict):
    """equal layers, the same S everywhere: lambda_m = 4 S nl^2 sin^2(m pi / (2 nl)), vr[k][m] = sqrt(2) cos((k + 1/2) m pi / nl)"""
    h = hard(nl, "eq", strict)
    f = h.uniform
    assert np.all(f.S == f.S[0, 0, 0]) and np.array_equal(f.dh, np.full(nl, 1.0 / nl))
    lam, vr = R.uniform_closed_form(f.S[0, 0, 0], nl)
    gap = np.diff(lam).min() / lam[-1]
    e_l = np.abs(-f.ibu[:, 0, 0].astype(R.LD) - lam).max() / (8 * nl * EPS * lam[-1])
    e_v = np.abs(f.m2l[:, 0, 0].reshape(nl, nl).astype(R.LD) - vr).max() / (4 * nl * EPS / gap * np.abs(vr).max())
    print(f"{h.tag}: closed form, worst over its bound: eigenvalue {float(e_l):.3f}, vector {float(e_v):.3f}")
    assert e_l <= 1 and e_v <= 1


# ------------------------------------------------------------------ the columns that must be refused

def refused_everywhere(g, nl):
    """every msom_modes_* getter answers MSOM_ERR_STATE and leaves its arguments alone; no modes held"""
    L, h = g.L, g.h
    big, x = np.full((nl * nl, NY, NX), 7.0), np.full((nl, NY, NX), 7.0)
    e = (C.c_double * nl)(*([7.0] * nl))
    for which in range(MD["N"]):
        assert L.msom_modes_layers(h, which) == MSOM_ERR_STATE
        assert L.msom_modes_get(h, which, big.ctypes.data) == MSOM_ERR_STATE
    assert L.msom_modes_project(h, 1, x.ctypes.data, x.ctypes.data) == MSOM_ERR_STATE
    assert L.msom_modes_energy(h, e, e) == MSOM_ERR_STATE
    assert L.msom_modes_set_rd(h, 1) == MSOM_ERR_STATE
    assert np.all(big == 7.0) and np.all(x == 7.0) and list(e) == [7.0] * nl
    assert g.param("modes_ready") == 0 and g.param("modes_bytes") == 0


def lam1_over_threshold(g, nl):
    dh = np.array([g.param(f"dh_{l}") for l in range(nl)])
    a, b = R.sym_tridiag(g.get(F["S"])[:nl - 1], dh)
    return R.eig_bisect(a, b, 1) / (8 * nl * R.LD(EPS) * R.eig_bisect(a, b, nl - 1))


@BOTH
@SETS
@pytest.mark.parametrize("nl", REFUSED_NLS)
def test_too_weak_an_interface_is_refused(nl, dhset, strict):
    """S_mid = 1e-17 S0 (eq) / 1e-20 S0 (thin): uniform over the grid (the compact one-column path), the same with modes_compact = 0, and
    a sound field with the weak column at the last cell only (any thread's flag reaches the host); then a sound field computes again"""
    S_weak = R.hard_S("weak", nl, T[:1], weak=WEAK[dhset])[:, 0]
    g = handle(nl, dhset, S_weak, strict)
    L, h = g.L, g.h

    def refused(where):
        assert L.msom_modes_compute(h) == MSOM_ERR_CONFIG, where
        msg = L.msom_last_error()
        assert b"weakly stratified" in msg and b"first baroclinic" in msg, (where, msg)
        refused_everywhere(g, nl)

    ratio = lam1_over_threshold(g, nl)
    print(f"nl = {nl} {dhset}: reference lambda_1 / (8 nl eps lambda_max) of the refused column {float(ratio.max()):.3g}")
    assert np.all(ratio <= 1 / 16)
    assert g.param("modes_compact") == 1
    refused("compact")
    g.option("modes_compact", 0)
    assert g.param("modes_compact") == 0
    refused("per column")
    S = np.repeat(np.full(nl - 1, R.S0)[:, None], NX, axis=1)
    fr = fr_field(S)
    fr[:, NY - 1, NX - 1] = ROM * np.sqrt(S_weak)
    g.set(F["FR"], fr)
    g.set_const()
    ratio = lam1_over_threshold(g, nl)
    assert ratio[NY - 1, NX - 1] <= 1 / 16 and np.sum(ratio >= 16) == NX * NY - 1
    refused("last cell")
    g.set(F["FR"], fr_field(S))
    g.set_const()
    assert L.msom_modes_compute(h) == 0                       # a sound stratification computes again
    assert g.param("modes_ready") == 1 and g.param("modes_bytes") == (nl * nl + nl) * 8 * NY * NX
    ibu = g.modes_get(MD["IBU"])
    assert np.all(ibu[0] == 0) and np.all(ibu[1:] < 0)
    g.close()


# ------------------------------------------------------------------ downstream of a success

@BOTH
def test_rd_of_a_hard_column_feeds_the_wavelet_filter(strict):
    h = hard(6, "thin", strict)
    h.g.modes_set_rd(1)
    rd = h.g.get(F["RD"])
    assert np.all(np.isfinite(rd)) and np.all(rd > 0)
    assert np.array_equal(rd[0], h.f.rd[1])
