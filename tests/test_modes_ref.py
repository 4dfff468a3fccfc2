"""Known answer of the vertical-mode recipe of tests/modes_ref.py (both routes) for two layers:

    lambda = {0, S / dhc * (1 / dh0 + 1 / dh1)},   m2l[:, 0] = [1, 1],   m2l[:, 1] = [sqrt(dh1 / dh0), -sqrt(dh0 / dh1)]

(Flierl's normalisation with htotal = 1 = dh0 + dh1, positive at the surface) and l2m @ m2l = I.  No GPU."""
import numpy as np
import pytest

import modes_ref as R


@pytest.mark.parametrize("route", [R.modes_dgeev, R.modes_eigh])
@pytest.mark.parametrize("dh0", [0.2, 0.5, 0.06])
def test_two_layer_known_answer(route, dh0):
    dh = np.array([dh0, 1.0 - dh0])
    S = np.array([[0.0089636, 0.0125], [2.5, 40.0]]).reshape(1, 2, 2)     # a stack of four columns
    ibu, m2l, l2m, lam = route(S, dh)
    dhc = 0.5 * (dh[0] + dh[1])
    want = S[0] / dhc * (1 / dh[0] + 1 / dh[1])
    tol = 16 * R.EPS
    assert np.all(ibu[0] == 0) and np.all(np.abs(lam[0]) <= tol * want)
    assert np.allclose(lam[1], want, rtol=tol, atol=0) and np.allclose(ibu[1], -want, rtol=tol, atol=0)
    M = m2l.reshape(2, 2, 2, 2)          # [k][m][columns]
    L = l2m.reshape(2, 2, 2, 2)          # [m][k][columns]
    for k, m, v in ((0, 0, 1.0), (1, 0, 1.0), (0, 1, np.sqrt(dh[1] / dh[0])), (1, 1, -np.sqrt(dh[0] / dh[1]))):
        assert np.allclose(M[k, m], v, rtol=tol, atol=0), (k, m)
    assert np.abs(np.einsum("mkyx,knyx->mnyx", L, M) - np.eye(2)[:, :, None, None]).max() <= tol
    assert np.allclose(L, dh[None, :, None, None] * np.swapaxes(M, 0, 1), rtol=tol, atol=0)     # the left vectors are dhf[k] * vr[k][m]


def test_routes_agree_and_one_layer():
    dh = np.array([0.06, 0.14, 0.8])
    S = (np.array([0.0023669, 0.0076173]) / 0.025)[:, None] ** 2 * (1 + 0.3 * (2 * np.random.default_rng(3).random((2, 50)) - 1))
    a, b = R.modes_dgeev(S, dh), R.modes_eigh(S, dh)
    gap = R.rel_gap(a[3])
    assert gap.min() > 1e-2 and R.surface_ratio(a[1], 3).min() > 1e-2
    assert np.all(np.abs(a[0] - b[0]) <= 8 * 3 * R.EPS * np.abs(a[0]).max(axis=0))
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        assert np.all(np.abs(x - y).max(axis=0) <= 4 * 3 * R.EPS / gap * np.abs(x).max(axis=0))
    ibu, m2l, l2m, lam = R.modes_dgeev(np.ones((1, 4)), np.array([1.0]))       # one layer: the 1 x 1 zero matrix
    assert np.all(ibu == 0) and np.all(m2l == 1) and np.all(l2m == 1) and R.rel_gap(lam).min() == 1


# ------------------------------------------------------------------ the helpers of the hard stratifications (tests/test_gpu_modes_hard.py)

HARD_NL = (2, 3, 6, 8, 9, 16)
T64 = np.arange(64) / 63.0


@pytest.mark.parametrize("n", [1, 2, 3, 7, 16])
def test_sturm_count_and_bisection_against_eigvalsh(n):
    """random symmetric tridiagonals, 40 columns: between two neighbouring eigenvalues of numpy.linalg.eigvalsh (and outside all) the
    count is the index, and the bisected eigenvalues are those of eigvalsh within 4 n eps |T|_2 <= 4 n eps gershgorin"""
    rng = np.random.default_rng(n)
    a, b = rng.standard_normal((n, 40)), rng.standard_normal((n - 1, 40))
    a[:, :5] *= 1e-6        # some columns graded over many orders
    b[n // 2:, 5:10] *= 1e-9
    T = np.zeros((40, n, n))
    for i in range(n):
        T[:, i, i] = a[i]
    for i in range(n - 1):
        T[:, i, i + 1] = T[:, i + 1, i] = b[i]
    w = np.linalg.eigvalsh(T).T                                 # [n, 40] ascending
    g = np.asarray(R.gershgorin(a.astype(R.LD), b.astype(R.LD)), dtype=np.float64)
    tol = 4 * n * R.EPS * g
    probes = np.vstack([w[:1] - 1, 0.5 * (w[:-1] + w[1:]), w[-1:] + 1])
    for k in range(n + 1):
        clear = np.ones(40, bool) if k in (0, n) else (w[k] - w[k - 1]) > 4 * tol      # a probe between two equal eigenvalues says nothing
        assert np.array_equal(R.sturm_count(a, b, probes[k])[clear], np.full(40, k)[clear]), k
    for k in range(n):
        assert np.all(np.abs(np.asarray(R.eig_bisect(a, b, k), dtype=np.float64) - w[k]) <= tol), k


@pytest.mark.parametrize("nl", HARD_NL)
def test_hard_families_are_fair_cases(nl):
    """every column that must succeed has lambda_1 >= 16 * 8 nl eps lambda_max, every column that must be refused lambda_1 <= 1 / 16 of it:
    none within a factor 16 of the threshold, where either answer of the device would be right"""
    cols = [(R.hard_S("graded", nl, T64), R.dh_eq(nl)), (R.hard_S("weak", nl, T64), R.dh_eq(nl)), (R.hard_S("weak", nl, T64), R.dh_thin(nl)),
            (R.hard_S("uniform", nl, T64[:1]), R.dh_eq(nl))]
    worst = np.inf
    for S, dh in cols:
        a, b = R.sym_tridiag(S, dh)
        ratio = R.eig_bisect(a, b, 1) / (8 * nl * R.EPS * R.eig_bisect(a, b, nl - 1))
        worst = min(worst, ratio.min())
        assert np.all(ratio >= 16)
    print(f"nl = {nl}: smallest lambda_1 over the threshold among the columns that must succeed: {float(worst):.3g}")
    if nl in (3, 6, 9, 16):
        for dh, weak in ((R.dh_eq(nl), 1e-17), (R.dh_thin(nl), 1e-20)):
            a, b = R.sym_tridiag(R.hard_S("weak", nl, T64[:1], weak=weak), dh)
            ratio = R.eig_bisect(a, b, 1) / (8 * nl * R.EPS * R.eig_bisect(a, b, nl - 1))
            print(f"nl = {nl}: refused column, weak = {weak}: lambda_1 over the threshold {float(ratio[0]):.3g}")
            assert np.all(ratio <= 1 / 16)


@pytest.mark.parametrize("nl", HARD_NL)
def test_hard_criteria_pass_lapack_and_catch_a_perturbation(nl):
    """the criteria of the device test, run on the CPU: LAPACK's decomposition (route "eigh") of the hard columns meets every one of them,
    and a decomposition with one vector scaled by 1 + 1e-12, one entry off by 1e-9 or one eigenvalue off by 64 nl eps lambda_max does not"""
    for S, dh in ((R.hard_S("graded", nl, T64), R.dh_eq(nl)), (R.hard_S("weak", nl, T64), R.dh_thin(nl))):
        ibu, m2l, _, _ = R.modes_eigh(S, dh)
        c = R.hard_criteria(S, dh, ibu, m2l)
        print(f"nl = {nl}: eigenvalue {float(c['lam_err'].max()):.3f}, residual {float(c['res'].max()):.3f}, orthonormality {float(c['orth'].max()):.3f}")
        assert np.all(c["sturm_ok"]) and c["res"].max() <= 1 and c["orth"].max() <= 1
        bad = m2l.copy()
        bad[nl - 1::nl] *= 1 + 1e-12                               # the last mode's vector
        assert R.hard_criteria(S, dh, ibu, bad)["orth"].min() > 1
        bad = m2l.copy()
        bad[nl - 1] += 1e-9 * np.abs(m2l).max(axis=0)               # its surface entry: no longer an eigenvector
        assert R.hard_criteria(S, dh, ibu, bad)["res"][nl - 1].min() > 1
        bad = ibu.copy()
        bad[nl - 1] -= 64 * nl * R.EPS * np.abs(ibu).max(axis=0)
        assert not np.any(R.hard_criteria(S, dh, bad, m2l)["sturm_ok"][nl - 2])


@pytest.mark.parametrize("nl", HARD_NL)
def test_uniform_closed_form(nl):
    lam, vr = R.uniform_closed_form(R.S0, nl)
    a, b = R.sym_tridiag(R.hard_S("uniform", nl, T64[:1]), R.dh_eq(nl))
    for m in range(nl):
        assert abs(R.eig_bisect(a, b, m)[0] - lam[m]) <= 4 * nl * R.EPS * lam[-1]       # 1 / nl is rounded in dh_eq
    assert np.abs(np.einsum("km,kn->mn", vr, vr) / nl - np.eye(nl)).max() <= 1e-17 * nl and np.all(vr[0] > 0)
