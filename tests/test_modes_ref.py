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
