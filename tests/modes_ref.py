"""numpy restatement of the reference's vertical-mode decomposition (msqg/eigmode.h), routine for routine, for the tests of
msom_modes_*.  Everything works on stacks of columns: S has shape (nl - 1, ...) and the results carry the same trailing shape.

route "dgeev": np.linalg.eig(A) for the right and np.linalg.eig(A.T) for the left vectors (LAPACK dgeev, the routine
eigmode.h:153 calls), both sorted by eigenvalue (:161-193), then the normalisations of :213-231.
route "eigh": np.linalg.eigh on the symmetrised matrix D^1/2 A D^-1/2, vectors scaled back by D^-1/2, same normalisation of the
right vectors; the left vectors are dhf[k] * vr[k][m] / htotal."""
import numpy as np

EPS = 2.0 ** -52
HTOTAL = 1.0


def sign(x):
    """Basilisk's sign: x > 0 ? 1 : -1"""
    return np.where(x > 0, 1.0, -1.0)


def amat(S, dh):
    """the tridiagonal of eigmode.h:86-109 for every column: shape (..., nl, nl)"""
    dh = np.asarray(dh, dtype=np.float64)
    nl = dh.size
    S = np.asarray(S, dtype=np.float64)[:nl - 1]     # a one-layer model still carries one (unused) interface array
    A = np.zeros(S.shape[1:] + (nl, nl))
    dhc = 0.5 * (dh[:-1] + dh[1:])
    for l in range(nl):
        lo = -S[l - 1] / (dhc[l - 1] * dh[l]) if l > 0 else 0.0
        up = -S[l] / (dhc[l] * dh[l]) if l < nl - 1 else 0.0
        if l > 0:
            A[..., l, l - 1] = lo
        if l < nl - 1:
            A[..., l, l + 1] = up
        A[..., l, l] = -lo - up
    return A


def _sorted(w, v):
    assert np.all(np.imag(w) == 0) and np.all(np.imag(v) == 0)
    w, v = np.real(w), np.real(v)
    o = np.argsort(w, axis=-1, kind="stable")
    return np.take_along_axis(w, o, axis=-1), np.take_along_axis(v, o[..., None, :], axis=-1)


def _flierl(vr, dh):
    """eigmode.h:213-222: sum_k dhf_k vr_km^2 = htotal, positive at the surface"""
    dotp = np.einsum("k,...km,...km->...m", dh, vr, vr)
    return vr * (sign(vr[..., 0, :]) * np.sqrt(HTOTAL / dotp))[..., None, :]


def _pack(w, vr, vl):
    """(iBu [nl, ...], M2L [nl*nl, ...] array k*nl+m = vr[k][m], L2M [nl*nl, ...] array m*nl+k = vl[k][m], lambda [nl, ...])"""
    nl = w.shape[-1]
    lam = np.moveaxis(w, -1, 0)
    ibu = -lam
    ibu[0] = 0.0          # eigmode.h:264-266
    m2l = np.moveaxis(vr.reshape(vr.shape[:-2] + (nl * nl,)), -1, 0)
    l2m = np.moveaxis(np.swapaxes(vl, -1, -2).reshape(vl.shape[:-2] + (nl * nl,)), -1, 0)
    return np.ascontiguousarray(ibu), np.ascontiguousarray(m2l), np.ascontiguousarray(l2m), np.ascontiguousarray(lam)


def modes_dgeev(S, dh):
    dh = np.asarray(dh, dtype=np.float64)
    A = amat(S, dh)
    wr, vr = _sorted(*np.linalg.eig(A))
    _, vl = _sorted(*np.linalg.eig(np.swapaxes(A, -1, -2)))
    vr = _flierl(vr, dh)
    dotp = np.einsum("...km,...km->...m", vr, vl)        # eigmode.h:223-231
    vl = vl / dotp[..., None, :]
    return _pack(wr, vr, vl)


def modes_eigh(S, dh):
    dh = np.asarray(dh, dtype=np.float64)
    A = amat(S, dh)
    r = np.sqrt(dh)
    T = A * r[:, None] / r[None, :]
    T = 0.5 * (T + np.swapaxes(T, -1, -2))
    w, v = np.linalg.eigh(T)
    vr = _flierl(v / r[:, None], dh)
    vl = dh[:, None] * vr / HTOTAL
    return _pack(w, vr, vl)


def rel_gap(lam):
    """smallest eigenvalue gap over the largest eigenvalue, per column (1 for a single layer)"""
    if lam.shape[0] < 2:
        return np.ones(lam.shape[1:])
    return np.min(np.diff(lam, axis=0), axis=0) / np.max(np.abs(lam), axis=0)


def surface_ratio(m2l, nl):
    """min_m |vr[0][m]| / max|vr| per column: how well the surface sign is defined"""
    return np.min(np.abs(m2l[:nl]), axis=0) / np.max(np.abs(m2l), axis=0)
