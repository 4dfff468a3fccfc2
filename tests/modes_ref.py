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


# ------------------------------------------------------------------ hard stratifications: columns, and criteria that need no gap
# (tests/test_gpu_modes_hard.py on the device, tests/test_modes_ref.py on the CPU; tools/modes_host_check.cpp restates them in C++)

LD = np.longdouble
S0 = 5000.0


def dh_eq(nl):
    return np.full(nl, 1.0 / nl)


def dh_thin(nl):
    """geometric, the bottom layer 1e3 times the top one, normalised to sum 1"""
    dh = 1e3 ** (np.arange(nl) / max(nl - 1, 1))
    return dh / dh.sum()


def hard_S(family, nl, t, weak=None):
    """S [nl - 1, len(t)] of a family at the parameters t in [0, 1]: "graded" S_l = S0 10^(-8 t l / max(nl - 2, 1)); "weak" S_l = S0 but
    S_mid = S0 10^(-8 t) at mid = (nl - 1) // 2 (or S0 * weak, whatever t); "uniform" S_l = S0"""
    t = np.asarray(t, dtype=np.float64)
    S = np.full((nl - 1, t.size), S0)
    if family == "graded":
        S = S0 * 10.0 ** (-8.0 * t[None, :] * np.arange(nl - 1)[:, None] / max(nl - 2, 1))
    elif family == "weak":
        S[(nl - 1) // 2] = S0 * (10.0 ** (-8.0 * t) if weak is None else weak)
    else:
        assert family == "uniform"
    return S


def sym_tridiag(S, dh):
    """T = D^1/2 amat D^-1/2 in longdouble: (diagonal [nl, ...], off-diagonal [nl - 1, ...]); dhc rounded to double as the handle holds it"""
    dh = np.asarray(dh, dtype=np.float64)
    nl = dh.size
    S = np.asarray(S, dtype=np.float64)[:nl - 1].astype(LD)
    dhc = (0.5 * (dh[:-1] + dh[1:])).astype(LD)
    dh = dh.astype(LD)
    a = np.zeros((nl,) + S.shape[1:], dtype=LD)
    b = np.zeros((nl - 1,) + S.shape[1:], dtype=LD)
    for l in range(nl - 1):
        a[l] += S[l] / (dhc[l] * dh[l])
        a[l + 1] += S[l] / (dhc[l] * dh[l + 1])
        b[l] = -S[l] / (dhc[l] * np.sqrt(dh[l] * dh[l + 1]))
    return a, b


def gershgorin(a, b):
    g = np.abs(a)
    g[1:] += np.abs(b)
    g[:-1] += np.abs(b)
    return g.max(axis=0)


def sturm_count(a, b, x):
    """number of eigenvalues below x of the symmetric tridiagonal (a, b), per column: the negative pivots of T - x = L D L^T"""
    a, b, x = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD), np.asarray(x, dtype=LD)
    g = gershgorin(a, b)
    tiny = -np.finfo(LD).eps ** 2 * np.where(g > 0, g, 1)       # a zero pivot counts as negative and does not divide
    cnt = np.zeros(np.broadcast(a[0], x).shape, dtype=np.int64)
    q = np.ones(cnt.shape, dtype=LD)
    for i in range(a.shape[0]):
        q = a[i] - x - (b[i - 1] * b[i - 1] / q if i else 0)
        q = np.where(q == 0, tiny, q)
        cnt += q < 0
    return cnt


def eig_bisect(a, b, k, iters=200, lo=None, hi=None):
    """eigenvalue k (ascending, 0-based) of every column by bisection on the Sturm count, longdouble; from Gershgorin's interval (200
    halvings: 1e-60 of it) or from a given bracket [lo, hi] (an eigenvalue outside comes back as the nearer end)"""
    if lo is None:
        hi = gershgorin(a, b)
        lo = -hi
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        left = sturm_count(a, b, mid) >= k + 1
        hi = np.where(left, mid, hi)
        lo = np.where(left, lo, mid)
    return 0.5 * (lo + hi)


def hard_criteria(S, dh, ibu, m2l):
    """the gap-independent criteria of a decomposition (iBu [nl, ...], M2L [nl*nl, ...]) of the columns (S, dh), in longdouble.  Returns
    lam1, lmax: reference eigenvalues 1 and nl - 1; thr = 8 nl eps lmax;
    sturm_ok [nl - 1, ...]: #{eig T < lam_m - thr} <= m and #{eig T < lam_m + thr} >= m + 1 for lam_m = -iBu_m, m >= 1;
    lam_err [nl - 1, ...]: |lam_m - reference| / thr, the reference bisected within lam_m +- thr (reported only; 1 where sturm_ok fails);
    res [nl, ...]: |T y_m - lam_m y_m|_2 / (8 nl eps |T|_F |y_m|_2), y_m = D^1/2 M2L[:, m], lam_0 = 0;
    orth [...]: max |M2L^T D M2L - I| / (8 nl eps)"""
    dh = np.asarray(dh, dtype=np.float64)
    nl = dh.size
    shape = ibu.shape[1:]
    a, b = sym_tridiag(S, dh)
    lam = -np.asarray(ibu).astype(LD)
    lam[0] = 0
    M = np.asarray(m2l).reshape((nl, nl) + shape).astype(LD)          # [k][m]
    out = {}
    if nl > 1:
        out["lmax"], out["lam1"] = eig_bisect(a, b, nl - 1), eig_bisect(a, b, 1)
    else:
        out["lmax"] = out["lam1"] = np.zeros(shape, dtype=LD)
    thr = out["thr"] = 8 * nl * LD(EPS) * out["lmax"]
    out["sturm_ok"] = np.array([(sturm_count(a, b, lam[m] - thr) <= m) & (sturm_count(a, b, lam[m] + thr) >= m + 1) for m in range(1, nl)]
                               ).reshape((nl - 1,) + shape)
    out["lam_err"] = np.array([np.abs(lam[m] - eig_bisect(a, b, m, 40, lam[m] - thr, lam[m] + thr)) / thr for m in range(1, nl)],
                              dtype=LD).reshape((nl - 1,) + shape)
    y = np.sqrt(dh.astype(LD)).reshape((nl, 1) + (1,) * len(shape)) * M
    Ty = a[:, None] * y
    if nl > 1:
        Ty[1:] += b[:, None] * y[:-1]
        Ty[:-1] += b[:, None] * y[1:]
    r = Ty - lam[None] * y
    frob = np.sqrt((a * a).sum(axis=0) + 2 * (b * b).sum(axis=0))
    bound = 8 * nl * LD(EPS) * frob * np.sqrt((y * y).sum(axis=0))
    out["res"] = np.sqrt((r * r).sum(axis=0)) / np.where(bound > 0, bound, 1)
    G = np.zeros((nl, nl) + shape, dtype=LD)
    for k in range(nl):
        G += dh[k].astype(LD) * M[k][:, None] * M[k][None, :]
    G -= np.eye(nl, dtype=LD).reshape((nl, nl) + (1,) * len(shape))
    out["orth"] = np.abs(G).max(axis=(0, 1)) / (8 * nl * LD(EPS))
    return out


def uniform_closed_form(s, nl):
    """equal layers 1 / nl and the same S = s on every interface: lambda_m = 4 s nl^2 sin^2(m pi / (2 nl)) and, with Flierl's normalisation,
    vr[k][m] = sqrt(2) cos((k + 1/2) m pi / nl) (vr[k][0] = 1).  Returns (lambda [nl], vr [nl (k), nl (m)]) in longdouble"""
    pi = np.arccos(LD(-1))
    m = np.arange(nl).astype(LD)
    lam = 4 * LD(s) * nl * nl * np.sin(m * pi / (2 * nl)) ** 2
    vr = np.sqrt(LD(2)) * np.cos((m[:, None] + LD(0.5)) * m[None, :] * pi / nl)
    vr[:, 0] = 1
    return lam, vr
