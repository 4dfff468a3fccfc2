"""numpy restatement of the modal PV inversion (option mode_pv_invert): nl independent multigrid solves of
lap(p_m) + iBu_m p_m = q_m between the projections q_m = sum_k l2m[m][k] q_k and psi_k = sum_m m2l[k][m] p_m.

Written from the rules of SURVEY appendix B (mg_solve / mg_cycle with minlevel = 1) and the expression orders include/msom.h
documents for the relaxation and the residual; every operation is a plain IEEE double operation in that order, so the strict build
can be held to the same bits.

Conventions: arrays are [mode][y][x]; a level is a (nx, ny) pair as the handle reports it (level 0 finest, each next one half as
wide and high); the cell size of level k is L0 / nx_k; `ibu` is a list with one array per level, broadcastable to the level's
[nl][ny][nx] (shape (nl, 1, 1) for a uniform stratification, else the mean-of-4 pyramid of ibu_pyramid).  Ghosts: homogeneous
Dirichlet at the faces (edges -v, corners +v) or wrapped (periodic = True).  Red = (i + j) even goes first."""
import numpy as np

NITERMIN, NITERMAX = 1, 100


def pad(a, periodic):
    """[nl][ny][nx] -> [nl][ny + 2][nx + 2] with the ghost ring"""
    nl, ny, nx = a.shape
    p = np.zeros((nl, ny + 2, nx + 2))
    p[:, 1:-1, 1:-1] = a
    if periodic:
        p[:, 1:-1, 0], p[:, 1:-1, -1] = a[:, :, -1], a[:, :, 0]
        p[:, 0, 1:-1], p[:, -1, 1:-1] = a[:, -1, :], a[:, 0, :]
        p[:, 0, 0], p[:, 0, -1], p[:, -1, 0], p[:, -1, -1] = a[:, -1, -1], a[:, -1, 0], a[:, 0, -1], a[:, 0, 0]
    else:
        p[:, 1:-1, 0], p[:, 1:-1, -1] = -a[:, :, 0], -a[:, :, -1]
        p[:, 0, 1:-1], p[:, -1, 1:-1] = -a[:, 0, :], -a[:, -1, :]
        p[:, 0, 0], p[:, 0, -1], p[:, -1, 0], p[:, -1, -1] = a[:, 0, 0], a[:, 0, -1], a[:, -1, 0], a[:, -1, -1]
    return p


def colour_mask(ny, nx, colour):
    j, i = np.mgrid[0:ny, 0:nx]
    return ((i + j) & 1) == colour


def relax_half(a, b, ibu, sqD, colour, active, periodic):
    """one half-sweep, in place, of the modes with active[m]:
    n = -sqD * b; n = n + (E + W); n = n + (N + S); d = (-(ibu * sqD) + 2) + 2; a = n / d"""
    p = pad(a, periodic)
    n = -sqD * b
    n = n + (p[:, 1:-1, 2:] + p[:, 1:-1, :-2])
    n = n + (p[:, 2:, 1:-1] + p[:, :-2, 1:-1])
    d = (-(ibu * sqD) + 2.0) + 2.0
    x = n / d
    mask = colour_mask(a.shape[1], a.shape[2], colour)
    for m in range(a.shape[0]):
        if active[m]:
            a[m][mask] = x[m][mask]


def relax(a, b, ibu, sqD, nhalf, periodic, count=None):
    """nhalf half-sweeps starting with colour 0; half-sweep h is sweep h // 2, which mode m takes while count[m] > h // 2"""
    a = np.array(a, dtype=np.float64)
    for h in range(nhalf):
        active = [count is None or count[m] > h // 2 for m in range(a.shape[0])]
        relax_half(a, b, ibu, sqD, h & 1, active, periodic)
    return a


def residual(a, b, ibu, D, periodic):
    """r = b - ibu * a; r = r + ((a - W) / D - (E - a) / D) / D; r = r + ((a - S) / D - (N - a) / D) / D; and max |r| per mode"""
    p = pad(a, periodic)
    c = p[:, 1:-1, 1:-1]
    r = b - ibu * c
    r = r + ((c - p[:, 1:-1, :-2]) / D - (p[:, 1:-1, 2:] - c) / D) / D
    r = r + ((c - p[:, :-2, 1:-1]) / D - (p[:, 2:, 1:-1] - c) / D) / D
    return r, np.abs(r).reshape(r.shape[0], -1).max(axis=1)


def restrict(f):
    """mean of the 4 children, summed in the order (2J, 2I), (2J + 1, 2I), (2J, 2I + 1), (2J + 1, 2I + 1)"""
    s = 0.0 + f[:, 0::2, 0::2]
    s = s + f[:, 1::2, 0::2]
    s = s + f[:, 0::2, 1::2]
    s = s + f[:, 1::2, 1::2]
    return s / 4


def prolong(c, periodic):
    """bilinear, (9 c + 3 (c[child.x] + c[0, child.y]) + c[child.x, child.y]) / 16 with the coarse ghosts"""
    nl, ny, nx = c.shape
    p = pad(c, periodic)
    j, i = np.mgrid[0:2 * ny, 0:2 * nx]
    J, I = (j >> 1) + 1, (i >> 1) + 1
    cx, cy = np.where(i & 1, 1, -1), np.where(j & 1, 1, -1)
    return (9.0 * p[:, J, I] + 3.0 * (p[:, J, I + cx] + p[:, J + cy, I]) + p[:, J + cy, I + cx]) / 16.0


def ibu_pyramid(ibu0, nlev):
    """per-cell iBu on every level: the mean of the 4 children, level by level"""
    out = [np.asarray(ibu0, dtype=np.float64)]
    for _ in range(1, nlev):
        out.append(restrict(out[-1]))
    return out


def ibu_levels(ibu, nlev):
    """`ibu`: nl numbers (uniform) or a [nl][ny][nx] array -> the per-level list the functions here take"""
    ibu = np.asarray(ibu, dtype=np.float64)
    if ibu.ndim == 1:
        return [ibu[:, None, None]] * nlev
    return ibu_pyramid(ibu, nlev)


def cycle(res0, ibu, dims, L0, nrelax, periodic):
    """the correction of one multigrid cycle: residual restricted to every level; from the coarsest level up, prolongation (zero on
    the coarsest) and nrelax[m] sweeps of mode m (0: the mode is frozen, its correction stays zero)"""
    nlev = len(dims)
    res = [res0]
    for k in range(1, nlev):
        res.append(restrict(res[-1]))
    da = None
    for k in range(nlev - 1, -1, -1):
        D = L0 / dims[k][0]
        da = np.zeros_like(res[k]) if k == nlev - 1 else prolong(da, periodic)
        da = relax(da, res[k], ibu[k], D * D, 2 * max(nrelax), periodic, count=nrelax)
    return da


class Stats:
    def __init__(self):
        self.i, self.nrelax, self.resb, self.resa, self.sum = 0, 4, 0.0, 0.0, 0.0
        self.history = []   # resa after every cycle this mode ran
        self.ratios = []    # resb / resa of those cycles (what the 1.2 / 10 rule on nrelax looks at)


def solve(pm, qm, ibu, dims, L0, tol, periodic, nitermin=NITERMIN, nitermax=NITERMAX, snapshots=None):
    """nl independent mg_solve loops, cycle by cycle for all modes that still run (a mode's own sequence does not depend on the
    others).  pm: warm start, returned updated.  snapshots: list that receives a copy of pm after every cycle.  Returns (pm, [Stats])"""
    pm = np.array(pm, dtype=np.float64)
    nl = pm.shape[0]
    D = L0 / dims[0][0]
    st = [Stats() for _ in range(nl)]
    res, mx = residual(pm, qm, ibu[0], D, periodic)
    resb = list(mx)
    for m in range(nl):
        st[m].resb = st[m].resa = mx[m]
        st[m].sum = float(qm[m].sum())
    while True:
        cnt = [s.nrelax if s.i < nitermax and (s.i < nitermin or s.resa > tol) else 0 for s in st]
        if max(cnt) == 0:
            break
        pm = pm + cycle(res, ibu, dims, L0, cnt, periodic)
        res, mx = residual(pm, qm, ibu[0], D, periodic)
        for m, s in enumerate(st):
            if cnt[m] == 0:
                continue
            s.resa = mx[m]
            s.history.append(mx[m])
            s.ratios.append(resb[m] / mx[m])
            if s.resa > tol:
                if resb[m] / s.resa < 1.2 and s.nrelax < 100:
                    s.nrelax += 1
                elif resb[m] / s.resa > 10 and s.nrelax > 2:
                    s.nrelax -= 1
            resb[m] = s.resa
            s.i += 1
        if snapshots is not None:
            snapshots.append(pm.copy())
    return pm, st


def project(coef, x, nl):
    """the documented order of msom_modes_project: acc = 0; acc = acc + c * x, inner index ascending; coef array o * nl + i"""
    out = np.empty_like(x)
    for o in range(nl):
        acc = np.zeros(x.shape[1:])
        for i in range(nl):
            acc = acc + coef[o * nl + i] * x[i]
        out[o] = acc
    return out


def invert(q, l2m, m2l, ibu, dims, L0, tol, periodic, pm0=None, **kw):
    """psi, pm, stats of the modal inversion of q from the warm start pm0 (zero if None)"""
    nl = q.shape[0]
    qm = project(l2m, q, nl)
    pm, st = solve(np.zeros_like(qm) if pm0 is None else pm0, qm, ibu, dims, L0, tol, periodic, **kw)
    return project(m2l, pm, nl), pm, st
