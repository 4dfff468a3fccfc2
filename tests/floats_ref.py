"""Numpy restatement of the arithmetic of the Lagrangian floats (include/msom_floats.h), written from the
formulas of the header in their expression order; generic in the dtype (float64: what the strict build must equal bit for bit;
longdouble: the yardstick of the product build's bars).  Its input is a ghosted field [nl][ny + 2][nx + 2]: index (j + 1, i + 1)
holds cell (i, j), the ring holds what boundary() left there.

    xi = x * idx - 0.5;  i0 = floor(xi);  a = xi - i0       (eta, j0, b likewise from y)
    walls:    i0 clamped to [-1, nx - 1];   periodic: i0 modulo nx
    u = -((1 - a) * (P01 - P00) + a * (P11 - P10)) * idx
    v =  ((1 - b) * (P10 - P00) + b * (P11 - P01)) * idx
"""
import numpy as np


class Geom:
    def __init__(self, nx, ny, L0, periodic=False):
        self.nx, self.ny, self.L0, self.periodic = int(nx), int(ny), float(L0), bool(periodic)
        self.idx = nx / float(L0)            # rounded once, in float64, as the library does
        self.Lx, self.Ly = float(L0), float(L0) * ny / nx


def axis(x, idx, n, periodic, dtype=np.float64):
    """(i0, a, xi) of positions x; i0 an int array.  Non-finite positions: i0 = 0, a = NaN"""
    x = np.asarray(x, dtype=dtype)
    xi = x * dtype(idx) - dtype(0.5)
    ok = np.isfinite(xi)
    f = np.floor(np.where(ok, xi, 0))
    a = np.where(ok, xi - f, np.nan)
    if periodic:
        f = np.fmod(f, dtype(n))
        f = np.where(f < 0, f + dtype(n), f)
        f = np.clip(f, 0, n - 1)
    else:
        f = np.clip(f, -1, n - 1)
    return f.astype(np.int64), a, xi


def corners(F, layer, i0, j0):
    """P00, P10, P01, P11 of a ghosted field"""
    return (F[layer, j0 + 1, i0 + 1], F[layer, j0 + 1, i0 + 2], F[layer, j0 + 2, i0 + 1], F[layer, j0 + 2, i0 + 2])


def locate(g, x, y, dtype=np.float64):
    i0, a, xi = axis(x, g.idx, g.nx, g.periodic, dtype)
    j0, b, eta = axis(y, g.idx, g.ny, g.periodic, dtype)
    return i0, j0, a, b, xi, eta


def velocity(g, F, x, y, layer, dtype=np.float64):
    """(u, v) at the floats; F ghosted (psi, or psi + psipg summed beforehand: the same sum per corner).  Lost floats: NaN"""
    F = np.asarray(F, dtype=dtype)
    i0, j0, a, b, _, _ = locate(g, x, y, dtype)
    P00, P10, P01, P11 = corners(F, layer, i0, j0)
    one, idx = dtype(1), dtype(g.idx)
    u = -((one - a) * (P01 - P00) + a * (P11 - P10)) * idx
    v = ((one - b) * (P10 - P00) + b * (P11 - P01)) * idx
    lost = np.isnan(a) | np.isnan(b)
    return np.where(lost, np.nan, u), np.where(lost, np.nan, v)


def sample(g, F, x, y, layer, dtype=np.float64):
    F = np.asarray(F, dtype=dtype)
    i0, j0, a, b, _, _ = locate(g, x, y, dtype)
    P00, P10, P01, P11 = corners(F, layer, i0, j0)
    one = dtype(1)
    s = (one - b) * ((one - a) * P00 + a * P10) + b * ((one - a) * P01 + a * P11)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, s)


def move(g, bx, by, u, v, h, dtype=np.float64):
    """(x, y, clamped, lost) = one stage from the base position (bx, by) with the velocity (u, v) over h"""
    bx, by = np.asarray(bx, dtype=dtype), np.asarray(by, dtype=dtype)
    x, y = bx + dtype(h) * u, by + dtype(h) * v
    lost = ~(np.isfinite(x) & np.isfinite(y))
    clamped = np.zeros(x.shape, dtype=bool)
    if not g.periodic:
        cx, cy = np.clip(x, 0, dtype(g.Lx)), np.clip(y, 0, dtype(g.Ly))
        clamped = ((cx != x) | (cy != y)) & ~lost
        x, y = cx, cy
    return np.where(lost, np.nan, x), np.where(lost, np.nan, y), clamped, lost


def stage1(g, F, x, y, layer, dt, dtype=np.float64):
    """(xh, yh) = (x, y) + dt / 2 U(x, y; F)"""
    u, v = velocity(g, F, x, y, layer, dtype)
    return move(g, x, y, u, v, dtype(dt) / dtype(2), dtype)[:2]


def stage2(g, F, x, y, xh, yh, layer, dt, dtype=np.float64):
    """(x, y) + dt U(xh, yh; F)"""
    u, v = velocity(g, F, xh, yh, layer, dtype)
    return move(g, x, y, u, v, dt, dtype)[:2]


def near_cell_line(g, x, y, tol=1e-9):
    """floats whose xi or eta lies within tol of an integer in the longdouble run: a different floor gives a different dual cell"""
    _, _, _, _, xi, eta = locate(g, x, y, np.longdouble)
    return (np.abs(xi - np.rint(xi)) < tol) | (np.abs(eta - np.rint(eta)) < tol)


def seeded_floats(g, n, nl, seed=0):
    """the random floats of the GPU tests: positions uniform in the box (periodic: in [-L, 2 L]), mixed layers"""
    rng = np.random.default_rng(seed)
    if g.periodic:
        x, y = rng.uniform(-g.Lx, 2 * g.Lx, n), rng.uniform(-g.Ly, 2 * g.Ly, n)
    else:
        x, y = rng.uniform(0, g.Lx, n), rng.uniform(0, g.Ly, n)
    return x, y, rng.integers(0, nl, n).astype(np.int32)


def wall_floats(g):
    """deliberately placed floats of a walled box: the four walls, the four corners, cell-centre lines (a = 0), the half cells next to the walls"""
    D = g.Lx / g.nx
    xs = [0.0, g.Lx, 0.5 * D, 1.5 * D, g.Lx - 0.5 * D, 0.25 * D, g.Lx - 0.25 * D, 0.37 * g.Lx]
    ys = [0.0, g.Ly, 0.5 * D, 2.5 * D, g.Ly - 0.5 * D, 0.25 * D, g.Ly - 0.25 * D, 0.61 * g.Ly]
    X, Y = np.meshgrid(xs, ys)
    return X.ravel().copy(), Y.ravel().copy()


def ghosted_dirichlet(interior):
    """[nl][ny][nx] -> ghosted with psi = 0 on the wall faces: ghost = -cell, corner ghost = + the interior corner cell (boundary())"""
    nl, ny, nx = interior.shape
    F = np.zeros((nl, ny + 2, nx + 2), dtype=interior.dtype)
    F[:, 1:-1, 1:-1] = interior
    F[:, 1:-1, 0], F[:, 1:-1, -1] = -interior[:, :, 0], -interior[:, :, -1]
    F[:, 0, :], F[:, -1, :] = -F[:, 1, :], -F[:, -2, :]
    return F
