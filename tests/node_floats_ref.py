"""Numpy restatement of the arithmetic of the Lagrangian floats of the vertex-grid model (include/msomn_floats.h, DESIGN.md section
8l), written from the formulas of the header in their expression order; generic in the dtype (float64: what the strict build must
equal bit for bit; longdouble: the yardstick of the product build's bars).  Its input is a vertex field [nl][N + 1][N + 1], as
NodeQG.get returns it: no ghost ring.

    xi = x * idx;  f = floor(xi) clamped to [0, N - 1];  i0 = int(f);  a = xi - f clamped to [0, 1]
    u = -((1 - a) * (P01 - P00) + a * (P11 - P10)) * idx
    v =  ((1 - b) * (P10 - P00) + b * (P11 - P01)) * idx        Pcd = P[layer][j0 + d][i0 + c]
"""
import numpy as np


class Geom:
    def __init__(self, N, L0):
        self.N, self.L0 = int(N), float(L0)
        self.idx = N / float(L0)            # rounded once, in float64, as the library does


def axis(x, idx, n, dtype=np.float64):
    """(i0, a, xi) of positions x; i0 an int array.  Non-finite positions: i0 = 0, a = NaN"""
    x = np.asarray(x, dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        xi = x * dtype(idx)
    ok = np.isfinite(xi)
    f = np.clip(np.floor(np.where(ok, xi, 0)), 0, n - 1)
    a = np.where(ok, np.clip(np.where(ok, xi, 0) - f, 0, 1), np.nan)
    return f.astype(np.int64), a, xi


def locate(g, x, y, dtype=np.float64):
    i0, a, xi = axis(x, g.idx, g.N, dtype)
    j0, b, eta = axis(y, g.idx, g.N, dtype)
    return i0, j0, a, b, xi, eta


def corners(P, layer, i0, j0):
    """P00, P10, P01, P11 of a vertex field"""
    return P[layer, j0, i0], P[layer, j0, i0 + 1], P[layer, j0 + 1, i0], P[layer, j0 + 1, i0 + 1]


def velocity(g, P, x, y, layer, dtype=np.float64):
    """(u, v) at the floats; P: psi, or psi + psipg summed beforehand in float64 (the same sum per corner).  Lost floats: NaN"""
    P = np.asarray(P, dtype=dtype)
    i0, j0, a, b, _, _ = locate(g, x, y, dtype)
    P00, P10, P01, P11 = corners(P, layer, i0, j0)
    one, idx = dtype(1), dtype(g.idx)
    u = -((one - a) * (P01 - P00) + a * (P11 - P10)) * idx
    v = ((one - b) * (P10 - P00) + b * (P11 - P01)) * idx
    lost = np.isnan(a) | np.isnan(b)
    return np.where(lost, np.nan, u), np.where(lost, np.nan, v)


def sample(g, P, x, y, layer, dtype=np.float64):
    P = np.asarray(P, dtype=dtype)
    i0, j0, a, b, _, _ = locate(g, x, y, dtype)
    P00, P10, P01, P11 = corners(P, layer, i0, j0)
    one = dtype(1)
    s = (one - b) * ((one - a) * P00 + a * P10) + b * ((one - a) * P01 + a * P11)
    return np.where(np.isnan(a) | np.isnan(b), np.nan, s)


def move(g, bx, by, u, v, h, dtype=np.float64):
    """(x, y, clamped, lost) = one stage from the base position (bx, by) with the velocity (u, v) over h"""
    bx, by = np.asarray(bx, dtype=dtype), np.asarray(by, dtype=dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        x, y = bx + dtype(h) * u, by + dtype(h) * v
    lost = ~(np.isfinite(x) & np.isfinite(y))
    cx, cy = np.clip(x, 0, dtype(g.L0)), np.clip(y, 0, dtype(g.L0))
    clamped = ((cx != x) | (cy != y)) & ~lost
    return np.where(lost, np.nan, cx), np.where(lost, np.nan, cy), clamped, lost


def stage1(g, P, x, y, layer, dt, dtype=np.float64):
    """(xh, yh) = (x, y) + dt / 2 U(x, y; P)"""
    u, v = velocity(g, P, x, y, layer, dtype)
    return move(g, x, y, u, v, dtype(dt) / dtype(2), dtype)[:2]


def stage2(g, P, x, y, xh, yh, layer, dt, dtype=np.float64):
    """(x, y) + dt U(xh, yh; P)"""
    u, v = velocity(g, P, xh, yh, layer, dtype)
    return move(g, x, y, u, v, dt, dtype)[:2]


def near_vertex_line(g, x, y, tol=1e-9):
    """floats whose xi or eta lies within tol of an interior vertex line 1 .. N - 1 in the longdouble run: a different floor gives a
    different cell.  The lines 0 and N are the walls: there the clamp of the index gives the same cell whatever the floor is"""
    _, _, _, _, xi, eta = locate(g, x, y, np.longdouble)

    def near(c):
        k = np.rint(c)
        return (np.abs(c - k) < tol) & (k >= 1) & (k <= g.N - 1)
    return near(xi) | near(eta)


def on_land(g, mask, x, y):
    """floats that are not lost and whose cell has mask == 0 at all four corners; mask [N + 1][N + 1]"""
    i0, j0, a, b, _, _ = locate(g, x, y)
    m = mask[None]
    z = np.zeros(i0.shape, dtype=np.int64)
    return ~(np.isnan(a) | np.isnan(b)) & np.all([c == 0 for c in corners(m, z, i0, j0)], axis=0)


def seeded_floats(g, n, nl, seed=0):
    """the random floats of the GPU tests: positions uniform in the box, mixed layers"""
    rng = np.random.default_rng(seed)
    return rng.uniform(0, g.L0, n), rng.uniform(0, g.L0, n), rng.integers(0, nl, n).astype(np.int32)


def land_cells(mask):
    """(i0, j0) of the cells with four land corners that touch no domain wall; mask [N + 1][N + 1]"""
    z = (mask[:-1, :-1] == 0) & (mask[:-1, 1:] == 0) & (mask[1:, :-1] == 0) & (mask[1:, 1:] == 0)
    z[0, :] = z[-1, :] = z[:, 0] = z[:, -1] = False
    j, i = np.nonzero(z)
    return i, j


def coast_edges(mask):
    """(i, j) of the vertical edges (i, j) - (i, j + 1) between two land vertices with sea on at least one side, off the domain walls"""
    N = mask.shape[0] - 1
    out = []
    for j in range(1, N - 1):
        for i in range(1, N):
            if mask[j, i] == 0 and mask[j + 1, i] == 0 and (mask[j, i - 1] != 0 or mask[j + 1, i - 1] != 0 or mask[j, i + 1] != 0 or mask[j + 1, i + 1] != 0):
                out.append((i, j))
    return out


def placed_floats(g, mask):
    """the deliberately placed floats of the GPU tests, with the names of the groups as slices: the four walls and the four corners,
    exact vertex lines and exact vertices, all-land cells of the island, a coast edge, the cells i0 = N - 1 and j0 = N - 1, x = L0
    and y = L0.  mask [N + 1][N + 1].  Returns x, y, dict name -> index array"""
    N, L, D = g.N, g.L0, g.L0 / g.N
    xs, ys, groups = [], [], {}

    def add(name, px, py):
        k0 = len(xs)
        xs.extend(np.atleast_1d(px).tolist())
        ys.extend(np.atleast_1d(py).tolist())
        groups[name] = np.arange(k0, len(xs))

    add("west", [0.0, 0.0], [0.31 * L, 0.77 * L])
    add("east", [L, L], [0.23 * L, 0.58 * L])
    add("south", [0.41 * L, 0.69 * L], [0.0, 0.0])
    add("north", [0.12 * L, 0.87 * L], [L, L])
    add("corners", [0.0, L, 0.0, L], [0.0, 0.0, L, L])
    add("vertex_lines", [5 * D, 0.37 * L], [0.43 * L, 9 * D])
    add("vertices", [3 * D, (N - 1) * D], [7 * D, (N - 1) * D])
    li, lj = land_cells(mask)
    assert li.size >= 2
    add("land", [(li[0] + 0.3) * D, (li[-1] + 0.75) * D], [(lj[0] + 0.6) * D, (lj[-1] + 0.2) * D])
    ci, cj = coast_edges(mask)[0]
    add("coast", [ci * D], [(cj + 0.4) * D])
    add("last_cells", [(N - 0.5) * D, (N - 0.25) * D, 0.3 * L], [0.6 * L, (N - 0.75) * D, (N - 0.1) * D])
    return np.array(xs), np.array(ys), groups
