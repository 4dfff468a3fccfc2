"""The arithmetic of the Lagrangian floats (include/msom_floats.h) in its numpy restatement tests/floats_ref.py,
on synthetic ghosted fields: the properties the contract promises.  No GPU."""
import numpy as np
import pytest

import floats_ref as fr

EPS = np.finfo(np.float64).eps


def random_ghosted(nl, ny, nx, seed=1):
    return fr.ghosted_dirichlet(np.random.default_rng(seed).standard_normal((nl, ny, nx)))


@pytest.mark.parametrize("nx,ny", [(32, 32), (64, 32), (1, 1), (2, 3)])
def test_wall_normal_velocity_is_exactly_zero_on_walls_and_corners(nx, ny):
    g = fr.Geom(nx, ny, 80.0)
    F = random_ghosted(2, ny, nx)
    t = np.linspace(0.0, 1.0, 41)
    lay = np.arange(t.size) % 2
    for x, y, normal in ((0 * t, t * g.Ly, 0), (0 * t + g.Lx, t * g.Ly, 0), (t * g.Lx, 0 * t, 1), (t * g.Lx, 0 * t + g.Ly, 1)):
        uv = fr.velocity(g, F, x, y, lay)
        assert np.all(uv[normal] == 0), (normal, uv[normal])
        assert nx * ny == 1 or np.any(uv[1 - normal] != 0)   # ... and the float slides along the wall
    cx, cy = np.array([0, g.Lx, 0, g.Lx]), np.array([0, 0, g.Ly, g.Ly])
    u, v = fr.velocity(g, F, cx, cy, np.zeros(4, dtype=int))
    assert np.all(u == 0) and np.all(v == 0)
    # a step from a wall stays on it bit for bit, and nothing is clamped
    x, y = 0 * t, t * g.Ly
    u, v = fr.velocity(g, F, x, y, lay)
    xn, yn, clamped, lost = fr.move(g, x, y, u, v, 0.3)
    assert np.array_equal(xn, x) and not lost.any() and not clamped[1:-1].any()


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_linear_psi_gives_uniform_flow(dtype):
    nx, ny, L0 = 64, 32, 80.0
    g = fr.Geom(nx, ny, L0)
    D = L0 / nx
    al, be = 0.7, -1.3
    X, Y = np.meshgrid((np.arange(-1, nx + 1) + 0.5) * D, (np.arange(-1, ny + 1) + 0.5) * D)
    F = (al * X + be * Y)[None]          # the ghost ring continues the plane: "away from the walls" everywhere
    x, y, lay = fr.seeded_floats(g, 1000, 1, seed=3)
    u, v = fr.velocity(g, F, x, y, lay, dtype)
    bar = 8 * EPS * np.abs(F).max() * g.idx
    assert np.abs(u - (-be)).max() <= bar and np.abs(v - al).max() <= bar


def test_velocity_is_non_divergent_inside_a_dual_cell():
    """u depends on x only through a, v on y only through b: du/dx + dv/dy = (-(d11 - d10 - d01 + d00) + (d11 - d01 - d10 + d00)) idx^2 = 0;
    checked by centred differences, which are exact for a field that is linear in each coordinate up to round-off"""
    nx, ny, L0 = 32, 32, 32.0            # Delta = 1: the positions below and their cell coordinates are exact
    g = fr.Geom(nx, ny, L0)
    F = random_ghosted(3, ny, nx, seed=5)
    D = L0 / nx
    rng = np.random.default_rng(7)
    i, j = rng.integers(-1, nx, 200), rng.integers(-1, ny, 200)
    # centres of dual cells, clipped into the box for the half cells of the ring; h keeps x +- h inside the cell
    h = 0.0625 * D
    x = np.clip((i + 1.0) * D, 0.25 * D, L0 - 0.25 * D)
    y = np.clip((j + 1.0) * D, 0.25 * D, L0 - 0.25 * D)
    lay = rng.integers(0, 3, 200)
    ld = np.longdouble
    up, _ = fr.velocity(g, F, x + h, y, lay, ld)
    um, _ = fr.velocity(g, F, x - h, y, lay, ld)
    _, vp = fr.velocity(g, F, x, y + h, lay, ld)
    _, vm = fr.velocity(g, F, x, y - h, lay, ld)
    div = (up - um) / (2 * h) + (vp - vm) / (2 * h)
    scale = np.abs(F).max() * g.idx * g.idx
    assert np.abs(div).max() <= 64 * np.finfo(ld).eps * scale * (D / h)


@pytest.mark.parametrize("nx,ny,periodic", [(32, 32, False), (64, 32, False), (32, 32, True)])
@pytest.mark.parametrize("n", [1, 1000])
def test_seeded_floats_keep_clear_of_cell_lines(nx, ny, periodic, n):
    """the random positions of the GPU tests: the product comparison leaves out floats within 1e-9 of a dual-cell line; none of these is"""
    g = fr.Geom(nx, ny, 80.0, periodic)
    x, y, lay = fr.seeded_floats(g, n, 3)
    assert not fr.near_cell_line(g, x, y).any()
    i64 = fr.locate(g, x, y, np.float64)
    ild = fr.locate(g, x, y, np.longdouble)
    assert np.array_equal(i64[0], ild[0]) and np.array_equal(i64[1], ild[1])
    assert lay.min() >= 0 and lay.max() < 3 and (n == 1 or len(set(lay)) == 3)


def test_indices_and_weights_stay_in_range_and_nan_is_lost():
    for periodic in (False, True):
        for n in (1, 2, 3, 32, 48):
            L = 80.0
            g = fr.Geom(n, n, L, periodic)
            D = L / n
            x = np.array([0.0, L, D / 2, np.nextafter(0.0, 1), np.nextafter(L, 0), np.nextafter(L, 2 * L), 1e300, -1e300, -0.0, -3.7 * L, 1e9 * L])
            i0, a, _ = fr.axis(x, g.idx, n, periodic)
            lo = 0 if periodic else -1
            assert i0.min() >= lo and i0.max() <= n - 1
            assert a.min() >= 0 and a.max() <= 1
            i0, a, _ = fr.axis(np.array([np.nan, np.inf, -np.inf]), g.idx, n, periodic)
            assert np.isnan(a).all()


def test_periodic_wrap_reads_the_same_cell():
    g = fr.Geom(32, 32, 80.0, True)
    F = np.random.default_rng(2).standard_normal((2, 32, 32))
    G = np.pad(F, ((0, 0), (1, 1), (1, 1)), mode="wrap")
    x, y, lay = fr.seeded_floats(fr.Geom(32, 32, 80.0), 500, 2, seed=4)
    u0, v0 = fr.velocity(g, G, x, y, lay, np.longdouble)
    u1, v1 = fr.velocity(g, G, x - 3 * 80.0, y + 2 * 80.0, lay, np.longdouble)
    s = np.abs(G).max() * g.idx
    assert np.abs(u1 - u0).max() <= 1e-9 * s and np.abs(v1 - v0).max() <= 1e-9 * s
