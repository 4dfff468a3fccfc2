"""Properties of the arithmetic of the vertex model's Lagrangian floats, on the numpy restatement (tests/node_floats_ref.py) that the
GPU tests compare the device with (include/msomn_floats.h): exact zeros on land and on constant edges, the wall column at x = L0, the
non-divergence of the cell's velocity, and that none of the seeded floats of the GPU tests starts on a vertex line.  No GPU."""
import numpy as np
import pytest

import node_floats_ref as nr

L0 = 100.0
DTYPES = [np.float64, np.longdouble]


def field(N, nl=2, seed=3):
    return np.random.default_rng(seed).standard_normal((nl, N + 1, N + 1))


def island_mask(N):
    mk = np.ones((N + 1, N + 1))
    mk[N // 4: N // 4 + 4, N // 2 - 2: N // 2 + 3] = 0
    mk[0, :] = mk[-1, :] = mk[:, 0] = mk[:, -1] = 0
    return mk


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_all_land_cell_has_exactly_zero_velocity(dtype):
    N = 32
    g, mk = nr.Geom(N, L0), island_mask(N)
    P = field(N) * mk
    li, lj = nr.land_cells(mk)
    assert li.size >= 6
    rng = np.random.default_rng(0)
    D = L0 / N
    x, y = (li + rng.uniform(0.01, 0.99, li.size)) * D, (lj + rng.uniform(0.01, 0.99, li.size)) * D
    lay = rng.integers(0, 2, li.size)
    u, v = nr.velocity(g, P, x, y, lay, dtype)
    assert np.all(u == 0) and np.all(v == 0)
    assert np.all(nr.on_land(g, mk, x, y))
    xh, yh = nr.stage1(g, P, x, y, lay, 0.3, dtype)
    assert np.array_equal(xh, x.astype(dtype)) and np.array_equal(yh, y.astype(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_a_constant_edge_has_exactly_zero_normal_velocity(dtype):
    N = 32
    g, mk = nr.Geom(N, L0), island_mask(N)
    P = field(N) * mk + 0.75 * (1 - mk)     # constant, not zero, on the land and the walls
    t = np.array([0.13, 0.5, 0.77, 0.999]) * L0
    z, lay = np.zeros(4), np.array([0, 1, 0, 1])
    for x, y, normal in ((z, t, 0), (z + L0, t, 0), (t, z, 1), (t, z + L0, 1)):
        uv = nr.velocity(g, P, x, y, lay, dtype)
        assert np.all(uv[normal] == 0) and np.any(uv[1 - normal] != 0)
    # a coast edge between two land vertices; L0 = 64 makes Delta = 2 and idx = 1 / 2 exact, so the float lies on the line (a = 0)
    g2 = nr.Geom(N, 64.0)
    edges = nr.coast_edges(mk)
    assert len(edges) >= 4
    for i, j in edges:
        i0, _, a, _, _, _ = nr.locate(g2, np.array([2.0 * i]), np.array([2.0 * (j + 0.4)]), dtype)
        assert i0[0] == i and a[0] == 0
        u, v = nr.velocity(g2, P, np.array([2.0 * i]), np.array([2.0 * (j + 0.4)]), np.array([1]), dtype)
        assert u[0] == 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [1, 2, 3, 32, 64])
def test_x_equal_L0_reads_column_N_with_weight_one(N, dtype):
    for L in (L0, 80.0, 1.0 / 3.0, 7e5):
        g = nr.Geom(N, L)
        i0, j0, a, b, xi, _ = nr.locate(g, np.array([L, 0.0]), np.array([0.0, L]), dtype)
        # idx is rounded in float64: where L * idx comes out above N the clamp makes the weight exactly 1, where it comes out below
        # (only the longdouble product of the float64 idx does, for these L) it is 1 - N eps at the least
        assert i0[0] == N - 1 and j0[1] == N - 1 and a[0] == b[1] and 1 - N * np.finfo(np.float64).eps <= a[0] <= 1
        if dtype is np.float64 or dtype(L) * dtype(g.idx) >= N:
            assert a[0] == 1
        assert i0[1] == 0 and a[1] == 0 and j0[0] == 0 and b[0] == 0
    # the value at the corner (L0, L0) is the vertex (N, N) itself
    g, P = nr.Geom(N, L0), field(N)
    s = nr.sample(g, P, np.array([L0]), np.array([L0]), np.array([1]), dtype)
    if dtype is np.float64:
        assert s[0] == P[1, N, N]
    assert abs(s[0] - dtype(P[1, N, N])) <= 4 * N * np.finfo(np.float64).eps * np.abs(P).max()
    # no finite or infinite input takes the index out of [0, N - 1]
    bad = np.array([-1e300, 1e300, -0.0, np.nextafter(0, -1), np.nextafter(L0, 2 * L0), np.inf, -np.inf, np.nan])
    i0, _, a, _, _, _ = nr.locate(g, bad, bad, dtype)
    assert i0.min() >= 0 and i0.max() <= N - 1 and np.all(np.isnan(a[-3:])) and np.all((a[:-3] >= 0) & (a[:-3] <= 1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_u_depends_on_x_alone_v_on_y_alone_and_the_divergence_is_zero(dtype):
    N = 32
    g, P = nr.Geom(N, L0), field(N)
    D = L0 / N
    rng = np.random.default_rng(1)
    i0, j0 = rng.integers(0, N, 200), rng.integers(0, N, 200)
    lay = rng.integers(0, 2, 200)
    fx, fy = rng.uniform(0.05, 0.95, (2, 200))
    base = nr.velocity(g, P, (i0 + fx) * D, (j0 + fy) * D, lay, dtype)
    for k in range(5):
        # u = -dpsi/dy of the bilinear psi is a function of x alone, v = dpsi/dx of y alone: moved along the other axis inside the cell
        # they keep their bits
        u, _ = nr.velocity(g, P, (i0 + fx) * D, (j0 + rng.uniform(0.05, 0.95, 200)) * D, lay, dtype)
        _, v = nr.velocity(g, P, (i0 + rng.uniform(0.05, 0.95, 200)) * D, (j0 + fy) * D, lay, dtype)
        assert np.array_equal(u, base[0]) and np.array_equal(v, base[1])
    # ... and du/dx + dv/dy = 0: both are linear, so the difference quotient across the cell is the derivative.  Each velocity carries
    # a few roundings of size eps * max |P| * idx, and the quotient divides their difference by the step h
    h = 0.5 * D
    x0, y0 = (i0 + 0.25) * D, (j0 + 0.25) * D
    u0, v0 = nr.velocity(g, P, x0, y0, lay, dtype)
    u1, _ = nr.velocity(g, P, x0 + h, y0, lay, dtype)
    _, v1 = nr.velocity(g, P, x0, y0 + h, lay, dtype)
    div = (u1 - u0) / dtype(h) + (v1 - v0) / dtype(h)
    bar = 64 * np.finfo(dtype).eps * float(np.abs(P).max()) * g.idx / h
    print(dtype.__name__, "max |div|", float(np.abs(div).max()), "bar", bar, "du/dx", float(np.abs((u1 - u0) / dtype(h)).max()))
    assert np.abs(div).max() <= bar and np.abs((u1 - u0) / dtype(h)).max() > 1e6 * bar


@pytest.mark.parametrize("N", [32, 64])
def test_no_seeded_float_of_the_gpu_tests_starts_on_a_vertex_line(N):
    g = nr.Geom(N, L0)
    for n in (1, 1000):
        x, y, lay = nr.seeded_floats(g, n, 3)
        assert not nr.near_vertex_line(g, x, y).any()
        assert lay.min() >= 0 and lay.max() <= 2
    # the placed ones: those on interior vertex lines are few enough for the 1 % rule of the product comparison
    x, y, groups = nr.placed_floats(g, island_mask(N))
    assert (1000 + x.size) % 64 != 0
    assert nr.near_vertex_line(g, x, y).sum() <= 0.01 * (1000 + x.size)
    assert np.all(nr.on_land(g, island_mask(N), x[groups["land"]], y[groups["land"]]))
