"""The owner rule and the two-phase migration pass of the Lagrangian floats on tiles in their numpy restatement
(tests/floats_tiles_ref.py) alone, psi frozen, and what tests/test_gpu_floats_tiled.py relies on for the hand-staged case it runs:
enough floats change owner, in every direction and diagonally, and none moves farther than a neighbouring tile.  No GPU."""
import numpy as np
import pytest

import floats_ref as fr
import floats_tiles_ref as ft

NSTEPS = 6
BIG = 10 ** 9


_runs = {}


def run_of(px, py, K=BIG, pick=ft.first_k, seed=0):
    key = (px, py, K, pick.__name__, seed)
    if key not in _runs:
        c = ft.Case(px, py)
        _runs[key] = (c,) + ft.run(c.t, c.G, c.x, c.y, c.layer, c.dt, NSTEPS, K, pick, seed)
    return _runs[key]


def test_owner_rule_on_seams_walls_and_centre_lines():
    g = fr.Geom(32, 32, ft.L0)
    t = ft.Tiling(g, 2, 2)
    D = ft.L0 / 32
    # the owner changes where i0 does: on the cell-centre line half a cell beyond the seam, not on the seam
    x = np.array([0.0, 16 * D, np.nextafter(16.5 * D, 0), 16.5 * D, 17 * D, ft.L0, 15.5 * D])
    col, row, ok, i0, j0 = ft.owner(t, x, x[::-1].copy())
    assert ok.all() and i0.tolist() == [-1, 15, 15, 16, 16, 31, 15]
    assert col.tolist() == [0, 0, 0, 1, 1, 1, 0] and row.tolist() == col[::-1].tolist()
    # the owner's local corners lie in its ghost ring
    for own, i in ((col, i0), (row, j0)):
        lo = i - own * t.tnx
        assert lo.min() >= -1 and (lo + 1).max() <= t.tnx
    # not finite: no owner, the float stays where it is
    assert not ft.owner(t, np.array([np.nan, np.inf, 1.0]), np.array([1.0, 1.0, -np.inf]))[2].any()
    # periodic: wrapped into [0, gnx - 1] first
    tp = ft.Tiling(fr.Geom(32, 32, ft.L0, periodic=True), 2, 2)
    col, row, ok, i0, _ = ft.owner(tp, np.array([-0.25 * D, -3.7 * ft.L0, 1e9 * ft.L0, ft.L0 + 0.6 * D]), np.zeros(4))
    assert ok.all() and i0[0] == 31 and i0[3] == 0 and col.tolist()[0] == 1 and col.tolist()[3] == 0 and set(col) <= {0, 1} and np.all(row == 1)


def test_hop_names_the_neighbour_or_says_farther():
    assert ft.hop([0, 1, 2, 3], [1, 1, 1, 1], 4, False).tolist() == [-1, 0, 1, 2]
    assert ft.hop([3, 0], [0, 3], 4, True).tolist() == [-1, 1]            # across the wrap seam
    assert ft.hop([1, 0], [0, 1], 2, True).tolist() == [1, 1]             # both neighbours are one tile: the upper message
    assert ft.hop([0], [0], 1, True).tolist() == [0]
    assert ft.hop([2], [0], 4, True).tolist() == [2]


def test_fused_cell_coordinate_differs_only_within_an_ulp_of_a_line():
    g = fr.Geom(32, 32, ft.L0)
    x, _, _ = fr.seeded_floats(g, 1000, 2, seed=11)
    a, _ = ft.lower_corner(x, g.idx, 32, False)
    b, _ = ft.lower_corner(x, g.idx, 32, False, fused=True)
    assert np.array_equal(a, b)


@pytest.mark.parametrize("px,py", [(2, 2), (2, 1), (1, 2), (2, 4)])
def test_hand_staged_case_moves_floats_between_tiles(px, py):
    c, pos, wh, tot = run_of(px, py)
    print(px, py, c.n, tot)
    assert c.n % 64 and c.n >= 1000
    assert tot["far"] == 0 and tot["unsent"] == 0          # no float moves farther than a neighbour
    assert tot["changed"] >= 50                              # owner changes; the records sent are at least as many
    assert tot["W"] + tot["E"] + tot["S"] + tot["N"] >= tot["changed"]
    if px > 1:
        assert tot["W"] >= 1 and tot["E"] >= 1
    if py > 1:
        assert tot["S"] >= 1 and tot["N"] >= 1
    if px > 1 and py > 1:
        assert tot["diag"] >= 1
    # a stage moves a float by at most about 0.4 cells
    D = ft.L0 / c.nx
    step = max(np.abs(pos[0][0] - c.x).max(), np.abs(pos[0][1] - c.y).max()) / D
    assert 0.2 <= step <= 0.45
    # every id is held by exactly one rank, the one the owner rule names for the position its next stage evaluates
    assert np.array_equal(wh[-1], ft.home(c.t, *pos[-1]))
    assert not np.isnan(pos[-1][0]).any()


def test_placed_floats_sit_where_the_issue_asks():
    c = ft.Case(2, 2)
    D = ft.L0 / 32
    s = 16 * D
    have = set(zip(c.x[1000:].tolist(), c.y[1000:].tolist()))
    assert (s, s) in have                                             # the corner of four tiles
    assert (s, 0.0) in have and (0.0, s) in have and (s, c.g.Ly) in have and (c.g.Lx, s) in have      # a wall at a seam
    assert any(x == s and 0 < y < c.g.Ly for x, y in have) and any(y == s and 0 < x < c.g.Lx for x, y in have)      # on the seams
    for line in (s - 0.5 * D, s + 0.5 * D):                          # the cell-centre lines on either side of a seam
        assert any(x == line for x, _ in have) and any(y == line for _, y in have)


def test_a_message_of_two_records_leaves_floats_behind_and_the_count_depends_on_which():
    """what the cap test on the GPU must cope with: the floats left behind are lost, so which ones a full message leaves decides
    the later traffic and with it the count of a whole run.  So the GPU test follows the run pass by pass and asks, for each, for the
    choice under which the numpy pass leaves behind exactly the floats the device did (explain)"""
    counts = set()
    for pick, seed in ((ft.first_k, 0), (ft.last_k, 0), (ft.random_k, 1), (ft.random_k, 2), (ft.random_k, 3)):
        c, pos, wh, tot = run_of(2, 2, 2, pick, seed)
        assert tot["unsent"] > 0 and tot["far"] == 0
        lost = np.isnan(pos[-1][0])
        assert lost.sum() == tot["unsent"] and np.array_equal(lost, np.isnan(pos[-1][1]))
        # every other float is where the uncapped run has it
        ref = run_of(2, 2)[1][-1]
        assert np.array_equal(pos[-1][0][~lost], ref[0][~lost]) and np.array_equal(pos[-1][1][~lost], ref[1][~lost])
        counts.add(tot["unsent"])
    print(sorted(counts))
    assert len(counts) > 1
    # one pass from one state, drawn choices: explain() finds each of them from the floats it left behind
    c = ft.Case(2, 2)
    xh, yh = fr.stage1(c.g, c.G, c.x, c.y, c.layer, c.dt)
    where = ft.home(c.t, c.x, c.y)
    for seed in range(4):
        w, uns, st = ft.migrate(c.t, where, xh, yh, 2, ft.random_k, np.random.default_rng(seed))
        got = ft.explain(c.t, where, xh, yh, 2, uns)
        here = np.ones(c.n, dtype=bool)
        here[uns] = False      # a float left behind stays on the rank the phase found it on, which is not seen; the others are at home
        assert uns.size > 0 and got is not None and np.array_equal(got[0][here], w[here])
        stays = int(np.flatnonzero(here & (w == where))[0])      # a float that wants nowhere cannot have been left behind
        assert ft.explain(c.t, where, xh, yh, 2, np.append(uns, stays), tries=20) is None
