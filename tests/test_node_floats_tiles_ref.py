"""The owner rule and the two-phase migration pass of the vertex model's Lagrangian floats on tiles in their numpy restatement
(tests/node_floats_tiles_ref.py) alone, psi frozen, and what tests/test_gpu_node_floats_tiled.py relies on for the hand-staged case
it runs: enough floats change owner, in every direction and diagonally, none moves farther than a neighbouring tile, and with
messages of two records the floats left behind depend on the cap.  These are conditions on the inputs.  No GPU."""
import functools

import numpy as np
import pytest

import node_floats_ref as nr
import node_floats_tiles_ref as nt

BIG = 10 ** 9


@functools.lru_cache(maxsize=None)
def case():
    return nt.Case()


@functools.lru_cache(maxsize=None)
def run_of(px, py, K=BIG, pick=nt.first_k, seed=0):
    c = case()
    return nt.run(c.tiling(px, py), c.P, c.x, c.y, c.layer, c.dt, nt.NSTEPS, K, pick, seed)


def test_owner_rule_on_seams_walls_and_their_neighbours():
    g = nr.Geom(64, 100.0)
    t = nt.Tiling(g, 2, 4)
    D = 100.0 / 64
    s = 32 * D
    x = np.array([0.0, -0.0, np.nextafter(s, 0), s, np.nextafter(s, 100), 100.0, 31.5 * D])
    col, _, ok, i0, _ = nt.owner(t, x, x)
    # the owner line is the seam itself: on it the float belongs to the upper tile; x = L0 belongs to the last tile
    assert ok.all() and i0.tolist() == [0, 0, 31, 32, 32, 63, 31] and col.tolist() == [0, 0, 0, 1, 1, 1, 0]
    y = np.array([0.0, np.nextafter(16 * D, 0), 16 * D, 32 * D, np.nextafter(48 * D, 0), 48 * D, 100.0])
    _, row, ok, _, j0 = nt.owner(t, y, y)
    assert ok.all() and j0.tolist() == [0, 15, 16, 32, 47, 48, 63] and row.tolist() == [0, 0, 1, 2, 2, 3, 3]
    # the owner's local corners are vertices it holds: [0, tx] x [0, ty], no halo
    li, lj = nt.local_corners(t, *nt.owner(t, x, y)[:2], *nt.owner(t, x, y)[3:])
    assert li.min() >= 0 and (li + 1).max() <= t.tx and lj.min() >= 0 and (lj + 1).max() <= t.ty
    assert (li + 1)[5] == t.tx and (lj + 1)[6] == t.ty          # x = L0 reads column tx, y = L0 row ty
    # not finite: no owner, the float stays where it is
    assert not nt.owner(t, np.array([np.nan, np.inf, 1.0]), np.array([1.0, 1.0, -np.inf]))[2].any()


def test_placed_floats_sit_where_the_issue_asks():
    c = case()
    D = nt.L0 / nt.N
    have = set(zip(c.x[1000:].tolist(), c.y[1000:].tolist()))
    sx, sy = 32 * D, [16 * D, 32 * D, 48 * D]
    for b in sy:
        assert (sx, b) in have                                                  # the cross points
        assert (0.0, b) in have and (nt.L0, b) in have                          # wall vertices at the seam ends
        assert any(y == b and 0 < x < nt.L0 for x, y in have)                  # exactly on a seam
        assert any(y == np.nextafter(b, 0) for _, y in have) and any(y == np.nextafter(b, nt.L0) for _, y in have)
    assert (sx, 0.0) in have and (sx, nt.L0) in have
    assert any(x == sx and 0 < y < nt.L0 for x, y in have)
    assert any(x == np.nextafter(sx, 0) for x, _ in have) and any(x == np.nextafter(sx, nt.L0) for x, _ in have)
    assert any(x == nt.L0 for x, _ in have) and any(y == nt.L0 for _, y in have) and (nt.L0, nt.L0) in have
    # all-land cells on both sides of the vertical seam and of the horizontal seam through the cross point
    la = c.groups["land_at_seam"]
    assert np.all(nr.on_land(c.g, c.mask, c.x[la], c.y[la]))
    i0, j0 = nr.locate(c.g, c.x[la], c.y[la])[:2]
    assert {31, 32} <= set(i0.tolist()) and {31, 32} <= set(j0.tolist())
    assert c.n % 64 and c.n >= 1000 and c.layer.min() == 0 and c.layer.max() == nt.NL - 1


@pytest.mark.parametrize("px,py", nt.TILINGS)
def test_hand_staged_case_moves_floats_between_tiles(px, py):
    c = case()
    pos, wh, per, tot = run_of(px, py)
    print(px, py, c.n, tot)
    assert tot["far"] == 0 and tot["unsent"] == 0          # no float moves farther than a neighbour, down to 32 x 16 cells a tile
    if px > 1:
        assert tot["W"] >= 1 and tot["E"] >= 1
    if py > 1:
        assert tot["S"] >= 1 and tot["N"] >= 1
    if (px, py) == (2, 2):
        assert tot["changed"] >= 50                          # owner changes; the records sent are at least as many
        assert tot["W"] + tot["E"] + tot["S"] + tot["N"] >= tot["changed"]
    if px > 1 and py > 1:
        assert tot["diag"] >= 1
    # a stage moves a float by at most about 0.4 cells
    D = nt.L0 / nt.N
    step = max(np.abs(pos[0][0] - c.x).max(), np.abs(pos[0][1] - c.y).max()) / D
    print("largest move of the first step", step, "cells")
    assert 0.2 <= step <= 0.45
    # every id is held by exactly one rank, the one the owner rule names for the position its next stage evaluates
    assert np.array_equal(wh[-1], nt.home(c.tiling(px, py), *pos[-1]))
    assert not np.isnan(pos[-1][0]).any()
    # the same run on every tiling: the single tile's
    ref = run_of(1, 1)[0]
    for a, b in zip(pos, ref):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_messages_of_two_records_leave_floats_behind_and_which_depends_on_the_cap_and_the_choice():
    """what the cap test on the GPU must cope with: the floats left behind are lost, so which ones a full message leaves decides the
    later traffic and with it the count of a whole run.  So the GPU test follows the run pass by pass and asks, for each, for the
    choice under which the numpy pass leaves behind exactly the floats the device did (explain)"""
    c = case()
    t = c.tiling(2, 2)
    ref = run_of(2, 2)[0][-1]
    left = {}
    for K in (2, 4, BIG):
        pos, wh, per, tot = run_of(2, 2, K)
        lost = np.isnan(pos[-1][0])
        assert lost.sum() == tot["unsent"] and np.array_equal(lost, np.isnan(pos[-1][1])) and tot["far"] == 0
        assert np.array_equal(pos[-1][0][~lost], ref[0][~lost]) and np.array_equal(pos[-1][1][~lost], ref[1][~lost])
        left[K] = frozenset(np.flatnonzero(lost).tolist())
    assert len(left[2]) > 0 and not left[BIG] and left[4] < left[2]
    counts = {run_of(2, 2, 2, pick, seed)[3]["unsent"] for pick, seed in ((nt.first_k, 0), (nt.last_k, 0), (nt.random_k, 1), (nt.random_k, 2))}
    print(sorted(counts))
    # one pass from one state, drawn choices: explain() finds each of them from the floats it left behind
    xh, yh = nr.stage1(c.g, c.P, c.x, c.y, c.layer, c.dt)
    where = nt.home(t, c.x, c.y)
    for seed in range(3):
        w, uns, st = nt.migrate(t, where, xh, yh, 2, nt.random_k, np.random.default_rng(seed))
        got = nt.explain(t, where, xh, yh, 2, uns)
        here = np.ones(c.n, dtype=bool)
        here[uns] = False      # a float left behind stays on the rank the phase found it on, which is not seen; the others are at home
        assert uns.size > 0 and got is not None and np.array_equal(got[0][here], w[here])
        stays = int(np.flatnonzero(here & (w == where))[0])      # a float that wants nowhere cannot have been left behind
        assert nt.explain(t, where, xh, yh, 2, np.append(uns, stays), tries=20) is None
