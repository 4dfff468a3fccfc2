"""Lagrangian floats on tiles (option floats_tiles, include/msom_floats.h, DESIGN.md section 8k "On tiles"): for every float id the
position on tiles equals the single tile's bit for bit, in both builds, because the per-float code is the same and the owner of a
float reads, from its own cells and its exchanged ghost ring, the very numbers the single tile reads.  The tiles run as host threads
of one process (run_tiled of tests/test_gpu_tiled.py); every floats call is collective, so every rank makes the same calls in the
same order.  The hand-staged case and the migration pass are those of tests/floats_tiles_ref.py, whose properties
tests/test_floats_tiles_ref.py asserts on the CPU.

Cap test: which floats a full message leaves behind is not fixed, and the CPU test shows that the count over a run depends on it.
So the numpy pass is run stage by stage with the choice the device was seen to make (floats_tiles_ref.leaving): it must leave
behind exactly the floats the device did, which fixes the count of every pass and their sum, floats_unsent.  The product build
forms the cell coordinate with a fused multiply-add; the numpy owner rule then rounds once too (lower_corner(fused=True))."""
import functools

import numpy as np
import pytest

import floats_ref as fr
import floats_tiles_ref as ft
from msom_amd import FIELDS as F
from msom_amd import NewQG, QG
from msom_amd.workloads import double_gyre_params, synthetic_psi
from test_gpu_tiled import run_tiled

pytestmark = pytest.mark.gpu

ERR_CONFIG, ERR_STATE = -3, -6
L0, TILE = ft.L0, ft.TILE
PER = "sbc = -1\ntau0 = 0\nbeta = 0\nupg = [0.3,-0.2]\nvpg = [0.1,0.25]\nflsrv = 1\n"
ON = {"floats_tiles": 1}


def params_of(px, py, nl, extra=""):
    gnx, gny = TILE * px, TILE * py
    return double_gyre_params(gnx, nl, extra=(f"Ny = {gny}\n" if gny != gnx else "") + "MGLEVELS = 4\n" + extra)


def single(params, psi, strict, opts=None, pg=None):
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    for k, v in (opts or {}).items():
        g.option(k, v)
    g.set(F["PSI"], psi)
    if pg is not None:
        g.set(F["PSIPG"], pg)
    g.set_const()
    g.set_tnext(float("inf"))
    return g


def window(G, px, py, rank):
    """the part of a ghosted global field [nl][gny + 2][gnx + 2] that tile `rank` holds, ghost ring included"""
    ix, iy = rank % px, rank // px
    tx, ty = (G.shape[2] - 2) // px, (G.shape[1] - 2) // py
    return G[:, iy * ty:(iy + 1) * ty + 2, ix * tx:(ix + 1) * tx + 2]


def same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


# ------------------------------------------------------------------ the premise: the ghost ring of a tile

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 2), (2, 1)])
@pytest.mark.parametrize("kind", ["walls_pg", "periodic_upg"])
def test_ghost_ring_of_a_tile_is_the_single_tiles_window(kind, px, py, strict):
    nl = 2
    gnx, gny = TILE * px, TILE * py
    params = params_of(px, py, nl, PER if kind == "periodic_upg" else "")
    psi = synthetic_psi(nl, gny, gnx, amp=5.0)
    pg = 0.3 * psi[::-1].copy() if kind == "walls_pg" else None
    tx, ty = gnx // px, gny // py

    def pre(g, rank):
        if pg is not None:
            ix, iy = rank % px, rank // px
            g.set(F["PSIPG"], pg[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx])

    def fn(g, rank):
        return g.floats_ghosted(F["PSI"]), g.floats_ghosted(F["PSIPG"])

    out = run_tiled(params, px, py, psi, 1, strict, fn=fn, opts=ON, pre=pre)
    g = single(params, psi, strict, pg=pg)
    g.step()
    P, PG = g.floats_ghosted(F["PSI"]), g.floats_ghosted(F["PSIPG"])
    assert np.abs(PG).max() > 0
    for r in range(px * py):
        tp, tpg = out[r]["extra"]
        assert np.array_equal(tp, window(P, px, py, r)), ("psi", r)
        assert np.array_equal(tpg, window(PG, px, py, r)), ("psipg", r)
    g.close()


# ------------------------------------------------------------------ stages by hand, psi frozen

NSTEPS = 6
COUNTERS = ("floats_clamped", "floats_lost", "floats_migrated", "floats_unsent")


@functools.lru_cache(maxsize=None)
def hand_single(px, py, strict):
    """the single tile's run of the hand-staged case: positions after every stage 2, psi ghosted, the counters"""
    c = ft.Case(px, py)
    g = single(params_of(px, py, c.nl), c.psi, strict, ON)      # on one rank the option has no effect
    g.floats_begin(c.x, c.y, c.layer)
    pos = []
    for _ in range(NSTEPS):
        g.floats_stage(1, c.dt)
        g.floats_stage(2, c.dt)
        pos.append(g.floats_get())
    res = dict(pos=pos, G=g.floats_ghosted(F["PSI"]), clamped=g.param("floats_clamped"), lost=g.param("floats_lost"),
               unsent=g.param("floats_unsent"), migrated=g.param("floats_migrated"), resident=g.param("floats_resident"))
    g.close()
    return c, res


def hand_tiled(c, strict, opts, every_stage=False):
    def fn(g, rank):
        g.floats_begin(c.x, c.y, c.layer)
        n0 = g.param("floats_resident")
        pos = []
        for _ in range(NSTEPS):
            g.floats_stage(1, c.dt)
            if every_stage:
                pos.append(g.floats_get())
            g.floats_stage(2, c.dt)
            pos.append(g.floats_get())
        return dict(pos=pos, n=g.param("floats"), n0=n0, resident=g.param("floats_resident"), **{k: g.param(k) for k in COUNTERS})

    out = run_tiled(params_of(c.px, c.py, c.nl), c.px, c.py, c.psi, 0, strict, fn=fn, opts=opts)
    return [o["extra"] for o in out]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 1), (1, 2), (2, 2), (2, 4)])
def test_hand_stages_on_tiles_equal_the_single_tile_bit_for_bit(px, py, strict):
    c, ref = hand_single(px, py, strict)
    assert ref["unsent"] == 0 and ref["migrated"] == 0 and ref["resident"] == c.n
    out = hand_tiled(c, strict, ON)
    home = ft.home(c.t, c.x, c.y, fused=not strict)
    for r, o in enumerate(out):
        assert o["n"] == c.n and o["n0"] == (home == r).sum()
        for k in range(NSTEPS):
            assert same(o["pos"][k][0], ref["pos"][k][0]) and same(o["pos"][k][1], ref["pos"][k][1]), (r, k)
        assert o["floats_clamped"] == ref["clamped"] and o["floats_lost"] == ref["lost"]
        assert o["floats_unsent"] == 0
        assert o["floats_migrated"] == out[0]["floats_migrated"]
    print(f"{px} x {py}: migrated {out[0]['floats_migrated']}, resident {[o['resident'] for o in out]}, clamped {ref['clamped']}")
    assert out[0]["floats_migrated"] >= 50
    assert sum(o["resident"] for o in out) == c.n
    # the floats did move, and every rank ends with the floats the owner rule gives it
    assert not same(ref["pos"][-1][0], c.x)
    last = ft.home(c.t, *ref["pos"][-1], fused=not strict)
    assert [o["resident"] for o in out] == [(last == r).sum() for r in range(px * py)]


@pytest.mark.parametrize("strict", [True, False])
def test_a_full_message_leaves_floats_behind_as_the_numpy_pass_predicts(strict):
    K = 2
    c, ref = hand_single(2, 2, strict)
    g = single(params_of(2, 2, c.nl), c.psi, strict)

    def half_stage(x, y):
        """(xh, yh) of a stage 1 from (x, y) with the bits of this build: a stage 1 over no time leaves xh = x, the stage 2 behind
        it over dt / 2 is x + (dt / 2) U(x)"""
        fin = np.isfinite(x)
        g.floats_begin(np.where(fin, x, 0.0), np.where(fin, y, 0.0), c.layer)
        g.floats_stage(1, 0.0)
        g.floats_stage(2, c.dt / 2)
        xh, yh = g.floats_get()
        return np.where(fin, xh, np.nan), np.where(fin, yh, np.nan)

    out = hand_tiled(c, strict, dict(ON, floats_msg_cap=K), every_stage=True)
    for o in out[1:]:
        for a, b in zip(o["pos"], out[0]["pos"]):
            assert same(a[0], b[0]) and same(a[1], b[1])
    pos = out[0]["pos"]
    where = ft.home(c.t, c.x, c.y)
    dead = np.zeros(c.n, dtype=bool)
    x, y = c.x.copy(), c.y.copy()
    total = 0
    for k in range(NSTEPS):
        xh, yh = half_stage(x, y)
        if strict:
            for a, b in zip((xh, yh), fr.stage1(c.g, ref["G"], x, y, c.layer, c.dt)):
                assert same(a, b)
        x, y = (a.copy() for a in ref["pos"][k])
        for stage, (hx, hy) in ((1, (xh, yh)), (2, (x, y))):
            seen = pos[2 * k + stage - 1]
            assert np.array_equal(np.isnan(seen[0]), np.isnan(seen[1]))
            gone = np.isnan(seen[0]) & ~np.isnan(ref["pos"][k][0])      # unsent so far, as the device chose
            new = np.flatnonzero(gone & ~dead)
            hx, hy = np.where(dead, np.nan, hx), np.where(dead, np.nan, hy)
            res = ft.explain(c.t, where, hx, hy, K, new, fused=not strict)
            assert res is not None, (k, stage, new, ft.migrate(c.t, where, hx, hy, K, ft.leaving(new), fused=not strict)[1])
            where, uns, st = res
            assert st["far"] == 0
            dead[new] = True
            total += new.size
            if stage == 2:       # every other id: the single tile's bits
                assert same(seen[0][~dead], ref["pos"][k][0][~dead]) and same(seen[1][~dead], ref["pos"][k][1][~dead])
        x[dead], y[dead] = np.nan, np.nan
    print(f"cap {K}: unsent {total}, migrated {out[0]['floats_migrated']}")
    assert total > 0
    for o in out:
        assert o["floats_unsent"] == total
    assert sum(o["resident"] for o in out) == c.n
    assert np.isnan(pos[-1][0][dead]).all() and np.isnan(pos[-1][1][dead]).all()
    g.close()


# ------------------------------------------------------------------ periodic: both neighbours of an axis are one rank

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 2), (2, 1)])
def test_periodic_tiles_carry_unwrapped_floats_across_the_wrap_seam(px, py, strict):
    nl, nsteps = 2, 8
    gnx, gny = TILE * px, TILE * py
    params = params_of(px, py, nl, PER)
    psi = np.zeros((nl, gny, gnx))
    geom = fr.Geom(gnx, gny, L0, periodic=True)
    x0, y0, lay = fr.seeded_floats(geom, 1000, nl)
    x0[:4], y0[:4] = [-3.7 * L0, 2.3 * L0, -0.01, L0], [5.2 * L0, -1.9 * L0, geom.Ly, -0.01]
    dt = 0.45 * (TILE * L0 / gnx) / 0.3          # the fastest component, 0.3, moves a float by 0.45 tiles per step

    def fn(g, rank):
        g.floats_begin(x0, y0, lay)
        pos = []
        for _ in range(nsteps):
            g.floats_stage(1, dt)
            g.floats_stage(2, dt)
            pos.append(g.floats_get())
        return pos, {k: g.param(k) for k in COUNTERS}, g.param("floats_resident")

    out = run_tiled(params, px, py, psi, 0, strict, fn=fn, opts=ON)
    g = single(params, psi, strict)
    g.floats_begin(x0, y0, lay)
    for k in range(nsteps):
        g.floats_stage(1, dt)
        g.floats_stage(2, dt)
        x, y = g.floats_get()
        for o in out:
            assert same(o["extra"][0][k][0], x) and same(o["extra"][0][k][1], y), k
    # every float crossed both seams of the x axis, the wrap seam among them; positions are unwrapped
    assert np.all(np.abs(x - x0) >= 2 * TILE * L0 / gnx * 0.9) and x[0] < -L0 and x[1] > L0
    cnt = out[0]["extra"][1]
    print(f"periodic {px} x {py}: {cnt}")
    assert cnt["floats_unsent"] == 0 and cnt["floats_lost"] == 0 and cnt["floats_clamped"] == 0 and cnt["floats_migrated"] >= 2 * x0.size
    assert sum(o["extra"][2] for o in out) == x0.size
    g.close()


# ------------------------------------------------------------------ msom_step, velocity and sample

def step_floats(nl):
    c = ft.Case(2, 2, nl=nl)
    return c.x, c.y, c.layer


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("async_solve", [1, 0])
def test_msom_step_on_tiles_moves_the_floats_as_the_single_tile(async_solve, strict):
    px = py = 2
    nl, nsteps = 3, 5
    params = params_of(px, py, nl)
    psi = synthetic_psi(nl, TILE * py, TILE * px, amp=5.0)
    x0, y0, lay = step_floats(nl)
    opts = dict(ON, async_solve=async_solve)

    def pre(g, rank):
        g.floats_begin(x0, y0, lay)
        g.floats_record(every=2, capacity=4)

    def fn(g, rank):
        res = dict(pos=g.floats_get(), track=g.floats_track(), vel=g.floats_velocity(), sp=g.floats_sample(F["PSI"]))
        res.update({k: g.param(k) for k in COUNTERS})
        # between a stage 1 and its stage 2 the floats are homed by (xh, yh): velocity and sample are refused, on every rank
        g.floats_stage(1, 0.0)
        s0, s1 = np.empty(x0.size), np.empty(x0.size)
        res["mid"] = (g.L.msom_floats_velocity(g.h, s0.ctypes.data, s1.ctypes.data), g.L.msom_last_error(),
                      g.L.msom_floats_sample(g.h, F["PSI"], s0.ctypes.data))
        g.floats_stage(2, 0.0)
        res["after"] = g.floats_velocity()
        return res

    out = run_tiled(params, px, py, psi, nsteps, strict, fn=fn, opts=opts, pre=pre)
    bare = run_tiled(params, px, py, psi, nsteps, strict, opts={"async_solve": async_solve})
    g = single(params, psi, strict, {"async_solve": async_solve})
    g.floats_begin(x0, y0, lay)
    g.floats_record(every=2, capacity=4)
    dts = [g.step() for _ in range(nsteps)]
    x, y = g.floats_get()
    t, tx, ty = g.floats_track()
    u, v = g.floats_velocity()
    sp = g.floats_sample(F["PSI"])      # a field whose ghost ring the tiles exchange (that of Q they do not: msom_floats.h)
    assert not same(x, x0) and t.size == 3
    for r, o in enumerate(out):
        e = o["extra"]
        assert o["dts"] == dts and bare[r]["dts"] == dts
        assert np.array_equal(o["q"], bare[r]["q"]) and np.array_equal(o["psi"], bare[r]["psi"])      # the model does not see the floats
        assert same(e["pos"][0], x) and same(e["pos"][1], y), r
        assert np.array_equal(e["track"][0], t) and same(e["track"][1], tx) and same(e["track"][2], ty), r
        assert same(e["vel"][0], u) and same(e["vel"][1], v) and same(e["sp"], sp), r
        assert e["mid"][0] == ERR_STATE and b"msom_floats_velocity" in e["mid"][1] and e["mid"][2] == ERR_STATE
        assert same(e["after"][0], u) and same(e["after"][1], v)
        assert e["floats_unsent"] == 0 and e["floats_lost"] == g.param("floats_lost") and e["floats_clamped"] == g.param("floats_clamped")
    print(f"msom_step async_solve {async_solve}: migrated {out[0]['extra']['floats_migrated']}")
    assert out[0]["extra"]["floats_migrated"] > 0
    g.close()


# ------------------------------------------------------------------ guards

@pytest.mark.parametrize("strict", [True, False])
def test_guards_pause_and_a_second_begin_on_tiles(strict):
    px, py, nl = 2, 1, 2
    params = params_of(px, py, nl)
    psi = synthetic_psi(nl, TILE * py, TILE * px, amp=5.0)
    c = ft.Case(px, py)
    x2, y2, l2 = c.x[:100][::-1].copy(), c.y[:100][::-1].copy(), c.layer[:100][::-1].copy()

    def fn(g, rank):
        res = {}
        g.option("floats_tiles", 0)      # without the option: refused as before
        res["off"] = (g.L.msom_floats_begin(g.h, c.n, c.x.ctypes.data, c.y.ctypes.data, c.layer.ctypes.data), g.L.msom_last_error(), g.param("floats"))
        g.option("floats_tiles", 1)
        g.floats_begin(c.x, c.y, c.layer)
        g.option("floats", 0)            # paused on all ranks
        g.step()
        res["paused"] = g.floats_get()
        g.option("floats", 1)
        g.step()
        res["moved"] = g.floats_get()
        g.floats_end()
        res["ended"] = g.param("floats")
        g.floats_begin(x2, y2, l2)
        res["again"] = (g.param("floats"), g.floats_get(), g.param("floats_migrated"))
        return res

    out = run_tiled(params, px, py, psi, 0, strict, fn=fn, opts=ON)
    g = single(params, psi, strict)
    g.floats_begin(c.x, c.y, c.layer)
    g.option("floats", 0)
    g.step()
    g.option("floats", 1)
    g.step()
    x, y = g.floats_get()
    for o in out:
        e = o["extra"]
        assert e["off"][0] == ERR_CONFIG and b"msom_floats_begin: floats that cross tiles are not supported" in e["off"][1] and e["off"][2] == 0
        assert same(e["paused"][0], c.x) and same(e["paused"][1], c.y)
        assert same(e["moved"][0], x) and same(e["moved"][1], y) and not same(x, c.x)
        assert e["ended"] == 0
        assert e["again"][0] == 100 and same(e["again"][1][0], x2) and same(e["again"][1][1], y2) and e["again"][2] == 0
    g.close()


@pytest.mark.parametrize("strict", [True, False])
def test_newqg_stays_refused_with_the_option(strict):
    import newqg_ref as nq

    n = NewQG(nq.sample_par(16, 16).text(), strict=strict)
    n.L.msom_set_option(n.h, b"floats_tiles", 1.0)      # whatever the dialect answers to the option
    one, lay = np.array([0.5]), np.zeros(1, dtype=np.int32)
    assert n.L.msom_floats_begin(n.h, 1, one.ctypes.data, one.ctypes.data, lay.ctypes.data) == ERR_CONFIG
    assert n.L.msom_floats_get(n.h, one.ctypes.data, one.ctypes.data) == ERR_CONFIG
    n.close()


# ------------------------------------------------------------------ the host side the two models share: record slots, begin, the cap

PER3 = "sbc = -1\ntau0 = 0\nbeta = 0\nupg = [0.3,-0.2,0.1]\nvpg = [0.1,0.25,-0.15]\nflsrv = 1\n"
CAP = 40


@functools.lru_cache(maxsize=None)
def shared_case(kind):
    """32 x 32 x 3, 160 floats of which 48 start beside a seam or beside the cell-centre line where the owner changes"""
    nl, gn, n = 3, 32, 160
    params = double_gyre_params(gn, nl, extra="MGLEVELS = 4\n" + (PER3 if kind == "periodic" else ""))
    psi = synthetic_psi(nl, gn, gn, amp=5.0)
    x, y, lay = fr.seeded_floats(fr.Geom(gn, gn, L0, periodic=kind == "periodic"), n, nl, seed=5)
    D = L0 / gn
    x[:24] = L0 / 2 + np.tile([-0.03, 0.02, 0.47, 0.53], 6) * D
    y[:24] = (np.arange(24) + 0.31) * L0 / 24
    y[24:48] = L0 / 2 + np.tile([-0.03, 0.02, 0.47, 0.53], 6) * D
    x[24:48] = (np.arange(24) + 0.31) * L0 / 24
    dmax = max(np.abs(np.diff(psi, axis=1)).max(), np.abs(np.diff(psi, axis=2)).max())
    return params, psi, (x, y, lay), 0.4 * D * D / dmax      # a stage by hand moves a float by at most about 0.4 cells


def shared_calls(g, fl, dt):
    """the calls whose host code the two models share, alike on a single tile and on every rank of a tiling"""
    from test_gpu_hooks import DevBuf

    x, y, lay = fl
    res = dict(cap=[g.param("floats_msg_cap")])      # the option, before any begin
    bufs = [DevBuf(a) for a in fl]
    g._chk(g.L.msom_floats_begin(g.h, x.size, *(b.ptr for b in bufs)))      # from device arrays
    for b in bufs:
        b.free()
    res["cap"].append(g.param("floats_msg_cap"))
    res["n0"] = g.param("floats_resident")
    g.floats_record(every=2, capacity=3)      # records behind steps 2 and 4 fill the buffer, those of steps 6 and 8 are dropped
    res["dts"] = [g.step() for _ in range(8)]
    res.update(records=g.param("floats_records"), dropped=g.param("floats_dropped"), track=g.floats_track(), pos=g.floats_get(),
               cnt={k: g.param(k) for k in COUNTERS}, resident=g.param("floats_resident"))
    g.option("floats_msg_cap", 0)
    g.floats_begin(x[:100], y[:100], lay[:100])      # a second begin with another n: messages and readouts follow it
    res["cap"].append(g.param("floats_msg_cap"))
    g.step()
    res["pos2"] = g.floats_get()
    g.floats_stage(1, dt)
    g.floats_stage(1, dt)      # a stage 1 over a stage 1: the floats are homed by (x, y) again first
    g.floats_stage(2, dt)
    res.update(pos3=g.floats_get(), cnt3={k: g.param(k) for k in COUNTERS}, resident3=g.param("floats_resident"))
    return res


@functools.lru_cache(maxsize=None)
def shared_single(kind, strict):
    params, psi, fl, dt = shared_case(kind)
    g = single(params, psi, strict, dict(ON, floats_msg_cap=CAP))
    res = shared_calls(g, fl, dt)
    g.close()
    return res


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("kind", ["walls", "periodic"])
def test_record_slots_begin_and_the_cap_on_tiles_equal_the_single_tile(kind, px, py, strict):
    params, psi, fl, dt = shared_case(kind)
    n = fl[0].size
    ref = shared_single(kind, strict)
    assert ref["cap"] == [CAP, CAP, 0] and ref["records"] == 3 and ref["dropped"] == 2 and ref["track"][0].size == 3
    assert not same(ref["track"][1][2], ref["track"][1][0]) and not same(ref["pos"][0], ref["track"][1][2]) and not same(ref["pos3"][0], ref["pos2"][0])
    out = [o["extra"] for o in run_tiled(params, px, py, psi, 0, strict, fn=lambda g, rank: shared_calls(g, fl, dt), opts=dict(ON, floats_msg_cap=CAP))]
    for r, o in enumerate(out):
        # the option; K of a begin with it; K of a begin without it: min(n, max(1024, n / 16)) of the second begin's 100 floats
        assert o["cap"] == [CAP, CAP, 100], (r, o["cap"])
        assert o["dts"] == ref["dts"] and o["records"] == 3 and o["dropped"] == 2, r
        assert np.array_equal(o["track"][0], ref["track"][0]) and same(o["track"][1], ref["track"][1]) and same(o["track"][2], ref["track"][2]), r
        for key in ("pos", "pos2", "pos3"):
            assert same(o[key][0], ref[key][0]) and same(o[key][1], ref[key][1]), (r, key)
        for key in ("cnt", "cnt3"):
            assert o[key]["floats_clamped"] == ref[key]["floats_clamped"] and o[key]["floats_lost"] == ref[key]["floats_lost"], (r, key)
            assert o[key]["floats_unsent"] == 0 and o[key]["floats_migrated"] == out[0][key]["floats_migrated"], (r, key)
    print(f"{kind} {px} x {py}: resident {[o['n0'] for o in out]} -> {[o['resident'] for o in out]}, migrated {out[0]['cnt']['floats_migrated']}, "
          f"second begin {[o['resident3'] for o in out]}, migrated {out[0]['cnt3']['floats_migrated']}")
    assert sum(o["n0"] for o in out) == n and sum(o["resident"] for o in out) == n - out[0]["cnt"]["floats_unsent"]
    assert sum(o["resident3"] for o in out) == 100 - out[0]["cnt3"]["floats_unsent"]
    assert out[0]["cnt"]["floats_migrated"] + out[0]["cnt3"]["floats_migrated"] > 0
