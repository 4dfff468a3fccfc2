"""Lagrangian floats of the vertex model on tiles (option floats_tiles, include/msomn_floats.h, DESIGN.md section 8l "On tiles"): for
every float id positions, velocities, samples, records and counters on tiles equal the single tile's bit for bit, in both builds,
because the per-float code is the same and the owner of a float reads, from vertices it holds, the very numbers the single tile
reads.  The tiles run as host threads of one process (run_tiled of tests/test_gpu_node_tiled.py); every floats call is collective, so
every rank makes the same calls in the same order.  The hand-staged case and the migration pass are those of
tests/node_floats_tiles_ref.py, whose properties tests/test_node_floats_tiles_ref.py asserts on the CPU.  No tolerance anywhere: the
single tile is the reference, and tests/test_gpu_node_floats.py holds it to the numpy restatement.

Cap test: which floats a full message leaves behind is not fixed, and the CPU test shows that the count over a run depends on it.
So the numpy pass is run stage by stage with the choice the device was seen to make (floats_tiles_ref.leaving): it must leave
behind exactly the floats the device did, which fixes the count of every pass and their sum, floats_unsent."""
import functools

import numpy as np
import pytest

import node_floats_tiles_ref as nt
from test_gpu_node_tiled import params, run_tiled, single

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CONFIG, ERR_STATE = -1, -3, -6
NSTEPS = nt.NSTEPS
BIG = 10 ** 9
# the tiles gather the levels of 8 cells a side and below; the single tile runs with the passes a tiled handle resolves to off
TILE_OPTS = {"floats_tiles": 1, "mg_coarse": 8}
SINGLE_OPTS = dict({k: 0 for k in ("node_pfused", "node_tile_s", "node_march_s", "node_march", "tiled_relax", "node_corr_fused", "node_rhs_fused")},
                   mg_coarse=8, floats_tiles=1)      # on one tile the option has no effect
COUNTERS = ("floats_clamped", "floats_lost", "floats_on_land", "floats_migrated", "floats_unsent")
PAR = params(nt.N, nt.NL)


@functools.lru_cache(maxsize=None)
def case():
    return nt.Case()


def same(a, b):
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


@functools.lru_cache(maxsize=None)
def hand_single(strict):
    """the single tile's run of the hand-staged case, psi frozen: positions and counters after every step, and the positions behind
    every stage 1 with the bits of this build (a stage 1 over no time leaves xh = x; the stage 2 behind it over dt / 2 is
    x + (dt / 2) U(x), what stage 1 over dt stores as xh)"""
    c = case()
    g, h = single(PAR, c.inp, strict, SINGLE_OPTS), single(PAR, c.inp, strict, SINGLE_OPTS)
    g.floats_begin(c.x, c.y, c.layer)
    assert g.param("floats_tiles") == 1 and g.param("floats_resident") == c.n
    pos, half, cnt = [], [], []
    x, y = c.x, c.y
    for _ in range(NSTEPS):
        fin = np.isfinite(x)
        h.floats_begin(np.where(fin, x, 0.0), np.where(fin, y, 0.0), c.layer)
        h.floats_stage(1, 0.0)
        h.floats_stage(2, c.dt / 2)
        xh, yh = h.floats_get()
        half.append((np.where(fin, xh, np.nan), np.where(fin, yh, np.nan)))
        g.floats_stage(1, c.dt)
        g.floats_stage(2, c.dt)
        x, y = g.floats_get()
        pos.append((x, y))
        cnt.append({k: g.param(k) for k in COUNTERS})
    assert cnt[-1]["floats_migrated"] == 0 and cnt[-1]["floats_unsent"] == 0 and g.param("floats_resident") == c.n
    g.close()
    h.close()
    return dict(pos=pos, half=half, cnt=cnt)


def hand_tiled(px, py, strict, opts, every_stage=False):
    c = case()

    def body(g, rank):
        g.floats_begin(c.x, c.y, c.layer)
        res = dict(n=g.param("floats"), n0=g.param("floats_resident"), m0=g.param("floats_migrated"), K=g.param("floats_msg_cap"), pos=[], cnt=[], resident=[])
        for _ in range(NSTEPS):
            g.floats_stage(1, c.dt)
            if every_stage:
                res["pos"].append(g.floats_get())
            g.floats_stage(2, c.dt)
            res["pos"].append(g.floats_get())
            res["cnt"].append({k: g.param(k) for k in COUNTERS})
            res["resident"].append(g.param("floats_resident"))
        return res

    return run_tiled(PAR, px, py, c.inp, strict, body, opts=opts)


# ------------------------------------------------------------------ stages by hand, psi frozen

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", nt.TILINGS)
def test_hand_stages_on_tiles_equal_the_single_tile_bit_for_bit(px, py, strict):
    c, ref = case(), hand_single(strict)
    t = c.tiling(px, py)
    out = hand_tiled(px, py, strict, TILE_OPTS)
    where = nt.home(t, c.x, c.y)
    sent = 0
    for r, o in enumerate(out):
        assert o["n"] == c.n and o["n0"] == (where == r).sum() and o["m0"] == 0 and o["K"] == 1024
    for k in range(NSTEPS):
        # the numpy pass behind each of the two stages, from the positions the single tile had
        for hx, hy in (ref["half"][k], ref["pos"][k]):
            where, uns, st = nt.migrate(t, where, hx, hy, BIG)
            assert uns.size == 0
            sent += st["W"] + st["E"] + st["S"] + st["N"]
        for r, o in enumerate(out):
            assert same(o["pos"][k][0], ref["pos"][k][0]) and same(o["pos"][k][1], ref["pos"][k][1]), (r, k)
            got, want = o["cnt"][k], ref["cnt"][k]
            print(f"{px} x {py} rank {r} step {k}: {got}, numpy pass sent {sent}")
            for key in ("floats_clamped", "floats_lost", "floats_on_land"):
                assert got[key] == want[key], (r, k, key)
            assert got["floats_migrated"] == sent and got["floats_unsent"] == 0, (r, k)
            assert o["resident"][k] == (where == r).sum(), (r, k)
    assert sent >= 50 and not same(ref["pos"][-1][0], c.x)
    assert ref["cnt"][-1]["floats_on_land"] > 0
    # -0.0 and NaN are compared as bits: the west wall is reached from inside by a clamp, which gives +0
    assert np.array_equal(where, nt.home(t, *ref["pos"][-1]))


# ------------------------------------------------------------------ msomn_step, records, velocity and sample

def step_body(floats):
    c = case()

    def body(g, rank):
        if floats:
            g.floats_begin(c.x, c.y, c.layer)
            g.floats_record(every=1, capacity=4, field="Q")
        dts = []
        for _ in range(3):
            g.step(True)
            dts.append(g.dt)
        s = g.mgstats()
        res = dict(dts=dts, t=g.t, iter=g.iter, st=(s.i, s.resa, s.resb), exchanges=g.param("exchanges"), q=g.get("Q"), psi=g.get("PSI"))
        if not floats:
            return res
        res.update(pos=g.floats_get(), track=g.floats_track(), vel=g.floats_velocity(), sq=g.floats_sample("Q"), sp=g.floats_sample("PSI"),
                   records=g.param("floats_records"), cnt={k: g.param(k) for k in COUNTERS})
        # between a stage 1 and its stage 2 the floats are homed by (xh, yh): velocity and sample are refused, on every rank
        g.floats_stage(1, 0.0)
        a, b = np.empty(c.n), np.empty(c.n)
        res["mid"] = (g.L.msomn_floats_velocity(g.h, a.ctypes.data, b.ctypes.data), g.L.msom_last_error(),
                      g.L.msomn_floats_sample(g.h, g._fid("PSI"), a.ctypes.data), g.L.msom_last_error(),
                      g.L.msomn_floats_record(g.h, 1, 2, g._fid("Q")))
        g.floats_stage(2, 0.0)
        res["after"] = g.floats_velocity()
        return res
    return body


@pytest.mark.parametrize("strict", [True, False])
def test_msomn_step_on_tiles_moves_and_records_the_floats_as_the_single_tile(strict):
    c = case()
    px = py = 2
    out = run_tiled(PAR, px, py, c.inp, strict, step_body(True), opts=TILE_OPTS)
    bare = run_tiled(PAR, px, py, c.inp, strict, step_body(False), opts=TILE_OPTS)
    ref = step_body(True)(single(PAR, c.inp, strict, SINGLE_OPTS), 0)
    t, X, Y, V = ref["track"]
    assert t.size == 4 and ref["records"] == 4 and not same(ref["pos"][0], c.x) and np.isfinite(V).all() and not same(V[3], V[0])
    for r, o in enumerate(out):
        # the model does not see the floats
        for key in ("dts", "t", "iter", "st", "exchanges"):
            assert o[key] == bare[r][key], (r, key)
        assert o["dts"] == ref["dts"] and o["exchanges"] > 0
        assert np.array_equal(o["q"], bare[r]["q"]) and np.array_equal(o["psi"], bare[r]["psi"]), r
        # every id: the single tile's bits
        assert same(o["pos"][0], ref["pos"][0]) and same(o["pos"][1], ref["pos"][1]), r
        assert o["records"] == 4 and np.array_equal(o["track"][0], t), r
        for name, a, b in zip("XYV", o["track"][1:], (X, Y, V)):
            assert same(a, b), (r, name, int((a != b).sum()))
        assert same(o["vel"][0], ref["vel"][0]) and same(o["vel"][1], ref["vel"][1]), r
        assert same(o["sq"], ref["sq"]) and same(o["sp"], ref["sp"]), r
        for key in ("floats_clamped", "floats_lost", "floats_on_land"):
            assert o["cnt"][key] == ref["cnt"][key], (r, key)
        assert o["cnt"]["floats_unsent"] == 0 and o["cnt"]["floats_migrated"] == out[0]["cnt"]["floats_migrated"]
        code_v, msg_v, code_s, msg_s, code_r = o["mid"]
        assert code_v == ERR_STATE and b"msomn_floats_velocity" in msg_v and code_s == ERR_STATE and b"msomn_floats_sample" in msg_s and code_r == ERR_STATE
        assert same(o["after"][0], ref["vel"][0]) and same(o["after"][1], ref["vel"][1]), r
    print("msomn_step on 2 x 2: migrated", out[0]["cnt"]["floats_migrated"], "on land", ref["cnt"]["floats_on_land"])
    assert out[0]["cnt"]["floats_migrated"] > 0


# ------------------------------------------------------------------ the cap

@pytest.mark.parametrize("strict", [True, False])
def test_a_full_message_leaves_floats_behind_as_the_numpy_pass_predicts(strict):
    K = 2
    c, ref = case(), hand_single(strict)
    t = c.tiling(2, 2)
    out = hand_tiled(2, 2, strict, dict(TILE_OPTS, floats_msg_cap=K), every_stage=True)
    for o in out:
        assert o["K"] == K
        for a, b in zip(o["pos"], out[0]["pos"]):
            assert same(a[0], b[0]) and same(a[1], b[1])
    pos = out[0]["pos"]
    where = nt.home(t, c.x, c.y)
    dead = np.zeros(c.n, dtype=bool)
    total = sent = 0
    for k in range(NSTEPS):
        for stage, (hx, hy) in ((1, ref["half"][k]), (2, ref["pos"][k])):
            seen = pos[2 * k + stage - 1]
            assert np.array_equal(np.isnan(seen[0]), np.isnan(seen[1]))
            gone = np.isnan(seen[0]) & ~np.isnan(ref["pos"][k][0])      # unsent so far, as the device chose
            assert not (dead & ~gone).any()                              # NaN stays NaN
            new = np.flatnonzero(gone & ~dead)
            hx, hy = np.where(dead, np.nan, hx), np.where(dead, np.nan, hy)
            res = nt.explain(t, where, hx, hy, K, new)
            assert res is not None, (k, stage, new, nt.migrate(t, where, hx, hy, K, nt.leaving(new))[1])
            where, uns, st = res
            assert st["far"] == 0
            sent += st["W"] + st["E"] + st["S"] + st["N"]
            dead[new] = True
            total += new.size
            if stage == 2:       # every other id: the single tile's bits
                assert same(seen[0][~dead], ref["pos"][k][0][~dead]) and same(seen[1][~dead], ref["pos"][k][1][~dead])
        for o in out:
            assert o["cnt"][k]["floats_unsent"] == total and o["cnt"][k]["floats_migrated"] == sent, k
            assert o["cnt"][k]["floats_lost"] == ref["cnt"][k]["floats_lost"]
    print(f"cap {K}: unsent {total}, migrated {sent}")
    assert total > 0
    assert sum(o["resident"][-1] for o in out) == c.n
    assert np.isnan(pos[-1][0][dead]).all() and np.isnan(pos[-1][1][dead]).all()


# ------------------------------------------------------------------ guards

@pytest.mark.parametrize("strict", [True, False])
def test_guards_on_tiles(strict):
    c = case()
    x2, y2, l2 = c.x[:100][::-1].copy(), c.y[:100][::-1].copy(), c.layer[:100][::-1].copy()
    bad = c.x.copy()
    bad[3] = np.nan

    def begin(g, n, x, y, lay):
        return g.L.msomn_floats_begin(g.h, n, x.ctypes.data, y.ctypes.data, lay.ctypes.data), g.L.msom_last_error()

    def body(g, rank):
        res = {}
        g.set_option("floats_msg_cap", 7)    # a cap that is no int is refused, as on a layered handle, and the option stays
        res["cap"] = (g.L.msomn_set_option(g.h, b"floats_msg_cap", 2e8), g.L.msom_last_error(), g.param("floats_msg_cap"))
        g.set_option("floats_msg_cap", 0)
        g.set_option("floats_tiles", 0)      # without the option: refused as before
        res["off"] = begin(g, c.n, c.x, c.y, c.layer) + (g.param("floats"), g.param("floats_tiles"))
        g.set_option("floats_tiles", 1)
        # ranks that do not pass the same floats all leave before a float message is posted
        res["n"] = begin(g, c.n - rank, c.x, c.y, c.layer) + (g.param("floats"),)
        res["bad"] = begin(g, c.n, bad if rank == 1 else c.x, c.y, c.layer) + (g.param("floats"),)
        g.floats_begin(c.x, c.y, c.layer)
        g.set_option("floats", 0)            # paused on all ranks
        g.step(True)
        res["paused"] = g.floats_get()
        g.set_option("floats", 1)
        g.step(True)
        res["moved"] = g.floats_get()
        g.floats_end()
        res["ended"] = g.param("floats")
        g.floats_begin(x2, y2, l2)
        res["again"] = (g.param("floats"), g.floats_get(), g.param("floats_migrated"), g.param("floats_records"))
        g.set_const()                        # drops the floats
        a = np.empty(100)
        res["dropped"] = (g.param("floats"), g.L.msomn_floats_get(g.h, a.ctypes.data, a.ctypes.data), g.L.msom_last_error())
        return res

    out = run_tiled(PAR, 2, 1, c.inp, strict, body, opts=TILE_OPTS)
    g = single(PAR, c.inp, strict, SINGLE_OPTS)
    g.floats_begin(c.x, c.y, c.layer)
    g.set_option("floats", 0)
    g.step(True)
    g.set_option("floats", 1)
    g.step(True)
    x, y = g.floats_get()
    g.close()
    for r, o in enumerate(out):
        assert o["cap"][0] == ERR_ARG and b"option floats_msg_cap" in o["cap"][1] and o["cap"][2] == 7, (r, o["cap"])
        assert o["off"][0] == ERR_CONFIG and b"msomn_floats_begin is not available on a tiled" in o["off"][1] and o["off"][2:] == (0, 0), r
        assert o["n"][0] == ERR_ARG and b"msomn_floats_begin: n = " in o["n"][1] and o["n"][2] == 0, (r, o["n"])
        assert o["bad"][0] == ERR_ARG and o["bad"][2] == 0 and (b"msomn_floats_begin: float 3" if r == 1 else b"another rank refuses") in o["bad"][1], (r, o["bad"])
        assert same(o["paused"][0], c.x) and same(o["paused"][1], c.y)
        assert same(o["moved"][0], x) and same(o["moved"][1], y) and not same(x, c.x)
        assert o["ended"] == 0
        assert o["again"][0] == 100 and same(o["again"][1][0], x2) and same(o["again"][1][1], y2) and o["again"][2:] == (0, 0)
        assert o["dropped"][0] == 0 and o["dropped"][1] == ERR_STATE and b"msomn_floats_get" in o["dropped"][2]


@pytest.mark.parametrize("strict", [True, False])
def test_a_one_by_one_tiled_handle_with_the_option_behaves_as_the_plain_one(strict):
    c, ref = case(), hand_single(strict)

    def body(g, rank):
        g.floats_begin(c.x, c.y, c.layer)
        pos = []
        for _ in range(2):
            g.floats_stage(1, c.dt)
            u = g.floats_velocity()          # one tile: allowed between the stages, as on the plain handle
            g.floats_stage(2, c.dt)
            pos.append(g.floats_get())
        return dict(pos=pos, u=u, cnt={k: g.param(k) for k in COUNTERS}, resident=g.param("floats_resident"), tiles=g.param("floats_tiles"))

    (o,) = run_tiled(PAR, 1, 1, c.inp, strict, body, opts={"floats_tiles": 1})
    for k in range(2):
        assert same(o["pos"][k][0], ref["pos"][k][0]) and same(o["pos"][k][1], ref["pos"][k][1])
    assert o["cnt"] == ref["cnt"][1] and o["resident"] == c.n and o["tiles"] == 1 and np.isfinite(o["u"][0]).all()


# ------------------------------------------------------------------ the host side the two models share: record slots, begin, the cap

CAP = 40
N32 = 32
PAR32 = params(N32, nt.NL)


@functools.lru_cache(maxsize=None)
def shared_case():
    """N = 32, 3 layers, 160 floats of which 48 start beside a seam of 2 tiles a side"""
    import node_floats_ref as nr
    from test_gpu_node_tiled import inputs

    inp = inputs(N32, nt.NL)
    geom = nr.Geom(N32, nt.L0)
    x, y, lay = nr.seeded_floats(geom, 160, nt.NL, seed=5)
    D = nt.L0 / N32
    x[:24] = nt.L0 / 2 + np.tile([-0.03, 0.02, -0.4, 0.45], 6) * D
    y[:24] = (np.arange(24) + 0.31) * nt.L0 / 24
    y[24:48] = nt.L0 / 2 + np.tile([-0.03, 0.02, -0.4, 0.45], 6) * D
    x[24:48] = (np.arange(24) + 0.31) * nt.L0 / 24
    return inp, (x, y, lay), nt.stage_dt(geom, inp["PSI"] + inp["PSIPG"])


def shared_calls(g, rank, field):
    """the calls whose host code the two models share, alike on a single tile (rank -1) and on every rank of a tiling"""
    import ctypes

    from test_gpu_hooks import DevBuf

    _, fl, dt = shared_case()
    x, y, lay = fl
    n = x.size
    res = dict(cap=[g.param("floats_msg_cap")])      # the option, before any begin
    bufs = [DevBuf(a) for a in fl]
    g._chk(g.L.msomn_floats_begin(g.h, n, *(b.ptr for b in bufs)))      # from device arrays
    for b in bufs:
        b.free()
    res["cap"].append(g.param("floats_msg_cap"))
    res["n0"] = g.param("floats_resident")
    g.floats_record(every=2, capacity=3, field=field)      # records behind steps 2 and 4 fill the buffer, those of steps 6 and 8 are dropped
    res["dts"] = []
    for _ in range(8):
        g.step(True)
        res["dts"].append(g.dt)
    res.update(records=g.param("floats_records"), dropped=g.param("floats_dropped"))
    # every rank makes the same gathers, whatever arrays it leaves out: rank 0 passes no x, rank 1 no val (no y when no field is recorded)
    t, X, Y, V = np.empty(3), np.full((3, n), -1.0), np.full((3, n), -1.0), np.full((3, n), -1.0)
    take = dict(x=rank != 0, y=not (rank == 1 and field is None), val=field is not None and rank != 1)
    ptr = lambda a, on: a.ctypes.data if on else None
    g._chk(g.L.msomn_floats_track(g.h, 0, 3, t.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ptr(X, take["x"]), ptr(Y, take["y"]), ptr(V, take["val"])))
    res.update(take=take, track=dict(t=t, x=X, y=Y, val=V), pos=g.floats_get(), cnt={k: g.param(k) for k in COUNTERS}, resident=g.param("floats_resident"))
    g.set_option("floats_msg_cap", 0)
    g.floats_begin(x[:100], y[:100], lay[:100])      # a second begin with another n: messages and readouts follow it
    res["cap"].append(g.param("floats_msg_cap"))
    g.step(True)
    res["pos2"] = g.floats_get()
    g.floats_stage(1, dt)
    g.floats_stage(1, dt)      # a stage 1 over a stage 1: the floats are homed by (x, y) again first
    g.floats_stage(2, dt)
    res.update(pos3=g.floats_get(), cnt3={k: g.param(k) for k in COUNTERS}, resident3=g.param("floats_resident"))
    return res


@functools.lru_cache(maxsize=None)
def shared_single(field, strict):
    g = single(PAR32, shared_case()[0], strict, dict(SINGLE_OPTS, floats_msg_cap=CAP))
    res = shared_calls(g, -1, field)
    g.close()
    return res


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("field", [None, "Q"])
def test_record_slots_begin_and_the_cap_on_tiles_equal_the_single_tile(field, px, py, strict):
    inp, fl, _ = shared_case()
    n = fl[0].size
    ref = shared_single(field, strict)
    assert ref["cap"] == [CAP, CAP, 0] and ref["records"] == 3 and ref["dropped"] == 2
    assert not same(ref["track"]["x"][2], ref["track"]["x"][0]) and not same(ref["pos"][0], ref["track"]["x"][2]) and not same(ref["pos3"][0], ref["pos2"][0])
    assert field is None or (np.isfinite(ref["track"]["val"]).all() and not same(ref["track"]["val"][2], ref["track"]["val"][0]))
    out = run_tiled(PAR32, px, py, inp, strict, lambda g, rank: shared_calls(g, rank, field), opts=dict(TILE_OPTS, floats_msg_cap=CAP))
    for r, o in enumerate(out):
        # the option; K of a begin with it; K of a begin without it: min(n, max(1024, n / 16)) of the second begin's 100 floats
        assert o["cap"] == [CAP, CAP, 100], (r, o["cap"])
        assert o["dts"] == ref["dts"] and o["records"] == 3 and o["dropped"] == 2, r
        assert np.array_equal(o["track"]["t"], ref["track"]["t"]), r
        for key, on in o["take"].items():      # an array that was passed: the single tile's; one that was not: untouched
            assert same(o["track"][key], ref["track"][key]) if on else (o["track"][key] == -1.0).all(), (r, key)
        for key in ("pos", "pos2", "pos3"):
            assert same(o[key][0], ref[key][0]) and same(o[key][1], ref[key][1]), (r, key)
        for key in ("cnt", "cnt3"):
            for c in ("floats_clamped", "floats_lost", "floats_on_land"):
                assert o[key][c] == ref[key][c], (r, key, c)
            assert o[key]["floats_unsent"] == 0 and o[key]["floats_migrated"] == out[0][key]["floats_migrated"], (r, key)
    print(f"field {field} {px} x {py}: resident {[o['n0'] for o in out]} -> {[o['resident'] for o in out]}, migrated {out[0]['cnt']['floats_migrated']}, "
          f"second begin {[o['resident3'] for o in out]}, migrated {out[0]['cnt3']['floats_migrated']}")
    assert sum(o["n0"] for o in out) == n and sum(o["resident"] for o in out) == n - out[0]["cnt"]["floats_unsent"]
    assert sum(o["resident3"] for o in out) == 100 - out[0]["cnt3"]["floats_unsent"]
    assert out[0]["cnt"]["floats_migrated"] + out[0]["cnt3"]["floats_migrated"] > 0
