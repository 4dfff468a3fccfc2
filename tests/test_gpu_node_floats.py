"""Lagrangian floats of the vertex-grid model on the device (msomn_floats_*, include/msomn_floats.h) against
tests/node_floats_ref.py, the numpy restatement of the header's formulas, fed with the vertex fields NodeQG.get returns.

Strict build: the bits of the float64 restatement, floats on the walls, in the corners, on vertex lines and vertices, on land and on
a coast edge included.  Product build: max |device - longdouble restatement| <= max(16 d_ref, 64 eps S) (hold() of
tests/test_gpu_floats.py), d_ref the distance of the float64 restatement from the longdouble one on the same input and S the scale
of the output.  Floats whose cell coordinate lies within 1e-9 of an interior vertex line in the longdouble run are left out of the
product comparison (a different floor is a different cell); at most 1 % may be, and tests/test_node_floats_ref.py shows that none of
the seeded ones and few enough of the placed ones are at the start."""
import ctypes
import functools
import os

import numpy as np
import pytest

import node_floats_ref as nr
import orn
from msom_amd import MsomError, NodeQG, node_from_state
from test_gpu_floats import hold
from test_gpu_node_tiled import inputs, params, run_tiled
from test_oracle_sqg_kat import bs_field, sqg_params

pytestmark = pytest.mark.gpu

LD = np.longdouble
ERR_ARG, ERR_CONFIG, ERR_STATE = -1, -3, -6
# name: N, nl.  island: TOPO and PSIPG, the mask of the tiled tests; plain: the same without PSIPG; baro: one layer with gp_low;
# sqg: the surface-QG variant with its surface buoyancy
SHAPES = {"island": (64, 3), "plain": (64, 3), "baro": (32, 1), "sqg": (32, 2)}


@functools.lru_cache(maxsize=None)
def setup(shape):
    N, nl = SHAPES[shape]
    if shape == "sqg":
        mk = np.ones((1, N + 1, N + 1))
        mk[0, N // 4: N // 4 + N // 8 + 1, N // 2: N // 2 + N // 8] = 0
        mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
        return sqg_params(N, nl, extra="tau1 = 5e-4\ntf1 = 0.3\ntf2 = 0.7\nTOLERANCE = 1e-9\n"), dict(MASK=mk, BS=bs_field(N), PSI=orn.node_psi(nl, N) * mk)
    inp = dict(inputs(N, nl))
    if shape == "plain":
        del inp["PSIPG"]
    return params(N, nl, tol=1e-9), inp


def make(shape, strict, const=True):
    par, inp = setup(shape)
    g = NodeQG(par, strict=strict)
    g.set_option("quiet", 1)
    for f, a in inp.items():
        g.set(f, a)
    if const:
        g.set_const()
        g.set_tnext(float("inf"))
    g.pg = "PSIPG" in inp
    return g, nr.Geom(g.N, g.param("L0")), inp["MASK"][0]


def stream(g):
    """what the velocity is taken from: psi, or psi + psipg"""
    return g.get("PSI") + g.get("PSIPG") if g.pg else g.get("PSI")


def floats_of(geom, mask, n, nl):
    """the seeded floats, and for n > 1 the placed ones behind them; the groups of the placed ones as index arrays"""
    x, y, lay = nr.seeded_floats(geom, n, nl)
    groups = {}
    if n > 1:
        px, py, groups = nr.placed_floats(geom, mask)
        groups = {k: v + n for k, v in groups.items()}
        x, y = np.concatenate([x, px]), np.concatenate([y, py])
        lay = np.concatenate([lay, (np.arange(px.size) % nl).astype(np.int32)])
        assert x.size % 64
    return x, y, lay, groups


# ------------------------------------------------------------------ 1. the operator

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_velocity_and_sample_equal_the_restatement(shape, n, strict):
    g, geom, mask = make(shape, strict)
    g.step()
    x, y, lay, groups = floats_of(geom, mask, n, g.nl)
    g.floats_begin(x, y, lay)
    assert g.param("floats") == x.size and g.param("floats_lost") == 0 and g.param("floats_clamped") == 0
    gx, gy = g.floats_get()
    assert np.array_equal(gx, x) and np.array_equal(gy, y)
    keep = ~nr.near_vertex_line(geom, x, y)
    P = stream(g)
    u, v = g.floats_velocity()
    scale = float(np.abs(np.concatenate(nr.velocity(geom, P, x, y, lay, LD))).max())
    hold(f"{shape} velocity", (u, v), lambda dt: nr.velocity(geom, P, x, y, lay, dt), strict, scale, keep)
    for name in ("PSI", "Q"):
        G = g.get(name)
        s = g.floats_sample(name)
        hold(f"{shape} sample {name}", (s,), lambda dt: (nr.sample(geom, G, x, y, lay, dt),), strict, float(np.abs(G).max()), keep)
    if n > 1 and not g.pg:   # both builds: the exact zeros of the header (psi is masked: constant on the walls and on land; psi_pg is not)
        for k in ("west", "east"):
            assert np.all(u[groups[k]] == 0), k
        for k in ("south", "north"):
            assert np.all(v[groups[k]] == 0), k
        assert np.all(u[groups["corners"]] == 0) and np.all(v[groups["corners"]] == 0)
        assert np.all(u[groups["land"]] == 0) and np.all(v[groups["land"]] == 0)
        assert np.all(u[groups["coast"]] == 0) or abs(x[groups["coast"]][0] * geom.idx - round(x[groups["coast"]][0] * geom.idx)) > 0
        assert np.any(u != 0) and np.any(v != 0)
    g.close()


# ------------------------------------------------------------------ 2. by hand, 3. msomn_step = by hand

def hand_step(g, geom, lay, strict, what):
    """one RK2 step through update / floats_stage(1) / advance / update / advance / floats_stage(2), each stage held to the restatement
    fed with the psi fetched just before it; returns dt"""
    x0, y0 = g.floats_get()
    dt = g.update("Q", "DQ")
    P1 = stream(g)
    g.floats_stage(1, dt)
    g.advance("QPRED", "Q", "DQ", dt / 2)
    g.update("QPRED", "DQ", dt)
    g.advance("Q", "Q", "DQ", dt)
    P2 = stream(g)
    g.floats_stage(2, dt)
    x1, y1 = g.floats_get()

    def ref(dtype):
        xh, yh = nr.stage1(geom, P1, x0, y0, lay, dt, dtype)
        return nr.stage2(geom, P2, x0, y0, xh, yh, lay, dt, dtype)

    xh, yh = nr.stage1(geom, P1, x0, y0, lay, dt, LD)
    keep = ~(nr.near_vertex_line(geom, x0, y0) | nr.near_vertex_line(geom, xh, yh))
    hold(what, (x1, y1), ref, strict, geom.L0, keep)
    return dt


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stages_by_hand_equal_the_restatement(shape, n, strict):
    g, geom, mask = make(shape, strict)
    x, y, lay, _ = floats_of(geom, mask, n, g.nl)
    g.floats_begin(x, y, lay)
    for k in range(3):
        hand_step(g, geom, lay, strict, f"{shape} step {k}")
    x1, y1 = g.floats_get()
    assert np.abs(x1 - x).max() + np.abs(y1 - y).max() > 0   # they did move
    assert g.param("floats_lost") == 0
    g.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_step_moves_the_floats_as_the_stages_by_hand_and_leaves_the_model_alone(shape, strict):
    a, geom, mask = make(shape, strict)    # step() with floats
    b, _, _ = make(shape, strict)          # the stages by hand
    c, _, _ = make(shape, strict)          # step() without floats
    x, y, lay, _ = floats_of(geom, mask, 1000, a.nl)
    for m in (a, b):
        m.floats_begin(x, y, lay)
    for k in range(3):
        a.step()
        c.step()
        dt_b = hand_step(b, geom, lay, strict, f"{shape} step {k}")
        assert a.dt == dt_b == c.dt
        for p, q in zip(a.floats_get(), b.floats_get()):
            assert np.array_equal(p, q, equal_nan=True)
    for f in ("Q", "PSI"):
        assert np.array_equal(a.get(f), c.get(f)) and np.array_equal(a.get(f), b.get(f)), f
    sa, sc = a.mgstats(), c.mgstats()
    assert a.t == c.t and a.iter == c.iter and (sa.i, sa.resa, sa.resb) == (sc.i, sc.resa, sc.resb)
    assert c.param("floats") == 0 and c.param("floats_records") == 0 and c.param("floats_clamped") == 0 and c.param("floats_on_land") == 0
    for m in (a, b, c):
        m.close()


# ------------------------------------------------------------------ 4. land and walls

@pytest.mark.parametrize("strict", [True, False])
def test_land_and_walls(strict):
    g, geom, mask = make("plain", strict)
    x, y, lay, gr = floats_of(geom, mask, 1000, g.nl)
    g.floats_begin(x, y, lay)
    want_land = int(nr.on_land(geom, mask, x, y).sum())
    assert want_land >= gr["land"].size and np.all(nr.on_land(geom, mask, x[gr["land"]], y[gr["land"]]))
    assert g.param("floats_on_land") == want_land
    for _ in range(5):
        g.step()
    x1, y1 = g.floats_get()
    L = geom.L0
    assert np.array_equal(x1[gr["land"]], x[gr["land"]]) and np.array_equal(y1[gr["land"]], y[gr["land"]])   # position bits kept
    assert np.all(x1[gr["west"]] == 0) and np.all(x1[gr["east"]] == L) and np.all(y1[gr["south"]] == 0) and np.all(y1[gr["north"]] == L)
    assert not np.signbit(x1[gr["west"]]).any() and not np.signbit(y1[gr["south"]]).any()
    assert np.array_equal(x1[gr["corners"]], x[gr["corners"]]) and np.array_equal(y1[gr["corners"]], y[gr["corners"]])
    assert np.any(y1[gr["west"]] != y[gr["west"]]) and np.any(x1[gr["south"]] != x[gr["south"]])    # they slide
    moved = (x1 != x) | (y1 != y)
    print("moved", int(moved.sum()), "of", x.size, "clamped", g.param("floats_clamped"), "lost", g.param("floats_lost"))
    assert moved.sum() > 900 and g.param("floats_lost") == 0
    assert g.param("floats_on_land") == int(nr.on_land(geom, mask, x1, y1).sum())
    # a stage over a large finite dt overshoots the box: clamped to it and counted, once per float and stage
    c0 = g.param("floats_clamped")
    P = stream(g)
    g.floats_stage(1, 1e9)
    xh, yh, clamped, lost = nr.move(geom, x1, y1, *nr.velocity(geom, P, x1, y1, lay), 1e9 / 2)
    c1 = g.param("floats_clamped")
    print("clamped by the stage", c1 - c0, "restatement", int(clamped.sum()))
    assert not lost.any() and clamped.sum() > 900 and c1 > c0
    if strict:
        assert c1 - c0 == clamped.sum()
    g.floats_stage(2, 0.0)
    x2, y2 = g.floats_get()
    assert np.array_equal(x2, x1) and np.array_equal(y2, y1) and g.param("floats_lost") == 0
    # a dt that overflows (times a velocity made large, the floats read what the handle holds): NaN, counted once, and NaN stays NaN
    g.set("PSI", 1e12 * g.get("PSI"))
    g.floats_stage(1, 1e308)
    g.floats_stage(2, 1e308)
    x3, y3 = g.floats_get()
    nlost = int(g.param("floats_lost"))
    print("lost", nlost)
    assert nlost > 900 and np.isnan(x3).sum() == nlost and np.array_equal(np.isnan(x3), np.isnan(y3))
    assert np.array_equal(x3[gr["land"]], x[gr["land"]])      # zero velocity times any finite dt is zero
    g.floats_stage(1, 0.1)
    g.floats_stage(2, 0.1)
    x4, y4 = g.floats_get()
    assert np.array_equal(np.isnan(x4), np.isnan(x3)) and np.array_equal(np.isnan(y4), np.isnan(x3)) and g.param("floats_lost") == nlost
    u, v = g.floats_velocity()
    assert np.array_equal(np.isnan(u), np.isnan(x3)) and np.array_equal(np.isnan(g.floats_sample("Q")), np.isnan(x3))
    g.close()


# ------------------------------------------------------------------ 5. records

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("shape", ["island", "baro"])
def test_records(shape, strict):
    g, geom, mask = make(shape, strict)
    x, y, lay, _ = floats_of(geom, mask, 1000, g.nl)
    g.floats_begin(x, y, lay)
    g.step()
    x0, y0 = g.floats_get()
    s0 = g.floats_sample("Q")
    g.floats_record(every=2, capacity=3, field="Q")
    assert g.param("floats_records") == 1 and g.param("floats_dropped") == 0
    ts, pos, smp = [g.t], [(x0, y0)], [s0]
    for k in range(7):
        g.step()
        if k % 2 == 1:
            ts.append(g.t); pos.append(g.floats_get()); smp.append(g.floats_sample("Q"))
    # record 0 at the call, one behind the 2nd and the 4th step, the 6th found the buffer full
    assert g.param("floats_records") == 3 and g.param("floats_dropped") == 1
    t, X, Y, V = g.floats_track()
    assert np.array_equal(t, np.array(ts[:3])) and t[0] > 0
    for k in range(3):
        assert np.array_equal(X[k], pos[k][0], equal_nan=True) and np.array_equal(Y[k], pos[k][1], equal_nan=True), k
        assert np.array_equal(V[k], smp[k], equal_nan=True), (k, np.abs(V[k] - smp[k]).max())
    assert not np.array_equal(X[2], X[1]) and not np.array_equal(V[2], V[1])
    t1, X1, Y1, V1 = g.floats_track(1, 2)
    assert np.array_equal(t1, t[1:]) and np.array_equal(X1, X[1:]) and np.array_equal(V1, V[1:], equal_nan=True)
    with pytest.raises(MsomError, match=f"error {ERR_ARG}: msomn_floats_track"):
        g.floats_track(2, 2)
    # only the times; then positions only: no value array is taken
    tt = np.empty(3)
    g._chk(g.L.msomn_floats_track(g.h, 0, 3, tt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), None, None, None))
    assert np.array_equal(tt, t)
    g.floats_record(every=1, capacity=2)
    g.step()
    out = g.floats_track()
    assert len(out) == 3 and out[1].shape == (2, x.size) and np.array_equal(out[1][1], g.floats_get()[0], equal_nan=True) and out[0][1] == g.t
    val = np.empty((2, x.size))
    assert g.L.msomn_floats_track(g.h, 0, 2, None, None, None, val.ctypes.data) == ERR_ARG and b"msomn_floats_track" in g.L.msom_last_error()
    g.close()


# ------------------------------------------------------------------ 6. lifecycle and errors

@pytest.mark.parametrize("strict", [True, False])
def test_lifecycle_and_errors(strict):
    from test_gpu_hooks import DevBuf

    g, geom, mask = make("plain", strict, const=False)
    L = geom.L0
    one, lay1 = np.array([0.4 * L]), np.zeros(1, dtype=np.int32)

    def refused(code, name, call):
        with pytest.raises(MsomError, match=f"error {code}: {name}"):
            call()

    refused(ERR_STATE, "msomn_floats_begin", lambda: g.floats_begin(one, one, lay1))      # before set_const
    g.set_const()
    g.set_tnext(float("inf"))
    g.step()
    q0, p0 = g.get("Q"), g.get("PSI")
    for name, call in (("msomn_floats_get", g.floats_get), ("msomn_floats_velocity", g.floats_velocity), ("msomn_floats_stage", lambda: g.floats_stage(1, 0.1)),
                       ("msomn_floats_sample", lambda: g.floats_sample("PSI")), ("msomn_floats_record", lambda: g.floats_record(1, 1)),
                       ("msomn_floats_track", lambda: g.floats_track(0, 1))):
        refused(ERR_STATE, name, call)
    g.floats_end()                # nothing to free: fine
    g.set_option("floats", 0)     # accepted, does nothing
    g.set_option("floats", 1)
    assert g.param("floats") == 0
    x, y, lay, _ = floats_of(geom, mask, 1000, g.nl)
    g.floats_begin(x, y, lay)
    # bad arguments: nothing is allocated and the earlier floats stay
    for bx, by, bl in ((np.array([np.nan]), one, lay1), (one, np.array([np.inf]), lay1), (np.array([-1e-9]), one, lay1), (one, np.array([np.nextafter(L, 2 * L)]), lay1),
                       (one, one, np.array([g.nl], dtype=np.int32)), (one, one, np.array([-1], dtype=np.int32))):
        refused(ERR_ARG, "msomn_floats_begin", lambda: g.floats_begin(bx, by, bl))
        assert g.param("floats") == x.size
    assert g.L.msomn_floats_begin(g.h, 0, one.ctypes.data, one.ctypes.data, lay1.ctypes.data) == ERR_ARG
    assert np.array_equal(g.floats_get()[0], x)
    refused(ERR_STATE, "msomn_floats_stage", lambda: g.floats_stage(2, 0.1))    # stage 2 first
    refused(ERR_ARG, "msomn_floats_stage", lambda: g.floats_stage(3, 0.1))
    refused(ERR_ARG, "msomn_floats_stage", lambda: g.floats_stage(1, float("nan")))
    refused(ERR_ARG, "msomn_floats_sample", lambda: g.floats_sample(999))
    refused(ERR_ARG, "msomn_floats_sample", lambda: g.floats_sample("MASK"))    # one layer, not nl
    refused(ERR_ARG, "msomn_floats_record", lambda: g.floats_record(0, 4))
    refused(ERR_ARG, "msomn_floats_record", lambda: g.floats_record(1, 4, "TOPO"))
    refused(ERR_STATE, "msomn_floats_track", lambda: g.floats_track(0, 1))
    g.floats_stage(1, 0.1)
    g.floats_stage(2, 0.1)
    refused(ERR_STATE, "msomn_floats_stage", lambda: g.floats_stage(2, 0.1))    # ... and not twice
    assert np.array_equal(g.get("Q"), q0) and np.array_equal(g.get("PSI"), p0)
    # option floats = 0 pauses the advection, 1 resumes it
    xa, ya = g.floats_get()
    g.set_option("floats", 0)
    g.step()
    for u, w in zip(g.floats_get(), (xa, ya)):
        assert np.array_equal(u, w)
    g.set_option("floats", 1)
    g.step()
    assert not np.array_equal(g.floats_get()[0], xa)
    # device-pointer arrays: begin, get, velocity and track give the numbers of the host-array calls
    bad = x.copy()
    bad[7] = np.nan
    dx, dy, dl, dbad = (DevBuf(a) for a in (x, y, lay, bad))
    n = x.size
    assert g.L.msomn_floats_begin(g.h, n, dx.ptr, dy.ptr, dl.ptr) == 0
    g.floats_record(every=1, capacity=2)
    g.step()
    hx, hy = g.floats_get()
    hu, hv = g.floats_velocity()
    ox, oy, ou, ov = (DevBuf(np.zeros(n)) for _ in range(4))
    tx = DevBuf(np.zeros((2, n)))
    g._chk(g.L.msomn_floats_get(g.h, ox.ptr, oy.ptr))
    g._chk(g.L.msomn_floats_velocity(g.h, ou.ptr, ov.ptr))
    g._chk(g.L.msomn_floats_track(g.h, 0, 2, None, tx.ptr, None, None))
    for d, h in ((ox, hx), (oy, hy), (ou, hu), (ov, hv)):
        assert np.array_equal(d.host(), h)
    assert np.array_equal(tx.host(), np.array([x, hx])) and not np.array_equal(hx, x)
    assert g.L.msomn_floats_begin(g.h, n, dbad.ptr, dy.ptr, dl.ptr) == ERR_ARG and b"msomn_floats_begin: float 7" in g.L.msom_last_error()
    assert g.param("floats") == n and np.array_equal(g.floats_get()[0], hx)
    for d in (dx, dy, dl, dbad, ox, oy, ou, ov, tx):
        d.free()
    # a second begin replaces the first; set_const drops the floats
    g.floats_begin(one, one, lay1)
    assert g.param("floats") == 1 and g.param("floats_records") == 0
    g.set_const()
    assert g.param("floats") == 0
    refused(ERR_STATE, "msomn_floats_get", g.floats_get)
    g.close()


def test_a_tiled_handle_refuses_every_call():
    par, inp = setup("plain")
    names = ["begin", "end", "get", "velocity", "sample", "stage", "record", "track"]

    def body(g, rank):
        q0, p0 = g.get("Q"), g.get("PSI")
        a, lay = np.array([1.0]), np.zeros(1, dtype=np.int32)
        p = a.ctypes.data
        args = dict(begin=(1, p, p, lay.ctypes.data), end=(), get=(p, p), velocity=(p, p), sample=(0, p), stage=(1, 0.1), record=(1, 1, -1),
                    track=(0, 1, None, p, p, None))
        seen = {}
        for nme in names:
            r = getattr(g.L, "msomn_floats_" + nme)(g.h, *args[nme])
            seen[nme] = (r, g.L.msom_last_error())
        g.set_option("floats", 1)     # accepted, without effect
        return dict(seen=seen, nf=g.param("floats"), same=np.array_equal(g.get("Q"), q0) and np.array_equal(g.get("PSI"), p0), a=a[0])
    out = run_tiled(par, 2, 1, inp, True, body)
    for o in out:
        for nme, (r, msg) in o["seen"].items():
            assert r == ERR_CONFIG and ("msomn_floats_" + nme).encode() in msg, (nme, r, msg)
        assert o["nf"] == 0 and o["same"] and o["a"] == 1.0


# ------------------------------------------------------------------ 7. the state file

@pytest.mark.parametrize("strict", [True, False])
def test_floats_and_the_state_file(strict, tmp_path):
    a, geom, mask = make("island", strict)     # floats, uninterrupted
    b, _, _ = make("island", strict)           # no floats
    x, y, lay, _ = floats_of(geom, mask, 1000, a.nl)
    a.floats_begin(x, y, lay)
    a.floats_record(every=1, capacity=8, field="Q")
    for _ in range(2):
        a.step(); b.step()
    pa, pb = str(tmp_path / "a.msom"), str(tmp_path / "b.msom")
    a.save_state(pa, constants=True)
    b.save_state(pb, constants=True)
    assert open(pa, "rb").read() == open(pb, "rb").read()
    xm, ym = a.floats_get()
    # a load into the handle that has floats leaves them alone
    a.load_state(pa)
    assert a.param("floats") == x.size and a.param("floats_records") == 3
    for u, w in zip(a.floats_get(), (xm, ym)):
        assert np.array_equal(u, w)
    # a handle made from the file, the floats begun again at the step boundary: the bits of the uninterrupted run
    c = node_from_state(pa, strict=strict)
    c.set_option("quiet", 1)
    c.set_tnext(float("inf"))
    assert c.param("floats") == 0
    c.floats_begin(xm, ym, lay)
    for _ in range(2):
        a.step(); c.step()
    assert a.t == c.t and np.array_equal(a.get("Q"), c.get("Q"))
    for u, w in zip(a.floats_get(), c.floats_get()):
        assert np.array_equal(u, w)
    assert not np.array_equal(a.floats_get()[0], xm)
    for m in (a, b, c):
        m.close()
    assert sorted(os.listdir(tmp_path)) == ["a.msom", "b.msom"]
