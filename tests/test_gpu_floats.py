"""Lagrangian floats on the device (msom_floats_*, include/msom_floats.h) against tests/floats_ref.py, the numpy
restatement of the header's formulas, fed with the ghosted fields the kernels read (msom_floats_dbg_ghosted).

Strict build: the bits of the float64 restatement, floats on the walls, in the corners, on cell-centre lines and in the half cells
next to a wall included.  Product build: max |device - longdouble restatement| <= max(16 d_ref, 64 eps S), d_ref the distance of the
float64 restatement from the longdouble one on the same input and S the scale of the output (max |u|, |v| or |sample|; L0 for
positions).  Floats whose cell coordinate lies within 1e-9 of an integer in the longdouble run are left out of the product
comparison (a different floor is a different dual cell); at most 1 % may be, and tests/test_floats_ref.py shows that none of the
seeded ones is at the start."""
import numpy as np
import pytest

import floats_ref as fr
from msom_amd import FIELDS as F
from msom_amd import MsomError, NewQG, QG
from msom_amd.workloads import double_gyre_params, synthetic_psi

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
L0 = 80.0
# name: nx, ny, nl, extra parameters
SHAPES = {"walls": (32, 32, 3, ""), "wide": (64, 32, 2, ""), "periodic": (32, 32, 2, "sbc = -1\ntau0 = 0\n"), "pg": (32, 32, 3, "")}
ERR_ARG, ERR_CONFIG, ERR_STATE = -1, -3, -6


def make(shape, strict, **opts):
    nx, ny, nl, extra = SHAPES[shape]
    g = QG(double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra), strict=strict)
    g.option("quiet", 1)
    g.option("TOLERANCE", 1e-9 if strict else 1e-12)
    for k, v in opts.items():
        g.option(k, v)
    g.set(F["PSI"], synthetic_psi(nl, ny, nx, amp=5.0))
    if shape == "pg":
        g.set(F["PSIPG"], 0.3 * synthetic_psi(nl, ny, nx, amp=5.0)[::-1].copy())
    g.set_const()
    g.set_tnext(float("inf"))
    g.pg = shape == "pg"
    return g, fr.Geom(nx, ny, L0, periodic=shape == "periodic")


def stream(g):
    """what the velocity is taken from, ghosted: psi, or psi + psipg"""
    P = g.floats_ghosted(F["PSI"])
    return P + g.floats_ghosted(F["PSIPG"]) if g.pg else P


def floats_of(geom, n, nl, strict, seed=0):
    x, y, lay = fr.seeded_floats(geom, n, nl, seed)
    if strict and n > 1 and not geom.periodic:   # the deliberately placed ones
        wx, wy = fr.wall_floats(geom)
        x, y = np.concatenate([x, wx]), np.concatenate([y, wy])
        lay = np.concatenate([lay, (np.arange(wx.size) % nl).astype(np.int32)])
    assert x.size % 64
    return x, y, lay


def hold(what, dev, ref, strict, scale, keep=None):
    """dev: arrays from the device; ref(dtype): the restatement's"""
    r64 = ref(np.float64)
    if strict:
        for d, r in zip(dev, r64):
            assert np.array_equal(d, r, equal_nan=True), (what, np.abs(d - r).max())
        return
    rld = ref(LD)
    keep = np.ones(dev[0].shape, dtype=bool) if keep is None else keep
    assert (~keep).sum() <= 0.01 * keep.size, f"{what}: {(~keep).sum()} of {keep.size} floats on a cell line"
    for d, a, b in zip(dev, r64, rld):
        d_ref = float(np.abs(a - b)[keep].max())
        err = float(np.abs(d - b)[keep].max())
        bar = max(16 * d_ref, 64 * EPS * scale)
        print(f"{what}: device {err:.3e}, d_ref {d_ref:.3e}, bar {bar:.3e}")
        assert err <= bar, what


# ------------------------------------------------------------------ 1. the operator

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_velocity_and_sample_equal_the_restatement(shape, n, strict):
    g, geom = make(shape, strict)
    g.step()
    nl = g.nl
    x, y, lay = floats_of(geom, n, nl, strict)
    g.floats_begin(x, y, lay)
    assert g.param("floats") == x.size and g.param("floats_lost") == 0 and g.param("floats_clamped") == 0
    gx, gy = g.floats_get()
    assert np.array_equal(gx, x) and np.array_equal(gy, y)
    keep = ~fr.near_cell_line(geom, x, y)
    S = stream(g)
    u, v = g.floats_velocity()
    scale = float(np.abs(np.concatenate(fr.velocity(geom, S, x, y, lay, LD))).max())
    hold(f"{shape} velocity", (u, v), lambda dt: fr.velocity(geom, S, x, y, lay, dt), strict, scale, keep)
    for name in ("PSI", "Q"):
        G = g.floats_ghosted(F[name])
        assert np.array_equal(G[:, 1:-1, 1:-1], g.get(F[name]))
        s = g.floats_sample(F[name])
        hold(f"{shape} sample {name}", (s,), lambda dt: (fr.sample(geom, G, x, y, lay, dt),), strict, float(np.abs(G).max()), keep)
    if shape == "walls" and strict and n > 1:   # the walls themselves: the normal velocity is exactly zero, corners included
        nw = fr.wall_floats(geom)[0].size
        wx, wy = x[-nw:], y[-nw:]
        assert np.all(u[-nw:][(wx == 0) | (wx == geom.Lx)] == 0) and np.all(v[-nw:][(wy == 0) | (wy == geom.Ly)] == 0)
        assert np.any(v[-nw:][wx == 0] != 0)
    g.close()


def test_arrays_may_live_on_the_device():
    """begin from device arrays, get / velocity / track into device arrays: the numbers of the host-array calls"""
    from test_gpu_hooks import DevBuf

    g, geom = make("wide", strict=False)
    x, y, lay = floats_of(geom, 1000, g.nl, strict=False)
    bad = x.copy()
    bad[7] = np.nan
    dx, dy, dl, dbad = (DevBuf(a) for a in (x, y, lay, bad))
    assert g.L.msom_floats_begin(g.h, 1000, dx.ptr, dy.ptr, dl.ptr) == 0
    g.floats_record(every=1, capacity=2)
    g.step()
    hx, hy = g.floats_get()
    hu, hv = g.floats_velocity()
    ox, oy, ou, ov = (DevBuf(np.zeros(1000)) for _ in range(4))
    tx = DevBuf(np.zeros((2, 1000)))
    g._chk(g.L.msom_floats_get(g.h, ox.ptr, oy.ptr))
    g._chk(g.L.msom_floats_velocity(g.h, ou.ptr, ov.ptr))
    g._chk(g.L.msom_floats_track(g.h, 0, 2, None, tx.ptr, None))
    for d, h in ((ox, hx), (oy, hy), (ou, hu), (ov, hv)):
        assert np.array_equal(d.host(), h)
    assert np.array_equal(tx.host(), np.array([x, hx])) and not np.array_equal(hx, x)
    # a bad value in a device array is found too, and the floats that were there stay
    assert g.L.msom_floats_begin(g.h, 1000, dbad.ptr, dy.ptr, dl.ptr) == ERR_ARG and b"msom_floats_begin: float 7" in g.L.msom_last_error()
    assert g.param("floats") == 1000 and np.array_equal(g.floats_get()[0], hx)
    for d in (dx, dy, dl, dbad, ox, oy, ou, ov, tx):
        d.free()
    g.close()


# ------------------------------------------------------------------ 2. by hand, 3. msom_step = by hand

def hand_step(g, geom, q, DT, lay, strict, what):
    """one RK2 step through update / floats_stage(1) / advance / update / floats_stage(2) / advance, the floats held to the
    restatement fed with the psi each update left; returns (q_new, dt)"""
    x0, y0 = g.floats_get()
    dq, dt = g.update(q, DT)
    S1 = stream(g)
    g.floats_stage(1, dt)
    qp = g.advance(q, dq, dt / 2)
    dq2, _ = g.update(qp, dt)
    S2 = stream(g)
    g.floats_stage(2, dt)
    x1, y1 = g.floats_get()

    def ref(dtype):
        xh, yh = fr.stage1(geom, S1, x0, y0, lay, dt, dtype)
        return fr.stage2(geom, S2, x0, y0, xh, yh, lay, dt, dtype)

    xh, yh = fr.stage1(geom, S1, x0, y0, lay, dt, LD)
    keep = ~(fr.near_cell_line(geom, x0, y0) | fr.near_cell_line(geom, xh, yh))
    hold(what, (x1, y1), ref, strict, L0, keep)
    return g.advance(q, dq2, dt), dt


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n", [1, 1000])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_stages_by_hand_equal_the_restatement(shape, n, strict):
    g, geom = make(shape, strict)
    x, y, lay = floats_of(geom, n, g.nl, strict)
    g.floats_begin(x, y, lay)
    q, DT = g.get(F["Q"]), g.param("DT")
    for k in range(3):
        q, _ = hand_step(g, geom, q, DT, lay, strict, f"{shape} step {k}")
    x1, y1 = g.floats_get()
    assert np.abs(x1 - x).max() + np.abs(y1 - y).max() > 0   # they did move
    g.close()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("async_solve", [1, 0])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_msom_step_moves_the_floats_as_the_stages_by_hand(shape, async_solve, strict):
    a, geom = make(shape, strict, async_solve=async_solve)
    b, _ = make(shape, strict)
    x, y, lay = floats_of(geom, 1000, a.nl, strict)
    idx = geom.idx
    for m in (a, b):
        m.floats_begin(x, y, lay)
    a.floats_record(every=1, capacity=4)
    q, DT = b.get(F["Q"]), b.param("DT")
    hand, bound = [b.floats_get()], 64 * EPS * L0
    for k in range(3):
        dt_a = a.step()
        q, dt_b = hand_step(b, geom, q, DT, lay, strict, f"{shape} step {k}")
        xa, ya = a.floats_get()
        xb, yb = b.floats_get()
        hand.append((xb, yb))
        if strict:
            assert dt_a == dt_b
            assert np.array_equal(xa, xb) and np.array_equal(ya, yb)
        else:
            # the two paths' psi differ by round-off; a velocity is a difference of two psi times idx, each stage moves by at most dt
            # times it, and stage 1's psi, which msom_step does not expose, is taken to differ as much as stage 2's
            dpsi = float(np.abs(a.get(F["PSI"]) - b.get(F["PSI"])).max())
            bound += 4 * dt_b * (2 * dpsi * idx)
            err = max(float(np.abs(xa - xb).max()), float(np.abs(ya - yb).max()))
            print(f"{shape} async_solve {async_solve} step {k}: |auto - by hand| {err:.3e}, bound {bound:.3e}, max |dpsi| {dpsi:.3e}")
            assert dt_a == pytest.approx(dt_b, rel=1e-12)
            assert err <= bound
    assert a.param("floats_records") == 4 and a.param("floats_dropped") == 0
    t, tx, ty = a.floats_track()
    assert t[0] == 0 and t[-1] == a.t and np.all(np.diff(t) > 0)
    assert np.array_equal(tx[0], x) and np.array_equal(ty[0], y)
    xa, ya = a.floats_get()
    assert np.array_equal(tx[-1], xa) and np.array_equal(ty[-1], ya)
    if strict:
        assert np.array_equal(tx, np.array([h[0] for h in hand])) and np.array_equal(ty, np.array([h[1] for h in hand]))
    a.close(); b.close()


# ------------------------------------------------------------------ 4. walls and periodicity

@pytest.mark.parametrize("strict", [True, False])
def test_a_float_on_a_wall_slides_along_it(strict):
    g, geom = make("wide", strict)
    y0 = np.array([0.3, 0.5, 0.77, 0.61]) * geom.Ly
    x0 = np.array([0, 0, 0, 0.37]) * geom.Lx          # three on the wall x = 0, one inside
    g.floats_begin(x0, y0, np.array([0, 1, 0, 1], dtype=np.int32))
    for _ in range(5):
        g.step()
    x, y = g.floats_get()
    assert np.array_equal(x[:3], x0[:3]) and not np.signbit(x[:3]).any()   # on x = 0 bit for bit
    assert np.all(y != y0)
    print("floats_clamped", g.param("floats_clamped"), "floats_lost", g.param("floats_lost"))
    assert g.param("floats_clamped") == 0 and g.param("floats_lost") == 0   # sliding needs no clamp
    # a stage that overshoots the box is clamped to it and counted, once per float and stage: stage 1 over no time, stage 2 over a long one
    g.floats_stage(1, 0.0)
    g.floats_stage(2, 1e9)
    x, y = g.floats_get()
    assert np.all(x[:3] == 0) and np.all((y == 0) | (y == geom.Ly)) and x[3] in (0, geom.Lx)
    assert g.param("floats_clamped") == 4 and g.param("floats_lost") == 0
    g.close()


@pytest.mark.parametrize("strict", [True, False])
def test_uniform_background_flow_carries_unwrapped_floats(strict):
    nx, ny, nl = 32, 32, 2
    upg, vpg = [0.3, -0.2], [0.1, 0.25]
    txt = double_gyre_params(nx, nl, extra="sbc = -1\ntau0 = 0\nbeta = 0\nupg = [0.3,-0.2]\nvpg = [0.1,0.25]\nflsrv = 1\n")
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], np.zeros((nl, ny, nx)))
    g.set_const()
    g.set_tnext(float("inf"))
    geom = fr.Geom(nx, ny, L0, periodic=True)
    x0, y0, lay = fr.seeded_floats(geom, 1000, nl)
    x0[:4], y0[:4] = [-3.7 * L0, 2.3 * L0, -0.01, L0], [5.2 * L0, -1.9 * L0, L0, -0.01]   # beyond L and below 0
    g.floats_begin(x0, y0, lay)
    T = sum(g.step() for _ in range(5))
    assert np.all(g.get(F["PSI"]) == 0)
    x, y = g.floats_get()
    bar = 32 * EPS * (np.abs(x0) + L0)
    assert np.all(np.abs((x - x0) - np.array(upg)[lay] * T) <= bar)
    assert np.all(np.abs((y - y0) - np.array(vpg)[lay] * T) <= 32 * EPS * (np.abs(y0) + L0))
    assert x[0] < -3 * L0 and x[1] > 2 * L0 and y[0] > 5 * L0 and y[1] < -L0   # unwrapped
    assert g.param("floats_clamped") == 0 and g.param("floats_lost") == 0
    g.close()


# ------------------------------------------------------------------ 5. restart, pause, record, guards

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("shape", ["walls", "periodic"])
def test_restart_from_get_and_begin_continues_with_the_same_bits(shape, strict):
    a, geom = make(shape, strict)
    b, _ = make(shape, strict)
    x, y, lay = floats_of(geom, 1000, a.nl, strict)
    for m in (a, b):
        m.floats_begin(x, y, lay)
    for _ in range(4):
        a.step()
    for _ in range(2):
        b.step()
    xm, ym = b.floats_get()
    b.floats_end()
    assert b.param("floats") == 0
    b.floats_begin(xm, ym, lay)
    for _ in range(2):
        b.step()
    assert np.array_equal(a.get(F["Q"]), b.get(F["Q"]))
    for u, w in zip(a.floats_get(), b.floats_get()):
        assert np.array_equal(u, w)
    a.close(); b.close()


@pytest.mark.parametrize("strict", [True, False])
def test_pause_record_and_a_handle_without_floats(strict):
    a, geom = make("walls", strict)      # floats, paused for one step, recorded
    b, _ = make("walls", strict)         # no floats: the run as it was before there were any
    b.option("floats", 0)                # accepted, does nothing
    b.option("floats", 1)
    assert b.param("floats") == 0 and b.param("floats_records") == 0 and b.param("floats_clamped") == 0
    x, y, lay = floats_of(geom, 1000, a.nl, strict)
    a.floats_begin(x, y, lay)
    a.floats_record(every=2, capacity=2)
    a.option("floats", 0)
    dts = [(a.step(), b.step())]
    for u, w in zip(a.floats_get(), (x, y)):
        assert np.array_equal(u, w)      # paused: untouched
    a.option("floats", 1)
    for _ in range(6):
        dts.append((a.step(), b.step()))
    assert all(p == q for p, q in dts)
    assert np.array_equal(a.get(F["Q"]), b.get(F["Q"])) and np.array_equal(a.get(F["PSI"]), b.get(F["PSI"]))
    # record 0 at the call, one more after the 2nd moving step; the 4th and the 6th found the buffer full
    assert a.param("floats_records") == 2 and a.param("floats_dropped") == 2
    t, tx, ty = a.floats_track()
    assert t[0] == 0 and t[1] == pytest.approx(sum(d[0] for d in dts[:3]), rel=1e-14)
    assert np.array_equal(tx[0], x) and not np.array_equal(tx[1], x) and not np.array_equal(tx[1], a.floats_get()[0])
    with pytest.raises(MsomError, match="msom_floats_track"):
        a.floats_track(1, 2)
    a.close(); b.close()


@pytest.mark.parametrize("strict", [True, False])
def test_guards_leave_the_model_unchanged(strict):
    g, geom = make("walls", strict)
    g.step()
    q0, p0 = g.get(F["Q"]), g.get(F["PSI"])
    one, lay = np.array([1.0]), np.zeros(1, dtype=np.int32)

    def refused(code, name, call):
        with pytest.raises(MsomError, match=f"error {code}: {name}") as e:
            call()
        return e

    # before any begin
    for name, call in (("msom_floats_get", g.floats_get), ("msom_floats_velocity", g.floats_velocity), ("msom_floats_stage", lambda: g.floats_stage(1, 0.1)),
                       ("msom_floats_sample", lambda: g.floats_sample(F["PSI"])), ("msom_floats_record", lambda: g.floats_record(1, 1))):
        refused(ERR_STATE, name, call)
    g.floats_end()   # nothing to free: fine
    # bad arguments: nothing is allocated
    for bx, by, bl in ((np.array([np.nan]), one, lay), (one, np.array([np.inf]), lay), (np.array([-1e-9]), one, lay), (one, np.array([np.nextafter(L0, 2 * L0)]), lay),
                       (one, one, np.array([3], dtype=np.int32)), (one, one, np.array([-1], dtype=np.int32))):
        refused(ERR_ARG, "msom_floats_begin", lambda: g.floats_begin(bx, by, bl))
        assert g.param("floats") == 0
    assert g.L.msom_floats_begin(g.h, 0, one.ctypes.data, one.ctypes.data, lay.ctypes.data) == ERR_ARG
    g.floats_begin(np.array([0.0, L0, 40.0]), np.array([L0, 0.0, 40.0]), np.array([0, 2, 1], dtype=np.int32))   # the box is closed
    assert g.param("floats") == 3
    refused(ERR_STATE, "msom_floats_stage", lambda: g.floats_stage(2, 0.1))    # stage 2 first
    refused(ERR_ARG, "msom_floats_stage", lambda: g.floats_stage(3, 0.1))
    refused(ERR_ARG, "msom_floats_stage", lambda: g.floats_stage(1, float("nan")))
    refused(ERR_ARG, "msom_floats_sample", lambda: g.floats_sample(999))
    refused(ERR_ARG, "msom_floats_record", lambda: g.floats_record(0, 4))
    refused(ERR_STATE, "msom_floats_track", lambda: g.floats_track(0, 1))
    g.floats_stage(1, 0.1)
    g.floats_stage(2, 0.1)
    refused(ERR_STATE, "msom_floats_stage", lambda: g.floats_stage(2, 0.1))    # ... and not twice
    assert np.array_equal(g.get(F["Q"]), q0) and np.array_equal(g.get(F["PSI"]), p0)
    # a float that leaves the numbers is lost: NaN, counted once, never read again
    g.set(F["PSI"], 1e12 * p0)
    g.floats_stage(1, 1e300)
    g.floats_stage(2, 1e300)
    g.floats_stage(1, 0.1)
    x, y = g.floats_get()
    assert np.isnan(x[2]) and np.isnan(y[2]) and g.param("floats_lost") == 1
    u, v = g.floats_velocity()
    assert np.isnan(u[2]) and np.isnan(v[2]) and np.all(np.isfinite(u[:2]))
    # a second begin replaces the first
    g.floats_begin(one, one, lay)
    assert g.param("floats") == 1 and g.param("floats_lost") == 0
    g.close()


@pytest.mark.parametrize("strict", [True, False])
def test_newqg_and_tiled_handles_are_refused(strict):
    import newqg_ref as nq
    from test_gpu_tiled import run_tiled

    n = NewQG(nq.sample_par(16, 16).text(), strict=strict)
    n.option("quiet", 1)
    one, lay = np.array([0.5]), np.zeros(1, dtype=np.int32)
    q0, p0 = n.get(F["Q"]), n.get(F["PSI"])
    assert n.L.msom_floats_begin(n.h, 1, one.ctypes.data, one.ctypes.data, lay.ctypes.data) == ERR_CONFIG
    assert b"msom_floats_begin" in n.L.msom_last_error()
    assert n.L.msom_floats_get(n.h, one.ctypes.data, one.ctypes.data) == ERR_CONFIG and b"msom_floats_get" in n.L.msom_last_error()
    assert n.L.msom_floats_stage(n.h, 1, 0.1) == ERR_CONFIG and n.L.msom_floats_end(n.h) == ERR_CONFIG
    assert np.array_equal(n.get(F["Q"]), q0) and np.array_equal(n.get(F["PSI"]), p0)
    n.close()

    def tile(g, rank):
        q0, p0 = g.get(F["Q"]), g.get(F["PSI"])
        x = np.array([1.0])
        r = g.L.msom_floats_begin(g.h, 1, x.ctypes.data, x.ctypes.data, lay.ctypes.data)
        msg = g.L.msom_last_error()
        r2 = g.L.msom_floats_dbg_ghosted(g.h, F["PSI"], np.empty((g.nl, g.ny + 2, g.nx + 2)).ctypes.data)
        return r, msg, r2, g.param("floats"), np.array_equal(g.get(F["Q"]), q0) and np.array_equal(g.get(F["PSI"]), p0)

    out = run_tiled(double_gyre_params(64, 2, extra="Ny = 32\nMGLEVELS = 4\n"), 2, 1, synthetic_psi(2, 32, 64), 1, strict, fn=tile)
    for o in out:
        r, msg, r2, nf, same = o["extra"]
        assert r == ERR_CONFIG and b"msom_floats_begin" in msg and r2 == ERR_CONFIG and nf == 0 and same
