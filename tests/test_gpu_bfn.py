"""The back-and-forth nudging loop run on the device: msom_bfn_begin / msom_bfn_steps / msom_bfn_misfit against the loop
of msqg/qg_bfn.py:47-73 written in numpy around pystep_bfn (msqg/qg_bfn.h:21-80), with the nudging term put where that
script says "BFN nudging goes here":

    f1  = tend + (k * gain) * (obs - q)                      (k == 0: f1 = tend)
    q   = q + (dt / 12) * ((23 * f1 - 16 * f2) + 5 * f3)     (dt / 12 formed once)
    f3, f2 = f2, f1                                          (the library rotates the slots F1 -> F2 -> F3 -> F1 instead of copying,
                                                              so after a step F2 is the newest tendency and F1 the slot the next
                                                              step overwrites: the reference below rotates the same way)

from a zero history, five steps (the rotation wraps).  The reference is that loop over the CPU oracle's pystep_bfn
(strict build: bit for bit) and over pystep_bfn of a handle of the same build (product build: round-off)."""
import functools

import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F
from msom_amd.api import MsomError
from test_gpu_hooks import DevBuf
from test_gpu_parity import make_pair, rand_field, rel
from test_gpu_tiled import assemble, run_tiled

pytestmark = pytest.mark.gpu

CASES = [(64, 64, 3, ""),
         (128, 32, 6, "sbc = 1.5\nRe = 300\nEks = 0.001\n"),
         (16, 16, 2, ""),                       # rows shorter than a wavefront
         (32, 32, 1, ""),
         (64, 64, 2, "sbc = -1\ntau0 = 0\n"),
         (32, 32, 10, "")]                      # above MSOM_FASTNL
VARIANTS = ["forward", "backward", "free"]      # (direction, sign of dt, k): (+1, +, k), (-1, -, -k), (+1, +, 0)
NSTEPS = 5
TOL = 1e-9              # strict runs
TOL_PRODUCT = 1e-12     # product runs and their oracle reference, as in test_gpu_hooks (round-off is compared, not the stopping point of the solver)
MSOM_ERR_ARG, MSOM_ERR_STATE = -1, -6
HIST = ("BFN_F1", "BFN_F2", "BFN_F3")


def variant(name, DT):
    k = 0.05 / DT
    return {"forward": (1.0, DT, k), "backward": (-1.0, -DT, -k), "free": (1.0, DT, 0.0)}[name]


def inputs(q0):
    """observations close to the state, and a gain that is zero on about half of the cells"""
    obs = q0 + rand_field(21, q0.shape, 1e-3 * np.abs(q0).max())
    rng = np.random.default_rng(22)
    gain = (rng.random(q0.shape) < 0.5) * (0.25 + rng.random(q0.shape))
    return obs, gain


def numpy_loop(tend_fn, q, nsteps, dt, direction, k, obs, gain, hist=None):
    """the loop of msqg/qg_bfn.py:62-73 with the nudging term, in the expression order msom_bfn_steps documents.
    Returns q after every step and the three history slots."""
    f1, f2, f3 = [np.zeros_like(q) for _ in range(3)] if hist is None else [h.copy() for h in hist]
    dt12 = dt / 12
    qs = []
    for _ in range(nsteps):
        f1 = tend_fn(q, direction)
        if k != 0:
            f1 = f1 + (k * (1.0 if gain is None else gain)) * (obs - q)
        q = q + dt12 * ((23 * f1 - 16 * f2) + 5 * f3)
        qs.append(q)
        f1, f2, f3 = f3, f1, f2
    return qs, (f1, f2, f3)


def tend_of(g):
    def fn(q, direction):
        t = np.empty_like(q)
        g.pystep_bfn(q, t, direction, 1)
        return t
    return fn


@functools.lru_cache(maxsize=None)
def oracle_run(case, name, tol=TOL):
    """the reference, computed once per (case, variant, TOLERANCE) and shared; nothing below writes into it"""
    nx, ny, nl, extra = CASES[case]
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)
    o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1)
    o.option("TOLERANCE", tol)
    o.set(orc.PSI, orc.synthetic_psi(nl, ny, nx))
    o.set_const()
    q0 = o.get(orc.Q)
    obs, gain = inputs(q0)
    direction, dt, k = variant(name, o.param("DT"))
    qs, hist = numpy_loop(lambda q, d: o.pystep_bfn(q, d), q0, NSTEPS, dt, direction, k, obs, gain)
    res = dict(q0=q0, obs=obs, gain=gain, qs=qs, hist=hist, psi=o.get(orc.PSI))
    for a in [q0, obs, gain, res["psi"], *qs, *hist]:
        a.setflags(write=False)
    return res


def handle(case, strict, tol=TOL, **opts):
    nx, ny, nl, extra = CASES[case]
    txt = orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    g.option("TOLERANCE", tol)
    for k_, v_ in opts.items():
        g.option(k_, v_)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    return g


def begin(g, obs=None, gain=None, q=None):
    g.bfn_begin()
    if q is not None:
        g.set(F["Q"], q)
    if obs is not None:
        g.set(F["BFN_OBS"], obs)
    if gain is not None:
        g.set(F["BFN_GAIN"], gain)


# ------------------------------------------------------------------ 1. strict build against the oracle

@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_strict_bfn_steps_bit_exact_against_the_oracle_loop(case, name):
    ref = oracle_run(case, name)
    g = handle(case, strict=True)
    direction, dt, k = variant(name, g.param("DT"))
    begin(g, ref["obs"], ref["gain"])
    assert np.array_equal(g.get(F["Q"]), ref["q0"])
    t0, it0 = g.t, g.iter
    for n in range(NSTEPS):
        g.bfn_steps(1, dt, direction, k)
        assert np.array_equal(g.get(F["Q"]), ref["qs"][n]), n
    for name_, h in zip(HIST, ref["hist"]):
        assert np.array_equal(g.get(F[name_]), h), name_
    assert np.array_equal(g.get(F["PSI"]), ref["psi"])
    assert (g.t, g.iter) == (t0, it0)
    g.close()


# ------------------------------------------------------------------ 2. product build

@pytest.mark.parametrize("name", VARIANTS)
@pytest.mark.parametrize("case", range(len(CASES)))
def test_product_bfn_steps_against_the_caller_side_loop_and_the_oracle(case, name):
    """rel <= 1e-12 against pystep_bfn + numpy on a handle of the same build (the bound of fused against separate advance,
    test_gpu_hooks), forward cases rel <= 1e-10 against the oracle."""
    ref = oracle_run(case, name, TOL_PRODUCT)
    a, b = handle(case, strict=False, tol=TOL_PRODUCT), handle(case, strict=False, tol=TOL_PRODUCT)
    direction, dt, k = variant(name, a.param("DT"))
    begin(a, ref["obs"], ref["gain"])
    a.bfn_steps(NSTEPS, dt, direction, k)
    qs, hist = numpy_loop(tend_of(b), b.get(F["Q"]), NSTEPS, dt, direction, k, ref["obs"], ref["gain"])
    qa = a.get(F["Q"])
    print(f"case {case} {name}: bfn_steps vs caller-side loop {rel(qa, qs[-1]):.3e}, vs oracle {rel(qa, ref['qs'][-1]):.3e}, "
          f"caller-side loop vs oracle {rel(qs[-1], ref['qs'][-1]):.3e}")
    assert rel(qa, qs[-1]) <= 1e-12
    assert rel(a.get(F["BFN_F2"]), hist[1]) <= 1e-12 and rel(a.get(F["BFN_F3"]), hist[2]) <= 1e-12
    if name != "backward":
        assert rel(qa, ref["qs"][-1]) <= 1e-10
    a.close(); b.close()


# ------------------------------------------------------------------ 3. equivalence of state

def test_state_after_bfn_steps_equals_the_caller_side_loop():
    """limiter state (`previous`) and warm start psi end up where three pystep_bfn calls leave them: the RK2 step that
    follows returns the same dt, q and mgstats, bit for bit (strict)"""
    case = 0
    ref = oracle_run(case, "forward")
    a, b = handle(case, strict=True), handle(case, strict=True)
    direction, dt, k = variant("forward", a.param("DT"))
    begin(a, ref["obs"], ref["gain"])
    a.bfn_steps(3, dt, direction, k)
    qs, _ = numpy_loop(tend_of(b), b.get(F["Q"]), 3, dt, direction, k, ref["obs"], ref["gain"])
    assert np.array_equal(a.get(F["Q"]), qs[-1])
    b.set(F["Q"], qs[-1])
    for g in (a, b):
        g.set_tnext(float("inf"))
    dta, dtb = a.step(), b.step()
    sa, sb = a.mgstats(), b.mgstats()
    assert dta == dtb
    assert (sa.i, sa.resb, sa.resa, sa.sum, sa.nrelax) == (sb.i, sb.resb, sb.resa, sb.sum, sb.nrelax)
    assert np.array_equal(a.get(F["Q"]), b.get(F["Q"])) and np.array_equal(a.get(F["PSI"]), b.get(F["PSI"]))
    a.close(); b.close()


# ------------------------------------------------------------------ 4. chunking and restart

def test_chunked_and_restarted_runs_equal_one_run():
    case = 1
    ref = oracle_run(case, "forward")
    direction, dt, k = variant("forward", oracle_dt(case))
    a = handle(case, strict=True)
    begin(a, ref["obs"], ref["gain"])
    a.bfn_steps(5, dt, direction, k)
    b = handle(case, strict=True)
    begin(b, ref["obs"], ref["gain"])
    b.bfn_steps(2, dt, direction, k)
    saved = {n: b.get(F[n]) for n in ("Q", "PSI") + HIST}
    b.bfn_steps(3, dt, direction, k)
    # restart: state, history and the warm start of the inversion through msom_set_field on a fresh handle
    c = handle(case, strict=True)
    c.set(F["PSI"], saved["PSI"])
    begin(c, ref["obs"], ref["gain"], q=saved["Q"])
    for n in HIST:
        c.set(F[n], saved[n])
    c.bfn_steps(3, dt, direction, k)
    for g in (b, c):
        for n in ("Q", "PSI") + HIST:
            assert np.array_equal(g.get(F[n]), a.get(F[n])), n
    assert np.array_equal(a.get(F["Q"]), ref["qs"][-1])
    a.close(); b.close(); c.close()


def oracle_dt(case):
    nx, ny, nl, extra = CASES[case]
    return orc.Oracle(orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra), quiet=1).param("DT")


# ------------------------------------------------------------------ 5. device pointers

def test_observations_and_gain_from_device_pointers():
    case = 0
    ref = oracle_run(case, "forward")
    g = handle(case, strict=True)
    direction, dt, k = variant("forward", g.param("DT"))
    g.bfn_begin()
    obs, gain = DevBuf(ref["obs"]), DevBuf(ref["gain"])
    assert g.L.msom_set_field(g.h, F["BFN_OBS"], obs.ptr) == 0
    assert g.L.msom_set_field(g.h, F["BFN_GAIN"], gain.ptr) == 0
    g.bfn_steps(NSTEPS, dt, direction, k)
    assert np.array_equal(g.get(F["Q"]), ref["qs"][-1])
    obs.free(); gain.free()
    g.close()


# ------------------------------------------------------------------ 6. tiles

@pytest.mark.parametrize("strict", [True, False])
def test_bfn_steps_on_tiles_equal_the_single_tile(strict):
    px = py = 2
    tile, nl = 32, 3
    gn = tile * px
    params = orc.double_gyre_params(gn, nl, extra="MGLEVELS = 5\n")
    psi = orc.synthetic_psi(nl, gn, gn)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    obs, gain = inputs(g.get(F["Q"]))
    direction, dt, k = variant("forward", g.param("DT"))
    begin(g, obs, gain)
    g.bfn_steps(NSTEPS, dt, direction, k)

    def sl(a, rank):
        ix, iy = rank % px, rank // px
        return np.ascontiguousarray(a[:, iy * tile:(iy + 1) * tile, ix * tile:(ix + 1) * tile])

    def fn(gt, rank):
        begin(gt, sl(obs, rank), sl(gain, rank))
        gt.bfn_steps(NSTEPS, dt, direction, k)
        return dict(q=gt.get(F["Q"]), misfit=gt.bfn_misfit())

    out = run_tiled(params, px, py, psi, nsteps=0, strict=strict, fn=fn)
    for o in out:
        o["qb"] = o["extra"]["q"]
        assert o["extra"]["misfit"] == pytest.approx(g.bfn_misfit(), rel=1e-13)     # sum order differs
    assert np.array_equal(assemble(out, "qb", px, py), g.get(F["Q"]))
    g.close()


# ------------------------------------------------------------------ 7. misfit

@pytest.mark.parametrize("strict", [True, False])
def test_misfit_against_numpy(strict):
    case = 0
    ref = oracle_run(case, "forward")
    g = handle(case, strict=strict)
    g.bfn_begin()
    with pytest.raises(MsomError):          # no observations yet
        g.bfn_misfit()
    g.set(F["BFN_OBS"], ref["obs"])
    q = g.get(F["Q"])
    d2 = (ref["obs"] - q) ** 2
    assert g.bfn_misfit() == pytest.approx(np.sqrt(d2.sum() / d2.size), rel=1e-13)          # gain unset: 1 everywhere
    g.set(F["BFN_GAIN"], ref["gain"])
    assert g.bfn_misfit() == pytest.approx(np.sqrt((ref["gain"] * d2).sum() / ref["gain"].sum()), rel=1e-13)
    g.close()


def test_unset_gain_is_one_everywhere():
    case = 2
    ref = oracle_run(case, "forward")
    a, b = handle(case, strict=True), handle(case, strict=True)
    direction, dt, k = variant("forward", a.param("DT"))
    begin(a, ref["obs"])
    begin(b, ref["obs"], np.ones_like(ref["obs"]))
    for g in (a, b):
        g.bfn_steps(3, dt, direction, k)
    assert np.array_equal(a.get(F["Q"]), b.get(F["Q"]))
    assert a.L.msom_field_layers(a.h, F["BFN_GAIN"]) == MSOM_ERR_ARG     # and no field of ones was allocated for it
    a.close(); b.close()


# ------------------------------------------------------------------ 8. errors

def test_call_order_and_argument_errors():
    g = handle(3, strict=True)
    L, h = g.L, g.h
    DT = g.param("DT")
    for n in HIST + ("BFN_OBS", "BFN_GAIN"):          # a handle that never nudged has allocated none of them
        assert L.msom_field_layers(h, F[n]) == MSOM_ERR_ARG, n
    assert L.msom_bfn_steps(h, 1, DT, 1.0, 0.0) == MSOM_ERR_STATE          # before begin
    g.bfn_begin()
    assert L.msom_bfn_steps(h, 1, DT, 1.0, 0.5) == MSOM_ERR_STATE          # k != 0 without observations
    assert L.msom_bfn_steps(h, -1, DT, 1.0, 0.0) == MSOM_ERR_ARG
    g.bfn_steps(2, DT, 1.0, 0.0)
    before = {n: g.get(F[n]) for n in ("Q",) + HIST}
    assert L.msom_bfn_steps(h, 0, DT, 1.0, 0.0) == 0
    for n, a in before.items():
        assert np.array_equal(g.get(F[n]), a), n
    g.set_const()
    assert L.msom_bfn_steps(h, 1, DT, 1.0, 0.0) == MSOM_ERR_STATE          # set_const ends the run
    g.close()


def test_pystep_bfn_unchanged_before_and_after_a_bfn_run():
    case = 0
    ref = oracle_run(case, "forward")
    nx, ny, nl, extra = CASES[case]
    for with_run in (False, True):
        o, g = make_pair(nx, ny, nl, strict=True, extra=extra, TOLERANCE=TOL)
        q = o.get(orc.Q)
        if with_run:
            direction, dt, k = variant("forward", g.param("DT"))
            begin(g, ref["obs"], ref["gain"])
            g.bfn_steps(NSTEPS, dt, direction, k)
            assert np.array_equal(g.get(F["Q"]), ref["qs"][-1])
            q = ref["qs"][-1]
            numpy_loop(lambda q_, d: o.pystep_bfn(q_, d), o.get(orc.Q), NSTEPS, dt, direction, k, ref["obs"], ref["gain"])   # same warm start
        for direction in (1.0, -1.0, 1.0):
            tend = np.empty_like(q)
            g.pystep_bfn(q, tend, direction, 1)
            assert np.array_equal(tend, o.pystep_bfn(q, direction))
        g.close()


# ------------------------------------------------------------------ 9. interior only

def test_update_writes_interior_cells_and_refills_the_ghost_ring():
    """partial slip (sbc = 1.5): one free step on the device and on the caller's side, then the pystep_bfn tendency of both
    handles.  The caller-side q went through upload's boundary fill; equal tendencies mean the ring of the device-side q
    was refilled after the update and not written by it."""
    case = 1
    a, b = handle(case, strict=True), handle(case, strict=True)
    DT = a.param("DT")
    a.bfn_begin()
    a.bfn_steps(1, DT, 1.0, 0.0)
    qs, _ = numpy_loop(tend_of(b), b.get(F["Q"]), 1, DT, 1.0, 0.0, None, None)
    qa = a.get(F["Q"])
    assert np.array_equal(qa, qs[0])
    # a's q stays in the library as bfn_steps left it: its next tendency is the newest history slot of a second free step,
    # b's comes from pystep_bfn on the same q
    a.bfn_steps(1, DT, 1.0, 0.0)
    assert np.array_equal(a.get(F["BFN_F2"]), tend_of(b)(qs[0], 1.0))
    a.close(); b.close()
