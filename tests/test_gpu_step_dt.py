"""The step-size arithmetic of the time loop (csrc/step_dt_inl.h: the limiter step and dtnext) is written once and called by the host
(msom_step, msomn_step, the newqg dialect) and by the device (k_step_dt, which computes dt in front of an accepted speculative tendency
pass).  The other async_solve comparisons run with no event ahead, so dtnext's branches towards an event time are held here:

* layered model: 6 steps towards set_tnext(2.5 dt0) and, once that is reached, towards t + 0.4 dt; the run with async_solve = 1 (dt and
  tnext from the device wherever a solve ends after its first cycle) EQUALS the run with async_solve = 0 (host arithmetic): every dt,
  every time, psi and q, and one step lands on the event time exactly;
* vertex model: msomn_step against the same step made by hand with dtnext transcribed to Python floats (IEEE double, no contraction)
  and applied to the dt that msomn_update returns."""
import math

import numpy as np
import pytest

import orc
import orn
from msom_amd import QG, NodeQG, FIELDS as F

pytestmark = pytest.mark.gpu

BUILDS = [True, False]
NSTEPS = 6
# 64 x 64 x 1: nothing marched, the speculative pass on; TOLERANCE 1e-7 (the pass is discarded: the host's dtnext behind a miss) and 1e-3.
# 512 x 64 x 2: the narrowest grid the chained smoother takes, the pass emits the next residual and closes the solve (rhs_close = 2)
# and is accepted at 1e-3, so that every dt of the run comes from the device
CASES = {
    "64x64x1_tol1e-7": (64, 64, 1, 1e-7, {}),
    "64x64x1_tol1e-3": (64, 64, 1, 1e-3, {}),
    "512x64x2_marched": (512, 64, 2, 1e-3, dict(march=2, uniform_S=1, rhs_resid=1, rhs_close=2)),
}


def dtnext(t, tnext, dt):
    """dtnext() of Basilisk's run() as step_dt_inl.h states it; returns (dt, time after the step, branch taken)"""
    if tnext != math.inf and tnext > t:
        n = int((tnext - t) / dt)
        if n == 0:
            return tnext - t, tnext, "n == 0"
        dt1 = (tnext - t) / n
        branch = "whole steps"
        if dt1 > dt * (1. + 1e-9):
            dt, branch = (tnext - t) / (n + 1), "n + 1"
        elif dt1 < dt:
            dt, branch = dt1, "dt1 < dt"
        return dt, t + dt, branch
    return dt, t + dt, "plain"


def towards_events(step, time, set_tnext, dt0):
    """NSTEPS steps towards 2.5 dt0, then once towards 0.4 dt past it; returns the dts, the times and the event time that was landed on"""
    event = 2.5 * dt0
    set_tnext(event)
    dts, ts, landed = [], [], None
    for _ in range(NSTEPS):
        dts.append(step())
        ts.append(time())
        if landed is None and ts[-1] == event:
            landed = event
            set_tnext(ts[-1] + 0.4 * dts[-1])
    return dts, ts, landed


def layered(nx, ny, nl, tol, opts, strict, async_solve):
    g = QG(orc.double_gyre_params(nx, nl, extra=f"Ny = {ny}\n" if ny != nx else ""), strict=strict)
    g.option("quiet", 1)
    g.option("TOLERANCE", tol)
    g.option("async_solve", async_solve)
    for k, v in opts.items():
        g.option(k, v)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    return g


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_dt_equals_host_dt(case, strict):
    nx, ny, nl, tol, opts = CASES[case]
    probe = layered(nx, ny, nl, tol, opts, strict, 0)
    dt0 = probe.step()
    probe.close()
    runs = []
    for async_solve in (1, 0):
        g = layered(nx, ny, nl, tol, opts, strict, async_solve)
        if "rhs_close" in opts:   # the pass closes the solve only where it is queued speculatively
            assert g.param("rhs_close") == (opts["rhs_close"] if async_solve else 0)
        cycles = []
        dts, ts, landed = towards_events(lambda: (g.step(), cycles.append(g.mgstats().i))[0], lambda: g.t, g.set_tnext, dt0)
        runs.append((dts, ts, g.get(F["PSI"]), g.get(F["Q"])))
        print(case, "strict" if strict else "fast", "async_solve", async_solve, "dt", dts, "t", ts, "cycles of the last solve", cycles)
        g.close()
        assert landed == 2.5 * dt0 and landed in ts, (ts, 2.5 * dt0)   # one step's t is the event time, exactly
        assert len(set(dts)) > 2, dts                                   # shortened towards the events, and plain steps after them
        if "rhs_close" in opts:
            assert cycles == [1] * NSTEPS, cycles                       # every speculative pass was accepted
    (dts1, ts1, psi1, q1), (dts0, ts0, psi0, q0) = runs
    assert dts1 == dts0, (dts1, dts0)
    assert ts1 == ts0, (ts1, ts0)
    assert np.array_equal(psi1, psi0), "psi"
    assert np.array_equal(q1, q0), "q"


@pytest.mark.parametrize("strict", BUILDS)
def test_vertex_model_dtnext(strict):
    N, nl = 32, 1   # 33 x 33 vertices

    def handle():
        g = NodeQG(orn.node_params(N, nl, bc_fac=1.0), strict=strict)
        g.set_option("quiet", 1)
        g.set("PSI", orn.node_psi(nl, N))
        g.set_const()
        return g

    probe = handle()
    probe.step()
    dt0 = probe.dt
    probe.close()
    g, h = handle(), handle()
    DT = h.param("DT")
    state = {"t": 0.0, "tnext": math.inf}
    branches = []

    def by_hand():   # msomn_step's calls with dtnext in Python
        d = h.update("Q", "DQ", DT)
        dt, tn, branch = dtnext(state["t"], state["tnext"], d)
        branches.append(branch)
        h.advance("QPRED", "Q", "DQ", dt / 2.)
        h.update("QPRED", "DQ", dt)
        h.advance("Q", "Q", "DQ", dt)
        state["t"] = tn
        return dt

    dts, ts, landed = towards_events(lambda: (g.step(), g.dt)[1], lambda: g.t, g.set_tnext, dt0)
    ref_dts, ref_ts, ref_landed = towards_events(by_hand, lambda: state["t"], lambda t: state.update(tnext=t), dt0)
    print("strict" if strict else "fast", "dt", dts, "t", ts, "branches", branches)
    assert landed == 2.5 * dt0 and ref_landed == landed
    assert dts == ref_dts, (dts, ref_dts)
    assert ts == ref_ts, (ts, ref_ts)
    assert {"n == 0", "plain"} <= set(branches) and len(set(branches)) >= 3, branches
    assert np.array_equal(g.get("Q"), h.get("Q")) and np.array_equal(g.get("PSI"), h.get("PSI"))
    g.close()
    h.close()
