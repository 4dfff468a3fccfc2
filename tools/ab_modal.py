"""modal PV inversion (option mode_pv_invert), product build, uniform table: msom_invertq on the handle's own q (no transfers) with the
option on against the layered solve of the same handle and the same q (option off), cold (zero first guess) and warm (the previous solution), wall
time around the call with its synchronisation; HIP-event times of k_helm_relax (one sweep = both colours) and k_helm_residual through
msom_bench_kernel, compact and general form, with the bytes counted from the shapes (w = 8 nl N^2: 3 w per sweep and per residual,
+ 1 w of iBu in the general form); and, from a separate profiled solve, the launch-bound levels (<= 64 cells a side) of a cycle.
Usage: python tools/ab_modal.py [N NL]   (default 4096 6) -> one JSON line, kept as profiles/modal_invert.json."""
import ctypes as C
import json
import sys
import time

sys.path.insert(0, '.')
import numpy as np
from msom_amd import QG, FIELDS as F, workloads as wl
from msom_amd.api import MGStats

N, nl = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (4096, 6)
w = 8.0 * nl * N * N


def solve(g):
    st = MGStats()
    g.sync()
    t0 = time.perf_counter()
    rc = g.L.msom_invertq(g.h, None, None, C.byref(st))   # q = the handle's Q, psi stays on the device; synchronises on return
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, g.L.msom_last_error()
    return ms, st


def handle(compact=None):
    g = QG(wl.double_gyre_params(N, nl))
    g.option("quiet", 1)
    if compact is not None:
        g.option("modes_compact", compact)
    g.set(F["PSI"], wl.synthetic_psi(nl, N, N))
    g.set_const()                                          # Q = comp_q(PSI)
    return g


row = {"N": N, "nl": nl, "w_bytes": w, "rounds": []}
g = handle()
zero = np.zeros((nl, N, N))
q0 = g.get(F["Q"])                                         # the one right-hand side of every solve below
# TOLERANCE 1e-3 is the reference's (msqg/qg.h:159): one cycle does it for this q.  1e-9 makes the modes stop at different cycles.
for tol, rnd in ((1e-3, 0), (1e-3, 1), (1e-3, 2), (1e-9, 0), (1e-9, 1)):     # the first round warms the code objects up and is reported too
    r = {"TOLERANCE": tol, "round": rnd}
    g.option("TOLERANCE", tol)
    g.option("mode_pv_invert", 0)
    g.set(F["PSI"], zero)
    ms, st = solve(g)
    r["layered_cold"] = {"ms": ms, "cycles": st.i, "nrelax": st.nrelax, "resa": st.resa}
    ms, st = solve(g)
    r["layered_warm"] = {"ms": ms, "cycles": st.i, "nrelax": st.nrelax, "resa": st.resa}
    g.option("mode_pv_invert", 1)
    g.set_const()                                          # zeroes p_m -- and recomputes Q from psi, so
    g.set(F["Q"], q0)                                      # the layered solve's q goes back in
    ms, st = solve(g)
    per = [g.modes_mgstats(m) for m in range(nl)]
    r["modal_cold"] = {"ms": ms, "cycles": [s.i for s in per], "nrelax": [s.nrelax for s in per], "resa": [s.resa for s in per]}
    ms, st = solve(g)
    per = [g.modes_mgstats(m) for m in range(nl)]
    r["modal_warm"] = {"ms": ms, "cycles": [s.i for s in per], "nrelax": [s.nrelax for s in per], "resa": [s.resa for s in per]}
    row["rounds"].append(r)
g.option("TOLERANCE", 1e-3)
# the profiled solve: event pairs around the finest level's sweeps, the residual passes and the launch-bound levels of every cycle
g.set_const()
g.set(F["Q"], q0)
g.option("profile", 1)
g.profile_reset()
ms, st = solve(g)
row["profiled_modal_cold"] = {"ms": ms, **{k: dict(zip(("avg_ms", "count"), g.profile_read(k))) for k in ("helm_relax", "helm_residual", "helm_coarse")}}
row["levels"] = [g.level_dims(k) for k in range(g.nlevels())]
g.option("profile", 0)
g.close()
for form, compact in (("compact", None), ("general", 0)):
    g = handle(compact)
    g.option("mode_pv_invert", 1)
    g.set_const()
    assert g.param("modes_compact") == (form == "compact")
    extra = 0 if form == "compact" else 1
    sweep = min(g.bench_kernel("helm_sweep", 20) for _ in range(3))
    resid = min(g.bench_kernel("helm_residual", 20) for _ in range(3))
    row[form] = {"sweep_ms": sweep, "sweep_bytes": (3 + extra) * w, "sweep_TBps": (3 + extra) * w / sweep / 1e9,
                 "residual_ms": resid, "residual_bytes": (3 + extra) * w, "residual_TBps": (3 + extra) * w / resid / 1e9}
    if form == "compact":
        g.option("mode_pv_invert", 0)
        row["layered_sweep_ms"] = min(g.bench_kernel("sweep", 20) for _ in range(3))          # k_relax_color, both colours
        row["layered_residual_ms"] = min(g.bench_kernel("residual", 20) for _ in range(3))
    g.close()
print(json.dumps(row), flush=True)
