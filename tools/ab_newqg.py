"""newqg dialect (msom_create_newqg), product build, the constants of the sample params.in at N x N x 1:
 * k_nq_rhs with the advance folded in ("nq_rhs", counted 4 w: psi and q_in read, zeta and q_out written, w = 8 N^2) and without
   ("nq_rhs_dq", 3 w) against k_rhs_lpw's one-layer case on an msqg handle of the same N ("rhs" 2 w: psi read, dq written; "rhs_adv" 3 w),
   HIP events, 20 back-to-back launches, best of 3, the handles alternating in one process;
 * msom_invertq at TOLERANCE 1e-5, zero and warm start, with cycle counts, gp_low = 2500 and gp_low = 0, and the msqg handle's layered
   nl = 1 solve of the same q (gp_low = 0 is the same Poisson problem);
 * msom_step per step, host clock around steps that end in a synchronise.
Usage: python tools/ab_newqg.py [N]   (default 4096) -> one JSON line, kept as profiles/newqg.json."""
import ctypes as C
import json
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np
from msom_amd import NewQG, QG, FIELDS as F, workloads as wl
from msom_amd.api import MGStats

N = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
w = 8.0 * N * N
SAMPLE = ("N = {N}\nL0 = 100\nf0 = 46.5\nhEkb = 0.0\ntau0 = 1e-3\nnu = 0.5\nbeta = 0.5\nsbc = 0.\ndh = [1.0]\ngp_low = {gp}\nDT = 5.e-2\ntend = 200.\n"
          "dtout = 0.1\nCFL = 0.2\nTOLERANCE = 1e-5\n")


def solve(g):
    st = MGStats()
    g.sync()
    t0 = time.perf_counter()
    rc = g.L.msom_invertq(g.h, None, None, C.byref(st))   # q = the handle's Q, psi stays on the device; synchronises on return
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0, g.L.msom_last_error()
    return {"ms": ms, "cycles": st.i, "nrelax": st.nrelax, "resa": st.resa}


psi0 = wl.synthetic_psi(1, N, N, amp=500.0)
zero = np.zeros((1, N, N))


def newqg(gp):
    g = NewQG(SAMPLE.format(N=N, gp=gp))
    g.option("quiet", 1)
    g.set(F["PSI"], psi0)
    g.set_const()
    return g


row = {"N": N, "w_bytes": w}
n = newqg(2500.0)
m = QG(wl.double_gyre_params(N, 1, L0=100.0))
m.option("quiet", 1)
m.set(F["PSI"], psi0)
m.set_const()
row["nq_rows"] = n.param("nq_rows")
kern = {"nq_rhs": (n, 4), "rhs_adv": (m, 3), "nq_rhs_dq": (n, 3), "rhs": (m, 2)}
best = {k: 1e30 for k in kern}
for _ in range(3):   # alternating
    for k, (g, _) in kern.items():
        best[k] = min(best[k], g.bench_kernel(k, 20))
row["kernels"] = {k: {"ms": best[k], "bytes": kern[k][1] * w, "TBps": kern[k][1] * w / best[k] / 1e9} for k in kern}
row["helm_sweep_ms"] = min(n.bench_kernel("helm_sweep", 20) for _ in range(3))
row["helm_residual_ms"] = min(n.bench_kernel("helm_residual", 20) for _ in range(3))

# the solves: one right-hand side per gp_low, q = comp_q(psi0)
row["solve"] = {}
for gp in (2500.0, 0.0):
    g = n if gp else newqg(0.0)
    q0 = g.get(F["Q"])
    r = {}
    for rnd in range(2):   # the first round warms the code objects up and is reported too
        g.set(F["PSI"], zero)
        r[f"zero_{rnd}"] = solve(g)
        r[f"warm_{rnd}"] = solve(g)
    if not gp:
        m.option("TOLERANCE", 1e-5)
        m.set(F["Q"], q0)
        for rnd in range(2):
            m.set(F["PSI"], zero)
            r[f"layered_zero_{rnd}"] = solve(m)
            r[f"layered_warm_{rnd}"] = solve(m)
        g.close()
    row["solve"][f"gp_low_{gp:g}"] = r

# steps
n.set(F["PSI"], psi0)
n.set_const()
for _ in range(3):
    n.step()
n.sync()
t0 = time.perf_counter()
for _ in range(10):
    n.step()
n.sync()
row["step_ms"] = (time.perf_counter() - t0) * 1e2
st = n.mgstats()
row["step_last_solve"] = {"cycles": st.i, "nrelax": st.nrelax, "resa": st.resa}
n.close()
m.close()
print(json.dumps(row), flush=True)
