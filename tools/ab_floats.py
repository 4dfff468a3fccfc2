"""Lagrangian floats, cost per step, product build, one process and GPU: ms per msom_step with the floats of a handle paused (option
"floats" = 0: the launches of a handle without floats) and moving (= 1), alternating 0 / n / 0 / n on the same handle, for n floats
placed uniformly at random in the box and clustered in one gyre (a disc of radius L0 / 16 around (L0 / 4, 3 L0 / 4)).  STEPS steps
after 3 warm-up steps, msom_sync before each clock read.  The kernels' own time comes from HIP events around the two k_floats_stage
launches of a step (option "profile" = 1, slot "floats", in a pass of its own so that the events are not in the timed steps).
Usage: python tools/ab_floats.py [N NL [out.json]]   (default 4096 6 profiles/floats.json); prints and writes one JSON document."""
import json, os, sys, time
sys.path.insert(0, '.')
import numpy as np
from msom_amd import QG, FIELDS as F, workloads as wl
STEPS, WARM, ROUNDS = 10, 3, 2
N, nl = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (4096, 6)
out = sys.argv[3] if len(sys.argv) > 3 else os.path.join("profiles", "floats.json")
g = QG(wl.double_gyre_params(N, nl)); g.option("quiet", 1)
g.set(F["PSI"], wl.synthetic_psi(nl, N, N)); g.set_const(); g.set_tnext(float("inf"))
L0 = g.param("L0")
rng = np.random.default_rng(0)


def place(kind, n):
    if kind == "uniform":
        return rng.uniform(0, L0, n), rng.uniform(0, L0, n)
    r, th = L0 / 16 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    return L0 / 4 + r * np.cos(th), 3 * L0 / 4 + r * np.sin(th)


def timed(steps):
    g.sync()
    t0 = time.perf_counter()
    for _ in range(steps): g.step()
    g.sync()
    return (time.perf_counter() - t0) / steps * 1e3


for _ in range(WARM): g.step()
res = {"N": N, "nl": nl, "steps": STEPS, "warmup": WARM, "cases": []}
for n in (1 << 16, 1 << 20):
    for kind in ("uniform", "clustered"):
        x, y = place(kind, n)
        g.floats_begin(x, y, rng.integers(0, nl, n).astype(np.int32))
        g.step()   # first touch of the float arrays
        off, on = [], []
        for _ in range(ROUNDS):
            g.option("floats", 0); off.append(timed(STEPS))
            g.option("floats", 1); on.append(timed(STEPS))
        g.option("profile", 1); g.profile_reset()
        for _ in range(STEPS): g.step()
        ms, launches = g.profile_read("floats")
        g.option("profile", 0)
        case = {"n": n, "placement": kind, "ms_per_step_0_floats": off, "ms_per_step_n_floats": on, "kernel_ms_per_stage": ms, "stage_launches": launches,
                "clamped": g.param("floats_clamped"), "lost": g.param("floats_lost")}
        print(json.dumps(case), flush=True)
        res["cases"].append(case)
        g.floats_end()
g.close()
os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
json.dump(res, open(out, "w"), indent=1)
