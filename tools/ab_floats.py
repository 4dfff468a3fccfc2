"""Lagrangian floats, cost per step, product build, one process and GPU: ms per msom_step with the floats of a handle paused (option
"floats" = 0: the launches of a handle without floats) and moving (= 1), alternating 0 / n / 0 / n on the same handle, for n floats
placed uniformly at random in the box and clustered in one gyre (a disc of radius L0 / 16 around (L0 / 4, 3 L0 / 4)).  STEPS steps
after 3 warm-up steps, msom_sync before each clock read.  The kernels' own time comes from HIP events around the two k_floats_stage
launches of a step (option "profile" = 1, slot "floats", in a pass of its own so that the events are not in the timed steps).
Usage: python tools/ab_floats.py [N NL [out.json]]   (default 4096 6 profiles/floats.json); prints and writes one JSON document.

python tools/ab_floats.py tiles [TILE NL [NFLOATS [out.json]]]   (default 1024 6 1048576 profiles/floats_tiles.json): floats on 2 x 2
in-process tiles of TILE^2 x NL (host threads of this process, one GPU; option floats_tiles): the time of k_floats_emigrate (with its
one-lane header launch) and of k_floats_immigrate per phase of the migration pass, from HIP events on the communication stream, next
to k_floats_stage, per rank; and the traffic (floats_migrated per stage).  The in-process transport waits on the host in every
exchange, so no wall time per step is taken here: it would be no figure for the RCCL path, which stays unmeasured."""
import json, os, sys, time
sys.path.insert(0, '.')
import numpy as np
from msom_amd import QG, FIELDS as F, workloads as wl
STEPS, WARM, ROUNDS = 10, 3, 2


def tiles_main(argv):
    import threading
    tile, nl = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (1024, 6)
    n = int(argv[2]) if len(argv) > 2 else 1 << 20
    out = argv[3] if len(argv) > 3 else os.path.join("profiles", "floats_tiles.json")
    px = py = 2
    gn, steps = tile * px, 5
    params = wl.double_gyre_params(gn, nl, extra=f"MGLEVELS = {int(np.log2(tile))}\n")
    psi = wl.synthetic_psi(nl, gn, gn, amp=5.0)   # an eddy field in which the floats move at the CFL limit
    uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
    rng = np.random.default_rng(0)
    res, errs = [None] * (px * py), []

    def worker(rank):
        try:
            g = QG(params, tiled=(px, py, rank, uid)); g.option("quiet", 1); g.option("floats_tiles", 1)
            ix, iy = rank % px, rank // px
            g.set(F["PSI"], psi[:, iy * tile:(iy + 1) * tile, ix * tile:(ix + 1) * tile]); g.set_const(); g.set_tnext(float("inf"))
            L0 = g.param("L0")
            g.floats_begin(x0 * L0, y0 * L0, lay)
            for _ in range(2): g.step()
            m0 = g.param("floats_migrated")
            g.option("profile", 1); g.profile_reset()
            for _ in range(steps): g.step()
            r = {"rank": rank}
            for slot, key in (("floats", "stage"), ("floats_emigrate", "emigrate"), ("floats_immigrate", "immigrate")):
                ms, launches = g.profile_read(slot)
                r[f"{key}_ms_per_launch"], r[f"{key}_launches"] = ms, launches
            g.option("profile", 0)
            r.update(resident=g.param("floats_resident"), migrated_per_stage=(g.param("floats_migrated") - m0) / (2 * steps), unsent=g.param("floats_unsent"),
                     lost=g.param("floats_lost"), clamped=g.param("floats_clamped"), msg_cap=g.param("floats_msg_cap"))
            res[rank] = r
            g.close()
        except Exception as e:  # noqa: BLE001
            errs.append((rank, repr(e)))

    x0, y0, lay = rng.uniform(0, 1, n), rng.uniform(0, 1, n), rng.integers(0, nl, n).astype(np.int32)
    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(px * py)]
    for t in th: t.start()
    for t in th: t.join(timeout=300)
    doc = {"tiles": [px, py], "tile": tile, "nl": nl, "floats": n, "placement": "uniform", "steps": steps, "errors": errs, "ranks": res}
    print(json.dumps(doc), flush=True)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(doc, open(out, "w"), indent=1)
    return 1 if errs or any(r is None for r in res) else 0


if len(sys.argv) > 1 and sys.argv[1] == "tiles":
    sys.exit(tiles_main(sys.argv[2:]))
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
