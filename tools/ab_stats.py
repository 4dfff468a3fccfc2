"""running statistics, ms per step, product build, same process and GPU:
 off     msom_step alone (option "stats" never set);
 (a)     msom_step with stats = 1: one k_stats_acc sample per step on the library's stream, mask PSI | Q and the full mask;
 (b)     the best a caller of the parent commit can do: msom_step, then msom_get_field of PSI and Q into device tensors and the same sums
         as torch elementwise operations on the device (the ghost ring of psi rebuilt with slices for the velocities).  After msom_step
         the handle's psi is the predictor's, not the one that belongs to q: (b) cannot sample the consistent pair (a) samples.
20 steps after 3 warm-up steps, msom_sync (and torch.cuda.synchronize for b) before each clock read; the loops alternate, two rounds, the
best counts.  Usage: python tools/ab_stats.py [off] [N NL ...]   (default 512 3 4096 6); prints one JSON line per size.  `off` measures
only msom_step and uses nothing newer than msom_step / msom_sync, so the same file run from the root of a checkout of the parent commit
gives the parent's number (built and run the same way); DESIGN section 8c compares the two."""
import json, sys, time
sys.path.insert(0, '.')
from msom_amd import QG, FIELDS as F, workloads as wl
STEPS, WARM = 20, 3
argv = sys.argv[1:]
off_only = bool(argv) and argv[0] == "off"
args = [int(a) for a in argv[off_only:]] or [512, 3, 4096, 6]
if not off_only:
    import torch
    from msom_amd import STATS as ST
    MASKS = {"psi_q": 1 << ST["PSI"] | 1 << ST["Q"], "full": (1 << ST["NACC"]) - 1}
for N, nl in zip(args[0::2], args[1::2]):
    def make():
        g = QG(wl.double_gyre_params(N, nl)); g.option("quiet", 1)
        g.set(F["PSI"], wl.synthetic_psi(nl, N, N)); g.set_const(); g.set_tnext(float("inf"))
        return g
    def stepper(g):
        def fn(n):
            for _ in range(n): g.step()
        return fn
    def caller_loop(b, full):
        shape = (nl, N, N)
        psi, q = (torch.empty(shape, dtype=torch.float64, device="cuda") for _ in range(2))
        S = [torch.zeros(shape, dtype=torch.float64, device="cuda") for _ in range(7 if full else 2)]
        pg = torch.zeros((nl, N + 2, N + 2), dtype=torch.float64, device="cuda") if full else None
        r2 = 1.0 / (2.0 * (b.param("L0") / N))
        def fn(n):
            for _ in range(n):
                dt = b.step()
                assert b.L.msom_get_field(b.h, F["PSI"], psi.data_ptr()) == 0 and b.L.msom_get_field(b.h, F["Q"], q.data_ptr()) == 0
                S[0].add_(psi, alpha=dt); S[1].add_(q, alpha=dt)
                if full:
                    S[2].addcmul_(psi, psi, value=dt); S[3].addcmul_(q, q, value=dt)
                    pg[:, 1:-1, 1:-1] = psi       # ghost ring of dirichlet(0): x walls, then y walls over the x ghosts
                    pg[:, 1:-1, 0] = -psi[:, :, 0]; pg[:, 1:-1, -1] = -psi[:, :, -1]
                    pg[:, 0, :] = -pg[:, 1, :]; pg[:, -1, :] = -pg[:, -2, :]
                    u = (pg[:, :-2, 1:-1] - pg[:, 2:, 1:-1]) * r2
                    v = (pg[:, 1:-1, 2:] - pg[:, 1:-1, :-2]) * r2
                    S[4].add_(u * u + v * v, alpha=0.5 * dt); S[5].addcmul_(u, q, value=dt); S[6].addcmul_(v, q, value=dt)
        return fn
    def timed(fn, g):
        g.sync()
        if not off_only: torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(STEPS)
        g.sync()
        if not off_only: torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3
    g = make()
    loops = {"off": (stepper(g), g)}
    if not off_only:
        for name, mask in MASKS.items():
            a, b = make(), make()
            a.stats_begin(mask); a.option("stats", 1)
            loops["stats_" + name] = (stepper(a), a)
            loops["caller_" + name] = (caller_loop(b, name == "full"), b)
    for fn, _ in loops.values(): fn(WARM)
    ms = {k: [] for k in loops}
    for rep in range(2):
        for k, (fn, g) in loops.items(): ms[k].append(timed(fn, g))
    print(json.dumps({"N": N, "nl": nl, "steps": STEPS, "warmup": WARM, "ms_per_step": {k: min(v) for k, v in ms.items()}, "rounds": ms}), flush=True)
    for _, g in loops.values(): g.close()
    loops.clear()
    if not off_only: torch.cuda.empty_cache()
