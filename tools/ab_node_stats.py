"""running statistics of the vertex model, ms per step, product build, same process and GPU:
 off     msomn_step alone (option "stats" never set);
 (a)     msomn_step with stats = 1: one k_n_stats_acc sample per step on the handle's stream, mask PSI | Q and the full mask;
 (b)     the best a caller of the parent commit can do: msomn_step, then msomn_get_field of PSI and Q into device tensors and the same
         sums as torch elementwise operations on the device (masked differences on the interior vertices for the full mask).  After
         msomn_step the handle's psi is the predictor's, not the one that belongs to q: (b) cannot sample the pair (a) samples.
The workload is the vertex leg of bench.py without the surface-QG option: (N + 1)^2 x nl vertices, island mask, TOLERANCE 1e-5.
20 steps after 3 warm-up steps, a device synchronisation before each clock read; the loops alternate, four rounds, the best counts
(every handle has taken the same number of steps when its round is timed: a solve's cycle count moves with the flow).  A step is
two multigrid solves, a sample one streaming pass: the difference of two step times does not resolve it, so the sample is also timed
alone, 50 msomn_stats_accumulate calls queued back to back on one tile (no exchange) between two synchronisations.
Usage: python tools/ab_node_stats.py [off] [N NL ...]   (default 2048 3); prints one JSON line per size.  `off` measures only
msomn_step and uses nothing newer than it, so the same file run from the root of a checkout of the parent commit gives the parent's
number."""
import ctypes, json, sys, time
sys.path.insert(0, '.')
import numpy as np
from msom_amd import NodeQG
STEPS, WARM, ROUNDS, NSAMPLE = 20, 3, 4, 50
argv = sys.argv[1:]
off_only = bool(argv) and argv[0] == "off"
args = [int(a) for a in argv[off_only:]] or [2048, 3]
hip = ctypes.CDLL("libamdhip64.so")     # the runtime the library has loaded
if not off_only:
    import torch
    from msom_amd import STATS as ST
    MASKS = {"psi_q": 1 << ST["PSI"] | 1 << ST["Q"], "full": (1 << ST["NACC"]) - 1}
for N, nl in zip(args[0::2], args[1::2]):
    x = np.arange(N + 1) / N
    mk = np.ones((1, N + 1, N + 1))
    mk[0, N // 4: N // 4 + N // 8, N // 2: N // 2 + N // 8] = 0
    mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
    psi0 = np.stack([1e-2 * (1 - 0.2 * l) * sum(np.sin(1.3 * k + 2.1 * m + 0.7 * l) / (k * m) * np.outer(np.sin(m * np.pi * x), np.sin(k * np.pi * x))
                                                for k in range(1, 4) for m in range(1, 4)) for l in range(nl)]) * mk
    dh, n2 = {1: ("[1.0]", "[1.0]"), 2: ("[0.3,0.7]", "[4000.]"), 3: ("[0.1,0.3,0.6]", "[9000.,3000.]")}[nl]
    txt = (f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\nbc_fac = 1.0\n"
           f"dh = {dh}\nN2 = {n2}\nDT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = 1e-5\n" + ("gp_low = 0.02\n" if nl == 1 else ""))
    def make():
        g = NodeQG(txt); g.set_option("quiet", 1)
        g.set("MASK", mk); g.set("PSI", psi0); g.set_const(); g.set_tnext(float("inf"))
        return g
    def stepper(g):
        def fn(n):
            for _ in range(n): g.step(True)
        return fn
    def caller_loop(b, full):
        shape = (nl, N + 1, N + 1)
        psi, q = (torch.empty(shape, dtype=torch.float64, device="cuda") for _ in range(2))
        S = [torch.zeros(shape, dtype=torch.float64, device="cuda") for _ in range(7 if full else 2)]
        m = torch.from_numpy(mk[:, 1:-1, 1:-1]).cuda() if full else None
        r2 = 1.0 / (2.0 * (b.param("L0") / N))
        def fn(n):
            for _ in range(n):
                b.step(True)
                dt = b.dt
                assert b.L.msomn_get_field(b.h, 0, psi.data_ptr()) == 0 and b.L.msomn_get_field(b.h, 1, q.data_ptr()) == 0
                S[0].add_(psi, alpha=dt); S[1].add_(q, alpha=dt)
                if full:
                    S[2].addcmul_(psi, psi, value=dt); S[3].addcmul_(q, q, value=dt)
                    u = (psi[:, :-2, 1:-1] - psi[:, 2:, 1:-1]) * r2 * m      # the boundary ring keeps its zeros
                    v = (psi[:, 1:-1, 2:] - psi[:, 1:-1, :-2]) * r2 * m
                    qi = q[:, 1:-1, 1:-1]
                    S[4][:, 1:-1, 1:-1].add_(u * u + v * v, alpha=0.5 * dt)
                    S[5][:, 1:-1, 1:-1].addcmul_(u, qi, value=dt); S[6][:, 1:-1, 1:-1].addcmul_(v, qi, value=dt)
        return fn
    def timed(fn):
        hip.hipDeviceSynchronize()
        t0 = time.perf_counter()
        fn(STEPS)
        hip.hipDeviceSynchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3
    g = make()
    loops = {"off": (stepper(g), g)}
    if not off_only:
        for name, mask in MASKS.items():
            a, b = make(), make()
            a.stats_begin(mask); a.set_option("stats", 1)
            loops["stats_" + name] = (stepper(a), a)
            loops["caller_" + name] = (caller_loop(b, name == "full"), b)
    for fn, _ in loops.values(): fn(WARM)
    ms = {k: [] for k in loops}
    for rep in range(ROUNDS):
        for k, (fn, _) in loops.items(): ms[k].append(timed(fn))
    out = {"N": N, "nl": nl, "vertices": f"{N + 1}x{N + 1}x{nl}", "steps": STEPS, "warmup": WARM, "ms_per_step": {k: min(v) for k, v in ms.items()}, "rounds": ms,
           "mg_cycles_last_solve": g.mgstats().i}
    if not off_only:
        w = 8.0 * (N + 1) ** 2 * nl      # one [nl][N + 1][N + 1] fp64 field; bytes per sample COUNTED from the design: 6 w and 16 w + the mask
        best = out["ms_per_step"]
        for name, nbytes in (("psi_q", 6 * w), ("full", 16 * w + w / nl)):
            a = loops["stats_" + name][1]
            alone = min(timed(lambda n: [a.stats_accumulate(0.5) for _ in range(NSAMPLE)]) * STEPS / NSAMPLE for _ in range(3))
            out["sample_" + name] = {"counted_bytes": nbytes, "ms_step_difference": best["stats_" + name] - best["off"], "ms_alone": alone,
                                     "counted_TB_per_s": nbytes / (alone * 1e-3) / 1e12}
    print(json.dumps(out), flush=True)
    for _, h in loops.values(): h.close()
    loops.clear()
    if not off_only: torch.cuda.empty_cache()
