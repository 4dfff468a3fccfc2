"""Lagrangian floats of the vertex model, cost of a stage, product build, one process and GPU: 2^20 floats placed uniformly at random
on the 2049^2 x 3 island workload of tools/prof_node.py's size (msomn_floats_*).

    python tools/ab_node_floats.py [N NL NFLOATS [out.json]]      (default 2048 3 1048576 profiles/node_floats.json)

Two figures, next to the counted bytes of a stage (4 corner doubles, or 8 with psi_pg, gathered; 5 state doubles read: x, y, xh, yh
and the layer word; 2 written):
  - call: one timed loop of ROUNDS pairs msomn_floats_stage(1), msomn_floats_stage(2) after WARM pairs; every call ends in a stream
    synchronise, so the figure is launch + kernel + synchronise;
  - kernel: the workload run once more as a child process under rocprofv3 --kernel-trace --stats (a run of its own); the average
    duration of k_nfloats_stage<PG, STAGE, REC> per instantiation, msomn_step's launches and the by-hand ones together.
`work` as the first argument runs the workload alone and prints the call figure as one JSON line."""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, time
sys.path.insert(0, '.')
import numpy as np
WARM, ROUNDS, STEPS = 10, 200, 5


def work(N, nl, n):
    from msom_amd import NodeQG
    dh, n2 = {1: ("[1.0]", "[1.0]"), 2: ("[0.3,0.7]", "[4000.]"), 3: ("[0.1,0.3,0.6]", "[9000.,3000.]")}[nl]
    g = NodeQG(f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\nbc_fac = 1.0\ndh = {dh}\nN2 = {n2}\n"
               f"DT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = 1e-5\n")
    g.set_option("quiet", 1)
    x = np.arange(N + 1) / N
    mk = np.ones((1, N + 1, N + 1))
    mk[0, N // 4: N // 4 + N // 8, N // 2: N // 2 + N // 8] = 0
    mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
    psi = np.stack([1e-2 * (1 - 0.2 * l) * sum(np.sin(1.3 * k + 2.1 * m + 0.7 * l) / (k * m) * np.outer(np.sin(m * np.pi * x), np.sin(k * np.pi * x))
                                              for k in range(1, 4) for m in range(1, 4)) for l in range(nl)]) * mk
    g.set("MASK", mk); g.set("PSI", psi); g.set_const(); g.set_tnext(float("inf"))
    g.step()
    rng = np.random.default_rng(0)
    L0 = g.param("L0")
    g.floats_begin(rng.uniform(0, L0, n), rng.uniform(0, L0, n), rng.integers(0, nl, n).astype(np.int32))
    g.floats_record(every=1, capacity=STEPS + 1, field="Q")
    for _ in range(STEPS):   # the launches of msomn_step: stage 1, and stage 2 with the record of q
        g.step()
    dt = g.dt
    for _ in range(WARM):
        g.floats_stage(1, dt); g.floats_stage(2, dt)
    t0 = time.perf_counter()
    for _ in range(ROUNDS):
        g.floats_stage(1, dt); g.floats_stage(2, dt)
    call_ms = (time.perf_counter() - t0) / (2 * ROUNDS) * 1e3
    res = {"N": N, "nl": nl, "floats": n, "placement": "uniform", "warmup_pairs": WARM, "timed_pairs": ROUNDS, "ms_per_stage_call": call_ms,
           "clamped": g.param("floats_clamped"), "lost": g.param("floats_lost"), "on_land": g.param("floats_on_land"),
           "counted_bytes_per_stage": n * (4 * 8 + 4 * 8 + 4 + 2 * 8), "counted": "4 corner doubles gathered, x y xh yh and the layer word read, 2 doubles written"}
    g.close()
    return res


if __name__ == "__main__":
    argv = sys.argv[1:]
    child = argv[:1] == ["work"]
    argv = argv[1:] if child else argv
    N, nl, n = (int(argv[0]), int(argv[1]), int(argv[2])) if len(argv) > 2 else (2048, 3, 1 << 20)
    if child:
        print(json.dumps(work(N, nl, n)), flush=True)
        sys.exit(0)
    out = argv[3] if len(argv) > 3 else os.path.join("profiles", "node_floats.json")
    # the traced child first, while this process has not touched the GPU
    d = tempfile.mkdtemp(prefix="node_floats_trace_")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "nfl", "--", sys.executable, __file__, "work",
                        str(N), str(nl), str(n)], capture_output=True, text=True, timeout=900)
    if p.returncode:
        print(p.stdout[-2000:], p.stderr[-2000:])
        sys.exit(1)
    res = work(N, nl, n)
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))[0]
    res["kernels"] = [{"name": r["Name"], "calls": int(r["Calls"]), "avg_ms": float(r["AverageNs"]) / 1e6, "min_ms": float(r["MinNs"]) / 1e6,
                       "max_ms": float(r["MaxNs"]) / 1e6} for r in csv.DictReader(open(f)) if "k_nfloats" in r["Name"]]
    shutil.rmtree(d, ignore_errors=True)
    for k in res["kernels"]:
        k["counted_GBps"] = res["counted_bytes_per_stage"] / (k["avg_ms"] * 1e-3) / 1e9 if "stage" in k["name"] else None
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)
