"""Lagrangian floats of the vertex model, cost of a stage, product build, one process and GPU: 2^20 floats placed uniformly at random
on the 2049^2 x 3 island workload of tools/prof_node.py's size (msomn_floats_*).

    python tools/ab_node_floats.py [N NL NFLOATS [out.json]]      (default 2048 3 1048576 profiles/node_floats.json)

Two figures, next to the counted bytes of a stage (4 corner doubles, or 8 with psi_pg, gathered; 5 state doubles read: x, y, xh, yh
and the layer word; 2 written):
  - call: one timed loop of ROUNDS pairs msomn_floats_stage(1), msomn_floats_stage(2) after WARM pairs; every call ends in a stream
    synchronise, so the figure is launch + kernel + synchronise;
  - kernel: the workload run once more as a child process under rocprofv3 --kernel-trace --stats (a run of its own); the average
    duration of k_nfloats_stage<PG, STAGE, REC> per instantiation, msomn_step's launches and the by-hand ones together.
`work` as the first argument runs the workload alone and prints the call figure as one JSON line.

    python tools/ab_node_floats.py tiles [N NL NFLOATS [out.json]]      (default 2048 3 1048576 profiles/node_floats_tiles.json)

The floats on tiles (option floats_tiles, "On tiles" in section 8l): 2 x 2 tiles of (N / 2)^2 cells as host threads of one process over
the in-process transport, the same island and the same floats; every rank steps STEPS times and then makes TILE_ROUNDS stage pairs by
hand with psi frozen and a dt of 0.4 cells per step for the fastest float, so that floats cross the seams (the model's own step moves
them by a small fraction of a cell).  Reported per rank, from a `rocprofv3 --kernel-trace` run of the workload as a child process with the launches told apart by
the launching thread: the durations of k_nfloats_stage_tiled, k_floats_emigrate, k_floats_header and k_floats_immigrate; and from the
counters the records that cross per stage.  The wall time of a stage call is that of four threads sharing one GPU and meeting in
host barriers: it says nothing about RCCL, which stays unmeasured.  `tiles_work` runs that workload alone."""
import csv, glob, json, os, shutil, subprocess, sys, tempfile, threading, time
sys.path.insert(0, '.')
import numpy as np
WARM, ROUNDS, STEPS = 10, 200, 5
TILE_ROUNDS = 50


def params_of(N, nl):
    dh, n2 = {1: ("[1.0]", "[1.0]"), 2: ("[0.3,0.7]", "[4000.]"), 3: ("[0.1,0.3,0.6]", "[9000.,3000.]")}[nl]
    return (f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\nbc_fac = 1.0\ndh = {dh}\nN2 = {n2}\n"
            f"DT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = 1e-5\n")


def fields_of(N, nl):
    x = np.arange(N + 1) / N
    mk = np.ones((1, N + 1, N + 1))
    mk[0, N // 4: N // 4 + N // 8, N // 2: N // 2 + N // 8] = 0
    mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
    psi = np.stack([1e-2 * (1 - 0.2 * l) * sum(np.sin(1.3 * k + 2.1 * m + 0.7 * l) / (k * m) * np.outer(np.sin(m * np.pi * x), np.sin(k * np.pi * x))
                                              for k in range(1, 4) for m in range(1, 4)) for l in range(nl)]) * mk
    return mk, psi


def work(N, nl, n):
    from msom_amd import NodeQG
    g = NodeQG(params_of(N, nl))
    g.set_option("quiet", 1)
    mk, psi = fields_of(N, nl)
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


def tiles_work(N, nl, n, px=2, py=2):
    """the floats on px x py in-process tiles; one dict per rank, with the native id of the thread that made the rank's launches"""
    from msom_amd import NodeQG
    from msom_amd.tiling import node_tile_window
    mk, psi = fields_of(N, nl)
    rng = np.random.default_rng(0)
    x0, y0, lay = rng.uniform(0, 100.0, n), rng.uniform(0, 100.0, n), rng.integers(0, nl, n).astype(np.int32)
    uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
    out, errs = [None] * (px * py), []
    dmax, meet = [0.0] * (px * py), threading.Barrier(px * py)

    def rank_body(rank):
        try:
            g = NodeQG(params_of(N, nl), tiled=(px, py, rank, uid))
            g.set_option("quiet", 1)
            g.set_option("floats_tiles", 1)
            sy, sx = node_tile_window(N, px, py, rank)
            g.set("MASK", mk[:, sy, sx]); g.set("PSI", psi[:, sy, sx]); g.set_const(); g.set_tnext(float("inf"))
            g.step()
            g.floats_begin(x0, y0, lay)
            res = {"rank": rank, "thread": threading.get_native_id(), "resident_begin": g.param("floats_resident"), "msg_cap": g.param("floats_msg_cap")}
            g.floats_record(every=1, capacity=STEPS + 1, field="Q")
            for _ in range(STEPS):
                g.step()
            # by hand with the dt that moves the fastest float by 0.4 cells per step (psi frozen), so that floats do cross the seams:
            # a velocity component is at most max |difference of neighbouring vertices| * idx, the maximum taken over the tiles
            P = g.get("PSI")
            dmax[rank] = max(np.abs(np.diff(P, axis=1)).max(), np.abs(np.diff(P, axis=2)).max())
            meet.wait(timeout=300)
            dt = 0.4 / (max(dmax) * (N / 100.0) ** 2)
            res["dt_by_hand"] = dt
            m0 = g.param("floats_migrated")
            t0 = time.perf_counter()
            for _ in range(TILE_ROUNDS):
                g.floats_stage(1, dt); g.floats_stage(2, dt)
            res["ms_per_stage_call_in_process"] = (time.perf_counter() - t0) / (2 * TILE_ROUNDS) * 1e3
            m1 = g.param("floats_migrated")
            res.update(records_crossing_per_stage_by_hand=(m1 - m0) / (2 * TILE_ROUNDS), records_crossing_per_stage_in_step=m0 / (2 * STEPS),
                       resident_end=g.param("floats_resident"), unsent=g.param("floats_unsent"), clamped=g.param("floats_clamped"),
                       lost=g.param("floats_lost"), on_land=g.param("floats_on_land"))
            g.close()
            out[rank] = res
        except Exception as e:  # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=rank_body, args=(r,), daemon=True) for r in range(px * py)]
    for t in th:
        t.start()
    deadline = time.monotonic() + 420
    for t in th:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    if errs or any(o is None for o in out):
        raise SystemExit(f"tiles_work: {errs or 'a tile thread hung'}")
    return {"N": N, "nl": nl, "floats": n, "px": px, "py": py, "placement": "uniform", "steps": STEPS, "stage_pairs_by_hand": TILE_ROUNDS, "ranks": out}


def tiles_main(N, nl, n, out):
    d = tempfile.mkdtemp(prefix="node_floats_tiles_trace_")
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "nflt", "--", sys.executable, __file__, "tiles_work",
                        str(N), str(nl), str(n)], capture_output=True, text=True, timeout=900)
    if p.returncode:
        print(p.stdout[-2000:], p.stderr[-2000:])
        sys.exit(1)
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    names = ("k_nfloats_stage_tiled", "k_nfloats_interp_tiled", "k_floats_emigrate", "k_floats_header", "k_floats_immigrate")
    by = {}
    for r in csv.DictReader(open(f)):
        nm = next((k for k in names if k in r["Kernel_Name"]), None)
        if nm:
            by.setdefault((int(r["Thread_Id"]), nm), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    shutil.rmtree(d, ignore_errors=True)
    for rk in res["ranks"]:
        rk["kernels"] = [{"name": nm, "calls": len(v), "avg_ms": float(np.mean(v)), "min_ms": float(np.min(v)), "max_ms": float(np.max(v))}
                         for (tid, nm), v in sorted(by.items()) if tid == rk["thread"]]
    res["note"] = "four tile threads share one GPU and meet in host barriers: the call time is not a figure for RCCL"
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(out) or ".", exist_ok=True)
    json.dump(res, open(out, "w"), indent=1)


if __name__ == "__main__":
    argv = sys.argv[1:]
    if argv[:1] in (["tiles"], ["tiles_work"]):
        mode, argv = argv[0], argv[1:]
        N, nl, n = (int(argv[0]), int(argv[1]), int(argv[2])) if len(argv) > 2 else (2048, 3, 1 << 20)
        if mode == "tiles_work":
            print(json.dumps(tiles_work(N, nl, n)), flush=True)
        else:
            tiles_main(N, nl, n, argv[3] if len(argv) > 3 else os.path.join("profiles", "node_floats_tiles.json"))
        sys.exit(0)
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
