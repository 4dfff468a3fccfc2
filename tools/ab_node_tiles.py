"""Vertex model on tiles, for information: ms per step of px x py tiles as host threads on ONE GPU over the in-process transport, next to
the single tile of the same global grid run with the option values the tiled handle resolves to, and with the defaults.  The tiles
share the device and meet in host barriers at every exchange, so this measures the tile layer's launch and copy overhead on one
device -- it says nothing about scaling.  Also prints the halo exchanges per step, counted by the library, and the count the cycle
structure predicts ("Vertex model on tiles").
usage: python tools/ab_node_tiles.py [--wavelet] [PX PY TILE NL [out.json]]      (default 2 2 1024 3: four tiles of 1024^2 cells, 2048^2 in all)
--wavelet: instead of steps, ms of one msomn_wavelet_filter and of one filtered msomn_noise_draw on the tiles (option wavelet_tiles) and on
the single tile, with the halo exchanges each posts ("Wavelet pyramid on tiles")."""
import json
import os
import sys
import threading
import time

sys.path.insert(0, ".")
import numpy as np

from msom_amd import NodeQG
from msom_amd.tiling import node_assemble, node_tile_window

WAVELET = "--wavelet" in sys.argv
sys.argv = [a for a in sys.argv if a != "--wavelet"]
px, py, tile, nl = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (2, 2, 1024, 3)
out_path = sys.argv[5] if len(sys.argv) > 5 else None
N = tile * px
assert tile * py == N, "square global grid: px == py, or give tiles of N / px by N / py cells"
WARM, STEPS = 2, 5
DH = {1: "[1.0]", 2: "[0.3,0.7]", 3: "[0.1,0.3,0.6]"}
N2 = {1: "[1.0]", 2: "[4000.]", 3: "[9000.,3000.]"}
par = (f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\nbc_fac = 1.0\ndh = {DH[nl]}\nN2 = {N2[nl]}\n"
       f"DT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = 1e-5\n" + ("gp_low = 0.02\n" if nl == 1 else "")
       + ("Lfmax = 25.0\nLfmin = 6.0\namp_stoch = 0.3\nL_filt = 8.0\n" if WAVELET else ""))
x = np.arange(N + 1) / N
mask = np.ones((1, N + 1, N + 1))
mask[0, N // 4: N // 4 + N // 8, N // 2 - N // 16: N // 2 + N // 16] = 0   # an island across the vertical seam
mask[0, 0, :] = mask[0, -1, :] = mask[0, :, 0] = mask[0, :, -1] = 0
psi = np.stack([1e-2 / (1 + 0.3 * l) * np.outer(np.sin((1 + l) * np.pi * x), np.sin(2 * np.pi * x)) for l in range(nl)]) * mask
KEYS = ["node_pfused", "node_tile_s", "node_march_s", "node_march", "tiled_relax", "node_corr_fused", "node_rhs_fused", "node_split", "mg_coarse"]


def run(g, sy=slice(None), sx=slice(None)):
    g.set_option("quiet", 1)
    g.set("MASK", mask[:, sy, sx])
    g.set("PSI", psi[:, sy, sx])
    g.set_const()
    g.set_tnext(float("inf"))
    for _ in range(WARM):
        g.step(True)
    g.profile_reset()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        g.step(True)
    g.get("PSI")
    ms = (time.perf_counter() - t0) / STEPS * 1e3
    return dict(ms=ms, psi=g.get("PSI"), exchanges=g.param("exchanges") / STEPS, agg=g.param("agg_level"), opts={k: g.param(k) for k in KEYS})


def run_wavelet(g, sy=slice(None), sx=slice(None)):
    for k, v in dict(quiet=1, wavelet_tiles=1, stochastic=1, noise_mode=1, seed=5).items():
        g.set_option(k, v)
    g.set("MASK", mask[:, sy, sx])
    g.set("PSI", psi[:, sy, sx])
    g.set_const()
    g.set_tnext(float("inf"))
    root = N.bit_length() - 1
    wait = lambda: g.csig(root)                # one cell to the host behind everything queued
    out = dict(agg=g.param("agg_level"), opts={k: g.param(k) for k in KEYS})
    for name, call in (("wavelet_filter", lambda: g.wavelet_filter(0.5)), ("noise_draw_filtered", lambda: g.noise_draw(filter=True))):
        for _ in range(WARM):
            call()
        wait()
        e0, t0 = g.param("exchanges"), time.perf_counter()
        for _ in range(STEPS):
            call()
        wait()
        out[name] = dict(ms=(time.perf_counter() - t0) / STEPS * 1e3, exchanges=(g.param("exchanges") - e0) / STEPS, cycles=g.mgstats().i)
    out["psi"], out["noise"] = g.get("PSI"), g.noise()
    return out


if WAVELET:
    run = run_wavelet
uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
res = [None] * (px * py)


def worker(rank):
    g = NodeQG(par, tiled=(px, py, rank, uid))
    res[rank] = run(g, *node_tile_window(N, px, py, rank))
    g.close()


th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(px * py)]
[t.start() for t in th]
[t.join(timeout=900) for t in th]
assert all(r is not None for r in res), "a tile thread hung"
tiled_ms = None if WAVELET else max(r["ms"] for r in res)
g = NodeQG(par)
for k, v in res[0]["opts"].items():
    g.set_option(k, v)
same = run(g)
g.close()
g = NodeQG(par)
dflt = run(g)
g.close()
if WAVELET:
    from msom_amd.tiling import cell_assemble
    kg = int(res[0]["agg"])
    report = dict(grid=f"{N}^2 x {nl}", tiles=f"{px} x {py} of {tile}^2 cells", calls_timed=STEPS, agg_level=kg, exchanges_per_transform_counted=2 * kg - 1,
                  psi_equals_single_tile=bool(np.array_equal(node_assemble([r["psi"] for r in res], N, px, py), same["psi"])),
                  noise_equals_single_tile=bool(np.array_equal(cell_assemble([r["noise"] for r in res], N, px, py), same["noise"])),
                  resolved_options=res[0]["opts"],
                  note="tiles are host threads sharing one device: launch and copy overhead of the tile layer, not scaling; wavelet_filter "
                       "includes its solve (cycles of the last one given) and comp_q; the RCCL path is not measured")
    for name in ("wavelet_filter", "noise_draw_filtered"):
        report[name] = dict(ms_tiled_threads_one_gpu=round(max(r[name]["ms"] for r in res), 3), ms_single_same_options=round(same[name]["ms"], 3),
                            ms_single_default_options=round(dflt[name]["ms"], 3), exchanges_tiled=res[0][name]["exchanges"],
                            cycles_of_last_solve=res[0][name]["cycles"])
    print(json.dumps(report, indent=1))
    if out_path:
        with open(out_path, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    sys.exit(0)
equal = bool(np.array_equal(node_assemble([r["psi"] for r in res], N, px, py), same["psi"]))
kg = int(res[0]["agg"])
report = dict(grid=f"{N}^2 x {nl}", tiles=f"{px} x {py} of {tile}^2 cells", steps=STEPS, agg_level=kg,
              ms_per_step_tiled_threads_one_gpu=round(tiled_ms, 3), ms_per_step_single_same_options=round(same["ms"], 3),
              ms_per_step_single_default_options=round(dflt["ms"], 3), exchanges_per_step=res[0]["exchanges"],
              exchanges_per_cycle_counted=1 + 12 * kg, exchanges_per_tendency_counted=3 if nl > 1 else 2,
              # a step is two solves and two tendencies: (c1 + c2) cycles, two closing residual passes
              cycles_per_step_implied=(res[0]["exchanges"] - 2 - 2 * (3 if nl > 1 else 2)) / (1 + 12 * kg),
              psi_equals_single_tile=equal, resolved_options=res[0]["opts"],
              note="tiles are host threads sharing one device: launch and copy overhead of the tile layer, not scaling")
print(json.dumps(report, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
