"""Vertex model on tiles, for information: the cost of the collective I/O calls of the option io_tiles -- one msomn_state_save (with the
constants), one msomn_state_load and one msomn_write_nc, once each, on px x py tiles as host threads on ONE GPU over the in-process
transport, next to the single tile of the same global grid.  The tiles share the device and rank 0 writes alone, so this is the cost of
the gathers, the host assembly and the file system on one machine; the RCCL path on several GPUs is not measured.
usage: python tools/ab_node_state_tiles.py [PX PY TILE NL [out.json]]      (default 2 2 1024 3: 2049^2 vertices x 3 layers)"""
import json
import os
import sys
import tempfile
import threading
import time

sys.path.insert(0, ".")
import numpy as np

from msom_amd import NodeQG
from msom_amd.tiling import node_tile_window

px, py, tile, nl = (int(a) for a in sys.argv[1:5]) if len(sys.argv) >= 5 else (2, 2, 1024, 3)
out_path = sys.argv[5] if len(sys.argv) > 5 else None
N = tile * px
assert tile * py == N, "square global grid"
DH = {1: "[1.0]", 2: "[0.3,0.7]", 3: "[0.1,0.3,0.6]"}
N2 = {1: "[1.0]", 2: "[4000.]", 3: "[9000.,3000.]"}
par = (f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\nbc_fac = 1.0\ndh = {DH[nl]}\nN2 = {N2[nl]}\n"
       f"DT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = 1e-5\n" + ("gp_low = 0.02\n" if nl == 1 else ""))
x = np.arange(N + 1) / N
mask = np.ones((1, N + 1, N + 1))
mask[0, N // 4: N // 4 + N // 8, N // 2 - N // 16: N // 2 + N // 16] = 0
mask[0, 0, :] = mask[0, -1, :] = mask[0, :, 0] = mask[0, :, -1] = 0
psi = np.stack([1e-2 / (1 + 0.3 * l) * np.outer(np.sin((1 + l) * np.pi * x), np.sin(2 * np.pi * x)) for l in range(nl)]) * mask
tmp = tempfile.mkdtemp()
KEYS = ["node_pfused", "node_tile_s", "node_march_s", "node_march", "tiled_relax", "node_corr_fused", "node_rhs_fused", "node_split", "mg_coarse"]


def run(g, tag, sy=slice(None), sx=slice(None), opts=None):
    g.set_option("quiet", 1)
    g.set_option("io_tiles", 1)
    for k, v in (opts or {}).items():
        g.set_option(k, v)
    g.set("MASK", mask[:, sy, sx])
    g.set("PSI", psi[:, sy, sx])
    g.set_const()
    g.set_tnext(float("inf"))
    g.step(True)
    out = dict(opts={k: g.param(k) for k in KEYS})
    for name, call in (("save", lambda: g.save_state(os.path.join(tmp, tag + ".msom"), constants=True)),
                       ("load", lambda: g.load_state(os.path.join(tmp, tag + ".msom"))),
                       ("write_nc", lambda: g.write_nc(os.path.join(tmp, tag + ".nc")))):
        g.get("MASK")                                  # the stream is idle
        t0 = time.perf_counter()
        call()
        out[name] = (time.perf_counter() - t0) * 1e3   # every call returns with its file in place / its fields loaded
    return out


uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
res = [None] * (px * py)


def worker(rank):
    g = NodeQG(par, tiled=(px, py, rank, uid))
    res[rank] = run(g, "tiled", *node_tile_window(N, px, py, rank))
    g.close()


th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(px * py)]
[t.start() for t in th]
[t.join(timeout=900) for t in th]
assert all(r is not None for r in res), "a tile thread hung"
g = NodeQG(par)
one = run(g, "single", opts=res[0]["opts"])   # the file is the single tile's with the option values the tiled handle reports
g.close()
size = lambda name: os.path.getsize(os.path.join(tmp, name))
same = lambda a, b: open(os.path.join(tmp, a), "rb").read() == open(os.path.join(tmp, b), "rb").read()
report = dict(grid=f"{N + 1}^2 vertices x {nl}", tiles=f"{px} x {py} of {tile}^2 cells", calls_timed=1,
              state_file_bytes=size("tiled.msom"), vars_nc_bytes=size("tiled.nc"),
              state_file_equals_single_tile=same("tiled.msom", "single.msom"), vars_nc_equals_single_tile=same("tiled.nc", "single.nc"),
              ms_tiled_threads_one_gpu={k: round(max(r[k] for r in res), 1) for k in ("save", "load", "write_nc")},
              ms_single_tile_same_options={k: round(one[k], 1) for k in ("save", "load", "write_nc")}, resolved_options=res[0]["opts"],
              note="one call each, wall clock of the slowest rank; tiles are host threads sharing one device and rank 0 assembles and writes "
                   "alone; the files go to the machine's temporary directory; the RCCL path is not measured")
print(json.dumps(report, indent=1))
if out_path:
    with open(out_path, "w") as f:
        json.dump(report, f, indent=1)
        f.write("\n")
for name in os.listdir(tmp):
    os.remove(os.path.join(tmp, name))
os.rmdir(tmp)
