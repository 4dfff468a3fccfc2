"""wavenumber spectra on the device, product build, N^2 x nl (default 4096 6): what msom_spec_energy and msom_spec_cross (with flux, device
arrays) cost -- wall time around the call, which synchronises -- each pass by msom_bench_kernel (HIP events, 20 back-to-back launches,
best of 3) with the bytes it moves counted from its arrays, the route a user had before (get(PSI) to the host, then tests/spec_ref.py in
numpy: wall time, the threads the process is given), and, where torch sees the GPU, torch.fft.fft2 of one complex128 [nl][N][N] array as
a yardstick for the bare transform (it is not linked into the library).
Usage: python tools/ab_spec.py [N NL] [--no-host]   prints one JSON line -> profiles/spec.json."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, '.')
sys.path.insert(0, 'tests')
import numpy as np

import spec_ref as R
from msom_amd import QG, FIELDS as F, workloads as wl

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N, nl = (int(args[0]), int(args[1])) if len(args) >= 2 else (4096, 6)
g = QG(wl.double_gyre_params(N, nl)); g.option("quiet", 1)
g.set(F["PSI"], wl.synthetic_psi(nl, N, N))
g.set_const()
g.step()
D = g.param("L0") / g.param("N")
row = {"N": N, "nl": nl, "nbins": g.spec_bins()}


def best(fn, n=3):
    t = []
    for _ in range(n):
        g.sync(); t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), t


g.spec_energy()   # first use: the work arrays
row["spec_bytes"], row["spec_batch"] = g.param("spec_bytes"), g.param("spec_batch")
row["spec_energy_ms"], row["spec_energy_rounds"] = best(g.spec_energy)

hip = C.CDLL("libamdhip64.so")
nbytes = nl * N * N * 8
da, db = C.c_void_p(), C.c_void_p()
assert hip.hipMalloc(C.byref(da), C.c_size_t(nbytes)) == 0 and hip.hipMalloc(C.byref(db), C.c_size_t(nbytes)) == 0
rng = np.random.default_rng(1)
for d in (da, db):
    x = rng.standard_normal((nl, N, N))
    assert hip.hipMemcpy(d, C.c_void_p(x.ctypes.data), C.c_size_t(nbytes), 1) == 0
sp, fl = np.empty((nl, row["nbins"])), np.empty((nl, row["nbins"]))
dp = C.POINTER(C.c_double)
cross = lambda: g._chk(g.L.msom_spec_cross(g.h, da, db, nl, sp.ctypes.data_as(dp), fl.ctypes.data_as(dp)))   # noqa: E731
cross()
row["spec_cross_flux_ms"], row["spec_cross_flux_rounds"] = best(cross)
hip.hipFree(da); hip.hipFree(db)

# the passes, on one batch of layers; bytes per point of a layer: rows read psi (8) and write Z (16); the transpose reads and writes 16;
# the column pass reads 16 and writes 8 on the half plane (nx / 2 + 1 of nx lines); the shell pass reads that half plane
lay = int(min(nl, row["spec_batch"]))
half = (N // 2 + 1) / N
per_point = {"spec_rows": 24, "spec_transpose": 32, "spec_cols": 16 + 8 * half, "spec_shells": 8 * half}
row["passes"] = {}
for name, b in per_point.items():
    ms = min(g.bench_kernel(name, 20) for _ in range(3))
    gb = b * N * N * lay / 1e9
    row["passes"][name] = {"ms": ms, "layers": lay, "GB": gb, "TB_per_s": gb / ms}

if "--no-host" not in sys.argv:   # the route it replaces: the fields to the host, numpy there
    t0 = time.perf_counter()
    psi = g.get(F["PSI"]); S = g.get(F["S"])
    t1 = time.perf_counter()
    p = np.zeros((nl, N + 2, N + 2)); p[:, 1:-1, 1:-1] = psi      # the ghost ring of boundary(): walls
    p[:, 1:-1, -1], p[:, 1:-1, 0] = -p[:, 1:-1, -2], -p[:, 1:-1, 1]
    p[:, -1, :], p[:, 0, :] = -p[:, -2, :], -p[:, 1, :]
    u, v = (p[:, :-2, 1:-1] - p[:, 2:, 1:-1]) / (2 * D), (p[:, 1:-1, 2:] - p[:, 1:-1, :-2]) / (2 * D)
    dh = np.array([g.param(f"dh_{l}") for l in range(nl)]); dhc = 0.5 * (dh[:-1] + dh[1:])
    ke = 0.5 * dh[:, None] * (R.spec_1d(u, u, D) + R.spec_1d(v, v, D))
    gg = np.sqrt(S[:nl - 1]) * (psi[1:] - psi[:-1]) / dhc[:, None, None]
    pe = 0.5 * dhc[:, None] * R.spec_1d(gg, gg, D)
    t2 = time.perf_counter()
    kd, pd = g.spec_energy()
    row["host_route"] = {"get_ms": (t1 - t0) * 1e3, "numpy_ms": (t2 - t1) * 1e3, "total_ms": (t2 - t0) * 1e3,
                         "threads": len(os.sched_getaffinity(0)), "runs": 1,
                         "ke_device_vs_numpy": float(np.abs(kd - ke).max() / np.abs(ke).max()),
                         "pe_device_vs_numpy": float(np.abs(pd - pe).max() / np.abs(pe).max())}
    row["speedup_vs_host_route"] = row["host_route"]["total_ms"] / row["spec_energy_ms"]
g.close()

try:   # yardstick for the bare transform, only where torch sees the device
    import torch
    if torch.cuda.is_available():
        z = torch.randn(nl, N, N, dtype=torch.complex128, device="cuda")
        for _ in range(2):
            torch.fft.fft2(z)
        t = []
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                torch.fft.fft2(z)
            b.record(); torch.cuda.synchronize()
            t.append(a.elapsed_time(b) / 5)
        row["torch_fft2_complex128_ms"] = min(t)
except Exception as e:   # noqa: BLE001
    row["torch_fft2_complex128_ms"] = None
    row["torch_note"] = repr(e)[:200]
print(json.dumps(row), flush=True)
