"""vertical normal modes, product build: wall time of msom_modes_compute (with its synchronisation) and HIP-event times of the
projection and energy kernels through msom_bench_kernel, in the compact form (uniform table) and the general form (MSOM_FR perturbed
per cell and interface, one eigenproblem per column), next to the bytes each kernel streams per column.
Usage: python tools/ab_modes.py [N NL ...]   (default 4096 6); prints one JSON line per size -> profiles/r09_modes.json."""
import json, sys, time
sys.path.insert(0, '.')
import numpy as np
from msom_amd import QG, FIELDS as F, workloads as wl
args = [int(a) for a in sys.argv[1:]] or [4096, 6]
for N, nl in zip(args[0::2], args[1::2]):
    row = {"N": N, "nl": nl}
    for form in ("compact", "general"):
        g = QG(wl.double_gyre_params(N, nl)); g.option("quiet", 1)
        g.set(F["PSI"], wl.synthetic_psi(nl, N, N))
        if form == "general":
            table = np.array(eval(wl.LAYERS[nl][0]))[:max(nl - 1, 1)]
            g.set(F["FR"], table[:, None, None] * (1 + 0.3 * (2 * np.random.default_rng(11).random((table.size, N, N)) - 1)))
        g.set_const()
        t = []
        for _ in range(3):
            g.sync(); t0 = time.perf_counter(); g.modes_compute(); t.append((time.perf_counter() - t0) * 1e3)
        assert g.param("modes_compact") == (form == "compact")
        coef = 0 if form == "compact" else nl * nl
        row[form] = {"compute_ms": min(t), "compute_rounds": t, "modes_bytes": g.param("modes_bytes"),
                     "project_ms": min(g.bench_kernel("modes_project", 20) for _ in range(2)), "project_bytes_per_column": (coef + 2 * nl) * 8,
                     "energy_ms": min(g.bench_kernel("modes_energy", 20) for _ in range(2)), "energy_bytes_per_column": (coef + (nl if coef else 0) + nl) * 8}
        g.close()
    print(json.dumps(row), flush=True)
