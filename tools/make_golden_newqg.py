"""Writes tests/golden/newqg_32.npz from tests/newqg_ref.py: three steps of the newqg dialect at 32 x 32 with the constants of the
sample params.in, once free slip (sbc = 0) and once no slip (sbc = 100).  Per case: the inputs in_psi, in_sbc and, after the steps,
psi, q, dq, the dt sequence and (i, nrelax, resb, resa) of each step's last solve.
usage: python tools/make_golden_newqg.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import newqg_ref as nq  # noqa: E402
from msom_amd.workloads import synthetic_psi  # noqa: E402

N, STEPS, AMP = 32, 3, 500.0   # the limiter takes D / max|u| (max|u| above D CFL / DT)


def main():
    out = {}
    for case, sbc in (("sbc0", 0.0), ("sbc100", 100.0)):
        par = nq.sample_par(N, sbc=sbc)
        psi0 = synthetic_psi(1, N, N, amp=AMP)[0]
        m = nq.Model(par, psi0)
        dts, stats = [], []
        for _ in range(STEPS):
            dts.append(m.step())
            stats.append((m.stats.i, m.stats.nrelax, m.stats.resb, m.stats.resa))
        out.update({f"{case}_in_psi": psi0, f"{case}_in_sbc": np.float64(sbc), f"{case}_psi": m.psi, f"{case}_q": m.q, f"{case}_dq": m.dq,
                    f"{case}_dt": np.array(dts), f"{case}_mgstats": np.array(stats, dtype=np.float64)})
    path = os.path.join(ROOT, "tests", "golden", "newqg_32.npz")
    np.savez_compressed(path, **out)
    print(path, {k: (v.shape if hasattr(v, "shape") else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
