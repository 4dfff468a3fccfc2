"""Time msom_state_save / msom_state_load (with constants) against a yardstick measured in the same process: one pinned hipMemcpy
D2H of the same bytes followed by one write of them.  The yardstick serialises copy and write; the save pipeline overlaps them.

    python tools/time_state.py [--sizes 512x512x3,4096x4096x6] [--reps 5] [--dir DIR]

Prints one JSON line per size: median and min..max of the repetitions after one warm-up, in ms, and the file's bytes.  The file goes
to DIR (default: a temporary directory, i.e. the local file system); the page cache takes the writes, as it does for the yardstick.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from msom_amd import FIELDS as F, QG  # noqa: E402
from msom_amd.workloads import double_gyre_params, synthetic_psi  # noqa: E402


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return dict(median=round(statistics.median(out), 3), min=round(min(out), 3), max=round(max(out), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512x512x3,4096x4096x6")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for size in a.sizes.split(","):
            nx, ny, nl = (int(v) for v in size.split("x"))
            g = QG(double_gyre_params(nx, nl, extra=f"Ny = {ny}\n" if ny != nx else ""))
            g.option("quiet", 1)
            g.set(F["PSI"], synthetic_psi(nl, ny, nx))
            g.set_const()
            g.step()
            path = os.path.join(d, "state.msom")
            save = timed(lambda: g.save_state(path, constants=True), a.reps)
            nbytes = os.path.getsize(path)
            load = timed(lambda: g.load_state(path), a.reps)
            # yardstick: the same bytes, device -> pinned host in one copy, then one write
            dev = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
            host = torch.empty(nbytes // 8, dtype=torch.float64).pin_memory()
            ypath = os.path.join(d, "yardstick.bin")

            def yard():
                host.copy_(dev)
                torch.cuda.synchronize()
                with open(ypath + ".tmp", "wb") as f:
                    f.write(memoryview(host.numpy()))
                os.replace(ypath + ".tmp", ypath)

            y = timed(yard, a.reps)
            print(json.dumps(dict(size=size, bytes=nbytes, reps=a.reps, save_ms=save, load_ms=load, yardstick_d2h_write_ms=y,
                                  save_GBps=round(nbytes / save["median"] / 1e6, 2), yardstick_GBps=round(nbytes / y["median"] / 1e6, 2))), flush=True)
            g.close()
            del dev, host


if __name__ == "__main__":
    main()
