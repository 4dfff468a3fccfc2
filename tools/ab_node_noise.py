"""vertex variant, one layer: stochastic step time with the host rand() stream (noise_mode 0) and the device generator (noise_mode 1)
next to the deterministic step, same process and GPU; then draw + filter alone.  Usage: python tools/ab_node_noise.py [N ...]"""
import ctypes, sys, time
sys.path.insert(0, '.'); sys.path.insert(0, 'tests')
import orn
from msom_amd import NodeQG
STEPS, WARM = 10, 3
def make(N, stochastic, mode):
    g = NodeQG(orn.node_params(N, 1, bc_fac=1.0, extra="gp_low = 0.02\namp_stoch = 1e-3\nL_filt = 10.\n"))
    for k, v in (("quiet", 1), ("stochastic", stochastic), ("seed", 5), ("noise_mode", mode)): g.set_option(k, v)
    g.set("PSI", orn.node_psi(1, N)); g.set_const()
    return g
for N in [int(a) for a in sys.argv[1:]] or [1024, 2048]:
    hs = {"deterministic": make(N, 0, 0), "noise_mode=0": make(N, 1, 0), "noise_mode=1": make(N, 1, 1)}
    hip = ctypes.CDLL("libamdhip64.so")     # the runtime the library has loaded
    def timed(fn, n):
        hip.hipDeviceSynchronize(); t0 = time.perf_counter()
        for _ in range(n): fn()
        hip.hipDeviceSynchronize()
        return (time.perf_counter() - t0) / n * 1e3
    for g in hs.values():
        for _ in range(WARM): g.step(True)
    for rep in range(2):
        for name, g in hs.items():
            ms = timed(lambda: g.step(True), STEPS)
            print(f"N={N} {name:14s} {ms:9.3f} ms/step  cycles of the last solve {g.mgstats().i}", flush=True)
    for name in ("noise_mode=0", "noise_mode=1"):
        g = hs[name]
        for f in (0, 1):
            g.noise_draw(filter=f)
            print(f"N={N} {name:14s} draw{' + filter' if f else '':9s} {timed(lambda: g.noise_draw(filter=f), 5 if name.endswith('0') else 500):9.3f} ms", flush=True)
    for g in hs.values(): g.close()
