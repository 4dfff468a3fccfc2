"""back-and-forth nudging loop, ms per step, product build, same process and GPU:
 (a) msom_bfn_steps: tendency, nudging, AB3 update and history rotation on the library's stream, state in HBM;
 (b) the caller-side loop of msqg/qg_bfn.py:62-73: pystep_bfn on device pointers, then the nudging term, the AB3 combination and the two
     history copies as torch elementwise operations on device tensors (torch's default stream and the library's blocking stream order
     themselves against each other).
20 steps after 3 warm-up steps, msom_sync (and torch.cuda.synchronize for b) before each clock read; the two loops alternate, two rounds.
Usage: python tools/ab_bfn.py [N NL ...]   (default 512 3 4096 6); prints one JSON line per size."""
import json, sys, time
sys.path.insert(0, '.')
import torch
from msom_amd import QG, FIELDS as F, workloads as wl
STEPS, WARM = 20, 3
args = [int(a) for a in sys.argv[1:]] or [512, 3, 4096, 6]
for N, nl in zip(args[0::2], args[1::2]):
    def make():
        g = QG(wl.double_gyre_params(N, nl)); g.option("quiet", 1)
        g.set(F["PSI"], wl.synthetic_psi(nl, N, N)); g.set_const()
        return g
    a, b = make(), make()
    DT = a.param("DT"); k = 0.05 / DT; dt12 = DT / 12
    q0 = torch.from_numpy(a.get(F["Q"])).cuda()
    gen = torch.Generator(device="cuda").manual_seed(1)
    obs = q0 + 1e-3 * q0.abs().max() * torch.randn(q0.shape, dtype=torch.float64, device="cuda", generator=gen)
    gain = (torch.rand(q0.shape, dtype=torch.float64, device="cuda", generator=gen) < 0.5).double()
    a.bfn_begin(); a.set(F["BFN_OBS"], obs); a.set(F["BFN_GAIN"], gain)
    var, F1, F2, F3 = q0.clone(), torch.zeros_like(q0), torch.zeros_like(q0), torch.zeros_like(q0)
    def loop_a(n):
        a.bfn_steps(n, DT, 1.0, k)
    def loop_b(n):
        global var
        for _ in range(n):
            assert b.L.pystep_bfn(b.h, var.data_ptr(), nl, N, N, F1.data_ptr(), nl, N, N, 1.0, 1) == 0
            F1.add_((k * gain) * (obs - var))
            var = var + dt12 * (23 * F1 - 16 * F2 + 5 * F3)
            F3.copy_(F2); F2.copy_(F1)
    def timed(fn, g):
        g.sync(); torch.cuda.synchronize(); t0 = time.perf_counter()
        fn(STEPS)
        g.sync(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) / STEPS * 1e3
    loop_a(WARM); loop_b(WARM)
    ms = {"bfn_steps": [], "caller_side": []}
    for rep in range(2):
        ms["bfn_steps"].append(timed(loop_a, a))
        ms["caller_side"].append(timed(loop_b, b))
    dq = float((torch.from_numpy(a.get(F["Q"])).cuda() - var).abs().max() / var.abs().max())
    print(json.dumps({"N": N, "nl": nl, "steps": STEPS, "warmup": WARM, "ms_per_step_bfn_steps": min(ms["bfn_steps"]),
                      "ms_per_step_caller_side": min(ms["caller_side"]), "rounds": ms, "rel_diff_q": dq}), flush=True)
    a.close(); b.close()
    del q0, obs, gain, var, F1, F2, F3
    torch.cuda.empty_cache()
