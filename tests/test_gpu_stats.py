"""Running time means and eddy statistics on the device (msom_stats_begin / _accumulate / _weight / _get, option "stats")
and time_filter (msqg/qg.h:491-507, msom_time_filter), against numpy in the expression order include/msom.h documents:

    acc = acc + w * x,   x = psi, q, psi*psi, q*q, 0.5 * (u*u + v*v), u*q, v*q,   W = W + w
    u = (psi[j-1][i] - psi[j+1][i]) / (2 D),   v = (psi[j][i+1] - psi[j][i-1]) / (2 D)          (2 D formed once)
    mean = acc / W;   EKE = mean(KE) - 0.5 * (um*um + vm*vm);   UQ_EDDY = mean(uq) - um * mean(q)   (um, vm from mean psi)

on psi with its ghost ring rebuilt the way the oracle's boundary() does it (dirichlet(0): ghost = -interior, x walls first,
then y walls over the x ghosts; sbc = -1: wrapped).  Strict build: bit for bit.  Product build (contraction, reciprocal of
2 D): relative error <= TOL_PRODUCT, the bound the project uses for contracted against uncontracted arithmetic
(test_gpu_hooks, named in test_gpu_bfn).  The automatic sample of msom_step is held to the numpy accumulation over the CPU
oracle's hook-level RK2 (update, dtnext, advance dt/2, update, advance dt), which samples (q_n, psi after the first update, dt_n)."""
import ctypes as C
import functools

import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F, STATS as ST
from test_gpu_bfn import CASES, TOL, TOL_PRODUCT
from test_gpu_hooks import DevBuf
from test_gpu_parity import rand_field, rel
from test_gpu_tiled import assemble, run_tiled

pytestmark = pytest.mark.gpu

MSOM_ERR_ARG, MSOM_ERR_STATE = -1, -6
ACC = ("PSI", "Q", "PSI2", "Q2", "KE", "UQ", "VQ")
DERIVED = ("EKE", "UQ_EDDY", "VQ_EDDY")
FULL = (1 << ST["NACC"]) - 1
NEEDS = dict(EKE=("PSI", "KE"), UQ_EDDY=("PSI", "Q", "UQ"), VQ_EDDY=("PSI", "Q", "VQ"))
WEIGHTS = (0.75, 0.013, 2.5)
NAUTO = 5


def bits(*names):
    return sum(1 << ST[n] for n in names)


def params(case):
    nx, ny, nl, extra = CASES[case]
    return orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)


def handle(case, strict, tol=TOL, **opts):
    nx, ny, nl, extra = CASES[case]
    g = QG(params(case), strict=strict)
    g.option("quiet", 1)
    g.option("TOLERANCE", tol)
    for k_, v_ in opts.items():
        g.option(k_, v_)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    g.set_tnext(float("inf"))
    return g


# ------------------------------------------------------------------ the numpy reference

def ghosted(psi, periodic):
    """[nl][ny + 2][nx + 2]: psi with the ghost ring of the oracle's boundary()"""
    nl, ny, nx = psi.shape
    p = np.zeros((nl, ny + 2, nx + 2))
    p[:, 1:-1, 1:-1] = psi
    if periodic:
        p[:, 1:-1, -1], p[:, 1:-1, 0] = p[:, 1:-1, 1], p[:, 1:-1, -2]
        p[:, -1, :], p[:, 0, :] = p[:, 1, :], p[:, -2, :]
    else:
        p[:, 1:-1, -1], p[:, 1:-1, 0] = -p[:, 1:-1, -2], -p[:, 1:-1, 1]
        p[:, -1, :], p[:, 0, :] = -p[:, -2, :], -p[:, 1, :]
    return p


def velocities(psi, periodic, D2):
    p = ghosted(psi, periodic)
    return (p[:, :-2, 1:-1] - p[:, 2:, 1:-1]) / D2, (p[:, 1:-1, 2:] - p[:, 1:-1, :-2]) / D2


class NumpyStats:
    def __init__(self, shape, periodic, D2):
        self.S = {n: np.zeros(shape) for n in ACC}
        self.W, self.periodic, self.D2 = 0.0, periodic, D2

    def sample(self, psi, q, w):
        u, v = velocities(psi, self.periodic, self.D2)
        x = dict(PSI=psi, Q=q, PSI2=psi * psi, Q2=q * q, KE=0.5 * (u * u + v * v), UQ=u * q, VQ=v * q)
        for n in ACC:
            self.S[n] = self.S[n] + w * x[n]
        self.W = self.W + w

    def get(self, name):
        if name in ACC:
            return self.S[name] / self.W
        um, vm = velocities(self.S["PSI"] / self.W, self.periodic, self.D2)
        if name == "EKE":
            return self.S["KE"] / self.W - 0.5 * (um * um + vm * vm)
        return self.S[name[:2]] / self.W - (um if name == "UQ_EDDY" else vm) * (self.S["Q"] / self.W)


def numpy_stats(g, case):
    return NumpyStats((g.nl, g.ny, g.nx), "sbc = -1" in CASES[case][3], 2.0 * (g.param("L0") / g.param("N")))


def check(g, ref, strict, names=ACC + DERIVED):
    for n in names:
        got, want = g.stats_get(ST[n]), ref.get(n)
        if strict:
            assert np.array_equal(got, want), n
        else:
            print(f"{n}: rel {rel(got, want):.3e}")
            assert rel(got, want) <= TOL_PRODUCT, n
    assert g.stats_weight() == ref.W        # W = W + w: nothing to contract


# ------------------------------------------------------------------ 1. the kernel against numpy

def manual_run(case, strict, mask):
    """three samples with three weights; a new random psi and q = comp_q(psi) between them.  Returns the handle and the
    (psi, q, w) the samples saw"""
    nx, ny, nl, _ = CASES[case]
    g = handle(case, strict)
    g.stats_begin(mask)
    seen = []
    for k, w in enumerate(WEIGHTS):
        if k > 0:
            g.comp_q(rand_field(40 + k, (nl, ny, nx), 1e-3))       # psi and q = comp_q(psi) now live in the handle
        seen.append((g.get(F["PSI"]), g.get(F["Q"]), w))
        g.stats_accumulate(w)
    return g, seen


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_accumulate_against_numpy(case, strict):
    g, seen = manual_run(case, strict, FULL)
    ref = numpy_stats(g, case)
    for psi, q, w in seen:
        ref.sample(psi, q, w)
    check(g, ref, strict)
    assert g.param("stats_mask") == FULL
    g.close()


# ------------------------------------------------------------------ 2. the mask

@functools.lru_cache(maxsize=None)
def full_mask_means(case):
    g, _ = manual_run(case, True, FULL)
    out = {n: g.stats_get(ST[n]) for n in ACC + DERIVED}
    for a in out.values():
        a.setflags(write=False)
    g.close()
    return out

@pytest.mark.parametrize("sel", [(n,) for n in ACC] + [("PSI", "Q")])
def test_mask_selects_accumulators(sel):
    case = 1
    full = full_mask_means(case)
    g, _ = manual_run(case, True, bits(*sel))
    assert g.param("stats_mask") == bits(*sel)
    assert g.param("stats_bytes") == len(sel) * g.nl * g.ny * g.nx * 8
    out = np.empty((g.nl, g.ny, g.nx))
    for n in ACC:
        if n in sel:
            assert np.array_equal(g.stats_get(ST[n]), full[n]), n
        else:
            assert g.L.msom_stats_get(g.h, ST[n], out.ctypes.data) == MSOM_ERR_ARG, n
    for n in DERIVED:
        assert g.L.msom_stats_get(g.h, ST[n], out.ctypes.data) == MSOM_ERR_ARG, n       # none of these masks holds what they need
    g.close()


def test_derived_need_exactly_their_accumulators():
    case = 2
    full = full_mask_means(case)
    out = np.empty(full["PSI"].shape)
    for n, need in NEEDS.items():
        g, _ = manual_run(case, True, bits(*need))
        assert np.array_equal(g.stats_get(ST[n]), full[n]), n
        for other in DERIVED:
            if other != n:
                assert g.L.msom_stats_get(g.h, ST[other], out.ctypes.data) == MSOM_ERR_ARG, (n, other)
        g.close()


# ------------------------------------------------------------------ 3. the automatic sample of msom_step against the oracle

@functools.lru_cache(maxsize=None)
def oracle_run(case, tol=TOL):
    """NAUTO hook-level RK2 steps of the CPU oracle; per step the pair (q_n, psi after the first update) and dt_n.
    Computed once per (case, TOLERANCE) and shared; nothing below writes into it"""
    nx, ny, nl, _ = CASES[case]
    o = orc.Oracle(params(case), smoother=orc.GS_RB, quiet=1)
    o.option("TOLERANCE", tol)
    o.set(orc.PSI, orc.synthetic_psi(nl, ny, nx))
    o.set_const()
    o.set_tnext(float("inf"))
    DT = o.param("DT")
    seen = []
    for _ in range(NAUTO):
        dt = o.update(orc.Q, orc.DQ, DT)            # dtnext() with no scheduled event ahead
        seen.append((o.get(orc.PSI), o.get(orc.Q), dt))
        o.advance(orc.QPRED, orc.Q, orc.DQ, dt / 2)
        o.update(orc.QPRED, orc.DQ, dt)
        o.advance(orc.Q, orc.Q, orc.DQ, dt)
    res = dict(seen=seen, q=o.get(orc.Q), psi=o.get(orc.PSI))
    for a in [res["q"], res["psi"]] + [x for s in seen for x in s[:2]]:
        a.setflags(write=False)
    return res


def auto_run(case, strict, stats, tol=TOL, every=None, **opts):
    g = handle(case, strict, tol, **opts)
    if stats:
        g.stats_begin(FULL)
        g.option("stats", 1)
        if every:
            g.option("stats_every", every)
    dts = [g.step() for _ in range(NAUTO)]
    st = g.mgstats()
    return g, dict(dts=dts, q=g.get(F["Q"]), psi=g.get(F["PSI"]), mg=(st.i, st.resb, st.resa, st.sum, st.nrelax))


def oracle_stats(g, case, tol=TOL, steps=range(NAUTO)):
    ref, seen = numpy_stats(g, case), oracle_run(case, tol)["seen"]
    for n in steps:
        ref.sample(*seen[n])
    return ref


def same_run(a, b):
    assert a["dts"] == b["dts"] and a["mg"] == b["mg"]
    assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["psi"], b["psi"])


@pytest.mark.parametrize("case", range(len(CASES)))
def test_strict_automatic_samples_bit_exact_against_the_oracle(case):
    g, run = auto_run(case, True, stats=True)
    o = oracle_run(case)
    assert run["dts"] == [s[2] for s in o["seen"]]
    assert np.array_equal(run["q"], o["q"]) and np.array_equal(run["psi"], o["psi"])
    ref = oracle_stats(g, case)
    check(g, ref, True)
    W = 0.0
    for dt in run["dts"]:
        W = W + dt
    assert g.stats_weight() == W
    g.close()
    g0, run0 = auto_run(case, True, stats=False)         # the option does not touch the run
    same_run(run, run0)
    g0.close()


@pytest.mark.parametrize("case", range(len(CASES)))
def test_product_run_is_untouched_by_the_option(case):
    """product build: q, psi, dt and mgstats with and without the samples, and W = the sum of the dt the steps returned
    (the sample reads the very double the step uses, from the device or by value)"""
    g, run = auto_run(case, False, stats=True, tol=TOL_PRODUCT)
    W = 0.0
    for dt in run["dts"]:
        W = W + dt
    assert g.stats_weight() == W
    assert np.isfinite(g.stats_get(ST["EKE"])).all()
    g.close()
    g0, run0 = auto_run(case, False, stats=False, tol=TOL_PRODUCT)
    same_run(run, run0)
    g0.close()


@pytest.mark.parametrize("opts", [dict(fused=0), dict(step_sync=0), dict(step_sync=1)], ids=["fused0", "lazy", "sync"])
def test_strict_automatic_samples_on_the_other_step_paths(opts):
    """the kernel-per-loop chain (host dt, by value) and the lazy step (dt read from the device scalar, no synchronisation)"""
    case = 0
    g, run = auto_run(case, True, stats=True, **opts)
    check(g, oracle_stats(g, case), True)
    ndev = g.param("stats_dev_samples")
    print(opts, "samples with the weight read on the device:", ndev)
    assert ndev == 0 if "fused" in opts else ndev > 0
    g0, run0 = auto_run(case, True, stats=False, **opts)
    same_run(run, run0)
    g.close(); g0.close()


def test_stats_every_two_samples_steps_0_2_4():
    case = 0
    g, run = auto_run(case, True, stats=True, every=2)
    check(g, oracle_stats(g, case, steps=(0, 2, 4)), True)
    assert g.stats_weight() == (run["dts"][0] + run["dts"][2]) + run["dts"][4]
    g.close()


def test_update_bfn_and_pystep_calls_do_not_sample():
    case = 3
    g = handle(case, True)
    g.stats_begin(FULL)
    g.option("stats", 1)
    q = g.get(F["Q"])
    g.update(q, g.param("DT"))
    tend = np.empty_like(q)
    g.pystep_bfn(q, tend, 1.0, 1)
    g.bfn_begin()
    g.bfn_steps(2, g.param("DT"), 1.0, 0.0)
    assert g.stats_weight() == 0.0
    g.step()
    assert g.stats_weight() > 0.0
    g.close()


# ------------------------------------------------------------------ 4. time_filter

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("tau_f", [None, 5.0])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_time_filter_against_numpy(case, tau_f, strict):
    nx, ny, nl, _ = CASES[case]
    g = handle(case, strict)
    if tau_f is not None:
        g.option("tau_f", tau_f)
    me = np.zeros((nl, ny, nx))          # the reference's freshly created field
    for k, dt in enumerate((0.1, 0.25, 1.5)):
        if k > 0:
            g.comp_q(rand_field(60 + k, (nl, ny, nx), 1e-3))
        q = g.get(F["Q"])
        a = dt / (20.0 if tau_f is None else tau_f)
        me = (1 - a) * me + a * q
        g.time_filter(dt)
        got = g.stats_get(ST["QME"])
        if strict:
            assert np.array_equal(got, me), k
        else:
            assert rel(got, me) <= TOL_PRODUCT, k
    assert g.param("stats_bytes") == nl * ny * nx * 8 and g.param("stats_mask") == 0
    g.close()


# ------------------------------------------------------------------ 5. tiles

@pytest.mark.parametrize("px,py,gn,nl,extra", [(2, 2, 64, 3, ""), (2, 1, 64, 2, "sbc = -1\ntau0 = 0\n")])
def test_statistics_on_tiles_equal_the_single_tile(px, py, gn, nl, extra):
    levels = int(np.log2(gn // max(px, py)))
    par = orc.double_gyre_params(gn, nl, extra=f"MGLEVELS = {levels}\n" + extra)
    psi = orc.synthetic_psi(nl, gn, gn)
    names = ACC + ("EKE",)

    def pre(g, rank):
        g.stats_begin(FULL)
        g.option("stats", 1)

    def fn(g, rank):
        return dict({n: g.stats_get(ST[n]) for n in names}, W=g.stats_weight())

    out = run_tiled(par, px, py, psi, nsteps=3, strict=True, fn=fn, pre=pre)
    g = QG(par, strict=True)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    pre(g, 0)
    dts = [g.step() for _ in range(3)]
    for o in out:
        assert o["dts"] == dts and o["extra"]["W"] == g.stats_weight()
        o.update(o["extra"])
    for n in names:
        assert np.array_equal(assemble(out, n, px, py), g.stats_get(ST[n])), n
    g.close()


# ------------------------------------------------------------------ 6. state and errors

def test_call_order_and_argument_errors():
    case = 3
    nx, ny, nl, _ = CASES[case]
    g = QG(params(case), strict=True)
    g.option("quiet", 1)
    L, h = g.L, g.h
    out = np.empty((nl, ny, nx))
    w = C.c_double(-1.0)
    assert g.param("stats_mask") == 0 and g.param("stats_bytes") == 0          # a fresh handle holds none of it
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    assert L.msom_stats_begin(h, FULL) == MSOM_ERR_STATE                       # before msom_set_const
    assert L.msom_time_filter(h, 0.1) == MSOM_ERR_STATE
    g.set_const()
    # no msom_stats_begin since msom_set_const
    assert L.msom_stats_accumulate(h, 1.0) == MSOM_ERR_STATE
    assert L.msom_stats_weight(h, C.byref(w)) == MSOM_ERR_STATE
    assert L.msom_stats_get(h, ST["PSI"], out.ctypes.data) == MSOM_ERR_STATE
    assert L.msom_stats_get(h, ST["QME"], out.ctypes.data) == MSOM_ERR_STATE   # and no msom_time_filter
    assert L.msom_set_option(h, b"stats", 1.0) == MSOM_ERR_STATE
    assert g.param("stats_mask") == 0 and g.param("stats_bytes") == 0
    # the mask
    assert L.msom_stats_begin(h, 0) == MSOM_ERR_ARG
    assert L.msom_stats_begin(h, 1 << ST["NACC"]) == MSOM_ERR_ARG
    assert L.msom_stats_begin(h, FULL | 1 << 20) == MSOM_ERR_ARG
    assert g.param("stats_bytes") == 0
    g.stats_begin(bits("PSI", "KE"))
    assert g.param("stats_mask") == bits("PSI", "KE") and g.param("stats_bytes") == 2 * nl * ny * nx * 8
    assert L.msom_stats_get(h, ST["PSI"], out.ctypes.data) == MSOM_ERR_STATE   # W == 0
    assert g.stats_weight() == 0.0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.msom_stats_accumulate(h, bad) == MSOM_ERR_ARG
        assert L.msom_time_filter(h, bad) == MSOM_ERR_ARG
    g.stats_accumulate(0.5)
    assert g.stats_weight() == 0.5
    for which in (-1, ST["NACC"], 15, 19, 31, 33):
        assert L.msom_stats_get(h, which, out.ctypes.data) == MSOM_ERR_ARG, which      # unknown id
    assert L.msom_stats_get(h, ST["Q"], out.ctypes.data) == MSOM_ERR_ARG              # not in the mask
    assert L.msom_stats_get(h, ST["UQ_EDDY"], out.ctypes.data) == MSOM_ERR_ARG
    assert L.msom_stats_get(h, ST["EKE"], out.ctypes.data) == 0
    assert L.msom_stats_get(h, ST["PSI"], None) == MSOM_ERR_ARG and L.msom_stats_weight(h, None) == MSOM_ERR_ARG
    assert np.array_equal(g.stats_get(ST["PSI"]), (0.5 * g.get(F["PSI"])) / 0.5)
    assert L.msom_set_option(h, b"stats_every", 0.0) == MSOM_ERR_ARG
    g.option("stats", 1)
    # msom_set_const drops the statistics
    g.time_filter(0.1)
    assert g.param("stats_bytes") == 3 * nl * ny * nx * 8
    g.set_const()
    assert g.param("stats_mask") == 0 and g.param("stats_bytes") == 0
    assert L.msom_stats_accumulate(h, 1.0) == MSOM_ERR_STATE
    assert L.msom_stats_get(h, ST["EKE"], out.ctypes.data) == MSOM_ERR_STATE
    assert L.msom_stats_get(h, ST["QME"], out.ctypes.data) == MSOM_ERR_STATE
    assert L.msom_step(h, C.byref(w)) == MSOM_ERR_STATE                       # "stats" is still 1 and nothing to sample into
    g.option("stats", 0)
    assert g.step() > 0
    g.close()


def test_begin_again_restarts_the_sums():
    case = 2
    g, seen = manual_run(case, True, FULL)
    g.stats_begin(bits("Q"))
    assert g.stats_weight() == 0.0 and g.param("stats_bytes") == g.nl * g.ny * g.nx * 8
    g.stats_accumulate(2.0)
    assert np.array_equal(g.stats_get(ST["Q"]), (2.0 * seen[-1][1]) / 2.0)
    g.close()


def test_stats_get_into_a_device_pointer():
    case = 0
    full = full_mask_means(case)
    g, _ = manual_run(case, True, FULL)
    for n in ("KE", "EKE"):
        d = DevBuf(np.zeros_like(full[n]))
        assert g.L.msom_stats_get(g.h, ST[n], d.ptr) == 0
        assert np.array_equal(d.host(), full[n]), n
        d.free()
    g.time_filter(0.3)
    d = DevBuf(np.zeros_like(full["Q"]))
    assert g.L.msom_stats_get(g.h, ST["QME"], d.ptr) == 0
    assert np.array_equal(d.host(), g.stats_get(ST["QME"]))
    d.free()
    g.close()
