"""The default kernels against the CPU oracle at BASELINE.json's sizes: C3 (2048^2 x 3), C4 (4096^2 x 6) and both halves of C5
(the serial-noise stochastic step at 2048^2 x 3, the vertex model at 2049^2 x 3).  No kernel option is set: what runs is what
runs by default, and several default paths switch on only at these sizes -- the chained smoother (march_min = 2^23 cell-layers)
with its lean interior body, many interior chunks, both marching directions and several workgroup rounds; the vertex model's
split marching pass k_n_relax_march_s (node_march_s = 2049 vertices a side).  Each case asserts the conditions that put
its path under test, so that a moved threshold fails here instead of quietly testing something else.

Strict build: bit for bit (dq, q, psi, dt, mgstats).  Product build: the suite's product bounds -- rel <= 1e-10 on dq, q and
psi (test_fast_ten_steps_tight_tolerance), same cycle counts, dt to 1e-12; the vertex model 1e-9 (test_gpu_node_parity.same).
First measured product maxima (MI355X), rel(dq), rel(q), rel(psi):
  C3 tol 1e-3: 7.3e-14, 2.5e-14, 2.2e-15;  C3 tol 1e-9: 7.3e-14, 2.1e-14, 1.3e-15;
  C4 tol 1e-3: 1.7e-13, 8.2e-15, 1.2e-15;  C4 tol 1e-7: 1.7e-13, 7.2e-15, 1.4e-15;
  vertex 2049^2 x 3, rel(PSI), rel(Q): 1.8e-14, 3.7e-16.
Negative control: the product result at C3 / 1e-3 against the lexicographic oracle, rel(psi) = 1.1e-2.

Each oracle result is computed once (module cache) and both builds are compared with it; an oracle instance is freed before
the next one is built (one at 4096^2 x 6 first-touches about 14 GB)."""
import ctypes
import gc

import numpy as np
import pytest

import orc
import orn
from msom_amd import QG, NodeQG, FIELDS as F
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

INF = float("inf")
# case -> (N, nl, TOLERANCE).  Tight tolerances: >= 3 cycles in the step's last solve, so nrelax adapts and passes of K = 2, 3
# and 4 half-sweeps all run (1e-7 gives 3 at C4 but only 2 at C3; 1e-9 gives 5 there)
CASES = {"C3_tol1e-3": (2048, 3, 1e-3), "C3_tol1e-9": (2048, 3, 1e-9), "C4_tol1e-3": (4096, 6, 1e-3), "C4_tol1e-7": (4096, 6, 1e-7)}

_cache = {}


def cached(key, compute):
    if key not in _cache:
        _cache[key] = compute()
        gc.collect()
    return _cache[key]


def run_cell(m, N, nl, tol, pre=None):
    """one update() (one RHS evaluation) then one RK2 step, on the oracle or on a QG handle; pre(m) sets further inputs
    before set_const"""
    is_o = isinstance(m, orc.Oracle)
    m.option("TOLERANCE", tol)
    m.set(orc.PSI if is_o else F["PSI"], orc.synthetic_psi(nl, N, N))
    if pre:
        pre(m)
    m.set_const()
    m.set_tnext(INF)
    if is_o:
        dtmax = m.update()
        dq = m.get(orc.DQ)
        m.step()
        dt = m.dt
    else:
        dq, dtmax = m.update()
        dt = m.step()
    st = m.mgstats()
    return dict(dq=dq, dtmax=dtmax, dt=dt, q=m.get(orc.Q if is_o else F["Q"]), psi=m.get(orc.PSI if is_o else F["PSI"]),
                st=(st.i, st.resb, st.resa, st.nrelax))


def expected_relax_paths(N, nl, march_min=23):
    """msom_get_param("relax_path_<k>") of every level (N, N / 2, ... 2 cells a side) of one walled tile of N^2 x nl cells with
    uniform S (or one layer) and no option set, written down from the documented thresholds (include/msom.h) and not read from
    the build: 3 marched -- at least 512 x 64 cells and 2^march_min cell-layers; 2 block8 -- 64 .. 1024 cells a side where not
    marched; 4 the one-launch coarse group, from 32 cells a side down; 0 per-colour launches -- whatever is left, and every
    level above MSOM_FASTNL = 8 layers, where none of the register-resident kernels exists"""
    paths, n = [], N
    while n >= 2:
        if nl > 8:
            paths.append(0)
        elif n <= 32:
            paths.append(4)
        elif n >= 512 and n * n * nl >= 2 ** march_min:
            paths.append(3)
        else:
            paths.append(2 if 64 <= n <= 1024 else 0)
        n //= 2
    return tuple(paths)


def relax_paths(g):
    return tuple(int(g.param(f"relax_path_{k}")) for k in range(int(g.param("nlevels"))))


def oracle_cell(case, smoother=orc.GS_RB):
    def compute():
        N, nl, tol = CASES[case]
        o = orc.Oracle(orc.double_gyre_params(N, nl), smoother=smoother, quiet=1)
        out = run_cell(o, N, nl, tol)
        del o
        gc.collect()
        return out
    return cached((case, smoother), compute)


def gpu_cell(case, strict):
    N, nl, tol = CASES[case]
    g = QG(orc.double_gyre_params(N, nl), strict=strict)
    g.option("quiet", 1)
    out = run_cell(g, N, nl, tol)
    if not strict:
        # what put the chained smoother on the finest level at this size (set_const decides uniform S): uniform S and at
        # least 2^march_min cell-layers
        assert g.param("uniform_S") == 1
        assert N * N * nl >= 2 ** g.param("march_min")
        assert g.param("march_levels") >= 1
        assert relax_paths(g) == expected_relax_paths(N, nl), relax_paths(g)   # C3: one marched level, C4: two
    g.close()
    return out


def product_c3():
    """the product result at C3, tolerance 1e-3: kept for the negative control"""
    return cached(("C3_tol1e-3", "product"), lambda: gpu_cell("C3_tol1e-3", False))


@pytest.mark.parametrize("case,strict", [(c, s) for c in CASES for s in (True, False)])
def test_default_cell_model_equals_oracle_at_baseline_sizes(case, strict):
    o = oracle_cell(case)
    if strict:
        g = gpu_cell(case, True)
    else:
        _cache.pop((case, orc.GS_RB))   # its last use (the strict build ran first): at most one 4096^2 result is kept
        if case == "C4_tol1e-3":
            _cache[(case, "psi")] = o["psi"]    # kept for the negative control of the general-S leg (test_gpu_oracle_legs.py)
        g = product_c3() if case == "C3_tol1e-3" else gpu_cell(case, False)
    if CASES[case][2] < 1e-3:
        assert o["st"][0] >= 3, o["st"]     # the tight case must run passes of K = 2, 3 and 4
    if strict:
        assert g["dtmax"] == o["dtmax"] and g["dt"] == o["dt"]
        assert g["st"] == o["st"]
        for k in ("dq", "q", "psi"):
            assert np.array_equal(g[k], o[k]), (k, rel(g[k], o[k]))
    else:
        assert (g["st"][0], g["st"][3]) == (o["st"][0], o["st"][3])
        assert g["dt"] == pytest.approx(o["dt"], rel=1e-12)
        errs = {k: rel(g[k], o[k]) for k in ("dq", "q", "psi")}
        print(f"{case} product vs oracle: " + ", ".join(f"rel({k}) = {v:.3g}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 1e-10, (k, v)


def test_bound_tells_red_black_from_lexicographic_at_c3():
    """negative control: the product result of C3 at 1e-3 against the oracle with the reference's lexicographic sweep order
    -- one cycle per solve, so psi depends on every half-sweep, and the 1e-10 bound above must see a change of ordering"""
    g = product_c3()
    lex = oracle_cell("C3_tol1e-3", smoother=orc.GS_LEX)
    _cache.pop(("C3_tol1e-3", orc.GS_LEX))
    d = rel(g["psi"], lex["psi"])
    print(f"C3 tol 1e-3, product (red-black) vs lexicographic oracle: rel(psi) = {d:.3g}")
    assert d > 1e-6


def test_serial_noise_stochastic_step_bit_exact_at_c5_size():
    """C5, first half: the stochastic variant with the reference's serial rand() stream (srand(7)) at 2048^2 x 3, two steps,
    strict build against the oracle"""
    N, nl = 2048, 3
    txt = orc.double_gyre_params(N, nl, extra="tr_stoch = 50\namp_stoch = 1e-5\n")
    sig = np.abs(np.random.default_rng(12).standard_normal((nl, N, N)))
    psi0 = orc.synthetic_psi(nl, N, N)
    libc = ctypes.CDLL(None)
    res = []
    for which in ("oracle", "strict"):
        m = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1) if which == "oracle" else QG(txt, strict=True)
        is_o = which == "oracle"
        m.option("quiet", 1)
        m.option("stochastic", 1)
        m.set(orc.PSI if is_o else F["PSI"], psi0)
        m.set_const()
        m.set(orc.SIGMA if is_o else F["SIGMA"], sig)
        libc.srand(7)
        m.set_tnext(INF)
        for _ in range(2):
            m.step()
        res.append((m.get(orc.Q if is_o else F["Q"]), m.get(orc.PSI if is_o else F["PSI"])))
        if not is_o:
            m.close()
        del m
        gc.collect()
    (qo, po), (qg, pg) = res
    assert np.array_equal(qg, qo), rel(qg, qo)
    assert np.array_equal(pg, po), rel(pg, po)


# C5, second half: the configuration of bench.py's vertex leg -- 2049^2 x 3 vertices, surface QG, an island, TOLERANCE 1e-5
NODE_N, NODE_NL = 2048, 3
NODE_TXT = (f"N = {NODE_N}\nnl = {NODE_NL}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\n"
            "bc_fac = 1.0\ndh = [0.1,0.3,0.6]\nN2 = [300.,9000.,3000.]\nDT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\n"
            "TOLERANCE = 1e-5\nsqg = 1\n")


def node_inputs(N, nl):
    x = np.arange(N + 1) / N
    mk = np.ones((1, N + 1, N + 1))
    mk[0, N // 4: N // 4 + N // 8, N // 2: N // 2 + N // 8] = 0
    mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
    psi = np.stack([1e-2 * (1 - 0.2 * l) * sum(np.sin(1.3 * k + 2.1 * m + 0.7 * l) / (k * m) * np.outer(np.sin(m * np.pi * x), np.sin(k * np.pi * x))
                                              for k in range(1, 4) for m in range(1, 4)) for l in range(nl)]) * mk
    bs = 0.3 * np.outer(np.sin(np.pi * x), np.sin(2 * np.pi * x))[None] + 0.05
    return dict(MASK=mk, BS=bs, PSI=psi)


def node_run(m, setf, getf):
    for f, a in node_inputs(NODE_N, NODE_NL).items():
        setf(f, a)
    m.set_const()
    for _ in range(2):
        m.step(True)          # with the forcing event
    st = m.mgstats()
    return dict(PSI=getf("PSI"), Q=getf("Q"), t=m.t, dt=m.dt, st=(st.i, st.resb, st.resa, st.nrelax))


def node_oracle():
    def compute():
        o = orn.NodeOracle(NODE_TXT, smoother=orn.GS_RB, quiet=1)
        out = node_run(o, lambda f, a: o.set(getattr(orn, f), a), lambda f: o.get(getattr(orn, f)))
        del o
        gc.collect()
        return out
    return cached("vertex", compute)


@pytest.mark.parametrize("strict", [True, False])
def test_vertex_model_equals_oracle_at_c5_size(strict):
    o = node_oracle()
    g = NodeQG(NODE_TXT, strict=strict)
    g.set_option("quiet", 1)
    # the split marching pass runs on the finest level: split layout there, and at least node_march_s vertices a side
    assert g.param("node_march_s") <= NODE_N + 1
    out = node_run(g, g.set, g.get)
    assert g.param("split_0") == 1 and g.param("s2_xuniform") == 1
    g.close()
    if strict:
        assert (out["t"], out["dt"]) == (o["t"], o["dt"])
        assert out["st"] == o["st"]
        for k in ("PSI", "Q"):
            assert np.array_equal(out[k], o[k]), (k, rel(out[k], o[k]))
    else:
        errs = {k: rel(out[k], o[k]) for k in ("PSI", "Q")}
        print("vertex 2049^2 x 3 product vs oracle: " + ", ".join(f"rel({k}) = {v:.3g}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 1e-9, (k, v)
