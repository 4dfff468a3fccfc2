"""The vertex model's default kernels against its CPU oracle at the layer counts 1-8, each at 2049^2 vertices: exactly
node_march_s, the smallest level on which the chained split pass k_n_relax_march_s runs (the >= of the threshold).  The hot
kernels are templated on the layer count (k_n_relax_march_s<NL, K>, k_n_relax_tile_s<NL>, k_n_relax_s / k_n_relax_prolong_s<NL>,
k_n_correct_residual_m<NL>, k_n_mg_coarse<NL>, n_col_solve<NL>): every NL is its own register allocation and instruction
schedule.  No kernel option is set.  Paths per level (msomn_get_param relax_path_<k>: 1 split colour passes, 2 LDS-tiled split
passes, 3 chained split passes, 4 inside the one-launch coarse group), node_march_kmax, corr_march = 1 in every case:

  nl1      barotropic (iRd2_low), no S2      level 0: 3, K <= 4;  level 1: 1;  levels 2-5: 2;  levels 6-10: 4
  nl2      sqg = 1                           same as nl1
  nl4      sqg = 1, largest nl of the tiles  same as nl1
  nl5      odd                               level 0: 3, K <= 3;  levels 1-5: 1;  levels 6-10: 4
  nl6      sqg = 1, largest nl of the chain  same as nl5
  nl7      odd, no chained pass              levels 0-5: 1;  levels 6-10: 4;  node_march_kmax 0
  nl8      sqg = 1, MSOM_FASTNL              same as nl7
  nl3_s2x  plain; S2 varies in x             same as nl7 (no row tables: s2_xuniform = 0)

The run: set_const, one update() (dq and its dt) from a zero first guess of psi, one step(True) with the forcing event; C5's
island mask and TOLERANCE 1e-5 (10-13 cycles in the update's solve, 7-9 in the step's; at least 3, resb > 0 and finite oracle
fields asserted: a degenerate oracle run can report NaN fields as a converged solve).  Layer thicknesses are distinct and sum to 1, every interface has its own N2, and
psi starts non-zero and different in every layer, so that swapping two layers changes the result.  Three checks per case:
  1. strict build against the oracle, bit for bit (dq, psi, q, t, dt, mgstats of the update and of the step);
  2. product build against the oracle, after the path queries above are asserted for every level: equal cycle counts and nrelax,
     dt to 1e-12, rel <= 1e-10 on dq, q and psi (the cell model's bound);
  3. once, at nl1: the product result against the lexicographic oracle must differ by more than 100 times that bound.
First measured product maxima (MI355X), rel(dq), rel(q), rel(psi):
  nl1 2.3e-16, 1.2e-16, 2.0e-14;  nl2 2.7e-15, 3.1e-16, 1.5e-13;  nl4 2.6e-15, 3.2e-16, 3.1e-14;  nl5 2.9e-15, 3.3e-16, 1.8e-14;
  nl6 2.8e-15, 3.3e-16, 1.7e-14;  nl7 2.8e-15, 3.0e-16, 1.9e-14;  nl8 3.0e-15, 3.3e-16, 1.9e-14;  nl3_s2x 2.7e-15, 3.5e-16, 4.3e-14.
Negative control: nl1 product against the lexicographic oracle, rel(psi) = 1.9e-4.  With the right-hand side of one layer scaled
by 1 + 1e-9 in the first stage of k_n_relax_march_s for NL = 5 alone, strict nl5 fails (resa of the update's solve), nl6 passes,
and the product build stays within its bound (rel(psi) 8.9e-14).  The file runs in about 255 s, nearly all of it in the
single-threaded vertex oracle.

Each oracle result is computed once (the module cache of test_gpu_oracle_fullsize.py) and freed after its last use."""
import gc

import numpy as np
import pytest

import orn
from msom_amd import NodeQG
from test_gpu_oracle_fullsize import _cache, cached
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

N = 2048
BOUND = 1e-10
# nl -> (dh, N2 of the interfaces).  Under sqg = 1 the surface N2 goes first (nl entries in all)
DH = {1: [1.0], 2: [0.35, 0.65], 3: [0.1, 0.3, 0.6], 4: [0.1, 0.2, 0.3, 0.4], 5: [0.05, 0.1, 0.2, 0.25, 0.4],
      6: [0.05, 0.08, 0.12, 0.2, 0.25, 0.3], 7: [0.03, 0.06, 0.09, 0.14, 0.18, 0.23, 0.27],
      8: [0.02, 0.04, 0.06, 0.09, 0.12, 0.16, 0.23, 0.28]}
N2 = {2: [4000.], 3: [9000., 3000.], 4: [9000., 5000., 2000.], 5: [9500., 7000., 4000., 2500.],
      6: [9500., 7500., 5500., 3500., 2000.], 7: [9800., 8200., 6600., 5100., 3700., 2400.],
      8: [9900., 8600., 7300., 6000., 4800., 3600., 2500.]}
N2_SURFACE = 300.
# case -> (nl, sqg, S2 varies in x, node_march_kmax, relax_path_<k> for k = 0 .. 10)
CHAIN4 = (3, 1, 2, 2, 2, 2, 4, 4, 4, 4, 4)
CHAIN3 = (3, 1, 1, 1, 1, 1, 4, 4, 4, 4, 4)
SPLIT = (1, 1, 1, 1, 1, 1, 4, 4, 4, 4, 4)
CASES = {"nl1": (1, 0, 0, 4, CHAIN4), "nl2": (2, 1, 0, 4, CHAIN4), "nl4": (4, 1, 0, 4, CHAIN4), "nl5": (5, 0, 0, 3, CHAIN3),
         "nl6": (6, 1, 0, 3, CHAIN3), "nl7": (7, 0, 0, 0, SPLIT), "nl8": (8, 1, 0, 0, SPLIT), "nl3_s2x": (3, 0, 1, 0, SPLIT)}


def params(case):
    nl, sqg, _, _, _ = CASES[case]
    n2 = ([N2_SURFACE] if sqg else []) + N2.get(nl, [1.0])
    fmt = lambda v: "[" + ",".join(repr(x) for x in v) + "]"
    return (f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\nnu = 5.0\nnu4 = 0.0\nbeta = 0.5\nbc_fac = 1.0\n"
            f"dh = {fmt(DH[nl])}\nN2 = {fmt(n2)}\nDT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = 1e-5\n"
            + ("sqg = 1\n" if sqg else "") + ("gp_low = 5e4\n" if nl == 1 else ""))


def inputs(case):
    """C5's island mask; psi with its own amplitude and phase in every layer (none zero); surface buoyancy under sqg; for
    nl3_s2x an S2 (N^2 until set_const) that varies in x"""
    nl, sqg, s2x, _, _ = CASES[case]
    x = np.arange(N + 1) / N
    mk = np.ones((1, N + 1, N + 1))
    mk[0, N // 4: N // 4 + N // 8, N // 2: N // 2 + N // 8] = 0
    mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
    sx = [np.sin(k * np.pi * x) for k in range(4)]
    psi = np.stack([1e-2 / (1 + 0.3 * l) * sum(np.sin(1.3 * k + 2.1 * m + 0.7 * l) / (k * m) * np.outer(sx[m], sx[k])
                                                for k in range(1, 4) for m in range(1, 4)) for l in range(nl)]) * mk
    out = dict(MASK=mk, PSI=psi)
    if sqg:
        out["BS"] = 0.3 * np.outer(np.sin(np.pi * x), np.sin(2 * np.pi * x))[None] + 0.05
    if s2x:
        out["S2"] = np.array(N2[nl])[:, None, None] * (1.0 + 0.3 * np.cos(np.linspace(0, 5, N + 1)))[None, None, :] * np.ones((1, N + 1, 1))
    return out


def run_node(m, case, setf, getf):
    """set_const, one update() (dq and its dt), one step(True); mgstats of both solves.  psi is cleared after set_const (which
    computed q from it): the update's solve recovers it from a zero first guess instead of stopping after one cycle"""
    for f, a in inputs(case).items():
        setf(f, a)
    m.set_const()
    setf("PSI", np.zeros_like(getf("PSI")))
    dtmax = m.update()
    s = m.mgstats()
    out = dict(dq=getf("DQ"), dtmax=dtmax, st_update=(s.i, s.resb, s.resa, s.nrelax))
    m.step(True)
    s = m.mgstats()
    out.update(psi=getf("PSI"), q=getf("Q"), t=m.t, dt=m.dt, st=(s.i, s.resb, s.resa, s.nrelax))
    return out


def run_oracle(case, smoother=orn.GS_RB):
    o = orn.NodeOracle(params(case), smoother=smoother, quiet=1)
    out = run_node(o, case, lambda f, a: o.set(getattr(orn, f), a), lambda f: o.get(getattr(orn, f)))
    del o
    gc.collect()
    return out


def oracle_node(case):
    return cached(("node_layers", case), lambda: run_oracle(case))


def gpu_node(case, strict):
    g = NodeQG(params(case), strict=strict)
    g.set_option("quiet", 1)
    out = run_node(g, case, g.set, g.get)
    nlev = int(g.param("nlevels"))
    out["switch"] = dict(nlevels=nlev, node_march_s=g.param("node_march_s"), split_0=g.param("split_0"),
                         s2_xuniform=g.param("s2_xuniform"), node_march_kmax=g.param("node_march_kmax"),
                         corr_march=g.param("corr_march"), paths=tuple(int(g.param(f"relax_path_{k}")) for k in range(nlev)))
    g.close()
    return out


def product_nl1():
    """the product result at nl1: kept for the negative control"""
    return cached(("node_layers", "nl1", "product"), lambda: gpu_node("nl1", False))


def assert_reference_sound(o):
    """a degenerate oracle run (NaN fields reported as a converged solve) must not pass as a reference"""
    for k in ("dq", "psi", "q"):
        assert np.isfinite(o[k]).all(), k
    for st in (o["st_update"], o["st"]):
        assert st[0] >= 3 and st[1] > 0, st


@pytest.mark.parametrize("case,strict", [(c, s) for c in CASES for s in (True, False)])
def test_vertex_default_kernels_equal_oracle_at_every_layer_count(case, strict):
    nl, sqg, s2x, kmax, paths = CASES[case]
    o = oracle_node(case)
    assert_reference_sound(o)
    if strict:
        g = gpu_node(case, True)
        assert (g["dtmax"], g["t"], g["dt"]) == (o["dtmax"], o["t"], o["dt"])
        assert (g["st_update"], g["st"]) == (o["st_update"], o["st"])
        for k in ("dq", "psi", "q"):
            assert np.array_equal(g[k], o[k]), (k, rel(g[k], o[k]), int(np.count_nonzero(g[k] != o[k])))
        return
    _cache.pop(("node_layers", case))      # its last use (the strict build ran first)
    g = product_nl1() if case == "nl1" else gpu_node(case, False)
    sw = g["switch"]
    # what puts the paths under test: 2049 vertices a side = node_march_s, the split layout on level 0, row tables unless S2
    # varies in x; then the path of every level
    assert sw["nlevels"] == len(paths) and sw["node_march_s"] == N + 1 and sw["split_0"] == 1, sw
    assert sw["s2_xuniform"] == (0 if s2x else 1) or nl == 1, sw
    assert sw["node_march_kmax"] == kmax and sw["corr_march"] == 1, sw
    assert sw["paths"] == paths, sw
    assert (g["st_update"][0], g["st_update"][3], g["st"][0], g["st"][3]) == (o["st_update"][0], o["st_update"][3], o["st"][0], o["st"][3])
    assert g["dtmax"] == pytest.approx(o["dtmax"], rel=1e-12) and g["dt"] == pytest.approx(o["dt"], rel=1e-12)
    errs = {k: rel(g[k], o[k]) for k in ("dq", "q", "psi")}
    print(f"vertex {case} product vs oracle: " + ", ".join(f"rel({k}) = {v:.3g}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= BOUND, (k, v)


def test_vertex_layer_bound_sees_sweep_order():
    """negative control: at nl1 the product result against the lexicographic oracle is far outside the bound"""
    g = product_nl1()
    _cache.pop(("node_layers", "nl1", "product"))
    o = run_oracle("nl1", orn.GS_LEX)
    d = rel(g["psi"], o["psi"])
    print(f"vertex nl1 product (red-black) vs lexicographic oracle: rel(psi) = {d:.3g}")
    assert d > 100 * BOUND
