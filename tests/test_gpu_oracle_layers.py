"""The default kernels against the CPU oracle at the layer counts other than 3 and 6, each at the smallest square grid on which the
default chain marches.  The register-resident kernels are templated on the layer count (march_dispatch<NL> with its lean interior
body, k_resmax_march<NL>, k_mg_coarse(_lean)<NL>, k_relax_block<NL, ..>, k_relax_red_prolong*<NL>): every NL is its own register
allocation and instruction schedule, and the one real bug of these paths (a hazard of the lean body's inline
assembly) showed only at 2048^2 x 6 and 4096^2 x 6.  No kernel option is set.

  nl1   4096^2 x 1   one layer (x = rhs / 4, no vertical coupling; uniform_S stays 0, sweep_path admits nl = 1 in both builds)
  nl2   2048^2 x 2   exactly 2^23 cell-layers: the >= of sweep_path
  nl4   2048^2 x 4   NL = 4
  nl5   2048^2 x 5   odd: the lean body's DMA repeats the last layer (NLE = 6)
  nl7   2048^2 x 7   at most 3 half-sweeps per pass (march_kmax); odd; the coarse group too large for the lean LDS form
  nl8   2048^2 x 8   march_kmax 3; two marched levels, level 1 (1024^2 x 8 = 2^23) with few strips and short chunks
  nl16  2048^2 x 16  MSOM_MAXNL: nothing marched, no k_resmax_march, no one-launch coarse group; the general kernels at several
                     workgroup rounds

Each case runs at the reference tolerance 1e-3 (one cycle per solve: psi depends on every half-sweep) and at 1e-9 (5 cycles in the
oracle's last solve for every case, asserted >= 3: nrelax adapts and passes of every allowed K run).  Three checks per case:
  1. strict build against the oracle, bit for bit (dq, q, psi, dtmax, dt, mgstats);
  2. product build against the oracle: equal cycle count and nrelax, dt to 1e-12, rel <= 1e-10 on dq, q and psi, after the path
     switches of the handle and the smoother of every level (relax_path_<k> against expected_relax_paths, a table written from
     the documented thresholds) are asserted (a moved threshold must fail here instead of quietly testing something else);
  3. strict build with uniform_S = 1 (the strict build never takes the uniform-S path, so check 1 does not march except at
     nl = 1) against the same through REFERENCE_CHAIN (test_gpu_fullsize.py), bit for bit: this one sees an ulp in one cell.
First measured product maxima (MI355X), rel(dq), rel(q), rel(psi), the larger of the two tolerances:
  nl1 5.7e-12, 4.4e-12, 3.9e-15;  nl2 2.8e-13, 3.2e-13, 1.7e-15;  nl4 6.6e-14, 1.5e-14, 1.5e-15;  nl5 3.9e-14, 3.1e-15, 1.6e-15;
  nl7 3.8e-14, 1.9e-15, 1.6e-15;  nl8 3.8e-14, 2.1e-15, 1.1e-15;  nl16 3.5e-14, 8.3e-16, 1.4e-15.
With march_lean's sqD one ulp off for NL = 7 alone, only check 3 of nl7 fails (q differs in 6050 cells at 1e-3, resa at 1e-9);
the product build stays within its bound (rel(q) 1.9e-15).  The file runs in about 120 s.

Each oracle result is computed once (the module cache of test_gpu_oracle_fullsize.py) and freed after its last use."""
import gc

import numpy as np
import pytest

import orc
from msom_amd import QG
from test_gpu_fullsize import REFERENCE_CHAIN
from test_gpu_oracle_fullsize import _cache, cached, expected_relax_paths, relax_paths, run_cell
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

# layers -> (N, what the product build's handle reports: march_levels, resmax_marching, mg_coarse_lean, march_kmax).
# mg_coarse_lean: the levels <= 32^2 of the group need 2996 nl doubles of the 19200-double LDS pool, which fits up to nl = 6;
# march_kmax is 3 from nl = 7 on (nl16 included, although nothing marches there)
LAYERS = {1: (4096, 1, 0, 1, 4), 2: (2048, 1, 1, 1, 4), 4: (2048, 1, 1, 1, 4), 5: (2048, 1, 1, 1, 4), 7: (2048, 1, 1, 0, 3),
          8: (2048, 2, 1, 0, 3), 16: (2048, 0, 0, 0, 3)}
TOLS = {"1e-3": 1e-3, "1e-9": 1e-9}
CASES = {f"nl{nl}_tol{t}": (nl, tol) for nl in LAYERS for t, tol in TOLS.items()}


def inputs(case):
    nl, tol = CASES[case]
    N = LAYERS[nl][0]
    return orc.double_gyre_params(N, nl), N, nl, tol


def oracle_layers(case):
    def compute():
        txt, N, nl, tol = inputs(case)
        o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1)
        out = run_cell(o, N, nl, tol)
        del o
        gc.collect()
        return out
    return cached(("layers", case), compute)


def gpu_layers(case, strict, opts=None):
    """run_cell on a QG handle; opts are set before set_const.  Returns the outputs and the handle's path switches"""
    txt, N, nl, tol = inputs(case)
    g = QG(txt, strict=strict)
    g.option("quiet", 1)

    def pre(h):
        for k, v in (opts or {}).items():
            h.option(k, v)
    out = run_cell(g, N, nl, tol, pre)
    out["switch"] = {k: g.param(k) for k in ("uniform_S", "march_levels", "march_min", "march_kmax", "resmax_marching",
                                             "mg_coarse_lean", "restrict2")}
    out["paths"] = relax_paths(g)
    g.close()
    return out


def assert_bit_equal(a, b):
    assert a["dtmax"] == b["dtmax"] and a["dt"] == b["dt"]
    assert a["st"] == b["st"]
    for k in ("dq", "q", "psi"):
        same = np.array_equal(a[k], b[k])
        assert same, (k, rel(a[k], b[k]), int(np.count_nonzero(a[k] != b[k])))   # field, rel(max), cells that differ


@pytest.mark.parametrize("case,strict", [(c, s) for c in CASES for s in (True, False)])
def test_default_kernels_equal_oracle_at_every_layer_count(case, strict):
    nl, tol = CASES[case]
    o = oracle_layers(case)
    if tol < 1e-3:
        assert o["st"][0] >= 3, o["st"]     # passes of every allowed K run
    if strict:
        assert_bit_equal(gpu_layers(case, True), o)
        return
    _cache.pop(("layers", case))            # its last use (the strict build ran first)
    g = gpu_layers(case, False)
    N, levels, resmax, lean, kmax = LAYERS[nl]
    sw = g["switch"]
    # what selects the paths under test: uniform S (the product default from nl = 2), 2^march_min cell-layers per marched level
    assert sw["uniform_S"] == (nl > 1) and sw["march_min"] == 23
    assert sw["march_levels"] == levels, sw
    assert sw["resmax_marching"] == resmax and sw["mg_coarse_lean"] == lean and sw["restrict2"] == 1, sw
    assert sw["march_kmax"] == kmax, sw
    assert g["paths"] == expected_relax_paths(N, nl), g["paths"]   # the smoother of every level
    assert (g["st"][0], g["st"][3]) == (o["st"][0], o["st"][3])
    assert g["dt"] == pytest.approx(o["dt"], rel=1e-12)
    errs = {k: rel(g[k], o[k]) for k in ("dq", "q", "psi")}
    print(f"{case} product vs oracle: " + ", ".join(f"rel({k}) = {v:.3g}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 1e-10, (k, v)


@pytest.mark.parametrize("case", list(CASES))
def test_strict_chained_defaults_equal_reference_chain_at_every_layer_count(case):
    nl, tol = CASES[case]
    a = gpu_layers(case, True, dict(uniform_S=1))
    b = gpu_layers(case, True, dict(REFERENCE_CHAIN, uniform_S=1))
    assert b["switch"]["march_levels"] == 0 and set(b["paths"]) == {0}     # march, block8 and mg_coarse are off: colour launches
    assert a["switch"]["march_min"] == 23           # the threshold expected_relax_paths is written for
    assert a["paths"] == expected_relax_paths(LAYERS[nl][0], nl), a["paths"]
    if nl <= 8:
        assert a["switch"]["march_levels"] == LAYERS[nl][1] >= 1, a["switch"]
    else:
        assert a["switch"]["march_levels"] == 0, a["switch"]
    assert_bit_equal(a, b)
