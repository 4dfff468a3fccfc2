"""The remaining legs of bench.py against the CPU oracle at the size they are timed at (test_gpu_oracle_fullsize.py covers C3,
C4 and both halves of C5's default cell and vertex paths).  No kernel option is set, and the inputs are built the way bench.py's
Leg builds them: the same params text and extras, the same synthetic psi, Fr field formula, sigma, seed and noise_mode.

- C4_periodic (4096^2 x 6, sbc = -1, tau0 = 0): the chained smoother on a doubly periodic single tile, whose deep halo is
  filled by local wrap copies (launch_split_wrap) rather than by walls.
- C4_general_S (4096^2 x 6, Fr(x, y) = Fr_l (1 + 0.3 sin 2 pi y cos 2 pi x)): the general column solver (S read per cell, no
  marching).  Negative control: the product result is far from the uniform-S C4 oracle result.
- the split leg (4096^2 x 6 on 2 x 4 tiles of 2048 x 1024 through the in-process transport): deep-halo marching on tiles,
  overlapped exchanges, agglomerated coarse levels.  A tile of 2048 x 1024 has 10 multigrid levels (its short side halves down
  to 2 cells) and the agglomerated levels are gathered copies of the tile levels, so the split layout solves on 10 levels
  where the whole 4096^2 grid has 12: the oracle runs with MGLEVELS = 10, everything else as benchmarked.
- C5 (2048^2 x 3, stochastic, noise_mode = 1, seed 7, sigma = 1): the device Philox noise against the numpy reference
  (philox_ref.py) for draws 0, 1, 2, single tile and 2 x 1 tiles; then the stochastic step against the oracle, which is
  handed the device's noise of each step (option noise_given).

Strict build: bit for bit.  Product build: rel <= 1e-10 on dq, q and psi, equal cycle counts and nrelax, dt to 1e-12.
The strict build never takes the uniform-S path, so it neither marches nor agglomerates: the path switches are asserted on
the product build.  First measured product maxima (MI355X), rel(dq), rel(q), rel(psi):
  C4_periodic tol 1e-3: 3.5e-11, 4.1e-15, 2.4e-15;  tol 1e-9: 3.5e-11, 4.4e-15, 3.3e-15 (march_levels 2);
  C4_general_S tol 1e-3: 1.6e-13, 5.5e-15, 4.1e-15;  tol 1e-7: 1.6e-13, 5.2e-15, 1.8e-15;
  split 2 x 4, rel(q), rel(psi): 2.4e-15, 7.8e-16 (march_levels 1, agg_level 3 on every tile);
  C5 with device noise, rel(q), rel(psi): 2.9e-14, 1.6e-15;  noise against the reference: <= 3.3e-16 amp (|a| + 1).
rel(dq) of the periodic leg is larger than C4's 1.7e-13 because its max|dq| is 190 times smaller (tau0 = 0: no wind
forcing in the top layer); the absolute difference is the same, about 2e-14.
Negative control: the general-S product result differs from the uniform-S C4 oracle by rel(psi) = 2.9e-2.
Each oracle result is computed once (the module cache of test_gpu_oracle_fullsize.py) and freed after its last use; at most
one 4096^2 x 6 oracle instance exists at a time."""
import gc

import numpy as np
import pytest

import orc
import philox_ref as ph
from msom_amd import QG, FIELDS as F
from test_gpu_oracle_fullsize import INF, _cache, cached, oracle_cell, run_cell
from test_gpu_parity import rel
from test_gpu_tiled import assemble, run_tiled

pytestmark = pytest.mark.gpu

N4, NL4 = 4096, 6
PERIODIC = "sbc = -1\ntau0 = 0\n"
# leg -> (params extra, Fr field, TOLERANCE).  Tight tolerance: >= 3 cycles in the oracle's last solve (asserted below); the
# periodic leg converges faster than the walled one (2 cycles at 1e-7, 3 at 1e-9), the general-S leg gives 3 at 1e-7
LEGS = {"C4_periodic_tol1e-3": (PERIODIC, False, 1e-3), "C4_periodic_tol1e-9": (PERIODIC, False, 1e-9),
        "C4_general_S_tol1e-3": ("", True, 1e-3), "C4_general_S_tol1e-7": ("", True, 1e-7)}


def fr_field(m, N, nl):
    """bench.py's Froude field on the whole grid, set with FR before set_const (oracle or QG handle)"""
    x = (np.arange(N) + 0.5) / N
    shape = 1.0 + 0.3 * np.outer(np.sin(2 * np.pi * x), np.cos(2 * np.pi * x))
    fr = np.stack([m.param(f"Fr_{l}") * shape for l in range(nl - 1)])
    m.set(orc.FR if isinstance(m, orc.Oracle) else F["FR"], fr)


def leg_inputs(leg):
    extra, fr, tol = LEGS[leg]
    return orc.double_gyre_params(N4, NL4, extra=extra), (lambda m: fr_field(m, N4, NL4)) if fr else None, tol


def oracle_leg(leg):
    def compute():
        txt, pre, tol = leg_inputs(leg)
        o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1)
        out = run_cell(o, N4, NL4, tol, pre)
        del o
        gc.collect()
        return out
    return cached((leg, orc.GS_RB), compute)


def gpu_leg(leg, strict):
    txt, pre, tol = leg_inputs(leg)
    g = QG(txt, strict=strict)
    g.option("quiet", 1)
    out = run_cell(g, N4, NL4, tol, pre)
    out["switch"] = {k: g.param(k) for k in ("uniform_S", "march_levels", "march_min")}
    g.close()
    sw = out["switch"]
    if LEGS[leg][1]:
        # the general column solver: S per cell, so no chained smoother on any level
        assert sw["uniform_S"] == 0 and sw["march_levels"] == 0, sw
    elif not strict:    # the strict build never takes the uniform-S path (set_const), so it does not march either
        # periodic: uniform S, at least 2^march_min cell-layers, the chained smoother on the finest level (wrap-filled halo)
        assert sw["uniform_S"] == 1 and N4 * N4 * NL4 >= 2 ** sw["march_min"] and sw["march_levels"] >= 1, sw
    return out


def uniform_c4_psi():
    """psi of the uniform-S C4 oracle cell at tolerance 1e-3: kept by test_gpu_oracle_fullsize.py, computed here if that file
    did not run first"""
    def compute():
        psi = oracle_cell("C4_tol1e-3")["psi"]
        _cache.pop(("C4_tol1e-3", orc.GS_RB))
        return psi
    return cached(("C4_tol1e-3", "psi"), compute)


def check(name, g, o, strict, keys=("dq", "q", "psi")):
    if strict:
        for k in keys:
            assert np.array_equal(g[k], o[k]), (k, rel(g[k], o[k]))
    else:
        errs = {k: rel(g[k], o[k]) for k in keys}
        print(f"{name} product vs oracle: " + ", ".join(f"rel({k}) = {v:.3g}" for k, v in errs.items()))
        for k, v in errs.items():
            assert v <= 1e-10, (k, v)


@pytest.mark.parametrize("leg,strict", [(c, s) for c in LEGS for s in (True, False)])
def test_periodic_and_general_S_legs_equal_oracle(leg, strict):
    o = oracle_leg(leg)
    g = gpu_leg(leg, strict)
    if not strict:
        _cache.pop((leg, orc.GS_RB))    # its last use (the strict build ran first)
    print(f"{leg} {'strict' if strict else 'product'}: {g['switch']}, oracle cycles {o['st'][0]}, nrelax {o['st'][3]}")
    if LEGS[leg][2] < 1e-3:
        assert o["st"][0] >= 3, o["st"]
    if strict:
        assert g["dtmax"] == o["dtmax"] and g["dt"] == o["dt"]
        assert g["st"] == o["st"]
    else:
        assert (g["st"][0], g["st"][3]) == (o["st"][0], o["st"][3])
        assert g["dt"] == pytest.approx(o["dt"], rel=1e-12)
    check(leg, g, o, strict)
    if leg == "C4_general_S_tol1e-3" and not strict:
        # negative control: the same psi and tolerance without the Fr field -- the field reached the kernels at this size
        d = rel(g["psi"], uniform_c4_psi())
        _cache.pop(("C4_tol1e-3", "psi"))
        print(f"C4_general_S tol 1e-3, product vs uniform-S C4 oracle: rel(psi) = {d:.3g}")
        assert d > 1e-6


# ---------------------------------------------------------------------------------------------------------------- split leg

SPLIT = (2, 4, 2048, 1024)
SPLIT_LEVELS = 10


def split_oracle():
    def compute():
        o = orc.Oracle(orc.double_gyre_params(N4, NL4, extra=f"MGLEVELS = {SPLIT_LEVELS}\n"), smoother=orc.GS_RB, quiet=1)
        assert o.nlevels() == SPLIT_LEVELS
        o.set(orc.PSI, orc.synthetic_psi(NL4, N4, N4))
        o.set_const()
        o.set_tnext(INF)
        o.step()
        st = o.mgstats()
        out = dict(q=o.get(orc.Q), psi=o.get(orc.PSI), dt=o.dt, st=(st.i, st.resb, st.resa, st.nrelax))
        del o
        gc.collect()
        return out
    return cached("split", compute)


@pytest.mark.parametrize("strict", [True, False])
def test_split_layout_2x4_tiles_equals_oracle(strict):
    """bench.py's split leg: the params of the benchmarked leg (no MGLEVELS cap: the tiles have 10 levels of their own), one
    RK2 step without a preceding update(), as the benchmark steps; the oracle steps the same way"""
    px, py, tx, ty = SPLIT
    o = split_oracle()
    params = orc.double_gyre_params(N4, NL4)
    out = run_tiled(params, px, py, orc.synthetic_psi(NL4, N4, N4), nsteps=1, strict=strict,
                    fn=lambda g, r: dict(march_levels=g.param("march_levels"), nlevels=g.nlevels(), overlap=g.param("overlap")))
    if not strict:
        _cache.pop("split")
    print(f"split 2x4 {'strict' if strict else 'product'}: " + ", ".join(f"tile {r}: {out[r]['extra']}, agg_level {out[r]['agg']}" for r in range(px * py)))
    for r in range(px * py):
        ex = out[r]["extra"]
        assert ex["nlevels"] == SPLIT_LEVELS and ex["overlap"] == 1, (r, ex)
        if not strict:
            # product: uniform S, so the finest tile level (2^24 cell-layers >= 2^march_min_tiled) marches with its deep halo
            # exchanged, and the coarse levels from 256 cells a side are gathered (agglomerated); the strict build does neither
            assert ex["march_levels"] >= 1 and out[r]["agg"] >= 0, (r, ex, out[r]["agg"])
        st = out[r]["st"]
        assert out[r]["dts"][0] == (o["dt"] if strict else pytest.approx(o["dt"], rel=1e-12)), r
        if strict:
            assert (st.i, st.resb, st.resa, st.nrelax) == o["st"], (r, st, o["st"])
        else:
            assert (st.i, st.nrelax) == (o["st"][0], o["st"][3]), (r, st, o["st"])
    got = {k: assemble(out, k, px, py) for k in ("q", "psi")}
    check("split 2x4 tiles of 2048x1024x6", got, o, strict, keys=("q", "psi"))


# ---------------------------------------------------------------------------------------------------------------- C5 noise

N5, NL5, SEED, AMP = 2048, 3, 7, 1e-5
C5_TXT = orc.double_gyre_params(N5, NL5, extra=f"tr_stoch = 50\namp_stoch = {AMP}\n")
C5_OPTS = {"stochastic": 1, "noise_mode": 1, "seed": SEED}


def check_noise(n, draw, gx0=0, gy0=0, gnx=N5, what=""):
    """elementwise to a few ulp of the Box-Muller result: device log / cos may differ from the host's by an ulp, a wrong
    counter or key differs by O(amp)"""
    ref, a = ph.noise(np.ones(n.shape), AMP, SEED, draw, gx0, gy0, gnx, radius=True)
    d = np.abs(n - ref)
    bound = 1e-14 * AMP * (a + 1)
    assert np.all(d <= bound), (what, draw, float((d / (AMP * (a + 1))).max()))
    return float((d / (AMP * (a + 1))).max())


def c5_gpu(strict):
    """3 steps of C5 on one tile: NOISE after every step, q / psi / dt after the first two"""
    def compute():
        g = QG(C5_TXT, strict=strict)
        g.option("quiet", 1)
        for k, v in C5_OPTS.items():
            g.option(k, v)
        g.set(F["PSI"], orc.synthetic_psi(NL5, N5, N5))
        g.set(F["SIGMA"], np.ones((NL5, N5, N5)))
        g.set_const()
        g.set_tnext(INF)
        out = dict(noise=[], dts=[])
        for s in range(3):
            out["dts"].append(g.step())
            out["noise"].append(g.get(F["NOISE"]))
            if s == 1:
                out["q"], out["psi"] = g.get(F["Q"]), g.get(F["PSI"])
        g.close()
        return out
    return cached(("C5", strict), compute)


@pytest.mark.parametrize("strict", [True, False])
def test_device_noise_equals_philox_reference_draw_by_draw(strict):
    """NOISE after step k is draw k - 1 of the counter-based generator: each of draws 0, 1, 2 against the reference, so a
    stream that does not advance, a counter collision between layers or a wrong key schedule fails"""
    out = c5_gpu(strict)
    errs = [check_noise(n, d, what="single tile") for d, n in enumerate(out["noise"])]
    print(f"C5 noise {'strict' if strict else 'product'}, max |n - ref| / (amp (|a| + 1)) per draw: " + ", ".join(f"{e:.3g}" for e in errs))
    for a, b in ((0, 1), (1, 2)):
        assert np.abs(out["noise"][a] - out["noise"][b]).max() > AMP


def test_device_noise_on_2x1_tiles_equals_philox_reference():
    """the tiled offsets: every tile's counter is its global cell (gx0 + i, gy0 + j) of the global grid"""
    px, py = 2, 1
    tx, ty = N5 // px, N5 // py

    def steps(g, rank):
        out = []
        for _ in range(3):
            g.step()
            out.append(g.get(F["NOISE"]))
        return out

    out = run_tiled(C5_TXT, px, py, orc.synthetic_psi(NL5, N5, N5), nsteps=0, strict=False, opts=C5_OPTS, fn=steps,
                    pre=lambda g, r: g.set(F["SIGMA"], np.ones((NL5, ty, tx))))
    for r in range(px * py):
        ix, iy = r % px, r // px
        for d, n in enumerate(out[r]["extra"]):
            check_noise(n, d, gx0=ix * tx, gy0=iy * ty, gnx=N5, what=f"tile {r}")


@pytest.mark.parametrize("strict", [True, False])
def test_stochastic_step_with_device_noise_equals_oracle(strict):
    """two stochastic steps at C5 against the oracle, which is given the device's noise of each step (noise_given): the
    stochastic RHS and advance of both builds at size"""
    g = c5_gpu(strict)
    o = orc.Oracle(C5_TXT, smoother=orc.GS_RB, quiet=1, stochastic=1)
    o.set(orc.PSI, orc.synthetic_psi(NL5, N5, N5))
    o.set_const()
    o.set_tnext(INF)
    dts = []
    for s in range(2):
        o.set_noise(g["noise"][s])
        o.step()
        dts.append(o.dt)
    res = dict(q=o.get(orc.Q), psi=o.get(orc.PSI))
    del o
    gc.collect()
    if strict:
        assert g["dts"][:2] == dts
    else:
        _cache.pop(("C5", True), None)
        _cache.pop(("C5", False), None)
        assert g["dts"][:2] == pytest.approx(dts, rel=1e-12)
    check("C5 stochastic, device noise", g, res, strict, keys=("q", "psi"))
