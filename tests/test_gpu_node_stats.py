"""Running time means and eddy statistics of the vertex model on the device (msomn_stats_begin / _accumulate / _weight / _get, options
"stats" and "stats_every"; include/msom.h) against tests/node_stats_ref.py, the numpy restatement of the
documented expression order.  Strict build: bit for bit.  Product build (contraction, reciprocal of 2 D): relative error to the
field's maximum <= TOL_PRODUCT, the project's bound for contracted against uncontracted arithmetic (tests/test_gpu_bfn.py).

The inputs are those of tests/test_gpu_node_tiled.py: an island across a seam, land over the cross point, a bay in the land along the
north wall -- the places where the land mask and the boundary rule of u and v can go wrong.  33 and 65 vertices a row: every row has
a tail vertex that goes alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import orn
from msom_amd import NodeQG, STATS as ST, api, node_from_state
from msom_amd.state import NODE_STATS_KEYS, NODE_STATS_RECORDS, read_state
from msom_amd.tiling import node_assemble
from node_stats_ref import ACC, DERIVED, NEEDS, NodeStats
from test_gpu_bfn import TOL_PRODUCT
from test_gpu_hooks import DevBuf
from test_gpu_node_tiled import OPTION_KEYS, inputs, params, run_tiled, single
from test_gpu_parity import rel

pytestmark = pytest.mark.gpu

MSOM_ERR_ARG, MSOM_ERR_STATE = -1, -6
FULL = (1 << ST["NACC"]) - 1
WEIGHTS = (0.75, 0.013, 2.5)
NAUTO = 4
SHAPES = [(32, 1), (32, 3), (64, 1), (64, 3), (32, 6)]


def bits(*names):
    return sum(1 << ST[n] for n in names)


def handle(N, nl, strict, **opts):
    return single(params(N, nl), inputs(N, nl), strict, opts)


def numpy_stats(g, N, nl):
    return NodeStats(nl, N, inputs(N, nl)["MASK"], 2.0 * (g.param("L0") / g.param("N")))


def mg(g):
    s = g.mgstats()
    return (s.i, s.resb, s.resa, s.sum, s.nrelax)


# ------------------------------------------------------------------ 1. the kernel against numpy

def manual_run(N, nl, strict, mask):
    """three samples with three weights; a new random psi (land and boundary ring included) and q = comp_q(psi) between them.
    Returns the handle and the (psi, q, w) the samples saw"""
    g = handle(N, nl, strict)
    g.stats_begin(mask)
    rng = np.random.default_rng(7 * N + nl)
    seen = []
    for k, w in enumerate(WEIGHTS):
        if k > 0:
            g.set("PSI", 1e-3 * rng.standard_normal((nl, N + 1, N + 1)))
            g.comp_q()
        seen.append((g.get("PSI"), g.get("Q"), w))
        g.stats_accumulate(w)
    return g, seen


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("N,nl", SHAPES)
def test_accumulate_against_numpy(N, nl, strict):
    g, seen = manual_run(N, nl, strict, FULL)
    ref = numpy_stats(g, N, nl)
    for s in seen:
        ref.sample(*s)
    assert g.param("stats_mask") == FULL and g.param("stats_samples") == len(WEIGHTS)
    assert g.param("stats_bytes") == ST["NACC"] * nl * (N + 1) * (N + 1) * 8
    got = {n: g.stats_get(ST[n]) for n in ACC + DERIVED}
    for n in ACC + DERIVED:
        want = ref.get(n)
        if strict:
            assert np.array_equal(got[n], want), (n, np.count_nonzero(got[n] != want))
        else:
            print(f"N {N} nl {nl} {n}: rel {rel(got[n], want):.3e}")
            assert rel(got[n], want) <= TOL_PRODUCT, n
    assert g.stats_weight() == ref.W        # W = W + w: nothing to contract
    # land and the boundary ring carry no velocity; the sea next to the island does
    dry = inputs(N, nl)["MASK"][0] == 0
    dry[0, :] = dry[-1, :] = dry[:, 0] = dry[:, -1] = True
    for n in ("KE", "UQ", "VQ"):
        assert np.all(got[n][:, dry] == 0), n
        assert np.all(got[n][:, N // 8 - 1, N // 2] != 0), n      # the vertex south of the island
    g.close()


# ------------------------------------------------------------------ 2. the mask selects

@functools.lru_cache(maxsize=None)
def full_mask_means():
    g, _ = manual_run(32, 3, True, FULL)
    out = {n: g.stats_get(ST[n]) for n in ACC + DERIVED}
    g.close()
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("sel", [("PSI", "Q"), ("KE",), ("PSI", "KE"), ("PSI", "Q", "UQ")], ids="|".join)
def test_the_mask_selects(sel):
    N, nl = 32, 3
    full = full_mask_means()
    g, _ = manual_run(N, nl, True, bits(*sel))
    assert g.param("stats_mask") == bits(*sel)
    assert g.param("stats_bytes") == len(sel) * nl * (N + 1) * (N + 1) * 8
    out = np.empty((nl, N + 1, N + 1))
    for n in ACC:
        if n in sel:
            assert np.array_equal(g.stats_get(ST[n]), full[n]), n
        else:
            assert g.L.msomn_stats_get(g.h, ST[n], out.ctypes.data) == MSOM_ERR_ARG, n
    for n in DERIVED:
        if all(k in sel for k in NEEDS[n]):
            assert np.array_equal(g.stats_get(ST[n]), full[n]), n
        else:
            assert g.L.msomn_stats_get(g.h, ST[n], out.ctypes.data) == MSOM_ERR_ARG, n
    g.close()


# ------------------------------------------------------------------ 3. the automatic sample of msomn_step against the oracle

@functools.lru_cache(maxsize=None)
def oracle_run(N, nl):
    """NAUTO RK2 steps of the CPU oracle driven at hook level: forcing, update, read PSI / Q, advance dt / 2, update, advance dt.
    The oracle's clock stands still at hook level, so its forcing is the one of t = 0 in every step: the device run below calls
    forcing() once and steps without the forcing event.  Computed once per shape and shared; nothing below writes into it"""
    o = orn.NodeOracle(params(N, nl), smoother=orn.GS_RB, quiet=1)
    for f, a in inputs(N, nl).items():
        o.set(getattr(orn, f), a)
    o.set_const()
    o.set_tnext(float("inf"))
    seen = []
    for _ in range(NAUTO):
        o.forcing()
        dt = o.update(orn.Q, orn.DQ, o.param("DT"))      # tnext = inf: the step's dt is update's
        seen.append((o.get(orn.PSI), o.get(orn.Q), dt))
        o.advance(orn.QPRED, orn.Q, orn.DQ, dt / 2)
        o.update(orn.QPRED, orn.DQ, dt)
        o.advance(orn.Q, orn.Q, orn.DQ, dt)
    res = dict(seen=seen, q=o.get(orn.Q))
    for a in [res["q"]] + [x for s in seen for x in s[:2]]:
        a.setflags(write=False)
    return res


def auto_run(g, stats, every=None, mask=FULL, nsteps=NAUTO, forcing_event=False):
    if stats:
        g.stats_begin(mask)
        g.set_option("stats", 1)
        if every:
            g.set_option("stats_every", every)
    g.forcing()
    dts = []
    for _ in range(nsteps):
        g.step(forcing_event)
        dts.append(g.dt)
    return dict(dts=dts, q=g.get("Q"), psi=g.get("PSI"), mg=mg(g), t=g.t, draw=g.param("noise_draw"))


@pytest.mark.parametrize("N,nl", [(32, 1), (32, 3), (64, 3)])
def test_strict_automatic_samples_bit_exact_against_the_oracle(N, nl):
    o = oracle_run(N, nl)
    g = handle(N, nl, True)
    run = auto_run(g, True)
    assert run["dts"] == [s[2] for s in o["seen"]] and np.array_equal(run["q"], o["q"])     # the two drivers made the same run
    ref = numpy_stats(g, N, nl)
    W = 0.0
    for s in o["seen"]:
        ref.sample(*s)
        W = W + s[2]
    for n in ACC + DERIVED:
        assert np.array_equal(g.stats_get(ST[n]), ref.get(n)), n
    assert g.stats_weight() == W == ref.W and g.param("stats_samples") == NAUTO
    g.close()
    # stats_every = 2 samples steps 0 and 2
    g = handle(N, nl, True)
    run = auto_run(g, True, every=2)
    ref = numpy_stats(g, N, nl)
    for k in (0, 2):
        ref.sample(*o["seen"][k])
    for n in ACC + DERIVED:
        assert np.array_equal(g.stats_get(ST[n]), ref.get(n)), n
    assert g.stats_weight() == run["dts"][0] + run["dts"][2] and g.param("stats_samples") == 2
    g.close()


# ------------------------------------------------------------------ 4. the option changes nothing

def same_run(a, b):
    assert a["dts"] == b["dts"] and a["mg"] == b["mg"] and a["t"] == b["t"] and a["draw"] == b["draw"]
    assert np.array_equal(a["q"], b["q"]) and np.array_equal(a["psi"], b["psi"])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("N,nl", [(32, 1), (64, 3)])
def test_the_option_changes_nothing_in_the_run(N, nl, strict):
    runs = []
    for stats in (True, False):
        g = handle(N, nl, strict)
        runs.append(auto_run(g, stats, forcing_event=True))
        if stats:
            W = 0.0
            for dt in runs[0]["dts"]:
                W = W + dt
            assert g.stats_weight() == W and np.isfinite(g.stats_get(ST["EKE"])).all()
        g.close()
    same_run(*runs)


@pytest.mark.parametrize("strict", [True, False])
def test_the_option_changes_nothing_in_a_stochastic_run(strict):
    N, nl = 32, 1
    par, inp = params(N, nl) + "amp_stoch = 0.3\nL_filt = 8\n", inputs(N, nl)
    runs, noise = [], []
    for stats in (True, False):
        g = single(par, inp, strict, dict(stochastic=1, noise_mode=1, seed=11))
        runs.append(auto_run(g, stats, forcing_event=True))
        noise.append(g.noise())
        g.close()
    assert runs[0]["draw"] > 0                          # the steps drew; same_run holds the counter of both runs equal
    same_run(*runs)
    assert np.array_equal(*noise)


# ------------------------------------------------------------------ 5. tiles equal the single tile

def tiled_body(g, rank):
    g.stats_begin(FULL)
    g.set_option("stats", 1)
    g.profile_reset()                                   # the exchange counter from 0
    for _ in range(3):
        g.step(True)
    ex = [g.param("exchanges")]
    g.stats_accumulate(0.37)                            # by hand: (q_3, the predictor's psi), one exchange of psi
    ex.append(g.param("exchanges"))
    out = {n: g.stats_get(ST[n]) for n in ACC}          # plain means: no exchange
    ex.append(g.param("exchanges"))
    for n in DERIVED:                                   # one exchange of the mean psi each
        out[n] = g.stats_get(ST[n])
    ex.append(g.param("exchanges"))
    return dict(out=out, W=g.stats_weight(), samples=g.param("stats_samples"), ex=ex, opts={k: g.param(k) for k in OPTION_KEYS},
                bytes=g.param("stats_bytes"), shape=(g.nl, g.ny, g.nx))


def plain_steps_body(g, rank):
    g.profile_reset()
    for _ in range(3):
        g.step(True)
    return dict(ex=g.param("exchanges"))


@functools.lru_cache(maxsize=None)
def single_tile_stats():
    N, nl = 64, 3
    opts = dict.fromkeys(OPTION_KEYS[:7], 0)            # what a tiled handle resolves the fused passes to
    opts.update(node_split=65, mg_coarse=8)
    g = single(params(N, nl), inputs(N, nl), True, opts)
    res = tiled_body(g, 0)
    g.close()
    return res


@pytest.mark.parametrize("px,py", [(2, 2), (2, 1), (4, 2)])
def test_tiles_equal_the_single_tile(px, py):
    N, nl = 64, 3
    par, inp = params(N, nl), inputs(N, nl)
    out = run_tiled(par, px, py, inp, True, tiled_body, opts=dict(mg_coarse=8))
    ref = single_tile_stats()
    assert out[0]["opts"] == ref["opts"]                # the single tile ran the passes the tiles ran
    for r, o in enumerate(out):
        assert (o["W"], o["samples"]) == (ref["W"], ref["samples"]) == (ref["W"], 4), r
        assert o["bytes"] == ST["NACC"] * int(np.prod(o["shape"])) * 8
        e = o["ex"]
        assert (e[1] - e[0], e[2] - e[1], e[3] - e[2]) == (1, 0, len(DERIVED)), (r, e)
    for n in ACC + DERIVED:
        a = node_assemble([o["out"][n] for o in out], N, px, py, check_shared=True)
        assert np.array_equal(a, ref["out"][n]), (n, np.count_nonzero(a != ref["out"][n]))
    if (px, py) == (2, 2):                              # the automatic samples added no exchange to the three steps
        plain = run_tiled(par, px, py, inp, True, plain_steps_body, opts=dict(mg_coarse=8))
        assert [p["ex"] for p in plain] == [o["ex"][0] for o in out] and plain[0]["ex"] > 0


# ------------------------------------------------------------------ 6. the state file

BASE_RECORDS = ["time", "mgstats", "node", "psi", "q", "q_forcing", "mask", "S2", "topo", "psi_pg"]


def stats_of(g):
    return dict({n: g.stats_get(ST[n]) for n in ACC + DERIVED}, W=g.stats_weight(), samples=g.param("stats_samples"),
                mask=g.param("stats_mask"), q=g.get("Q"), dt=g.dt, t=g.t)


def same_stats(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("strict", [True, False])
def test_state_file_restarts_the_statistics(strict, tmp_path):
    N, nl = 32, 3
    path, plain = tmp_path / "stats.msom", tmp_path / "plain.msom"
    g = handle(N, nl, strict)
    g.save_state(plain, constants=True)
    assert list(read_state(plain)["records"]) == api.state_info(plain)["names"] == BASE_RECORDS       # what it wrote before
    auto_run(g, True, every=None, nsteps=2, forcing_event=True)
    g.save_state(path, constants=True)
    for _ in range(2):
        g.step(True)
    want = stats_of(g)
    g.close()
    d = read_state(path)
    assert list(d["records"]) == BASE_RECORDS[:3] + ["stats"] + BASE_RECORDS[3:6] + list(NODE_STATS_RECORDS) + BASE_RECORDS[6:]
    assert api.state_check(path) == len(d["records"])
    s = dict(zip(NODE_STATS_KEYS, d["records"]["stats"]))
    assert (s["mask"], s["count"], s["every"], s["on"], s["samples"]) == (FULL, 2, 1, 1, 2) and s["W"] > 0
    assert d["records"]["st_psi"].shape == (nl, N + 1, N + 1)
    # a handle made from the file alone
    c = node_from_state(path, strict=strict)
    c.set_option("quiet", 1)
    assert c.param("stats_mask") == FULL and c.param("stats_samples") == 2 and c.stats_weight() == s["W"]
    for _ in range(2):
        c.step(True)
    same_stats(stats_of(c), want)
    c.close()
    # a handle that has its constants and no statistics takes the file's
    b = handle(N, nl, strict)
    b.load_state(path)
    for _ in range(2):
        b.step(True)
    same_stats(stats_of(b), want)
    b.close()


# ------------------------------------------------------------------ 7. errors and life cycle

def test_errors_and_life_cycle():
    N, nl = 32, 3
    par, inp = params(N, nl), inputs(N, nl)
    g = NodeQG(par, strict=True)
    g.set_option("quiet", 1)
    L, h = g.L, g.h
    out, w = np.empty((nl, N + 1, N + 1)), C.c_double()
    assert g.param("stats_mask") == 0 and g.param("stats_bytes") == 0 and g.param("stats_samples") == 0
    # before msomn_set_const
    assert L.msomn_stats_begin(h, FULL) == MSOM_ERR_STATE
    assert L.msomn_stats_accumulate(h, 1.0) == MSOM_ERR_STATE
    assert L.msomn_stats_weight(h, C.byref(w)) == MSOM_ERR_STATE
    assert L.msomn_stats_get(h, ST["PSI"], out.ctypes.data) == MSOM_ERR_STATE
    assert L.msomn_set_option(h, b"stats", 1.0) == MSOM_ERR_STATE
    for f, a in inp.items():
        g.set(f, a)
    g.set_const()
    g.set_tnext(float("inf"))
    # no msomn_stats_begin since msomn_set_const
    assert L.msomn_stats_accumulate(h, 1.0) == MSOM_ERR_STATE
    assert L.msomn_stats_weight(h, C.byref(w)) == MSOM_ERR_STATE
    assert L.msomn_stats_get(h, ST["PSI"], out.ctypes.data) == MSOM_ERR_STATE
    assert L.msomn_set_option(h, b"stats", 1.0) == MSOM_ERR_STATE
    assert g.param("stats_mask") == 0 and g.param("stats_bytes") == 0
    # arguments
    for call in (lambda: L.msomn_stats_begin(None, FULL), lambda: L.msomn_stats_accumulate(None, 1.0), lambda: L.msomn_stats_weight(None, C.byref(w)),
                 lambda: L.msomn_stats_get(None, 0, out.ctypes.data)):
        assert call() == MSOM_ERR_ARG
    assert L.msomn_stats_begin(h, 0) == MSOM_ERR_ARG
    assert L.msomn_stats_begin(h, 1 << ST["NACC"]) == MSOM_ERR_ARG
    assert L.msomn_stats_begin(h, FULL | 1 << 20) == MSOM_ERR_ARG
    assert g.param("stats_bytes") == 0
    per = nl * (N + 1) * (N + 1) * 8
    g.stats_begin(bits("PSI", "KE"))
    assert g.param("stats_mask") == bits("PSI", "KE") and g.param("stats_bytes") == 2 * per
    assert L.msomn_stats_get(h, ST["PSI"], out.ctypes.data) == MSOM_ERR_STATE      # W == 0
    assert g.stats_weight() == 0.0
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert L.msomn_stats_accumulate(h, bad) == MSOM_ERR_ARG
    assert g.stats_weight() == 0.0 and g.param("stats_samples") == 0
    psi = g.get("PSI")
    g.stats_accumulate(0.5)
    assert g.stats_weight() == 0.5 and g.param("stats_samples") == 1
    for which in (-1, ST["NACC"], 15, 19, ST["QME"], 99):
        assert L.msomn_stats_get(h, which, out.ctypes.data) == MSOM_ERR_ARG, which  # unknown id; QME is not offered
    assert L.msomn_stats_get(h, ST["Q"], out.ctypes.data) == MSOM_ERR_ARG           # not in the mask
    assert L.msomn_stats_get(h, ST["UQ_EDDY"], out.ctypes.data) == MSOM_ERR_ARG
    assert L.msomn_stats_get(h, ST["EKE"], out.ctypes.data) == 0
    assert L.msomn_stats_get(h, ST["PSI"], None) == MSOM_ERR_ARG and L.msomn_stats_weight(h, None) == MSOM_ERR_ARG
    assert np.array_equal(g.stats_get(ST["PSI"]), (0.5 * psi) / 0.5)
    assert L.msomn_set_option(h, b"stats_every", 0.0) == MSOM_ERR_ARG
    # update, advance and invert_q on their own never sample, with the option on
    g.set_option("stats", 1)
    dt = g.update()
    g.advance("QPRED", "Q", "DQ", dt / 2)
    g.invert_q()
    assert g.stats_weight() == 0.5 and g.param("stats_samples") == 1
    g.step(True)
    assert g.stats_weight() == 0.5 + g.dt and g.param("stats_samples") == 2
    # get into a device pointer
    d = DevBuf(np.zeros((nl, N + 1, N + 1)))
    for n in ("PSI", "KE", "EKE"):
        assert L.msomn_stats_get(h, ST[n], d.ptr) == 0
        assert np.array_equal(d.host(), g.stats_get(ST[n])), n
    d.free()
    # begin again: another mask, the sums restart
    g.stats_begin(bits("Q"))
    assert g.stats_weight() == 0.0 and g.param("stats_samples") == 0 and g.param("stats_bytes") == per
    q = g.get("Q")
    g.stats_accumulate(2.0)
    assert np.array_equal(g.stats_get(ST["Q"]), (2.0 * q) / 2.0)
    # msomn_set_const drops everything
    g.set_const()
    assert g.param("stats_mask") == 0 and g.param("stats_bytes") == 0 and g.param("stats_samples") == 0
    assert L.msomn_stats_accumulate(h, 1.0) == MSOM_ERR_STATE
    assert L.msomn_stats_get(h, ST["Q"], out.ctypes.data) == MSOM_ERR_STATE
    assert L.msomn_step(h, 0) == MSOM_ERR_STATE          # "stats" is still 1 and there is nothing to sample into
    g.set_option("stats", 0)
    g.step(True)
    g.close()
