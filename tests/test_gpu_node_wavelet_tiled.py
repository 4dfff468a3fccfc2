"""The wavelet pyramid of the vertex model on tiles (option wavelet_tiles, msom_amd/csrc/msomn_cells.hip): the scale filter and the
stochastic forcing.  px x py tiles run as host threads over the in-process transport (test_gpu_node_tiled.run_tiled) with the island
across the seam and the land over the cross point; every number is held to the single tile of the same global grid with
np.array_equal, in the strict and in the product build: the tiles run the single tile's device functions on the single tile's
operands.  Cell fields are cut and put together with msom_amd.tiling.cell_tile_window / cell_assemble."""
import numpy as np
import pytest

import orn
from msom_amd.api import MsomError
from msom_amd.tiling import cell_assemble, cell_tile_window, node_assemble
from test_gpu_node_tiled import OPTION_KEYS, inputs, params, run_tiled, single

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_CONFIG = -1, -3
AMP, SEED = 0.3, 5
# (px, py, N, nl, mg_coarse); the last: tiles of 4 cells whose coarsest tiled level has 2 cells a side
CASES = [(2, 1, 64, 3, 8), (1, 2, 64, 3, 8), (2, 2, 64, 1, 8), (4, 2, 64, 2, 8), (2, 4, 64, 3, 8), (8, 1, 32, 2, 4)]
KG = {64: 3, 32: 2}   # N = 64, mg_coarse 8: 64, 32, 16 on the tiles; N = 32 on 8 tiles a side: 32, 16 (4 and 2 cells a tile side)


def filt(Lfmax, Lfmin, fac=0.0):
    return f"Lfmax = {Lfmax}\nLfmin = {Lfmin}\nfac_filt_Rd = {fac}\n"


GRADIENT = filt(25.0, 6.0)


def levels(N):
    return N.bit_length()   # N >> k >= 1: down to the 1-cell root


def tile_opts(g):
    return {k: g.param(k) for k in OPTION_KEYS}


def check_levels(out, get_ref, key, N, px, py, kg):
    """level k of a coefficient pyramid: the tile's window below the gather level, the whole level from it on"""
    for k in range(levels(N)):
        want = get_ref(k)
        if k < kg:
            got = cell_assemble([o[key + (k,)] for o in out], N, px, py, k)
            assert np.array_equal(got, want), (key, k)
        else:
            for r, o in enumerate(out):
                assert o[key + (k,)].shape == want.shape and np.array_equal(o[key + (k,)], want), (key, k, r)


# ---- 1. the transform alone
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py,N,nl,mgc,ftxt", [pytest.param(*c, GRADIENT, id="%dx%d-N%d-nl%d-mgc%d-gradient" % c) for c in CASES]
                         + [pytest.param(4, 2, 64, 2, 8, filt(30.0, 30.0, 40.0), id="4x2-N64-nl2-mgc8-fac_filt_Rd")])
def test_transform_and_coefficients_equal_the_single_tile(px, py, N, nl, mgc, ftxt, strict):
    par, inp = params(N, nl) + ftxt, inputs(N, nl)
    cells = np.random.default_rng(7).standard_normal((nl, N, N))

    def body(g, rank):
        sy, sx = cell_tile_window(N, px, py, rank)
        res = {"agg": g.param("agg_level"), "opts": tile_opts(g), "apply": g.wv_apply(cells[:, sy, sx])}
        for what in (0, 1):
            for k in range(levels(N)):
                res["get", what, k] = g.wv_get(what, k)
        return res
    out = run_tiled(par, px, py, inp, strict, body, opts=dict(mg_coarse=mgc, wavelet_tiles=1))
    kg = KG[N]
    assert all(o["agg"] == kg for o in out)
    g = single(par, inp, strict, out[0]["opts"])
    want = g.wv_apply(cells)
    assert np.any(want != cells) and np.any(want != 0)
    assert np.array_equal(cell_assemble([o["apply"] for o in out], N, px, py), want)
    for what in (0, 1):
        check_levels(out, lambda k: g.wv_get(what, k), ("get", what), N, px, py, kg)
    sig = [g.wv_get(0, k) for k in range(levels(N))]
    assert any(0 < s.min() < 1 or s.min() != s.max() for s in sig)   # the coefficients vary in space or across levels


# ---- 2. the filter event
def filter_body(g, rank):
    g.wavelet_filter(0.5)
    g.wavelet_filter(0.5)
    dts = []
    for _ in range(2):
        g.step(True)
        dts.append(g.dt)
    s = g.mgstats()
    return dict(psi=g.get("PSI"), psif=g.get("PSIF"), q=g.get("Q"), dts=dts, t=g.t, st=(s.i, s.resa, s.resb), opts=tile_opts(g), agg=g.param("agg_level"))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py,N,nl,mgc", [CASES[0], CASES[1], CASES[3], CASES[4], CASES[5]])
def test_filter_event_and_steps_equal_the_single_tile(px, py, N, nl, mgc, strict):
    par, inp = params(N, nl) + GRADIENT, inputs(N, nl)
    out = run_tiled(par, px, py, inp, strict, filter_body, opts=dict(mg_coarse=mgc, wavelet_tiles=1))
    assert all(o["agg"] == KG[N] for o in out)
    ref = filter_body(single(par, inp, strict, out[0]["opts"]), 0)
    for r, o in enumerate(out):
        assert (o["dts"], o["t"], o["st"]) == (ref["dts"], ref["t"], ref["st"]), r
    assert np.any(ref["psif"] != 0)
    for f in ("psi", "psif", "q"):
        a = node_assemble([o[f] for o in out], N, px, py, check_shared=True)
        assert np.array_equal(a, ref[f]), f"{f}: {np.count_nonzero(a != ref[f])} vertices differ"


def test_filter_event_on_tiles_equals_the_oracle_bit_for_bit():
    px, py, N, nl = 2, 2, 64, 3
    par, inp = params(N, nl, 0.5) + GRADIENT, inputs(N, nl)
    out = run_tiled(par, px, py, inp, True, filter_body, opts=dict(mg_coarse=8, wavelet_tiles=1))
    o = orn.NodeOracle(par, smoother=orn.GS_RB, quiet=1)
    for f, a in inp.items():
        o.set(getattr(orn, f), a)
    o.set_const()
    o.set_tnext(float("inf"))
    o.wavelet_filter(0.5)
    o.wavelet_filter(0.5)
    for _ in range(2):
        o.step(True)
    for f, of in (("psi", orn.PSI), ("psif", orn.PSIF), ("q", orn.Q)):
        assert np.array_equal(node_assemble([t[f] for t in out], N, px, py), o.get(of)), f


# ---- 3. noise
def noise_params(N, L_filt):
    return params(N, 1) + f"amp_stoch = {AMP}\nL_filt = {L_filt}\n"


NOISE_OPTS = dict(wavelet_tiles=1, stochastic=1, seed=SEED, noise_mode=1)


def noise_body(N):
    def body(g, rank):
        res = {"agg": g.param("agg_level"), "opts": tile_opts(g), "count": []}
        for filtered in (False, True):
            g.set_const()                                   # rewinds the draw counter
            for draw in range(3):
                res["count"].append(g.param("noise_draw"))
                g.noise_draw(filter=filtered)
                res["noise", filtered, draw] = g.noise()
        res["count"].append(g.param("noise_draw"))
        for k in range(levels(N)):
            res["csig", k] = g.csig(k)
        return res
    return body


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("L_filt", [8.0, 1e6])
@pytest.mark.parametrize("px,py,N,mgc", [(2, 2, 64, 8), (4, 2, 64, 8), (1, 2, 64, 8), (8, 1, 32, 4)])
def test_noise_draws_equal_the_single_tile(px, py, N, mgc, L_filt, strict):
    par, inp = noise_params(N, L_filt), inputs(N, 1)
    out = run_tiled(par, px, py, inp, strict, noise_body(N), opts=dict(NOISE_OPTS, mg_coarse=mgc))
    kg = KG[N]
    assert all(o["agg"] == kg for o in out)
    assert all(o["count"] == [0, 1, 2, 0, 1, 2, 3] for o in out)      # the counter moves alike on every rank
    g = single(par, inp, strict, dict(out[0]["opts"], **NOISE_OPTS))
    ref = noise_body(N)(g, 0)
    for filtered in (False, True):
        for draw in range(3):
            a = cell_assemble([o["noise", filtered, draw] for o in out], N, px, py)
            assert np.array_equal(a, ref["noise", filtered, draw]), (filtered, draw, np.count_nonzero(a != ref["noise", filtered, draw]))
    assert np.any(ref["noise", True, 0] != ref["noise", False, 0])
    assert np.abs(ref["noise", False, 1] - ref["noise", False, 0]).max() > AMP
    check_levels(out, lambda k: ref["csig", k], ("csig",), N, px, py, kg)


# ---- 4. stochastic steps
def stoch_body(g, rank):
    dts = []
    for _ in range(4):
        g.step(True)
        dts.append(g.dt)
    return dict(q=g.get("Q"), psi=g.get("PSI"), dts=dts, opts=tile_opts(g), draws=g.param("noise_draw"))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 2), (4, 2)])
def test_stochastic_steps_equal_the_single_tile(px, py, strict):
    N = 64
    par, inp = noise_params(N, 8.0), inputs(N, 1)
    out = run_tiled(par, px, py, inp, strict, stoch_body, opts=dict(NOISE_OPTS, mg_coarse=8))
    ref = stoch_body(single(par, inp, strict, dict(out[0]["opts"], **NOISE_OPTS)), 0)
    assert ref["draws"] == 4 and all(o["draws"] == 4 and o["dts"] == ref["dts"] for o in out)
    quiet = stoch_body(single(par, inp, strict, out[0]["opts"]), 0)
    assert np.any(quiet["q"] != ref["q"])                              # the forcing is felt
    for f in ("q", "psi"):
        a = node_assemble([o[f] for o in out], N, px, py, check_shared=True)
        assert np.array_equal(a, ref[f]), f"{f}: {np.count_nonzero(a != ref[f])} vertices differ"


# ---- 5. exchange count
@pytest.mark.parametrize("px,py,N,mgc", [(2, 2, 64, 8), (8, 1, 32, 4)])
def test_exchanges_of_a_transform(px, py, N, mgc):
    """One transform posts 2 kg - 1 halo exchanges (kg - 1 of s going down, kg of r and of the result going up) and one all-gather.
    wavelet_filter adds those of its solve (msomn_invert_q alone posts the same, NITERMIN = NITERMAX fixes its cycles) and the one
    of comp_q."""
    nl = 2
    par, inp = params(N, nl) + GRADIENT + f"amp_stoch = {AMP}\nL_filt = 8.0\n", inputs(N, nl)

    def body(g, rank):
        sy, sx = cell_tile_window(N, px, py, rank)
        g.set_option("NITERMIN", 2)
        g.set_option("NITERMAX", 2)
        g.wv_get(0, 0)                                       # the lazy setup of the filter pyramid is behind us
        count = lambda: g.param("exchanges")
        e = [count()]
        g.wv_apply(np.ones((nl, N, N))[:, sy, sx]); e.append(count())
        g.noise_draw(filter=True); e.append(count())
        g.noise_draw(filter=False); e.append(count())
        g.invert_q(); e.append(count())
        g.wavelet_filter(0.5); e.append(count())
        return dict(kg=int(g.param("agg_level")), d=[int(b - a) for a, b in zip(e, e[1:])])
    out = run_tiled(par, px, py, inp, True, body, opts=dict(NOISE_OPTS, mg_coarse=mgc))
    for o in out:
        kg = o["kg"]
        apply_, draw, raw, solve, event = o["d"]
        print("kg", kg, "exchanges: wv_apply", apply_, "filtered draw", draw, "unfiltered draw", raw, "invert_q", solve, "wavelet_filter", event)
        assert kg == KG[N]
        assert apply_ == draw == 2 * kg - 1 <= 2 * kg
        assert raw == 0
        assert event == solve + (2 * kg - 1) + 1


# ---- 6. the gate
def test_gate_off_refuses_and_leaves_the_handle_unchanged():
    N, nl = 64, 2
    par, inp = params(N, nl) + GRADIENT, inputs(N, nl)

    def body(g, rank):
        q, psi = g.get("Q"), g.get("PSI")
        assert g.param("wavelet_tiles") == 0
        calls = {
            "option stochastic": lambda: g.set_option("stochastic", 1),
            "msomn_noise_draw": lambda: g.noise_draw(),
            "msomn_dbg_noise": lambda: g.noise(),
            "msomn_dbg_csig": lambda: g.csig(0),
            "msomn_wavelet_filter": lambda: g.wavelet_filter(0.1),
            "msomn_dbg_wv_get": lambda: g.wv_get(0, 0),
            "msomn_dbg_wv_apply": lambda: g.wv_apply(np.zeros((nl, N, N))),
        }
        seen = {}
        for name, call in calls.items():
            try:
                call()
                seen[name] = "no error"
            except MsomError as e:
                seen[name] = (getattr(e, "code", None), str(e))
        try:
            g.set_option("wavelet_tiles", 2)
            seen["two"] = "no error"
        except MsomError as e:
            seen["two"] = (e.code, str(e))
        return dict(seen=seen, same=np.array_equal(q, g.get("Q")) and np.array_equal(psi, g.get("PSI")), gate=g.param("wavelet_tiles"))
    out = run_tiled(par, 2, 1, inp, True, body)
    for o in out:
        two = o["seen"].pop("two")
        assert two != "no error" and two[0] == ERR_ARG and o["gate"] == 0
        for name, got in o["seen"].items():
            assert got != "no error", name
            assert got[0] == ERR_CONFIG and name in got[1], (name, got)
        assert o["same"]


def test_gate_on_still_refuses_the_host_stream_and_the_files(tmp_path):
    N = 64
    par, inp = noise_params(N, 8.0), inputs(N, 1)

    def body(g, rank):
        assert g.param("wavelet_tiles") == 1 and g.param("noise_mode") == 0
        res = {"seen": {}}
        before = g.param("exchanges")
        calls = {
            "noise_mode": lambda: g.noise_draw(),                  # refused before any message is posted
            "msomn_step": lambda: g.step(True),
            "msomn_run": lambda: g.run(str(tmp_path)),
            "msomn_state_save": lambda: g.save_state(str(tmp_path / f"s{rank}.bin")),
        }
        for name, call in calls.items():
            try:
                call()
                res["seen"][name] = "no error"
            except MsomError as e:
                res["seen"][name] = (e.code, str(e))
        res["posted"] = g.param("exchanges") - before
        res["count"] = g.param("noise_draw")
        g.set_option("noise_mode", 1)
        g.noise_draw(filter=True)
        res["noise"] = g.noise()
        return res
    out = run_tiled(par, 2, 2, inp, True, body, opts=dict(wavelet_tiles=1, stochastic=1, seed=SEED, mg_coarse=8))
    for o in out:
        for name, got in o["seen"].items():
            assert got != "no error", name
            assert got[0] == ERR_CONFIG and name in got[1], (name, got)
        assert "rand()" in o["seen"]["noise_mode"][1]
        assert o["posted"] == 0 and o["count"] == 0
    g = single(par, inp, True, dict(NOISE_OPTS, mg_coarse=8))
    g.noise_draw(filter=True)
    assert np.array_equal(cell_assemble([o["noise"] for o in out], N, 2, 2), g.noise())


def test_the_option_changes_nothing_on_one_tile():
    N = 64
    par, inp = noise_params(N, 8.0), inputs(N, 1)
    res = []
    for gate in (0, 1):
        g = single(par, inp, False, dict(NOISE_OPTS, wavelet_tiles=gate))
        assert g.param("wavelet_tiles") == gate
        g.noise_draw(filter=True)
        res.append(g.noise())
        with pytest.raises(MsomError) as e:
            g.set_option("wavelet_tiles", 2)
        assert e.value.code == ERR_ARG
    assert res[0].shape == (N, N) and np.array_equal(res[0], res[1])
