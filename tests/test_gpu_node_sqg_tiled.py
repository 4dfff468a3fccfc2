"""The surface-QG variant of the vertex model (params key sqg) on tiles: px x py tiles as host threads of one process equal the single tile
of the same global grid bit for bit, in both builds, with the holders of a shared vertex agreeing.  What the tiles change for sqg: the
surface stratification S2S = f / N^2 takes f at the GLOBAL row, and laplacian(bs) (k_n_lap_bs) copies the first interior value onto a
boundary vertex at walls of the domain only -- on a rectangular tile, with a vertex on an interior edge taking the laplacian from the
halo of bs.  bs carries seeded noise and the mask is that of test_gpu_node_tiled.inputs, so nothing is symmetric about a seam; the
rectangular tilings catch a square assumption.  Without the feature msomn_create_tiled refuses sqg = 1 on more than one tile."""
import numpy as np
import pytest

import orn
from msom_amd.tiling import node_assemble
from test_gpu_node_tiled import OPTION_KEYS, inputs, run_tiled, single
from test_oracle_sqg_kat import bs_field, sqg_params

pytestmark = pytest.mark.gpu

TILINGS = [(2, 1), (1, 2), (2, 2), (4, 2)]
EXTRA = "tau1 = 5e-4\ntf1 = 0.3\ntf2 = 0.7\nflag_ms = 1\n"   # flag_ms: f, and with it S2S = f / N^2, depends on the row


def sqg_inputs(N, nl, bs=None):
    inp = inputs(N, nl)   # mask with islands on the seams, noisy psi, topography, psi_pg
    rng = np.random.default_rng(77 + N)
    inp = dict(MASK=inp["MASK"], BS=bs_field(N) + 0.02 * rng.standard_normal((1, N + 1, N + 1)) if bs is None else bs,
               **{k: v for k, v in inp.items() if k != "MASK"})
    return inp


def body(g, rank):
    st = lambda s: (s.i, s.resb, s.resa)
    res = dict(opts={k: g.param(k) for k in OPTION_KEYS}, sqg=g.param("sqg"), S2S=g.get("S2S"), S2=g.get("S2"))
    g.comp_q()
    res["q0"] = g.get("Q")
    g.rhs_pv()                                   # laplacian(bs) in both dissipation operators
    res["dq"] = g.get("DQ")
    g.set("PSI", np.zeros(g.shape("PSI")))
    res["st_inv"] = st(g.invert_q())             # the surface term on the right-hand side
    res["psi1"] = g.get("PSI")
    g.set_tnext(0.11)
    res["dts"] = []
    for _ in range(4):
        g.step(True)
        res["dts"].append((g.dt, g.t, st(g.mgstats())))
    res["psi"], res["q"] = g.get("PSI"), g.get("Q")
    return res


FIELDS = ("S2S", "S2", "q0", "dq", "psi1", "psi", "q")


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", TILINGS)
@pytest.mark.parametrize("N", [32, 64])
def test_sqg_on_tiles_equals_the_single_tile_bit_for_bit(N, px, py, strict):
    nl = 3
    par, inp = sqg_params(N, nl, bc_fac=1.0, nu4=1.5, extra=EXTRA), sqg_inputs(N, nl)
    opts = dict(mg_coarse=8, TOLERANCE=1e-9)
    out = run_tiled(par, px, py, inp, strict, body, opts=opts)
    assert all(o["sqg"] == 1 for o in out)
    ref = body(single(par, inp, strict, dict(opts, **out[0]["opts"])), 0)
    for o in out:
        assert (o["st_inv"], o["dts"]) == (ref["st_inv"], ref["dts"])
    for f in FIELDS:
        a = node_assemble([o[f] for o in out], N, px, py, check_shared=True)
        assert np.array_equal(a, ref[f]), f"{f}: {np.count_nonzero(a != ref[f])} vertices differ"
    assert np.ptp(ref["S2S"][0, :, 0]) > 0       # f depends on the row: a tile that took its local row would differ


def test_sqg_on_tiles_equals_the_oracle_bit_for_bit():
    px, py, N, nl = 2, 2, 32, 3
    par, inp = sqg_params(N, nl, bc_fac=0.5, nu4=1.5, extra=EXTRA), sqg_inputs(N, nl)
    out = run_tiled(par, px, py, inp, True, body, opts=dict(mg_coarse=8, TOLERANCE=1e-9))
    o = orn.NodeOracle(par, smoother=orn.GS_RB, quiet=1, TOLERANCE=1e-9)
    for f, a in inp.items():
        o.set(getattr(orn, f), a)
    o.set_const()
    want = {"S2S": o.get(orn.S2S)}
    o.comp_q()
    want["q0"] = o.get(orn.Q)
    o.rhs_pv()
    want["dq"] = o.get(orn.DQ)
    o.set(orn.PSI, np.zeros((nl, N + 1, N + 1)))
    o.invert_q()
    want["psi1"] = o.get(orn.PSI)
    o.set_tnext(0.11)
    for _ in range(4):
        o.step(True)
    want["psi"], want["q"] = o.get(orn.PSI), o.get(orn.Q)
    for f, w in want.items():
        a = node_assemble([t[f] for t in out], N, px, py, check_shared=True)
        assert np.array_equal(a, w), f"{f}: {np.count_nonzero(a != w)} vertices differ"


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 2), (4, 2)])
def test_the_neumann_copy_of_lap_bs_happens_on_walls_not_on_seams(px, py, strict):
    """bs with a gradient normal to every wall and a laplacian that changes from vertex to vertex: a copy of the first interior value
    onto a seam vertex changes laplacian(bs) there, and with it dq = ... + nu S2S d2bs - nu4 S2S d2bs (a wall vertex itself is
    masked in dq; its neighbours read only their own d2bs)."""
    N, nl = 32, 3
    x = np.arange(N + 1) / N
    bs = (np.add.outer(2.0 * x ** 3, x ** 2) + 0.3 * np.outer(x ** 2, x ** 3))[None]
    par, inp = sqg_params(N, nl, bc_fac=1.0, nu4=1.5, extra=EXTRA), sqg_inputs(N, nl, bs=bs)
    inp["MASK"] = np.ones_like(inp["MASK"])      # no land: dq is not masked away along the seams
    inp["PSI"] = 0.0 * inp["PSI"]                # and nothing but the surface term and the forcing moves it

    def lap_body(g, rank):
        res = dict(opts={k: g.param(k) for k in OPTION_KEYS})
        g.rhs_pv()
        res["dq"] = g.get("DQ")
        return res
    out = run_tiled(par, px, py, inp, strict, lap_body, opts=dict(mg_coarse=8))
    ref = lap_body(single(par, inp, strict, out[0]["opts"]), 0)
    a = node_assemble([o["dq"] for o in out], N, px, py, check_shared=True)
    assert np.array_equal(a, ref["dq"]), f"{np.count_nonzero(a != ref['dq'])} vertices differ"
    # the surface term reaches the top layer of dq along the seams and next to the walls
    tx, ty = N // px, N // py
    assert np.all(ref["dq"][0, 2:-2, tx] != 0) and np.all(ref["dq"][0, ty, 2:-2] != 0) and np.all(ref["dq"][0, 1, 2:-2] != 0)
