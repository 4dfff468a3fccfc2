"""The vertex (masked-domain) model on tiles, on ONE GPU: px x py tiles run as host threads of one process over the library's
in-process transport.  Gate of SURVEY 8(e): the tiled result equals the single-tile result of the same global grid bit for bit --
a tile holds the vertices on its interior edges, every holder computes them, and the assembly checks that all holders agree.
The inputs are not symmetric about any seam: noise on psi, an island across a vertical seam, land over the cross point, a bay in
the land along the north wall, topography, psi_pg and the time-dependent wind."""
import functools
import os
import threading
import time

import numpy as np
import pytest

import orn
from msom_amd import NodeQG
from msom_amd.api import MsomError
from msom_amd.tiling import node_assemble, node_tile_window

pytestmark = pytest.mark.gpu

DH = {1: [1.0], 2: [0.3, 0.7], 3: [0.1, 0.3, 0.6], 6: [0.05, 0.08, 0.12, 0.2, 0.25, 0.3]}
N2 = {1: [1.0], 2: [4000.], 3: [9000., 3000.], 6: [9500., 7500., 5500., 3500., 2000.]}
# the passes a tiled handle resolves to off, and what decides the layouts and the gather level: the single tile runs with the values
# the tiled handle reports
OPTION_KEYS = ["node_pfused", "node_tile_s", "node_march_s", "node_march", "tiled_relax", "node_corr_fused", "node_rhs_fused", "node_split", "mg_coarse"]
NRP_COLOR, NRP_SPLIT = 0, 1


def params(N, nl, bc_fac=1.0, tol=1e-5):
    fmt = lambda v: "[" + ",".join(repr(x) for x in v) + "]"
    return (f"N = {N}\nnl = {nl}\nL0 = 100\nf0 = 46.5\nhEkb = 0.01\ntau0 = 1e-3\ntau1 = 5e-4\ntf1 = 0.3\ntf2 = 0.7\nnu = 5.0\nnu4 = 1.0\nbeta = 0.5\n"
            f"bc_fac = {bc_fac}\nflag_ms = 1\ndh = {fmt(DH[nl])}\nN2 = {fmt(N2[nl])}\nDT = 5.e-2\ntend = 100.\ndtout = 1\nCFL = 0.2\nTOLERANCE = {tol}\n"
            + ("gp_low = 0.02\n" if nl == 1 else ""))


def inputs(N, nl):
    rng = np.random.default_rng(1000 * N + nl)
    h, x = N // 2, np.arange(N + 1) / N
    mk = np.ones((1, N + 1, N + 1))
    mk[0, N // 8: N // 8 + 5, h - 3: h + 4] = 0          # island across the vertical seam of 2 tiles a side
    mk[0, h - 2: h + 2, h - 2: h + 3] = 0                # land over the cross point
    mk[0, N - 5:, N // 3: 2 * N // 3] = 0                # land along the north wall ...
    mk[0, N - 5: N - 1, h - 1: h + 3] = 1                # ... with a bay cut into it
    mk[0, 3 * N // 4 - 1: 3 * N // 4 + 2, N // 4 - 2: N // 4 + 1] = 0   # and a rock on the seams of 4 tiles a side
    mk[0, 0, :] = mk[0, -1, :] = mk[0, :, 0] = mk[0, :, -1] = 0
    psi = (orn.node_psi(nl, N) + 1e-3 * rng.standard_normal((nl, N + 1, N + 1))) * mk
    topo = 0.05 * np.outer(np.cos(2.3 * np.pi * x + 0.4), np.sin(1.7 * np.pi * x + 0.2))[None]
    out = dict(MASK=mk, PSI=psi)
    if nl > 1:
        out["TOPO"] = topo
        out["PSIPG"] = 0.3 * orn.node_psi(nl, N)[::-1].copy() * (1 + 0.2 * x)[None, None, :]
    return out


def run_tiled(par, px, py, inp, strict, body, opts=None):
    """body(g, rank) on every tile, each a daemon thread with its own handle; the tile arrays are the windows of the global inputs"""
    n = px * py
    assert n <= 8
    uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
    N = inp["MASK"].shape[-1] - 1
    out, errs = [None] * n, []

    def worker(rank):
        try:
            g = NodeQG(par, strict=strict, tiled=(px, py, rank, uid))
            g.set_option("quiet", 1)
            for k, v in (opts or {}).items():
                g.set_option(k, v)
            sy, sx = node_tile_window(N, px, py, rank)
            assert g.tile == (px, py, rank % px, rank // px) and (g.nx, g.ny) == (N // px + 1, N // py + 1)
            for f, a in inp.items():
                g.set(f, a[:, sy, sx])
            g.set_const()
            g.set_tnext(float("inf"))
            out[rank] = body(g, rank)
            g.close()
        except Exception as e:  # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(n)]
    for t in th:
        t.start()
    deadline = time.monotonic() + 120
    for t in th:
        t.join(timeout=max(0.0, deadline - time.monotonic()))
    assert not errs, errs
    assert all(o is not None for o in out), "a tile thread hung"
    return out


def single(par, inp, strict, opts):
    g = NodeQG(par, strict=strict)
    g.set_option("quiet", 1)
    for k, v in opts.items():
        g.set_option(k, v)
    for f, a in inp.items():
        g.set(f, a)
    g.set_const()
    g.set_tnext(float("inf"))
    return g


def steps_body(nsteps):
    def body(g, rank):
        dts = []
        for _ in range(nsteps):
            g.step(True)
            dts.append(g.dt)
        s = g.mgstats()
        res = dict(dts=dts, t=g.t, iter=g.iter, st=(s.i, s.resa, s.resb), ke=g.ke(), diag=g.diag1d(), q=g.get("Q"), psi=g.get("PSI"),
                   opts={k: g.param(k) for k in OPTION_KEYS}, agg=g.param("agg_level"), path0=g.param("relax_path_0"), exchanges=g.param("exchanges"))
        g.rhs_pv()
        res["zeta"] = g.get("ZETA")
        return res
    return body


def check_against_single(out, ref, N, px, py):
    for r, o in enumerate(out):
        assert o["dts"] == ref["dts"], r
        assert (o["t"], o["iter"], o["st"]) == (ref["t"], ref["iter"], ref["st"]), r
        print("rank", r, "ke", o["ke"], ref["ke"], "diag1d", o["diag"], ref["diag"])
        assert o["ke"] == pytest.approx(ref["ke"], rel=1e-13)         # the sum order differs
        assert o["diag"] == pytest.approx(ref["diag"], rel=1e-13)
    for f in ("q", "psi", "zeta"):
        a = node_assemble([o[f] for o in out], N, px, py, check_shared=True)
        assert np.array_equal(a, ref[f]), f"{f}: {np.count_nonzero(a != ref[f])} vertices differ"


CASES = [(2, 1, 64, 3, 1.0), (1, 2, 64, 3, 1.0), (2, 2, 64, 1, 1.0), (2, 2, 64, 3, 0.0), (2, 2, 64, 3, 0.5), (2, 2, 64, 3, 1.0), (4, 2, 64, 2, 1.0),
         (2, 4, 64, 6, 1.0)]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py,N,nl,bc_fac", CASES)
def test_node_tiled_equals_single_tile_bit_for_bit(px, py, N, nl, bc_fac, strict):
    par, inp = params(N, nl, bc_fac), inputs(N, nl)
    out = run_tiled(par, px, py, inp, strict, steps_body(5), opts=dict(mg_coarse=8))
    assert out[0]["agg"] == 3 and out[0]["exchanges"] > 0      # n = 64, 32, 16 on the tiles, 8 and below gathered
    assert all(out[0]["opts"][k] == 0 for k in OPTION_KEYS[:7]) and out[0]["opts"]["mg_coarse"] == 8
    ref = steps_body(5)(single(par, inp, strict, out[0]["opts"]), 0)
    check_against_single(out, ref, N, px, py)


def test_node_tiled_equals_the_oracle_bit_for_bit():
    px, py, N, nl = 2, 2, 64, 3
    par, inp = params(N, nl, 0.5), inputs(N, nl)

    def body(g, rank):
        for _ in range(3):
            g.step(True)
        return dict(q=g.get("Q"), psi=g.get("PSI"))
    out = run_tiled(par, px, py, inp, True, body, opts=dict(mg_coarse=8))
    o = orn.NodeOracle(par, smoother=orn.GS_RB, quiet=1)
    for f, a in inp.items():
        o.set(getattr(orn, f), a)
    o.set_const()
    o.set_tnext(float("inf"))
    for _ in range(3):
        o.step(True)
    assert np.array_equal(node_assemble([t["q"] for t in out], N, px, py), o.get(orn.Q))
    assert np.array_equal(node_assemble([t["psi"] for t in out], N, px, py), o.get(orn.PSI))


@pytest.mark.parametrize("strict", [True, False])
def test_default_options_with_the_split_layout_live(strict):
    px, py, N, nl = 2, 2, 256, 3
    par, inp = params(N, nl, 1.0, tol=1e-9), inputs(N, nl)
    out = run_tiled(par, px, py, inp, strict, steps_body(3))
    assert out[0]["path0"] == NRP_SPLIT and out[0]["agg"] == 3     # 256, 128, 64 on the tiles; n = 32 is level 3
    ref = steps_body(3)(single(par, inp, strict, out[0]["opts"]), 0)
    assert ref["st"][0] >= 3, ref["st"]                            # a solve takes several cycles: every exchange of the cycle matters
    check_against_single(out, ref, N, px, py)


@pytest.mark.parametrize("split", [0, 9])
@pytest.mark.parametrize("px,py,N,nl", [(2, 2, 64, 3), (4, 2, 64, 2)])
def test_multigrid_pieces_equal_the_single_tiles_windows(px, py, N, nl, split):
    par, inp = params(N, nl), inputs(N, nl)
    opts = dict(mg_coarse=8, node_split=split)
    rng = np.random.default_rng(5)
    kg = 3
    rnd = {k: rng.standard_normal((2, nl, (N >> k) + 1, (N >> k) + 1)) for k in range(kg)}
    win = lambda a, k, r: a[(Ellipsis,) + node_tile_window(N >> k, px, py, r)]

    def body(g, rank):
        res = dict(split0=g.param("split_0"), agg=g.param("agg_level"))
        for k in range(kg):
            da, rs = win(rnd[k][0], k, rank), win(rnd[k][1], k, rank)
            res["mask", k] = g.dbg_level_mask(k)
            for ns in (1, 2, 5):
                res["relax", k, ns] = g.dbg_relax(k, da, rs, ns)
            if k + 1 < kg:
                res["restrict", k] = g.dbg_restrict(k, rs)
            if k >= 1:
                res["prolong", k] = g.dbg_prolong(k, da)
        res["residual"] = g.dbg_residual(win(rnd[0][0], 0, rank), win(rnd[0][1], 0, rank))
        with pytest.raises(MsomError):
            g.dbg_level_mask(kg)                                   # a gathered level has no tile-sized array
        return res
    out = run_tiled(par, px, py, inp, True, body, opts=opts)
    assert out[0]["split0"] == (1 if split else 0) and out[0]["agg"] == kg
    g = single(par, inp, True, dict(opts, node_pfused=0, node_tile_s=0, node_march_s=0, node_corr_fused=0, node_rhs_fused=0))
    for k in range(kg):
        want = {("mask", k): g.dbg_level_mask(k)}
        for ns in (1, 2, 5):
            want["relax", k, ns] = g.dbg_relax(k, rnd[k][0], rnd[k][1], ns)
        if k + 1 < kg:
            want["restrict", k] = g.dbg_restrict(k, rnd[k][1])
        if k >= 1:
            want["prolong", k] = g.dbg_prolong(k, rnd[k][0])
        for key, w in want.items():
            lev = k + 1 if key[0] == "restrict" else k - 1 if key[0] == "prolong" else k
            got = node_assemble([o[key] for o in out], N >> lev, px, py, check_shared=True)
            assert np.array_equal(got, w), (key, np.count_nonzero(got != w))
    wres, wmax = g.dbg_residual(rnd[0][0], rnd[0][1])
    assert all(o["residual"][1] == wmax for o in out)
    assert np.array_equal(node_assemble([o["residual"][0] for o in out], N, px, py, check_shared=True), wres)


def test_calls_one_by_one_equal_the_single_tile():
    px, py, N, nl = 2, 2, 64, 3
    par, inp = params(N, nl), inputs(N, nl)
    st = lambda s: (s.i, s.resa, s.resb)

    def body(g, rank):
        res = {}
        g.comp_q()
        res["q0"] = g.get("Q")
        g.set("PSI", np.zeros(g.shape("PSI")))
        res["st_inv"] = st(g.invert_q())
        res["psi1"] = g.get("PSI")
        res["dt"] = g.update()
        res["st_upd"] = st(g.mgstats())
        res["dq"] = g.get("DQ")
        g.advance("QPRED", "Q", "DQ", 0.5 * res["dt"])
        res["qpred"] = g.get("QPRED")
        return res
    out = run_tiled(par, px, py, inp, True, body, opts=dict(mg_coarse=8))
    ref = body(single(par, inp, True, dict(mg_coarse=8, node_pfused=0, node_tile_s=0, node_march_s=0, node_corr_fused=0, node_rhs_fused=0)), 0)
    for o in out:
        assert (o["st_inv"], o["dt"], o["st_upd"]) == (ref["st_inv"], ref["dt"], ref["st_upd"])
    for f in ("q0", "psi1", "dq", "qpred"):
        assert np.array_equal(node_assemble([o[f] for o in out], N, px, py, check_shared=True), ref[f]), f


def exits_body(g, rank):
    """One q, inverted from psi = 0 four times, so that the solve's loop leaves by each of its ways: the iteration count, NITERMIN
    holding it open, convergence, and converged before the first cycle.  Per solve: mgstats, psi, halo exchanges posted."""
    q = g.get("Q")
    res = dict(opts={k: g.param(k) for k in OPTION_KEYS}, agg=g.param("agg_level"))

    def solve(tag, zero_psi=True, **opts):
        for k, v in dict(dict(NITERMAX=100, NITERMIN=1), **opts).items():
            g.set_option(k, v)
        if zero_psi:
            g.set("PSI", np.zeros(g.shape("PSI")))
        g.set("Q", q)
        before = g.param("exchanges")
        s = g.invert_q()
        res[tag] = dict(st=(s.i, s.resb, s.resa), psi=g.get("PSI"), exchanges=g.param("exchanges") - before)
    solve("itermax", NITERMAX=2, TOLERANCE=1e-30)
    solve("itermin", NITERMIN=3, TOLERANCE=1e-1)
    solve("converged", TOLERANCE=1e-9)
    solve("again", zero_psi=False, NITERMIN=0, TOLERANCE=1e-9)   # NITERMIN = 0: the loop may leave before its first cycle
    return res


@functools.lru_cache(maxsize=None)
def solve_exits(px, py, strict):
    N, nl = 64, 2
    par, inp = params(N, nl), inputs(N, nl)
    out = run_tiled(par, px, py, inp, strict, exits_body, opts=dict(mg_coarse=8))
    assert out[0]["agg"] == 3
    ref = exits_body(single(par, inp, strict, out[0]["opts"]), 0)
    for tag in ("itermax", "itermin", "converged", "again"):
        print(px, py, strict, tag, "tiles", out[0][tag]["st"], out[0][tag]["exchanges"], "one tile", ref[tag]["st"])
    return out, ref


def assembled_psi(out, tag, px, py):
    return node_assemble([o[tag]["psi"] for o in out], 64, px, py, check_shared=True)


EXIT_CASES = [(2, 2), (2, 1)]


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", EXIT_CASES)
def test_solve_ended_by_the_iteration_count(px, py, strict):
    out, ref = solve_exits(px, py, strict)
    assert ref["itermax"]["st"][0] == 2 and ref["itermax"]["st"][2] > 1e-30
    assert all(o["itermax"]["st"] == ref["itermax"]["st"] for o in out)
    # the correction of the last cycle is applied after the loop
    assert np.array_equal(assembled_psi(out, "itermax", px, py), ref["itermax"]["psi"])
    assert np.any(ref["itermax"]["psi"] != 0)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", EXIT_CASES)
def test_solve_that_starts_converged_runs_no_cycle(px, py, strict):
    out, ref = solve_exits(px, py, strict)
    for r in [ref] + out:
        assert r["converged"]["st"][0] >= 1 and r["converged"]["st"][2] < 1e-9
        assert r["again"]["st"][0] == 0
        assert np.array_equal(r["again"]["psi"], r["converged"]["psi"])
    assert all(o["again"]["st"] == ref["again"]["st"] for o in out)
    assert np.array_equal(assembled_psi(out, "converged", px, py), ref["converged"]["psi"])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", EXIT_CASES)
def test_nitermin_holds_the_solve_open(px, py, strict):
    out, ref = solve_exits(px, py, strict)
    assert ref["itermin"]["st"][0] == 3
    assert all(o["itermin"]["st"] == ref["itermin"]["st"] for o in out)
    assert np.array_equal(assembled_psi(out, "itermin", px, py), ref["itermin"]["psi"])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", EXIT_CASES)
def test_exchanges_of_a_solve(px, py, strict):
    """Per cycle one exchange of psi for the residual pass, kg of the residual going down and, per tiled level going up, one after the
    prolongation and one per colour of the nrelax = 5 sweeps: 1 + 12 kg.  A solve that ends by convergence has posted the exchange of
    its last residual pass and nothing of the cycle it does not run; one that ends by NITERMAX has not computed another residual."""
    out, ref = solve_exits(px, py, strict)
    per_cycle = 1 + 12 * int(out[0]["agg"])
    for o in out:
        assert o["itermax"]["exchanges"] == o["itermax"]["st"][0] * per_cycle
        for tag in ("itermin", "converged", "again"):
            assert o[tag]["exchanges"] == o[tag]["st"][0] * per_cycle + 1, tag
    assert all(ref[tag]["exchanges"] == 0 for tag in ("itermax", "itermin", "converged", "again"))


ERR_CONFIG = -3


def test_refusals_leave_the_handle_unchanged(tmp_path):
    N, nl = 64, 3
    par, inp = params(N, nl), inputs(N, nl)

    def body(g, rank):
        q, psi = g.get("Q"), g.get("PSI")
        cells = np.zeros((N, N))
        calls = {
            "option stochastic": lambda: g.set_option("stochastic", 1),
            "msomn_noise_draw": lambda: g.noise_draw(),
            "msomn_dbg_noise": lambda: g.noise(),
            "msomn_dbg_csig": lambda: g.csig(0),
            "msomn_wavelet_filter": lambda: g.wavelet_filter(0.1),
            "msomn_dbg_wv_get": lambda: g.wv_get(0, 0),
            "msomn_dbg_wv_apply": lambda: g.wv_apply(np.zeros((nl, N, N))),
            "msomn_run": lambda: g.run(str(tmp_path)),
            "msomn_write_nc": lambda: g.write_nc(str(tmp_path / f"x{rank}.nc")),
            "msomn_read_nc": lambda: g.read_nc("PSI", str(tmp_path / "none.nc"), "psi"),
            "msomn_state_save": lambda: g.save_state(str(tmp_path / f"s{rank}.bin")),
            "msomn_state_load": lambda: g.load_state(str(tmp_path / "none.bin")),
            "msomn_dbg_del2_zeta": lambda: g.dbg_del2_zeta(),
        }
        seen = {}
        for name, call in calls.items():
            try:
                call()
                seen[name] = "no error"
            except MsomError as e:
                seen[name] = (getattr(e, "code", None), str(e))
        return dict(seen=seen, same=np.array_equal(q, g.get("Q")) and np.array_equal(psi, g.get("PSI")), files=sorted(os.listdir(tmp_path)))
    out = run_tiled(par, 2, 1, inp, True, body)
    for o in out:
        for name, got in o["seen"].items():
            assert got != "no error", name
            assert got[0] == ERR_CONFIG and name in got[1], (name, got)
        assert o["same"] and o["files"] == []


def test_create_errors_and_the_plain_handle():
    par = params(64, 3)
    uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
    for px, py, rank, word in [(3, 1, 0, "power"), (64, 1, 0, "2 cells"), (2, 2, 4, "rank")]:
        with pytest.raises(MsomError, match=word):
            NodeQG(par, strict=True, tiled=(px, py, rank, uid))
    with pytest.raises(MsomError, match="bc_fac"):
        NodeQG(params(64, 3, bc_fac=-1), strict=True, tiled=(2, 1, 0, uid))
    inp = inputs(64, 3)
    g1 = NodeQG(par, strict=True, tiled=(1, 1, 0, None))
    g2 = NodeQG(par, strict=True)
    assert g1.tile == (1, 1, 0, 0) and (g1.nx, g1.ny) == (65, 65) == (g2.nx, g2.ny) and g1.param("agg_level") == g1.param("nlevels")
    res = []
    for g in (g1, g2):
        g.set_option("quiet", 1)
        for f, v in inp.items():
            g.set(f, v)
        g.set_const()
        g.set_tnext(float("inf"))
        res.append(steps_body(2)(g, 0))
    for k in ("dts", "t", "st", "ke"):
        assert res[0][k] == res[1][k]
    for f in ("q", "psi", "zeta"):
        assert np.array_equal(res[0][f], res[1][f])
