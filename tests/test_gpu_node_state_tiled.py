"""State files of the vertex model on tiles (option io_tiles; include/msomn_state.h): px x py tiles as host threads
of one process over the in-process transport save, load and are created from the state file of the single tile.

A record is the global array and a rank's digest word covers the vertices it OWNS (msom_amd.tiling.node_owned_window), so the file does
not know its tiling: the tiled save equals the single tile's save byte for byte, and a file written on any tiling loads on any other.
Everything compared is compared bit for bit or byte for byte, in both builds: saving, loading and gathering move fp64 bits, and the
tile layer's promise is bit identity, so there is no tolerance to state.  Every test here fails without the option with MSOM_ERR_CONFIG
(sqg: at msomn_create_tiled).
"""
import os
import threading
import time

import numpy as np
import pytest

import orn
from msom_amd import MsomError, NodeQG, api, node_from_state
from msom_amd.state import read_state, write_state
from msom_amd.tiling import cell_assemble, node_assemble, node_tile_window
from test_gpu_node_state import CASES, N_nl, assert_same_run, first_half, second_half, snapshot, steps
from test_gpu_node_state import inputs as case_inputs
from test_gpu_node_tiled import OPTION_KEYS, inputs, params, run_tiled, single
from test_node_state_host import GOLDEN_NODE, NODE_SCALARS, golden_oracle

pytestmark = pytest.mark.gpu

MSOM_ERR_ARG, MSOM_ERR_IO, MSOM_ERR_CONFIG = -1, -2, -3
TILINGS = [(2, 1), (1, 2), (2, 2), (4, 2)]
STATS_MASK = 0b1111111
# the cases of test_gpu_node_state.py that the issue names, and one with the running statistics on
TILED_CASES = dict({k: CASES[k] for k in ("n64x3_island", "stochastic_64x1", "stochastic_midstep", "wavelet_32x3", "sqg_32x3")},
                   stats_32x2=dict(par=orn.node_params(32, 2, bc_fac=1.0), mask=True, topo=True, forcing=True, stats=True))
WITHOUT_CONSTANTS = ("n64x3_island",)


def tile_opts(c, **more):
    """the options of every handle of a tiled run of case c (options are not state)"""
    o = dict(io_tiles=1, mg_coarse=8)
    if c.get("stochastic") or c.get("wavelet"):
        o["wavelet_tiles"] = 1
    o.update(c.get("opts", {}))
    o.update(more)
    return o


def global_inputs(c):
    inp = dict(case_inputs(c))
    if "MASK" not in inp:   # run_tiled reads the grid size from it; ones are what msomn_create leaves
        N, _ = N_nl(c)
        inp = dict(MASK=np.ones((1, N + 1, N + 1)), **inp)
    return inp


def after_set_const(g, c):
    if "tnext" in c:
        g.set_tnext(c["tnext"])
    if c.get("stats"):
        g.stats_begin(STATS_MASK)
        g.set_option("stats", 1)


def bare_tiled(make, px, py, body):
    """body(g, rank) on handles made by make(rank, uid), each a daemon thread: handles that take everything from a file"""
    n = px * py
    uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
    out, errs = [None] * n, []

    def worker(rank):
        try:
            g = make(rank, uid)
            g.set_option("quiet", 1)
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


def fresh_tiled(c, px, py, strict, body, **more):
    """handles with the options of the case and nothing else: what loads a file that holds the constants"""
    def make(rank, uid):
        g = NodeQG(c["par"], strict=strict, tiled=(px, py, rank, uid))
        for k, v in tile_opts(c, **more).items():
            g.set_option(k, v)
        return g
    return bare_tiled(make, px, py, body)


def snap_tile(g, c):
    s = snapshot(g, c)
    if c.get("stats"):
        for name in ("PSI", "Q2", "KE", "UQ", "VQ"):
            s["st_" + name] = g.stats_get(api.STATS[name])
        s["stats_samples"] = g.param("stats_samples")
    return s


def assembled(out, c, px, py):
    """(log, snapshot of global arrays) of a tiled run whose ranks returned (log, snapshot of the tile)"""
    N, _ = N_nl(c)
    logs, snaps = [o[0] for o in out], [o[1] for o in out]
    assert all(l == logs[0] for l in logs)
    glob = {}
    for k in snaps[0]:
        v = [s[k] for s in snaps]
        if np.ndim(v[0]) == 0:
            assert all(x == v[0] for x in v), k
            glob[k] = v[0]
        elif k == "noise":
            glob[k] = cell_assemble(v, N, px, py)
        else:
            glob[k] = node_assemble(v, N, px, py, check_shared=True)
    return logs[0], glob


def whole_run(c, px, py, strict, **more):
    def body(g, rank):
        after_set_const(g, c)
        log = []
        second_half(g, c, log, first_half(g, c, log))
        return log, snap_tile(g, c)
    return assembled(run_tiled(c["par"], px, py, global_inputs(c), strict, body, opts=tile_opts(c, **more)), c, px, py)


def first_half_saved(c, px, py, strict, path, constants, **more):
    """the first half on tiles, saved; per rank (log, carried, the options the handle reports, the arrays the file must hold)"""
    def body(g, rank):
        after_set_const(g, c)
        log = []
        carried = first_half(g, c, log)
        g.save_state(path, constants=constants)
        held = {n: g.get(f) for n, f in (("psi", "PSI"), ("q", "Q"), ("q_forcing", "QFORC"), ("mask", "MASK"))}
        return log, carried, {k: g.param(k) for k in OPTION_KEYS}, held
    return run_tiled(c["par"], px, py, global_inputs(c), strict, body, opts=tile_opts(c, **more))


def continue_body(c, path, first):
    def body(g, rank):
        g.load_state(path)
        log = list(first[min(rank, len(first) - 1)][0])
        second_half(g, c, log, first[0][1])
        return log, snap_tile(g, c)
    return body


# ------------------------------------------------------------------ 1. resume on tiles is exact

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", TILINGS)
@pytest.mark.parametrize("case", list(TILED_CASES))
def test_resume_on_tiles_is_exact(case, px, py, strict, tmp_path):
    c = TILED_CASES[case]
    log_a, snap_a = whole_run(c, px, py, strict)
    p = str(tmp_path / "s.msom")
    constants = case not in WITHOUT_CONSTANTS
    first = first_half_saved(c, px, py, strict, p, constants)
    assert not os.path.exists(p + ".tmp")
    if constants:
        out = fresh_tiled(c, px, py, strict, continue_body(c, p, first))
    else:   # the second handles are set up as the first were, then load
        def body(g, rank):
            after_set_const(g, c)
            return continue_body(c, p, first)(g, rank)
        out = run_tiled(c["par"], px, py, global_inputs(c), strict, body, opts=tile_opts(c))
    assert_same_run(log_a, snap_a, *assembled(out, c, px, py))


# ------------------------------------------------------------------ 2. the file does not know its tiling

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py,case", [(2, 2, "n64x3_island"), (4, 2, "stochastic_64x1"), (2, 1, "sqg_32x3"), (1, 2, "stats_32x2")])
def test_tiled_save_equals_the_single_tiles_byte_for_byte(px, py, case, strict, tmp_path):
    c = TILED_CASES[case]
    N, _ = N_nl(c)
    pt, ps = str(tmp_path / "tiled.msom"), str(tmp_path / "single.msom")
    first = first_half_saved(c, px, py, strict, pt, True)
    # the single tile with the option values the tiled handle reports
    g = single(c["par"], global_inputs(c), strict, dict(c.get("opts", {}), **first[0][2]))
    after_set_const(g, c)
    log = []
    first_half(g, c, log)
    assert log == first[0][0]
    g.save_state(ps, constants=True)
    g.close()
    a, b = read_state(pt), read_state(ps)
    assert list(a["records"]) == list(b["records"])
    for k in a["records"]:     # record by record first, so that a failure names the record
        assert np.array_equal(a["records"][k], b["records"][k], equal_nan=True), k
    assert open(pt, "rb").read() == open(ps, "rb").read()
    # the records are the assembled arrays the handles hold, and the digests are those of the global arrays
    for name in ("psi", "q", "q_forcing", "mask"):
        assert np.array_equal(a["records"][name], node_assemble([o[3][name] for o in first], N, px, py, check_shared=True)), name
    assert api.state_check(pt, strict=strict) == len(a["records"])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", ["n64x3_island", "stochastic_midstep"])
def test_a_file_of_one_tiling_loads_on_another(case, strict, tmp_path):
    c = TILED_CASES[case]
    log_a, snap_a = whole_run(c, 2, 2, strict)
    p22, p11 = str(tmp_path / "s22.msom"), str(tmp_path / "s11.msom")
    first = first_half_saved(c, 2, 2, strict, p22, True)
    opts = dict(c.get("opts", {}), **first[0][2])
    # 2 x 2 -> 4 x 2
    assert_same_run(log_a, snap_a, *assembled(fresh_tiled(c, 4, 2, strict, continue_body(c, p22, first)), c, 4, 2))
    # 2 x 2 -> one tile
    g = NodeQG(c["par"], strict=strict)
    for k, v in dict(opts, quiet=1).items():
        g.set_option(k, v)
    g.load_state(p22)
    log = list(first[0][0])
    second_half(g, c, log, first[0][1])
    assert_same_run(log_a, snap_a, log, snap_tile(g, c))
    g.close()
    # one tile -> 2 x 2
    g = single(c["par"], global_inputs(c), strict, opts)
    after_set_const(g, c)
    log1 = []
    carried = first_half(g, c, log1)
    g.save_state(p11, constants=True)
    g.close()
    assert open(p11, "rb").read() == open(p22, "rb").read()
    assert_same_run(log_a, snap_a, *assembled(fresh_tiled(c, 2, 2, strict, continue_body(c, p11, [(log1, carried)])), c, 2, 2))


# ------------------------------------------------------------------ 3. the golden file

def test_golden_file_continues_to_the_oracle_on_tiles():
    txt, o = golden_oracle()
    for _ in range(6):
        o.step(True)
    N = int(o.get(orn.PSI).shape[-1]) - 1

    def body(g, rank):
        g.load_state(GOLDEN_NODE)
        assert g.iter == 3
        for _ in range(3):
            g.step(True)
        return (g.t, g.dt, g.iter, g.mgstats().i), g.get("PSI"), g.get("Q")

    def make(rank, uid):
        g = NodeQG(txt, strict=True, tiled=(2, 2, rank, uid))
        g.set_option("io_tiles", 1)
        return g
    out = bare_tiled(make, 2, 2, body)
    assert all(t[0] == (o.t, o.dt, 6, o.mgstats().i) for t in out)
    assert np.array_equal(node_assemble([t[1] for t in out], N, 2, 2, check_shared=True), o.get(orn.PSI))
    assert np.array_equal(node_assemble([t[2] for t in out], N, 2, 2, check_shared=True), o.get(orn.Q))


# ------------------------------------------------------------------ 4. the file alone makes the tiles

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py,case", [(2, 2, "stochastic_64x1"), (4, 2, "sqg_32x3"), (2, 1, "wavelet_32x3")])
def test_node_from_state_on_tiles(px, py, case, strict, tmp_path):
    c = dict(TILED_CASES[case])
    opts = dict(c.get("opts", {}))
    tol = opts.pop("TOLERANCE", None)   # an option is not state: a tolerance goes in the params text (test_node_from_state)
    if tol is not None:
        c["par"] += f"TOLERANCE = {tol}\n"
    c["opts"] = opts
    # a handle made from a file has its constants: mg_coarse keeps its default in every run of this test
    log_a, snap_a = whole_run(c, px, py, strict, mg_coarse=32)
    p, p2 = str(tmp_path / "s.msom"), str(tmp_path / "again.msom")
    first = first_half_saved(c, px, py, strict, p, True, mg_coarse=32)

    def body(g, rank):
        assert (g.N, g.nl) == N_nl(c) and g.tile[:2] == (px, py) and g.param("io_tiles") == 1
        assert g.param("wavelet_tiles") == (1 if c.get("stochastic") or c.get("wavelet") else 0)
        g.save_state(p2, constants=True)   # a handle made from a file saves the same file again
        log = list(first[rank][0])
        second_half(g, c, log, first[0][1])
        return log, snap_tile(g, c)
    out = bare_tiled(lambda rank, uid: node_from_state(p, strict=strict, tiled=(px, py, rank, uid)), px, py, body)
    assert_same_run(log_a, snap_a, *assembled(out, c, px, py))
    assert open(p, "rb").read() == open(p2, "rb").read()
    # without constants the file cannot make a handle, on any rank
    first_half_saved(c, px, py, strict, p, False, mg_coarse=32)

    def refused(rank, uid):
        with pytest.raises(MsomError, match="MSOM_STATE_CONSTANTS"):
            node_from_state(p, strict=strict, tiled=(px, py, rank, uid))
        return NodeQG(c["par"], strict=strict)   # something for bare_tiled to close
    bare_tiled(refused, px, py, lambda g, rank: True)


# ------------------------------------------------------------------ 5. failures are collective and leave no trace

@pytest.mark.parametrize("strict", [True, False])
def test_failures_are_collective_and_leave_no_trace(strict, tmp_path):
    px, py, N, nl = 2, 2, 32, 3
    c = dict(par=orn.node_params(N, nl, bc_fac=1.0), mask=True, topo=True, forcing=True)
    good = str(tmp_path / "good.msom")
    first_half_saved(c, px, py, strict, good, True)
    b = open(good, "rb").read()
    (tmp_path / "cut.msom").write_bytes(b[:len(b) // 2])
    d = read_state(good)
    rec = dict(d["records"])
    kw = dict(params=c["par"], dialect=2, flag_topo=1)
    write_state(tmp_path / "stochastic.msom", rec, N + 1, N + 1, nl, stochastic=1, noise_mode=1, **kw)
    sq = dict(rec, node=rec["node"].copy())
    sq["node"][NODE_SCALARS.index("sqg")] = 1
    write_state(tmp_path / "sqg.msom", sq, N + 1, N + 1, nl, **kw)
    write_state(tmp_path / "nl2.msom", rec, N + 1, N + 1, nl - 1, **kw)   # the header is refused before any record is looked at
    tx = N // px                                 # held 17 x 17, owned 16 x 16 (rank 0)
    flips = [3 * tx + 5, tx]                     # an owned interior element; column tx of row 0 of the held window: a shared column
    attempts = [("save", str(tmp_path / "nowhere" / "s.msom"), MSOM_ERR_IO, None), ("load", str(tmp_path / "none.msom"), MSOM_ERR_IO, None),
                ("load", str(tmp_path / "cut.msom"), MSOM_ERR_IO, None)] + [("load", good, MSOM_ERR_IO, e) for e in flips] + \
               [("load", str(tmp_path / f"{n}.msom"), MSOM_ERR_CONFIG, None) for n in ("nl2", "sqg", "stochastic")]

    def body(g, rank):
        steps(g, c, 2, [])
        held = lambda: (g.get("PSI"), g.get("Q"), g.get("TOPO"), g.t, g.dt, g.iter, g.param("exchanges"))
        before, seen = held(), []
        for what, path, code, flip in attempts:
            if flip is not None:
                g.state_dbg_flip(flip)
            try:
                g.save_state(path, constants=True) if what == "save" else g.load_state(path)
                seen.append((0, ""))
            except MsomError as e:
                seen.append((e.code, str(e)))
            now = held()
            assert all(np.array_equal(x, y) for x, y in zip(before, now)), (what, path)
        g.load_state(good)   # the flips were for one load each: the good file still loads
        return seen, g.iter
    out = run_tiled(c["par"], px, py, global_inputs(c), strict, body, opts=tile_opts(c))
    for k, (what, path, code, flip) in enumerate(attempts):
        got = [o[0][k] for o in out]
        print(what, os.path.basename(path), flip, got)
        assert all(g[0] == code for g in got), (what, path, flip, got)       # the same code on every rank
        if flip is not None:
            assert all("digest" in g[1] for g in got)
        if what == "save" or "none" in path:                                 # rank 0 saw the cause, the others say so
            assert sum("another rank" in g[1] for g in got) == (px * py - 1 if what == "save" else 0)
    assert all(o[1] == 3 for o in out)
    assert sorted(os.listdir(tmp_path)) == ["cut.msom", "good.msom", "nl2.msom", "sqg.msom", "stochastic.msom"]


# ------------------------------------------------------------------ 6. the gate

def test_the_gate(tmp_path):
    N, nl = 32, 2
    par, inp = params(N, nl), inputs(N, nl)
    # one tile: accepted, no effect
    files = []
    for v in (0, 1):
        g = single(par, inp, False, dict(io_tiles=v))
        assert g.param("io_tiles") == v
        with pytest.raises(MsomError, match=f"error {MSOM_ERR_ARG}: .*io_tiles"):
            g.set_option("io_tiles", 2)
        g.step(True)
        g.save_state(str(tmp_path / f"one{v}.msom"), constants=True)
        files.append(open(tmp_path / f"one{v}.msom", "rb").read())
        g.close()
    assert files[0] == files[1]

    # tiles: 2 is refused, the default is 0, and a step posts the same exchanges with the option on
    def body(g, rank):
        on = g.param("io_tiles")
        try:
            g.set_option("io_tiles", 2)
            code = 0
        except MsomError as e:
            code = e.code
        for _ in range(2):
            g.step(True)
        return on, code, g.param("io_tiles"), g.param("exchanges"), g.get("PSI")
    off = run_tiled(par, 2, 2, inp, False, body, opts=dict(mg_coarse=8))
    on = run_tiled(par, 2, 2, inp, False, body, opts=dict(mg_coarse=8, io_tiles=1))
    for a, b in zip(off, on):
        assert a[:3] == (0, MSOM_ERR_ARG, 0) and b[:3] == (1, MSOM_ERR_ARG, 1)
        assert a[3] == b[3] > 0 and np.array_equal(a[4], b[4])
