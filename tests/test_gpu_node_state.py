"""Lossless checkpoint and bit-exact restart of the vertex model (include/msomn_state.h).

Run A takes its steps without stopping.  Run B takes the first half, saves, is destroyed; a new handle loads the file and takes the
second half.  Everything compared is compared bit for bit, in both builds: saving and loading move fp64 bits, no arithmetic, so there
is no tolerance to state.  The strict resumed run is also held to the CPU oracle stepped without stopping.
"""
import os
import re

import numpy as np
import pytest

import orn
from msom_amd import MsomError, NodeQG, api, node_from_state
from msom_amd.state import digest, read_state, write_state
from test_gpu_node_parity import land_mask, topo_field
from test_node_state_host import GOLDEN_NODE, NODE_SCALARS, golden_oracle
from test_oracle_node_wavelet_kat import params as wavelet_params
from test_oracle_sqg_kat import bs_field, sqg_params

pytestmark = pytest.mark.gpu

MSOM_ERR_IO, MSOM_ERR_CONFIG = -2, -3
STOCH = "gp_low = 0.02\namp_stoch = 0.3\nL_filt = 8\n"
DTFLT = 0.05

# name -> how the run is made.  par: params text; opts: options set on every handle of the run (they are not state); the rest is read by
# set_inputs / first_half / second_half
CASES = {
    "n32x1": dict(par=orn.node_params(32, 1, bc_fac=1.0, extra="gp_low = 0.02\n"), mask=True),
    "n64x3_island": dict(par=orn.node_params(64, 3, bc_fac=1.0, nu4=1.0, extra="gp_low = 0.02\ntau1 = 5e-4\ntf1 = 0.3\ntf2 = 0.7\n"), mask=True, topo=True,
                         pg=True, opts=dict(TOLERANCE=1e-8), tnext=0.11, forcing=True),
    "n128x4": dict(par=orn.node_params(128, 4, bc_fac=0.5), mask=True, opts=dict(TOLERANCE=1e-8), cycles=True),
    "n64x2_s2x": dict(par=orn.node_params(64, 2), s2x=True),
    "sqg_32x3": dict(par=sqg_params(32, 3, extra="tau1 = 5e-4\ntf1 = 0.3\ntf2 = 0.7\n"), mask=True, sqg=True, forcing=True, opts=dict(TOLERANCE=1e-9)),
    "forcing3d_32x3": dict(par=orn.node_params(32, 3), mask=True, f3d=True, forcing=True),
    "user_forcing_32x2": dict(par=orn.node_params(32, 2, bc_fac=1.0), mask=True, user_forcing=True),
    "stochastic_64x1": dict(par=orn.node_params(64, 1, bc_fac=1.0, extra=STOCH), opts=dict(stochastic=1, noise_mode=1, seed=11), stochastic=True, forcing=True),
    "stochastic_midstep": dict(par=orn.node_params(64, 1, bc_fac=1.0, extra=STOCH), opts=dict(stochastic=1, noise_mode=1, seed=11), stochastic=True, forcing=True,
                               midstep=True),
    "wavelet_32x3": dict(par=wavelet_params(32, 3, 12.0, 3.0), mask=True, wavelet=True, forcing=True),
}
WITHOUT_CONSTANTS = ("n64x3_island", "user_forcing_32x2")   # the second handle is set up as the first was, then loads


def N_nl(c):
    return int(re.search(r"^N\s*=\s*(\d+)", c["par"], re.M).group(1)), int(re.search(r"^nl\s*=\s*(\d+)", c["par"], re.M).group(1))


def configure(c, strict):
    g = NodeQG(c["par"], strict=strict)
    g.set_option("quiet", 1)
    for k, v in c.get("opts", {}).items():
        g.set_option(k, v)
    return g


def inputs(c):
    """field name -> array, in the order they are set (psi last)"""
    N, nl = N_nl(c)
    out, mk = {}, np.ones((1, N + 1, N + 1))
    if c.get("mask"):
        mk = land_mask(N)
        out["MASK"] = mk
    if c.get("topo"):
        out["TOPO"] = topo_field(N)
    if c.get("pg"):
        out["PSIPG"] = 0.3 * orn.node_psi(nl, N)[::-1].copy()
    if c.get("s2x"):      # N2 that varies in x: no row tables
        n2 = np.array([float(v) for v in orn.NODE_LAYERS[nl][1].strip("[]").split(",")])[:, None, None] * np.ones((nl - 1, N + 1, N + 1))
        out["S2"] = n2 * (1.0 + 0.3 * np.cos(np.linspace(0, 5, N + 1))[None, None, :])
    if c.get("sqg"):
        out["BS"] = bs_field(N)
    if c.get("f3d"):
        out["QFORC3D"] = 1e-3 * np.random.default_rng(8).standard_normal((nl, N + 1, N + 1))
    out["PSI"] = orn.node_psi(nl, N) * mk
    return out


def set_inputs(g, c):
    for k, a in inputs(c).items():
        g.set(k, a)
    g.set_const()
    if c.get("user_forcing"):
        N, _ = N_nl(c)
        x = np.arange(N + 1) / N
        g.set("QFORC", 1e-3 * np.outer(np.sin(2 * np.pi * x), np.cos(np.pi * x))[None])
    if "tnext" in c:
        g.set_tnext(c["tnext"])


def steps(g, c, n, log):
    for _ in range(n):
        g.step(bool(c.get("forcing")))
        st = g.mgstats()
        log.append((g.dt, g.t, g.iter, st.i, st.resb, st.resa, st.nrelax))


def first_half(g, c, log):
    """3 steps (and what the case adds); the value a driver carries across the save (mid-step: the step's dt)"""
    if c.get("wavelet"):
        steps(g, c, 2, log)
        g.wavelet_filter(DTFLT)
        steps(g, c, 1, log)
        return None
    steps(g, c, 3, log)
    if c.get("midstep"):   # the first stage of a fourth step: update, advance(QPRED, Q, DQ, dt / 2) -- the noise is drawn here
        g.forcing()
        dt = g.update("Q", "DQ")
        g.advance("QPRED", "Q", "DQ", dt / 2)
        return dt
    return None


def second_half(g, c, log, carried):
    if c.get("wavelet"):
        steps(g, c, 1, log)
        g.wavelet_filter(DTFLT)
        steps(g, c, 2, log)
        return
    if c.get("midstep"):   # the second stage: corrector_step = 1, so this advance must not draw again
        log.append(g.update("QPRED", "DQ", carried))
        g.advance("Q", "Q", "DQ", carried)
        steps(g, c, 2, log)
        return
    steps(g, c, 3, log)


def snapshot(g, c):
    out = {"psi": g.get("PSI"), "q": g.get("Q"), "q_forcing": g.get("QFORC")}
    if c.get("stochastic"):
        out["noise"] = g.noise()
        out["noise_draw"] = g.param("noise_draw")
    if c.get("wavelet"):
        out["psi_f"] = g.get("PSIF")
    return out


def assert_same_run(log_a, snap_a, log_b, snap_b):
    assert log_a == log_b, [(a, b) for a, b in zip(log_a, log_b) if a != b][:2]
    assert snap_a.keys() == snap_b.keys()
    for k in snap_a:
        assert np.array_equal(snap_a[k], snap_b[k]), f"{k}: max diff {np.abs(np.asarray(snap_a[k]) - np.asarray(snap_b[k])).max():g}"


def run_a(c, strict):
    g, log = configure(c, strict), []
    set_inputs(g, c)
    second_half(g, c, log, first_half(g, c, log))
    snap = snapshot(g, c)
    g.close()
    return log, snap


def run_b_first(c, strict, path, constants):
    g, log = configure(c, strict), []
    set_inputs(g, c)
    carried = first_half(g, c, log)
    g.save_state(path, constants=constants)
    g.close()
    return log, carried


# ------------------------------------------------------------------ 1. resume is exact

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", list(CASES))
def test_resume_is_exact(case, strict, tmp_path):
    c = CASES[case]
    log_a, snap_a = run_a(c, strict)
    if c.get("cycles"):   # the correction rides in the next residual pass: psi has been swapped with the second buffer
        assert max(row[3] for row in log_a) > 1
    for constants in ((True, False) if case in WITHOUT_CONSTANTS else (True,)):
        p = str(tmp_path / f"s{int(constants)}.msom")
        log_b, carried = run_b_first(c, strict, p, constants)
        g = configure(c, strict)
        if not constants:
            set_inputs(g, c)
            if c.get("user_forcing"):   # must come from the file
                g.set("QFORC", np.zeros((1,) + g.shape("QFORC")[1:]))
        g.load_state(p)
        if c.get("s2x"):
            assert g.param("s2_xuniform") == 0
        second_half(g, c, log_b, carried)
        assert_same_run(log_a, snap_a, log_b, snapshot(g, c))
        g.close()


# ------------------------------------------------------------------ 2. the strict resumed run equals the oracle

def test_strict_resumed_run_equals_the_oracle(tmp_path):
    c = CASES["n64x3_island"]
    o = orn.NodeOracle(c["par"], smoother=orn.GS_RB, quiet=1, **c["opts"])
    for k, a in inputs(c).items():
        o.set(getattr(orn, k), a)
    o.set_const()
    o.set_tnext(c["tnext"])
    ref = []
    for _ in range(6):
        o.step(True)
        ref.append((o.dt, o.t, o.mgstats().i))
    p = str(tmp_path / "s.msom")
    log, _ = run_b_first(c, True, p, True)
    g = configure(c, True)
    g.load_state(p)
    steps(g, c, 3, log)
    assert [(r[0], r[1], r[3]) for r in log] == ref
    assert np.array_equal(g.get("PSI"), o.get(orn.PSI)) and np.array_equal(g.get("Q"), o.get(orn.Q))
    g.close()


# ------------------------------------------------------------------ 3. a used handle and a fresh one load alike

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", ["n128x4", "n64x3_island"])
def test_used_and_fresh_handles_load_alike(case, strict, tmp_path):
    c = CASES[case]
    p = str(tmp_path / "s.msom")
    run_b_first(c, strict, p, True)
    N, nl = N_nl(c)
    fresh, used = configure(c, strict), configure(c, strict)
    # the used handle has solved on other data: its second psi buffer exists, the pointers have been swapped an odd number of times
    # or an even one, the correction and residual buffers of every level hold the last solve
    other = dict(inputs(c))
    other["PSI"] = 7.0 * other["PSI"][::-1].copy() + 0.01 * other["MASK"]
    for k, a in other.items():
        used.set(k, a)
    used.set_const()
    for n in range(2):
        used.step(True)
    outs = []
    for g in (fresh, used):
        g.load_state(p)
        log = []
        steps(g, c, 3, log)
        outs.append((log, snapshot(g, c)))
        g.close()
    assert_same_run(*outs[0], *outs[1])
    # one more swap before the load (an odd and an even count must both work)
    used2 = configure(c, strict)
    for k, a in other.items():
        used2.set(k, a)
    used2.set_const()
    used2.step(True)
    used2.rhs_pv()
    used2.load_state(p)
    log = []
    steps(used2, c, 3, log)
    assert_same_run(*outs[0], log, snapshot(used2, c))
    used2.close()


# ------------------------------------------------------------------ 4. digest and layout

# every small shape on both builds; and, on one build, the smallest at which a layer does not fit one staging chunk of 4 Mi doubles:
# 2049 vertices a side, so 2047 rows in the first chunk and 2 in the second
LAYOUT_SHAPES = [(N, nl, strict) for strict in (True, False) for nl in (1, 2, 3) for N in (16, 32, 64)] + [(2048, 1, True)]


@pytest.mark.parametrize("N,nl,strict", LAYOUT_SHAPES)
def test_digest_and_layout(N, nl, strict, tmp_path):
    par = orn.node_params(N, nl, bc_fac=1.0, extra=STOCH)
    c = dict(par=par, mask=True, topo=nl > 1, opts=dict(stochastic=1, noise_mode=1, seed=5), stochastic=True)
    g = configure(c, strict)
    set_inputs(g, c)
    steps(g, c, 2, [])
    p = str(tmp_path / "s.msom")
    g.save_state(p, constants=True)
    assert not os.path.exists(p + ".tmp")
    d = read_state(p)
    assert (d["dialect"], d["nx"], d["ny"], d["nl"], d["nptr"], d["mode_pv_invert"], d["stochastic"], d["noise_mode"]) == (2, N + 1, N + 1, nl, 0, 0, 1, 1)
    assert d["flag_topo"] == int(nl > 1) and d["params"] == par
    want = ["time", "mgstats", "node", "psi", "q", "q_forcing", "noise", "mask"] + (["S2", "topo"] if nl > 1 else [])
    assert list(d["records"]) == want and d["ring"] == []
    for name, f in (("psi", "PSI"), ("q", "Q"), ("q_forcing", "QFORC"), ("mask", "MASK")) + ((("S2", "S2"), ("topo", "TOPO")) if nl > 1 else ()):
        assert np.array_equal(d["records"][name], g.get(f)), name
        assert d["digests"][name] == digest(g.get(f)), name
    assert d["records"]["noise"].shape == (1, N, N) and np.array_equal(d["records"]["noise"][0], g.noise())
    assert d["digests"]["noise"] == digest(g.noise())
    st = g.mgstats()
    assert (d["t"], d["dt"], d["iter"]) == (g.t, g.dt, 2) and list(d["records"]["mgstats"]) == [st.i, st.resb, st.resa, st.nrelax]
    node = dict(zip(NODE_SCALARS, d["records"]["node"]))
    assert (node["seed"], node["noise_draw"], node["corrector_step"], node["topo_set"], node["DT"]) == (5, g.param("noise_draw"), 0, int(nl > 1), g.param("DT"))
    assert api.state_check(p, strict=strict) == len(want)
    # save is pure: the same file again, and the handle goes on as one that never saved (test_resume_is_exact's run A never saves)
    g.save_state(p + "2", constants=True)
    assert open(p, "rb").read() == open(p + "2", "rb").read()
    # a bit flipped on the device between the upload and the digest: the load fails and changes nothing
    before = (g.get("PSI"), g.get("Q"), g.t, g.noise())
    steps(g, c, 1, [])
    after = (g.get("PSI"), g.get("Q"), g.t, g.noise())
    g.state_dbg_flip(3 * (N + 1) + 5)
    with pytest.raises(MsomError, match=f"error {MSOM_ERR_IO}: .*psi.*digest"):
        g.load_state(p)
    for a, b in zip(after, (g.get("PSI"), g.get("Q"), g.t, g.noise())):
        assert np.array_equal(a, b)
    g.load_state(p)   # the flip was for one load
    for a, b in zip(before, (g.get("PSI"), g.get("Q"), g.t, g.noise())):
        assert np.array_equal(a, b)
    g.close()
    h = configure(c, strict)   # and a handle that has nothing but the file
    h.load_state(p)
    for a, b in zip(before, (h.get("PSI"), h.get("Q"), h.t, h.noise())):
        assert np.array_equal(a, b)
    h.close()


# ------------------------------------------------------------------ 5. refusals leave the handle as it was

def test_refusals_leave_the_handle_as_it_was(tmp_path):
    c = dict(par=orn.node_params(32, 2, bc_fac=1.0), mask=True, topo=True)
    good = str(tmp_path / "good.msom")
    run_b_first(c, False, good, True)
    g = configure(c, False)
    set_inputs(g, c)
    steps(g, c, 1, [])
    held = (g.get("PSI"), g.get("Q"), g.get("TOPO"), g.t, g.dt, g.iter, g.param("DT"))

    def refused(path, code, handle=g, word=""):
        with pytest.raises(MsomError, match=f"error {code}: .*{word}"):
            handle.load_state(str(path))

    def untouched():
        now = (g.get("PSI"), g.get("Q"), g.get("TOPO"), g.t, g.dt, g.iter, g.param("DT"))
        assert all(np.array_equal(a, b) for a, b in zip(held, now))

    # wrong N, wrong nl
    for other in (dict(par=orn.node_params(16, 2, bc_fac=1.0), mask=True, topo=True), dict(par=orn.node_params(32, 3, bc_fac=1.0), mask=True, topo=True)):
        p = tmp_path / "other.msom"
        run_b_first(other, False, str(p), True)
        refused(p, MSOM_ERR_CONFIG, word="grid")
    # a dialect-0 file of the same numbers, and the same file read the other way round
    p0 = tmp_path / "d0.msom"
    write_state(p0, {"psi": np.zeros((2, 33, 33)), "q": np.zeros((2, 33, 33))}, 33, 33, 2, params=c["par"])
    refused(p0, MSOM_ERR_CONFIG, word="dialect 0")
    with pytest.raises(MsomError, match="msom_create_from_state"):
        node_from_state(p0)
    with pytest.raises(MsomError, match="msomn_create_from_state"):
        api.from_state(good)
    # stochastic mismatch
    s = configure(dict(c, opts=dict(stochastic=1, noise_mode=1)), False)
    refused(good, MSOM_ERR_CONFIG, handle=s, word="stochastic")
    s.close()
    # topo_set mismatch on a handle that has its constants
    t = configure(c, False)
    set_inputs(t, dict(c, topo=False))
    refused(good, MSOM_ERR_CONFIG, handle=t, word="topo_set")
    t.close()
    # truncated file, corrupted payload, bad magic
    b = open(good, "rb").read()
    for name, data in (("cut", b[:len(b) // 2]), ("magic", b"XSOM" + b[4:])):
        (tmp_path / name).write_bytes(data)
        refused(tmp_path / name, MSOM_ERR_IO)
    x = bytearray(b)
    x[bytes(b).index(b"q_forcing\0") - 8 * 40] ^= 0x01   # inside the payload of q, the record before q_forcing
    (tmp_path / "payload").write_bytes(bytes(x))
    refused(tmp_path / "payload", MSOM_ERR_IO, word="digest")
    # the clamped DT: a handle whose DT is another one, with constants and without
    d = read_state(good)
    rec = dict(d["records"])
    rec["node"] = rec["node"].copy()
    rec["node"][NODE_SCALARS.index("DT")] *= 0.5
    write_state(tmp_path / "dt.msom", rec, 33, 33, 2, params=c["par"], dialect=2, flag_topo=1)
    refused(tmp_path / "dt.msom", MSOM_ERR_CONFIG, word="DT")
    u = configure(c, False)
    u.set_option("DT", 1e-3)
    refused(good, MSOM_ERR_CONFIG, handle=u, word="DT")
    u.close()
    untouched()
    # the good file still loads into the same handle
    g.load_state(good)
    assert g.iter == 3
    g.close()
    # noise_mode = 0 draws from rand(): nothing to save
    n0 = configure(dict(par=orn.node_params(32, 1, bc_fac=1.0, extra=STOCH), opts=dict(stochastic=1, noise_mode=0)), False)
    n0.set("PSI", orn.node_psi(1, 32))
    n0.set_const()
    with pytest.raises(MsomError, match=f"error {MSOM_ERR_CONFIG}: .*noise_mode"):
        n0.save_state(str(tmp_path / "n0.msom"))
    assert not os.path.exists(tmp_path / "n0.msom")
    n0.close()


# ------------------------------------------------------------------ 6. the file alone restarts a run

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("case", ["n32x1", "stochastic_64x1", "sqg_32x3"])
def test_node_from_state(case, strict, tmp_path):
    c = dict(CASES[case])
    opts = dict(c.get("opts", {}))
    tol = opts.pop("TOLERANCE", None)   # an option is not state: the file records the stochastic ones, a tolerance goes in the params text
    if tol is not None:
        c["par"] += f"TOLERANCE = {tol}\n"
    c["opts"] = opts
    log_a, snap_a = run_a(c, strict)
    p = str(tmp_path / "s.msom")
    log_b, carried = run_b_first(c, strict, p, True)
    g = node_from_state(p, strict=strict)
    g.set_option("quiet", 1)
    assert (g.N, g.nl) == N_nl(c)
    second_half(g, c, log_b, carried)
    assert_same_run(log_a, snap_a, log_b, snapshot(g, c))
    g.close()
    # without constants the file cannot make a handle
    run_b_first(c, strict, p, False)
    with pytest.raises(MsomError, match="MSOM_STATE_CONSTANTS"):
        node_from_state(p, strict=strict)


@pytest.mark.parametrize("strict", [True, False])
def test_a_handle_made_from_a_file_saves_the_same_file(strict, tmp_path):
    """save with the constants, msomn_create_from_state, save again with the same flags: the two files are equal byte for byte"""
    c = CASES["n32x1"]
    pa, pb = str(tmp_path / "a.msom"), str(tmp_path / "b.msom")
    run_b_first(c, strict, pa, True)
    g = node_from_state(pa, strict=strict)
    g.save_state(pb, constants=True)
    g.close()
    a, b = read_state(pa), read_state(pb)
    assert list(a["records"]) == list(b["records"])
    for k in a["records"]:     # record by record first, so that a failure names the record
        assert np.array_equal(a["records"][k], b["records"][k], equal_nan=True), k
    assert open(pa, "rb").read() == open(pb, "rb").read()


# ------------------------------------------------------------------ 7. the golden file

@pytest.mark.parametrize("how", ["load_state", "node_from_state"])
def test_golden_file_continues_to_the_oracle(how):
    txt, o = golden_oracle()
    for _ in range(6):
        o.step(True)
    if how == "load_state":
        g = NodeQG(txt, strict=True)
        g.load_state(GOLDEN_NODE)
    else:
        g = node_from_state(GOLDEN_NODE, strict=True)
    g.set_option("quiet", 1)
    assert g.iter == 3
    for _ in range(3):
        g.step(True)
    assert (g.t, g.dt, g.iter, g.mgstats().i) == (o.t, o.dt, 6, o.mgstats().i)
    assert np.array_equal(g.get("PSI"), o.get(orn.PSI)) and np.array_equal(g.get("Q"), o.get(orn.Q))
    g.close()


# ------------------------------------------------------------------ 8. the driver

@pytest.mark.parametrize("strict", [True, False])
def test_driver_resumes_from_its_checkpoint(strict, tmp_path):
    N, nl = 32, 2
    c = dict(par=orn.node_params(N, nl, bc_fac=1.0, extra="tend = 0.4\ndtout = 0.1\ndtdiag = 0.05\n"), mask=True)

    def handle(**opts):
        g = configure(c, strict)
        for k, v in opts.items():
            g.set_option(k, v)
        return g

    whole, died = tmp_path / "whole", tmp_path / "died"
    whole.mkdir(); died.mkdir()
    g = handle(ckpt_steps=5)
    set_inputs(g, c)
    n_whole = g.run(str(whole))
    g.close()
    g = handle(ckpt_steps=5)
    set_inputs(g, c)
    assert g.run(str(died), 8) == 8
    # what a run writes after its last checkpoint and before it dies: one more record and one more line
    g.write_nc(str(died / "outdir_0001" / "vars.nc"))
    with open(died / "outdir_0001" / "diag_1d.dat", "a") as f:
        f.write("%e, %e, %e, %e\n" % (g.t, 1.0, 2.0, 3.0))
    g.close()   # dies
    assert read_state(died / "state.msom")["iter"] == 5 and list(read_state(died / "state.msom")["records"]["run"][3:5]) == [1, 1]
    g = handle(resume=1)   # no inputs, no set_const: the checkpoint holds the constants
    assert g.run(str(died)) == n_whole and n_whole > 10
    assert abs(g.t - 0.4) < 1e-12
    g.close()
    assert sorted(os.listdir(died)) == ["outdir_0001", "state.msom"]
    for name in ("vars.nc", "diag_1d.dat"):
        a, b = (whole / "outdir_0001" / name).read_bytes(), (died / "outdir_0001" / name).read_bytes()
        assert len(a) > 100 and a == b, name
    assert len((whole / "outdir_0001" / "diag_1d.dat").read_text().splitlines()) == 9
    # without the file, resume = 1 starts normally
    fresh = tmp_path / "fresh"
    fresh.mkdir()
    g = handle(resume=1)
    set_inputs(g, c)
    assert g.run(str(fresh), 2) == 2 and os.listdir(fresh) == ["outdir_0001"]
    g.close()
