"""Lossless checkpoint and bit-exact restart (include/msom_state.h): a run that is stopped, saved, destroyed, re-created, loaded and
continued gives the bits of the run that was never stopped.

STATE_ROWS is the table of the header's entry points that take a msom_t * (tests/test_state_host.py holds it to the header): "pure"
means the call changes nothing the next step reads, "mutating" that it does and the handle's caches go.

1. resume is exact: run A takes 3 + 3 steps; run B takes 3, saves, is destroyed, a new handle with the same params text and options
   loads the file and takes 3 more.  psi, q, every dt, t, iter and (i, resb, resa, nrelax) bit for bit, mgstats().sum to rel 1e-12 as
   test_gpu_call_sequences compares it (a sum over the grid whose order differs between the cached and the plain path), plus what the
   case adds (budgets, statistics, AB3 history, tracers).  Saved with the constants, the second handle does nothing but load; saved
   without, it is set up as the first was and then loads.
2. save is pure and ordered, by the play of test_gpu_call_sequences.py; load is a mutating row.
3. digest and layout against the numpy restatement of msom_amd.state; a device copy altered after the upload is refused.
4. refusals leave the handle as it was.
5. the golden file of format version 1 continues to the oracle's bits.
6. 2 x 2 tiles (threads on one device, as tests/test_gpu_tiled.py).
7. the driver: msom_qg params.in 5 ckpt_steps=5, then msom_qg params.in -1 resume=1, against one run to the end.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import newqg_ref as nq
import orc
import test_gpu_call_sequences as cs
from msom_amd import FIELDS as F, STATS, NewQG, QG, from_state, read_state, state_check, write_state
from msom_amd.api import MsomError
from msom_amd.state import digest
from test_gpu_rhs_resid import params, same
from test_gpu_tiled import assemble, run_tiled

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.path.join(ROOT, "msom_amd", "lib", "msom_qg")
GOLDEN = os.path.join(HERE, "golden", "state_32x32x3.msom")
BUILDS = [True, False]
CACHED, PLAIN = cs.CACHED, cs.PLAIN
MSOM_ERR_IO, MSOM_ERR_CONFIG = -2, -3

STATE_ROWS = {"msom_state_save": "pure", "msom_state_load": "mutating", "msom_state_dbg_flip": "pure"}


# ------------------------------------------------------------------ 1. resume is exact

class Case:
    """one run: `make` a handle with its options, `setup` what a user sets before the first step, `advance(g, n)` for n = 0 .. 5 (a
    step unless the case says otherwise; returns dt or None), `final` the extra values compared at the end"""
    nsplit, ntotal = 3, 6

    def __init__(self, grid, extra="", opts=None, tol=1e-3, pre=None, begin=None, advance=None, final=None, conf=None):
        self.grid, self.extra, self.opts, self.tol = grid, extra, opts or {}, tol
        self.pre, self.begin, self._advance, self.final, self.conf = pre, begin, advance, final, conf

    def text(self):
        return params(*self.grid, self.extra)

    def make(self, strict, conf=None):
        g = QG(self.text(), strict=strict)
        g.option("quiet", 1)
        g.option("TOLERANCE", self.tol)
        for k, v in {**(conf or self.conf or {}), **self.opts}.items():
            g.option(k, v)
        return g

    def setup(self, g):
        nx, ny, nl = self.grid
        if self.pre:
            self.pre(g)
        g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
        g.set_const()
        if self.begin:
            self.begin(g)

    def advance(self, g, n):
        return self._advance(g, n) if self._advance else g.step()

    def snap(self, g, dts):
        st = g.mgstats()
        out = [(g.get(F["PSI"]), g.get(F["Q"]), list(dts) + [g.t, g.iter], (st.i, st.resb, st.resa, st.nrelax), st.sum)]
        return out, (self.final(g) if self.final else [])


def run_straight(c, strict, conf=None):
    g = c.make(strict, conf)
    c.setup(g)
    dts = [c.advance(g, n) for n in range(c.ntotal)]
    out = c.snap(g, dts)
    g.close()
    return out


def run_resumed(c, strict, path, constants=True, conf=None, conf2=None):
    g = c.make(strict, conf)
    c.setup(g)
    dts = [c.advance(g, n) for n in range(c.nsplit)]
    g.save_state(path, constants=constants)
    g.close()
    del g
    assert not os.path.exists(str(path) + ".tmp") and state_check(path) > 0
    g = c.make(strict, conf2 or conf)
    if not constants:
        c.setup(g)
    g.load_state(path)
    dts += [c.advance(g, n) for n in range(c.nsplit, c.ntotal)]
    out = c.snap(g, dts)
    g.close()
    return out


def same_run(a, b):
    same(a[0], b[0])
    cs.same_returned(a[1], b[1], "final values")


def rng_field(seed, shape, scale=1.0):
    return scale * np.random.default_rng(seed).standard_normal(shape)


# -- the cases
def tracers_pre(g):
    g.set(F["PTR"], rng_field(31, g.shape(F["PTR"])))
    g.set(F["PTR_RELAX"], rng_field(32, g.shape(F["PTR_RELAX"])))


def stoch_pre(g):
    g.set(F["SIGMA"], 0.5 + np.random.default_rng(33).random(g.shape(F["SIGMA"])))


def ediag_advance(g, n):
    g.energy_tend(0.01 * (n + 1))
    return g.step()


def ediag_final(g):
    return [g.get(F[k]) for k in ("DE_BF", "DE_VD", "DE_J1", "DE_J2", "DE_J3", "DE_FT", "PO_MFT")]


ST2 = (1 << STATS["PSI"]) | (1 << STATS["KE"])


def stats_begin(g):
    g.stats_begin(ST2)
    g.option("stats", 1)


def stats_advance(g, n):
    g.time_filter(0.1 + 0.01 * n)
    return g.step()


def stats_final(g):
    return [g.stats_get(STATS["PSI"]), g.stats_get(STATS["KE"]), g.stats_weight(), g.stats_get(STATS["QME"]), g.param("stats_mask")]


def bfn_pre(g):
    g.set(F["BFN_OBS"], rng_field(41, (g.nl, g.ny, g.nx), 1e-3))
    g.set(F["BFN_GAIN"], (np.random.default_rng(42).random((g.nl, g.ny, g.nx)) < 0.5) * 0.75)


def bfn_advance(g, n):
    """4 steps of the nudging loop before the save (2 + 1 + 1), 4 after it, one of them backwards"""
    dt = g.param("DT")
    k = 0.05 / dt
    if n == 4:
        g.bfn_steps(1, -dt, -1.0, -k)
    else:
        g.bfn_steps(2 if n in (0, 3) else 1, dt, 1.0, k)
    return None


def bfn_final(g):
    return [g.get(F[k]) for k in ("BFN_F1", "BFN_F2", "BFN_F3")] + [g.param(k) for k in ("iRe", "iRe4", "Ekb", "Eks")]


def modal_final(g):
    return [cs.mg(g.modes_mgstats(m)) for m in range(g.nl)]


def de_advance(g, n):
    """a step; the one before the save is followed by pystep_de, which zeroes the cells of psi and leaves its ghost values"""
    dt = g.step()
    if n == 2:
        out = [np.empty((g.nl, g.ny, g.nx)) for _ in range(6)]
        g.pystep_de(cs.noisy(g.get(F["PSI"]), np.random.default_rng(51)), *out, 0)
    return dt


EX = cs.EXTRA
CASES = {
    "dg32x3": Case((32, 32, 3)),
    "128x64x2_cached": Case((128, 64, 2), conf=CACHED),
    "128x64x2_plain": Case((128, 64, 2), conf=PLAIN),
    "16x16x6": Case((16, 16, 6)),
    "32x32x1": Case((32, 32, 1)),
    "periodic_64x64x2": Case((64, 64, 2), "sbc = -1\ntau0 = 0\n"),
    "tol1e-7": Case((128, 64, 2), tol=1e-7, conf=CACHED),
    "tracers": Case((32, 32, 3), "nptr = 1\nptr_r = [10]\nPe = [200]\n", pre=tracers_pre, final=lambda g: [g.get(F["PTR"])]),
    "stochastic": Case((32, 32, 3), "tr_stoch = 50\namp_stoch = 1e-5\n", opts=dict(stochastic=1, noise_mode=1, seed=11), pre=stoch_pre,
                       final=lambda g: [g.get(F["NOISE"])]),
    "ediag": Case((32, 32, 3), EX, advance=ediag_advance, final=ediag_final),
    "stats_time_filter": Case((128, 64, 2), begin=stats_begin, advance=stats_advance, final=stats_final, conf=CACHED),
    "bfn": Case((32, 32, 3), pre=bfn_pre, begin=lambda g: g.bfn_begin(), advance=bfn_advance, final=bfn_final),
    "mode_pv_invert": Case((32, 32, 3), opts=dict(mode_pv_invert=1), final=modal_final),
    "pystep_de_stale_ghosts": Case((32, 32, 3), EX, advance=de_advance, tol=1e-7),
}


@gpu
@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_resume_is_exact(name, strict, tmp_path):
    c = CASES[name]
    a = run_straight(c, strict)
    same_run(a, run_resumed(c, strict, tmp_path / "s.msom", constants=True))
    if name in ("dg32x3", "tol1e-7", "stats_time_filter", "periodic_64x64x2"):
        same_run(a, run_resumed(c, strict, tmp_path / "t.msom", constants=False))
    if name == "pystep_de_stale_ghosts":
        assert read_state(tmp_path / "s.msom")["ring"] == ["psi"]
    if name == "tol1e-7":
        assert a[0][0][3][0] > 1 and a[0][0][3][3] != 4, a[0][0][3]   # several cycles, nrelax adapted


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_a_file_saved_by_a_cached_handle_resumes_a_plain_one(strict, tmp_path):
    c = CASES["128x64x2_cached"]
    same_run(run_straight(c, strict, PLAIN), run_resumed(c, strict, tmp_path / "s.msom", conf=CACHED, conf2=PLAIN))
    same_run(run_straight(c, strict, CACHED), run_resumed(c, strict, tmp_path / "t.msom", conf=PLAIN, conf2=CACHED))


@gpu
def test_strict_resumed_run_equals_the_oracle(tmp_path):
    c = CASES["dg32x3"]
    b = run_resumed(c, True, tmp_path / "s.msom")
    o = orc.Oracle(c.text(), smoother=orc.GS_RB, quiet=1, TOLERANCE=c.tol)
    o.set(orc.PSI, orc.synthetic_psi(3, 32, 32))
    o.set_const()
    dts = []
    for _ in range(c.ntotal):
        o.step()
        dts.append(o.dt)
    psi, q, tail, mg, _ = b[0][0]
    assert np.array_equal(q, o.get(orc.Q)) and np.array_equal(psi, o.get(orc.PSI))
    assert tail == dts + [o.t, o.iter]
    st = o.mgstats()
    assert mg == (st.i, st.resb, st.resa, st.nrelax)


def nq_handle(gp_low, strict):
    g = NewQG(nq.sample_par(32, gp_low=gp_low).text(), strict=strict)
    g.option("quiet", 1)
    return g


@gpu
@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("gp_low", [0.0, 2500.0])
@pytest.mark.parametrize("constants", [True, False])
def test_newqg_resume_is_exact(gp_low, strict, constants, tmp_path):
    gold = np.load(os.path.join(HERE, "golden", "newqg_32.npz"))
    forc = rng_field(61, (1, 32, 32), 1e-3)

    def start():
        g = nq_handle(gp_low, strict)
        g.set(F["QFORC"], forc)
        g.set(F["PSI"], gold["sbc0_in_psi"][None])
        g.set_const()
        return g

    def snap(g, dts):
        st = g.mgstats()
        return [(g.get(F["PSI"]), g.get(F["Q"]), dts + [g.t, g.iter], (st.i, st.resb, st.resa, st.nrelax), st.sum)]

    a = start()
    da = [a.step() for _ in range(6)]
    b = start()
    db = [b.step() for _ in range(3)]
    b.save_state(tmp_path / "n.msom", constants=constants)
    b.close()
    b = start() if not constants else nq_handle(gp_low, strict)
    b.load_state(tmp_path / "n.msom")
    db += [b.step() for _ in range(3)]
    same(snap(a, da), snap(b, db))
    c = from_state(tmp_path / "n.msom", strict=strict)     # the dialect comes from the file
    assert isinstance(c, NewQG) and c.iter == 3 and c.param("gp_low") == gp_low
    if constants:
        c.option("quiet", 1)
        dc = db[:3] + [c.step() for _ in range(3)]
        same(snap(a, da), snap(c, dc))
    for g in (a, b, c):
        g.close()


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_from_state_makes_the_handle_from_the_file_alone(strict, tmp_path):
    c = CASES["stochastic"]
    a = run_straight(c, strict)
    g = c.make(strict)
    c.setup(g)
    dts = [c.advance(g, n) for n in range(3)]
    g.save_state(tmp_path / "s.msom", constants=True)
    g.close()
    g = from_state(tmp_path / "s.msom", strict=strict)      # stochastic, noise_mode and seed come from the file
    g.option("quiet", 1)
    g.option("TOLERANCE", c.tol)
    dts += [g.step() for _ in range(3)]
    same_run(a, c.snap(g, dts))
    g.close()


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_a_handle_made_from_a_file_saves_the_same_file(strict, tmp_path):
    """save with the constants, msom_create_from_state, save again with the same flags: the two files are equal byte for byte"""
    c = CASES["dg32x3"]
    g = c.make(strict)
    c.setup(g)
    for n in range(c.nsplit):
        c.advance(g, n)
    g.save_state(tmp_path / "a.msom", constants=True)
    g.close()
    h = from_state(tmp_path / "a.msom", strict=strict)
    h.save_state(tmp_path / "b.msom", constants=True)
    h.close()
    a, b = read_state(tmp_path / "a.msom"), read_state(tmp_path / "b.msom")
    assert list(a["records"]) == list(b["records"])
    for k in a["records"]:     # record by record first, so that a failure names the record
        assert np.array_equal(a["records"][k], b["records"][k], equal_nan=True), k
    assert (tmp_path / "a.msom").read_bytes() == (tmp_path / "b.msom").read_bytes()


# ------------------------------------------------------------------ 2. save is pure and ordered; load is a mutating row

def save_call(h, rng, ctx):
    p = ctx.tmp / "row.msom"
    h.save_state(p, constants=True)
    return [p.read_bytes()]


def load_call(h, rng, ctx):
    """the state the handle holds, saved and loaded back: the values stay, every cache goes"""
    p = ctx.tmp / "row.msom"
    h.save_state(p)
    h.load_state(p)
    return []


SAVE_ROW = cs.Row("state_save", ["msom_state_save"], save_call, True, cs.BOTH, False, None, None, None, None, (True, False), False)
LOAD_ROW = cs.Row("state_load", ["msom_state_load"], load_call, False, cs.BOTH, False, None, None, None, None, (True, False), False)


@gpu
@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("grid", cs.BOTH)
@pytest.mark.parametrize("row", [SAVE_ROW, LOAD_ROW], ids=["save", "load"])
def test_rows_cached_equals_plain(row, grid, strict, tmp_path):
    for form in cs.FORMS:
        a, ra = cs.run_gpu(row, grid, strict, CACHED, form, 1e-3, tmp_path)
        b, rb = cs.run_gpu(row, grid, strict, PLAIN, form, 1e-3, tmp_path)
        same(a, b)
        if row is SAVE_ROW:
            da, db = (read_state_bytes(x[0], tmp_path) for x in (ra, rb))
            for k in da["records"]:     # record by record first, so that a failure names the record
                assert np.array_equal(da["records"][k], db["records"][k], equal_nan=True), k
            assert ra[0] == rb[0], "the files of the CACHED and the PLAIN run differ"
        # both rows leave the values alone: the run equals the CACHED run without any call (for the load, because what it loads is what
        # the handle held)
        assert a[0][3][0] == 1, a[0][3]
        same(a, cs.untouched(row, grid, strict, form, tmp_path))


def read_state_bytes(b, tmp_path):
    p = tmp_path / "bytes.msom"
    p.write_bytes(b)
    return read_state(p)


@gpu
@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("grid", cs.BOTH)
def test_load_sends_the_next_solve_back_to_the_residual_pass(grid, strict, tmp_path):
    counts = {}
    for name, call in (("nothing", lambda g: None), ("save", lambda g: g.save_state(tmp_path / "a.msom")),
                       ("load", lambda g: (g.save_state(tmp_path / "b.msom"), g.load_state(tmp_path / "b.msom")))):
        g = cs.gpu_handle(grid, strict, CACHED, 1e-3, profile=1)
        assert g.param("rhs_resid") == 1
        g.step()
        g.profile_reset()
        g.step()
        call(g)
        g.step()
        g.sync()
        counts[name] = {k: g.profile_read(k)[1] for k in ("resid_restrict", "rhs")}
        assert g.mgstats().i == 1
        g.close()
    assert counts["nothing"] == counts["save"] == dict(resid_restrict=0, rhs=4), counts
    assert counts["load"]["resid_restrict"] >= 1 and counts["load"]["rhs"] == 4, counts


# ------------------------------------------------------------------ 3. digest and layout

# every small shape on both builds; and, on one build, the smallest at which a layer does not fit one staging chunk of 4 Mi doubles:
# 4096 wide, so 1024 rows a chunk and two chunks for the 2048 rows of the layer
LAYOUT_SHAPES = [(nx, ny, nl, strict) for strict in BUILDS for nl in (1, 2, 3) for nx, ny in ((16, 16), (32, 16), (64, 32), (128, 64))]
LAYOUT_SHAPES.append((4096, 2048, 1, False))


@gpu
@pytest.mark.parametrize("nx,ny,nl,strict", LAYOUT_SHAPES)
def test_digest_and_layout(nx, ny, nl, strict, tmp_path):
    g = QG(params(nx, ny, nl), strict=strict)
    g.option("quiet", 1)
    psi = rng_field(7, (nl, ny, nx))
    g.set(F["PSI"], psi)
    g.set_const()
    q = g.get(F["Q"])
    p = tmp_path / "d.msom"
    g.save_state(p, constants=True)
    d = read_state(p)                      # verifies every digest against the numpy restatement
    assert state_check(p) == len(d["records"])
    assert (d["nx"], d["ny"], d["nl"], d["dialect"]) == (nx, ny, nl, 0) and d["params"] == params(nx, ny, nl)
    assert np.array_equal(d["records"]["psi"], psi) and np.array_equal(d["records"]["q"], q)
    assert d["digests"]["psi"] == digest(g.get(F["PSI"])) and d["digests"]["q"] == digest(q)
    assert d["records"]["rd"].shape == (1, ny, nx) and d["records"]["dh"].shape == (nl,)
    # a device copy that changes between the upload and the device digest is refused, wherever the element lies, and the handle keeps
    # its fields; psi is the first field record
    assert list(d["records"]).index("psi") < list(d["records"]).index("q")
    for element in (0, nx * ny // 2 + 3, nx * ny - 1):
        g.state_dbg_flip(element)
        with pytest.raises(MsomError, match="error -2.*psi.*the device holds"):
            g.load_state(p)
        assert np.array_equal(g.get(F["PSI"]), psi) and np.array_equal(g.get(F["Q"]), q)
    g.load_state(p)                        # the aid is spent: the same file loads
    assert np.array_equal(g.get(F["PSI"]), psi) and np.array_equal(g.get(F["Q"]), q)
    g.close()
    h = QG(params(nx, ny, nl), strict=strict)   # and a handle that has nothing but the file
    h.option("quiet", 1)
    h.load_state(p)
    assert np.array_equal(h.get(F["PSI"]), psi) and np.array_equal(h.get(F["Q"]), q)
    h.close()


# ------------------------------------------------------------------ 4. refusals

def saved_file(tmp_path, name, grid, extra="", opts=None, newqg=False):
    p = tmp_path / name
    if newqg:
        g = nq_handle(0.0, True)
    else:
        g = Case(grid, extra, opts).make(True)
        g.set(F["PSI"], orc.synthetic_psi(grid[2], grid[1], grid[0]))
    g.set_const()
    g.save_state(p)
    g.close()
    return p


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_refusals_leave_the_handle_as_it_was(strict, tmp_path):
    grid = (32, 32, 2)
    c = Case(grid)
    ref = run_refusal(c, strict, None)
    good = saved_file(tmp_path, "good.msom", grid)
    b = bytearray(good.read_bytes())
    config = {"other_N": saved_file(tmp_path, "n.msom", (64, 64, 2)), "other_Ny": saved_file(tmp_path, "ny.msom", (32, 16, 2)),
              "other_nl": saved_file(tmp_path, "nl.msom", (32, 32, 3)),
              "other_nptr": saved_file(tmp_path, "ptr.msom", grid, "nptr = 1\nptr_r = [10]\nPe = [200]\n"),
              "other_dialect": saved_file(tmp_path, "nq.msom", None, newqg=True),
              "other_flags": saved_file(tmp_path, "st.msom", grid, "tr_stoch = 50\namp_stoch = 1e-5\n", dict(stochastic=1, noise_mode=1)),
              "mode_pv_invert": saved_file(tmp_path, "mo.msom", grid, "", dict(mode_pv_invert=1))}
    io = {}
    for name, data in (("flipped_byte", flip(b, len(b) - 16 - 8 * 100)), ("truncated", b[:len(b) // 2]), ("bad_magic", b"X" + bytes(b[1:])),
                       ("version_2", bytes(b[:8]) + b"\x02" + bytes(b[9:]))):
        io[name] = tmp_path / f"{name}.msom"
        io[name].write_bytes(bytes(data))
    io["missing"] = tmp_path / "nope.msom"
    for files, code in ((config, MSOM_ERR_CONFIG), (io, MSOM_ERR_IO)):
        for name, p in files.items():
            def call(g, p=p, code=code, name=name):
                with pytest.raises(MsomError, match=f"error {code}: .+") as e:
                    g.load_state(p)
                assert name != "flipped_byte" or "the device holds" in str(e.value)   # the host walks the structure, the device the payloads
            same_run(ref, run_refusal(c, strict, call))
    # a file whose payload and digest disagree in one element is refused by the host checker too
    with pytest.raises(MsomError, match="error -2"):
        state_check(io["flipped_byte"])


def flip(b, at):
    x = bytearray(b)
    x[at] ^= 0x04
    return x


def run_refusal(c, strict, call):
    g = c.make(strict, CACHED)
    c.setup(g)
    dts = [g.step()]
    if call:
        call(g)
    dts.append(g.step())
    out = c.snap(g, dts)
    g.close()
    return out


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_rand_stream_noise_cannot_be_saved(strict, tmp_path):
    c = Case((32, 32, 2), "tr_stoch = 50\namp_stoch = 1e-5\n", opts=dict(stochastic=1, noise_mode=0, seed=5), pre=stoch_pre)

    def call(g):
        with pytest.raises(MsomError, match="error -3: .*noise_mode = 1"):
            g.save_state(tmp_path / "r.msom")
        assert not (tmp_path / "r.msom").exists() and not (tmp_path / "r.msom.tmp").exists()

    same_run(run_refusal(c, strict, None), run_refusal(c, strict, call))


# ------------------------------------------------------------------ 5. golden

@gpu
@pytest.mark.parametrize("how", ["load_state", "from_state"])
def test_golden_file_continues_to_the_oracle(how):
    txt = orc.double_gyre_params(32, 3)
    o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1)
    o.set(orc.PSI, orc.synthetic_psi(3, 32, 32))
    o.set_const()
    dts = []
    for _ in range(6):
        o.step()
        dts.append(o.dt)
    if how == "from_state":
        g = from_state(GOLDEN, strict=True)
        g.option("quiet", 1)
    else:
        g = QG(txt, strict=True)
        g.option("quiet", 1)
        g.load_state(GOLDEN)
    assert g.iter == 3
    got = [g.step() for _ in range(3)]
    assert got == dts[3:] and g.t == o.t and g.iter == 6
    assert np.array_equal(g.get(F["Q"]), o.get(orc.Q)) and np.array_equal(g.get(F["PSI"]), o.get(orc.PSI))
    st, so = g.mgstats(), o.mgstats()
    assert (st.i, st.resb, st.resa, st.nrelax) == (so.i, so.resb, so.resa, so.nrelax)
    g.close()


# ------------------------------------------------------------------ 6. tiles

TP = dict(px=2, py=2)
TGRID = (64, 64, 2)


def tiled_params():
    return orc.double_gyre_params(64, 2, extra="MGLEVELS = 5\n")     # the levels a 32 x 32 tile has, on one tile too


def tile_of(a, rank, px=2, py=2):
    ty, tx = a.shape[1] // py, a.shape[2] // px
    iy, ix = rank // px, rank % px
    return a[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx]


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_tiled_resume_is_exact(strict, tmp_path):
    psi = orc.synthetic_psi(2, 64, 64)
    a = run_tiled(tiled_params(), 2, 2, psi, 6, strict)
    p = tmp_path / "tiles.msom"
    run_tiled(tiled_params(), 2, 2, psi, 3, strict, fn=lambda g, rank: g.save_state(p, constants=True))
    assert state_check(p) > 0 and not os.path.exists(str(p) + ".tmp")
    # new handles; their own psi is another one, the file's replaces it
    b = run_tiled(tiled_params(), 2, 2, 0.5 * psi, 3, strict, pre=lambda g, rank: g.load_state(p))
    for k in ("q", "psi"):
        assert np.array_equal(assemble(a, k, 2, 2), assemble(b, k, 2, 2)), k
    for r in range(4):
        assert a[r]["dts"][3:] == b[r]["dts"] and a[r]["t"] == b[r]["t"]
        assert cs.mg(a[r]["st"]) == cs.mg(b[r]["st"])


@gpu
@pytest.mark.parametrize("strict", BUILDS)
def test_a_file_does_not_know_its_tiling(strict, tmp_path):
    psi = rng_field(71, (2, 64, 64))
    qf = rng_field(72, (2, 64, 64))
    pt, p1 = tmp_path / "tiles.msom", tmp_path / "one.msom"

    def set_and_save(path):
        def fn(g, rank):
            g.set(F["Q"], tile_of(qf, rank) if g.tile[0] > 1 else qf)
            g.save_state(path, constants=True)
        return fn

    run_tiled(tiled_params(), 2, 2, psi, 0, strict, fn=set_and_save(pt))
    g = QG(tiled_params(), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    set_and_save(p1)(g, 0)
    dt, d1 = read_state(pt), read_state(p1)
    assert list(dt["records"]) == list(d1["records"]) and dt["digests"] == d1["digests"]
    for k in dt["records"]:
        assert dt["records"][k].shape == d1["records"][k].shape and np.array_equal(dt["records"][k], d1["records"][k], equal_nan=True), k
    assert np.array_equal(d1["records"]["psi"], psi) and np.array_equal(d1["records"]["q"], qf)
    # the 2 x 2 file on one tile
    g.set(F["Q"], 0 * qf)
    g.load_state(pt)
    assert np.array_equal(g.get(F["PSI"]), psi) and np.array_equal(g.get(F["Q"]), qf)
    g.close()
    # the one-tile file on 2 x 2
    out = run_tiled(tiled_params(), 2, 2, 0.5 * psi, 0, strict, pre=lambda g, rank: g.load_state(p1))
    assert np.array_equal(assemble(out, "psi", 2, 2), psi) and np.array_equal(assemble(out, "q", 2, 2), qf)


# ------------------------------------------------------------------ 7. driver

def i_lines(out):
    return re.findall(r"^i = .*$", out, flags=re.M)


def dir_bytes(d):
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


@gpu
def test_driver_checkpoint_and_resume(tmp_path):
    N, nl = 32, 3
    txt = orc.double_gyre_params(N, nl).replace("tend  = 500.", "tend = 0.06").replace("dtout = 1.", "dtout = 0.02")
    o = orc.Oracle(txt, smoother=orc.GS_RB, quiet=1)
    o.set(orc.PSI, orc.synthetic_psi(nl, N, N) + 2e-4)
    outs = {}
    for name, runs in (("A", [["params.in"]]), ("B", [["params.in", "5", "ckpt_steps=5"], ["params.in", "-1", "resume=1"]])):
        d = tmp_path / name
        d.mkdir()
        (d / "params.in").write_text(txt)
        assert o.write_bas(orc.PSI, str(d / "p0.bas")) == 0
        outs[name] = []
        for args in runs:      # one after the other; the first failure ends the test
            res = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=120)
            assert res.returncode == 0, res.stdout + res.stderr
            outs[name].append(res.stdout)
    a, b = tmp_path / "A", tmp_path / "B"
    assert not (a / "state.msom").exists()                      # neither option: no checkpoint
    assert (b / "state.msom").exists() and not (b / "state.msom.tmp").exists()
    assert state_check(b / "state.msom") > 0 and read_state(b / "state.msom")["iter"] == 5
    assert sorted(os.listdir(b)) == sorted(os.listdir(a) + ["state.msom"])     # no second output directory
    fa, fb = dir_bytes(a / "outdir_0001"), dir_bytes(b / "outdir_0001")
    assert list(fa) == list(fb) and len(fa) > 10
    for f in fa:
        assert fa[f] == fb[f], f
    la, lb = i_lines(outs["A"][0]), i_lines(outs["B"][0]) + i_lines(outs["B"][1])
    assert len(la) == 13 and la == lb
    assert "Backup config" in outs["B"][0] and "Backup config" not in outs["B"][1] and "Resuming from" in outs["B"][1]
    # resume = 1 with no checkpoint starts normally
    c = tmp_path / "C"
    c.mkdir()
    (c / "params.in").write_text(txt)
    assert o.write_bas(orc.PSI, str(c / "p0.bas")) == 0
    res = subprocess.run([EXE, "params.in", "2", "resume=1"], cwd=c, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and i_lines(res.stdout) == la[:3] and "Backup config" in res.stdout
