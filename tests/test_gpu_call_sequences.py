"""Every entry point of the layered model between two steps, against a run that shares none of the state a handle keeps across calls.

msom_step keeps state alive that it used to recompute ("State a handle keeps across calls"): the first residual of the next solve
that the tendency pass left behind (res_ready with res[0], res[1], SC_RESF, partial_rr), the spare q buffer, a last tendency pass that is still
running when the step returns, captured graphs, wv_ready, the modes with the modal solver's coarse iBu, the spectrum work arrays.  A call
that forgets to drop or to wait for one of them does not crash: the next solve opens with a residual of other data, takes its one cycle and
returns a psi that is slightly wrong.  So every call is played between steps of two configurations of the same run,

  CACHED  rhs_resid = 1, async_solve = 1, step_sync = 0    (by-product handed from step to step, lazy steps)
  PLAIN   rhs_resid = 0, async_solve = 0, step_sync = 1    (nothing cached, every step synchronised)

which give the same bits in both builds when nothing is called in between (test_gpu_rhs_resid.py).  ROWS is the table: one row per entry
point of include/msom.h that takes a msom_t *, a small function call(h, rng, ctx) -> returned values plus a declaration.  Each row runs as
`step, step, CALL, step, step` (two steps queued with nothing read in between: the call meets a lazy stream) and as `step, CALL, step`:

  1. both builds: CACHED against PLAIN with the same call -- psi, q, every dt, t and (i, resb, resa, nrelax) bit for bit, mgstats().sum to
     rel 1e-12 (its summation order differs), everything the call returned bit for bit (arrays, scalars, files byte for byte: what
     catches a call that read before the lazy pass had finished);
  2. pure rows (the header says the call changes nothing the next step reads), both builds: CACHED with the call equals CACHED without it;
  3. strict build, rows with a twin in orc.Oracle: CACHED against the oracle making the same sequence, at TOLERANCE 1e-3 (one cycle per
     solve: the speculative passes are accepted and the by-product is handed on) and 1e-7 (several cycles, nrelax adapts, the speculative
     pass is discarded); (i, resb, resa, nrelax) bit for bit as the other oracle tests compare them, sum to rel 1e-12;
  4. liveness: without a call the CACHED run launches no pre-cycle residual pass after the first step, with a mutating call it does.
Random sequences of rows (fixed seeds) follow.  test_every_entry_point_has_a_row needs no GPU and is the one test here without the gpu
mark, so that the CPU suite runs it: a new entry point of the header must get a row or an exemption with a reason.

Where the rows depart from the list they were written from, because the code says otherwise:
  * pystep_de, comp_q and pyp2q are mutating rows: pystep_de uploads the caller's psi, recomputes q from it and leaves MSOM_PSI zeroed
    (filter_de with po_mft = pol); msom_comp_q / pyp2q upload into MSOM_PSI and write MSOM_Q, and the header promises nothing else;
  * .bas files need a square grid (msom_write_bas / msom_read_bas answer MSOM_ERR_STATE otherwise): write_bas, read_bas, read_inputs and
    run play on 128 x 128 x 2, the 128 x 64 x 2 grid with more rows;
  * the chained smoother needs a level of 512 x 64 cells: the march switches and the march* kernels of msom_bench_kernel play on
    512 x 64 x 2, the smallest grid on which relax_path_0 can move to 3 (asserted); on the two small grids they would test nothing;
  * uniform_S, the march switches (which need uniform_S = 1 in the strict build) and mode_pv_invert are compared CACHED against PLAIN only:
    the oracle has the general column solver and no modal inversion, and the header lists uniform_S and mode_pv_invert outside the
    result-preserving switches.

No sequence is repeated: a race that does not show in one run is not found by this file.
The file runs in about 34 s on an MI355X (635 cases, none above 0.4 s)."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

import orc
from msom_amd import FIELDS as F, MODES, STATS
from msom_amd.api import MGStats
from test_cabi_host import declared_symbols
from test_gpu_rhs_resid import handle, params, same

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CACHED = dict(rhs_resid=1, async_solve=1, step_sync=0)
PLAIN = dict(rhs_resid=0, async_solve=0, step_sync=1)
G2, G5, GSQ, GM = (128, 64, 2), (256, 64, 5), (128, 128, 2), (512, 64, 2)
EVERY, BOTH = (G2,), (G2, G5)
BUILDS = [True, False]
FORMS = ("lazy", "short")     # step, step, CALL, step, step / step, CALL, step
EXTRA = "afilt = 4\ndtflt = 0.25\nediag = 0\n"   # the wavelet filter and the budgets have what they need; no step reads these keys
SEED = 20251019
# implementation switches: the oracle makes no call
DEFAULTS = dict(fused=1, adv_fused=1, rhs_variant=6, mg_fused=1, prolong_fused=1, mg_coarse=4, restrict2=1, restrict_pyr=1, march=1, march_min=23,
                march_k=4, march_prolong=1, march_correct=1, block8=1, block_sweeps=0, uniform_S=-1, graph=0, mode_pv_invert=0)


# ------------------------------------------------------------------ the two kinds of handle

class OracleHandle:
    """orc.Oracle behind the part of QG's surface the rows use (same field ids, same argument order)"""
    is_gpu = False

    def __init__(self, o):
        self.o = o
        self.nl, self.ny, self.nx = o.nl, o.ny, o.nx
        for k in ("set", "get", "remove_mean", "set_const", "set_tnext", "param", "wavelet_filter", "wavelet_apply", "energy_tend", "filter_de",
                  "reset_de", "write_bas", "mgstats"):
            setattr(self, k, getattr(o, k))

    t = property(lambda self: self.o.t)

    def step(self):
        self.o.step()
        return self.o.dt

    def option(self, key, v):
        if key not in DEFAULTS and key not in CACHED:
            self.o.option(key, v)

    def read_bas(self, field, path):
        assert self.o.read_bas(field, path) == 0

    def invertq(self, q=None, psi0=None):
        if q is not None:
            self.o.set(orc.QPRED, q)
        if psi0 is not None:
            self.o.set(orc.PSI, psi0)
        st = self.o.invertq(orc.PSI, orc.Q if q is None else orc.QPRED)
        return self.o.get(orc.PSI), st

    def update(self, q=None, dtmax=None):
        if q is not None:
            self.o.set(orc.QPRED, q)
        d = self.o.update(orc.Q if q is None else orc.QPRED, orc.DQ, dtmax)
        return self.o.get(orc.DQ), d

    def advance(self, qin, dqdt, dt):
        if qin is not None:
            self.o.set(orc.QPRED, qin)
        self.o.set(orc.DQ, dqdt)
        f = orc.Q if qin is None else orc.QPRED
        self.o.advance(f, f, orc.DQ, dt)
        return self.o.get(f)

    def pystep_bfn(self, var, tend, direction=1.0, vartype=1):
        tend[:] = self.o.pystep_bfn(var, direction, vartype)

    def pyq2p(self, p, q):
        p[:] = self.o.pyq2p(q)

    def pyp2q(self, p, q):
        q[:] = self.o.pyp2q(p)

    def comp_q(self, psi):
        self.o.set(orc.PSI, psi)
        self.o.comp_q()
        return self.o.get(orc.Q)

    def pystep_de(self, po, bf, vd, j1, j2, j3, ft, onlyKE=0):
        for dst, src in zip((bf, vd, j1, j2, j3, ft), self.o.pystep_de(po, onlyKE)):
            dst[:] = src

    def close(self):
        self.o = None


def gpu_handle(grid, strict, conf, tol, hopts=None, **more):
    g = handle(*grid, strict, conf["rhs_resid"], extra=EXTRA, tol=tol, async_solve=conf["async_solve"], step_sync=conf["step_sync"], **more)
    for k, v in (hopts or {}).items():
        g.option(k, v)
    g.is_gpu = True
    return g


def oracle_handle(grid, tol):
    nx, ny, nl = grid
    o = orc.Oracle(params(nx, ny, nl, EXTRA), smoother=orc.GS_RB, quiet=1, TOLERANCE=tol)
    o.set(orc.PSI, orc.synthetic_psi(nl, ny, nx))
    o.set_const()
    return OracleHandle(o)


def state(h, dts):
    """what the steps return, in the layout test_gpu_rhs_resid.same compares; t rides at the end of the dt list"""
    st = h.mgstats()
    return h.get(F["PSI"]), h.get(F["Q"]), list(dts) + [h.t], (st.i, st.resb, st.resa, st.nrelax), st.sum


def same_returned(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y, equal_nan=True), f"{what}: returned value {k}"
        else:
            assert x == y, f"{what}: returned value {k}: {x!r} / {y!r}"


def noisy(a, rng, eps=0.05):
    """the field plus noise of its own magnitude: no symmetry left for a swapped neighbour to hide behind"""
    return a + eps * a.std() * rng.standard_normal(a.shape)


def like(h, rng, scale=1.0, layers=None):
    return scale * rng.standard_normal((h.nl if layers is None else layers, h.ny, h.nx))


def mg(st):
    return (st.i, st.resb, st.resa, st.nrelax)


# ------------------------------------------------------------------ the table

class Row:
    def __init__(self, name, syms, call, pure, grids, oracle, setup, early, undo, hopts, builds, random):
        self.name, self.syms, self.call, self.pure, self.grids, self.oracle = name, tuple(syms), call, pure, grids, oracle
        self.setup, self.early, self.undo, self.hopts, self.builds, self.random = setup, early, undo, hopts, builds, random


ROWS = {}


def row(name, syms, pure, grids=EVERY, oracle=False, setup=None, early=None, undo=None, hopts=None, builds=(True, False), random=True):
    """hopts: options set on the handle before the first step (both configurations, and the run without the call); a callable takes `strict`.
    random: the row may be drawn into a random sequence (not one whose call needs the handle as the steps leave it)"""
    def deco(fn):
        assert name not in ROWS
        ROWS[name] = Row(name, syms, fn, pure, grids, oracle, setup, early, undo, hopts, builds, random)
        return fn
    return deco


# ---- pure rows

@row("nothing", ["msom_step"], True, BOTH, oracle=True)
def _(h, rng, ctx):
    return []


@row("get", ["msom_get_field", "msom_field_layers"], True, BOTH, oracle=True)
def _(h, rng, ctx):
    if not h.is_gpu:
        return [h.get(f) for f in (F["PSI"], F["Q"], F["DQ"], F["QPRED"])]
    out = [h.L.msom_field_layers(h.h, f) for f in range(len(F))]
    for f in range(len(F)):     # every allocated field; QOF and the ids from DE_BF on (nl layers each) are allocated by the first get
        if out[f] > 0 or f == F["QOF"] or f >= F["DE_BF"]:
            a = np.empty((out[f] if out[f] > 0 else h.nl, h.ny, h.nx))
            assert h.L.msom_get_field(h.h, f, a.ctypes.data_as(C.c_void_p)) == 0, f
            out.append(a)
    return out


@row("param", ["msom_get_param"], True)
def _(h, rng, ctx):
    return [h.param(k) for k in ("N", "ny", "nl", "DT", "TOLERANCE", "nlevels", "relax_path_0", "relax_path_1", "march_levels", "uniform_S", "split_pad")]


@row("ke", ["msom_ke"], True, BOTH)
def _(h, rng, ctx):
    return [h.ke()]


@row("mgstats", ["msom_last_mgstats"], True)
def _(h, rng, ctx):
    return [mg(h.mgstats())]


@row("t_iter", ["msom_time", "msom_iter"], True)
def _(h, rng, ctx):
    return [h.t, h.iter]


@row("sync", ["msom_sync"], True)
def _(h, rng, ctx):
    h.sync()
    return []


@row("profile_read", ["msom_profile_read"], True)
def _(h, rng, ctx):
    return [h.profile_read(k)[1] for k in ("sweep", "march_visit", "helm_relax")]   # slots that count the same in both configurations


@row("profile_reset", ["msom_profile_reset"], True)
def _(h, rng, ctx):
    h.profile_reset()
    return []


@row("tile_info", ["msom_tile_info"], True)
def _(h, rng, ctx):
    v = [C.c_int() for _ in range(6)]
    assert h.L.msom_tile_info(h.h, *(C.byref(x) for x in v)) == 0
    return [x.value for x in v]


@row("levels", ["msom_dbg_nlevels", "msom_dbg_level_dims"], True)
def _(h, rng, ctx):
    return [h.nlevels()] + [h.level_dims(k) for k in range(h.nlevels())]


@row("wavelet_levels_siglev", ["msom_dbg_wavelet_levels", "msom_dbg_siglev"], True)
def _(h, rng, ctx):
    return [h.wavelet_levels(), h.siglev(0), h.siglev(2)]


ST_MASK = sum(1 << STATS[k] for k in ("PSI", "Q", "KE", "UQ"))


def stats_setup(h, rng, ctx):
    h.stats_begin(ST_MASK)


@row("stats_begin", ["msom_stats_begin"], True)
def _(h, rng, ctx):
    h.stats_begin(ST_MASK)
    return [h.param("stats_mask")]


@row("stats_accumulate_weight", ["msom_stats_accumulate", "msom_stats_weight"], True, BOTH, setup=stats_setup)
def _(h, rng, ctx):
    h.stats_accumulate(0.25)
    return [h.stats_weight()]


@row("stats_get", ["msom_stats_get"], True, BOTH, setup=stats_setup)
def _(h, rng, ctx):
    h.stats_accumulate(0.5)
    return [h.stats_get(STATS["PSI"]), h.stats_get(STATS["UQ"]), h.stats_get(STATS["EKE"])]   # stored ids and a derived one (through MSOM_TMP)


@row("time_filter", ["msom_time_filter"], True, BOTH)
def _(h, rng, ctx):
    h.time_filter(0.1)
    return [h.stats_get(STATS["QME"])]


def modes_setup(h, rng, ctx):
    h.modes_compute()


@row("modes_compute", ["msom_modes_compute"], True, BOTH)
def _(h, rng, ctx):
    h.modes_compute()
    return [h.param("modes_ready")]


@row("modes_get", ["msom_modes_get", "msom_modes_layers"], True, setup=modes_setup)
def _(h, rng, ctx):
    return [h.L.msom_modes_layers(h.h, w) for w in range(MODES["N"])] + [h.modes_get(w) for w in range(MODES["N"])]


@row("modes_project", ["msom_modes_project"], True, BOTH, setup=modes_setup)
def _(h, rng, ctx):
    a = like(h, rng)
    return [h.modes_project(a, True), h.modes_project(a, False)]


@row("modes_energy", ["msom_modes_energy"], True, BOTH, setup=modes_setup)
def _(h, rng, ctx):
    return list(h.modes_energy())


@row("modes_set_rd", ["msom_modes_set_rd"], True, setup=modes_setup)
def _(h, rng, ctx):
    h.modes_set_rd(1)
    return [h.get(F["RD"])]


@row("spec_bins_kr", ["msom_spec_bins", "msom_spec_kr"], True)
def _(h, rng, ctx):
    return [h.spec_bins(), h.spec_kr()]


@row("spec_2d", ["msom_spec_2d"], True, BOTH)
def _(h, rng, ctx):
    return [h.spec_2d(like(h, rng), like(h, rng))]


@row("spec_cross", ["msom_spec_cross"], True, BOTH)
def _(h, rng, ctx):
    a, b = like(h, rng), like(h, rng)
    return [h.spec_cross(a, b), h.spec_cross(a, flux=True)]


@row("spec_fields", ["msom_spec_fields"], True, BOTH)
def _(h, rng, ctx):
    return [h.spec_fields(F["PSI"], F["Q"]), h.spec_fields(F["Q"], F["Q"], flux=True)]


@row("spec_energy", ["msom_spec_energy"], True, BOTH)
def _(h, rng, ctx):
    return list(h.spec_energy())


@row("write_bas", ["msom_write_bas"], True, (GSQ,))
def _(h, rng, ctx):
    out = []
    for f in ("PSI", "Q"):
        p = ctx.tmp / f"{f}.bas"
        h.write_bas(F[f], str(p))
        out.append(p.read_bytes())
    return out


@row("write_nc", ["msom_write_nc"], True, BOTH)
def _(h, rng, ctx):
    p = ctx.tmp / "vars.nc"
    h.write_nc(str(p))
    h.write_nc(str(p))    # the second record appends
    return [p.read_bytes()]


@row("energy_tend", ["msom_energy_tend"], True, BOTH, oracle=True)
def _(h, rng, ctx):
    h.energy_tend(0.01)
    return [h.get(F[k]) for k in ("DE_BF", "DE_VD", "DE_J1", "DE_J2", "DE_J3", "PO_MFT")]


@row("reset_de", ["msom_reset_de"], True, oracle=True)
def _(h, rng, ctx):
    h.energy_tend(0.01)
    h.reset_de()
    return [h.get(F["DE_J1"]), h.get(F["PO_MFT"])]


def obs_setup(h, rng, ctx):
    h.set(F["BFN_OBS"], noisy(h.get(F["Q"]), rng))


@row("bfn_misfit", ["msom_bfn_misfit"], True, BOTH, setup=obs_setup)
def _(h, rng, ctx):
    return [h.bfn_misfit()]


# ---- pure rows: hooks that overwrite named scratch (da[k], res[k], da_alt[0], MSOM_TMP, MSOM_DQ, MSOM_QPRED) and nothing the steps return

def level_arrays(h, rng, lev):
    lx, ly = h.level_dims(lev)
    return rng.standard_normal((h.nl, ly, lx)), rng.standard_normal((h.nl, ly, lx))


@row("dbg_relax", ["msom_dbg_relax"], True, BOTH)
def _(h, rng, ctx):
    return [h.relax(lev, *level_arrays(h, rng, lev), 2) for lev in (0, 1, h.nlevels() - 1)]


@row("dbg_residual", ["msom_dbg_residual"], True, BOTH)
def _(h, rng, ctx):
    return list(h.residual(like(h, rng), like(h, rng)))


@row("dbg_restrict", ["msom_dbg_restrict"], True, BOTH)
def _(h, rng, ctx):
    return [h.restrict(lev, level_arrays(h, rng, lev)[0]) for lev in (0, 1)]


@row("dbg_prolong", ["msom_dbg_prolong"], True, BOTH)
def _(h, rng, ctx):
    return [h.prolong(lev, level_arrays(h, rng, lev)[0]) for lev in (1, 2)]


@row("dbg_op_del2", ["msom_dbg_op"], True, BOTH)
def _(h, rng, ctx):
    h.op("del2", F["PSI"], F["TMP"], 0.0, 1.0)
    return [h.get(F["TMP"])]


@row("dbg_op_stretch", ["msom_dbg_op"], True, BOTH)
def _(h, rng, ctx):
    h.op("stretch", F["PSI"], F["TMP"], 0.0, 1.0)
    return [h.get(F["TMP"])]


@row("dbg_rhs_resid_fused", ["msom_dbg_rhs_resid"], True, BOTH, random=False)     # needs the fused tendency pass: no topography, fused = 1
def _(h, rng, ctx):
    return list(h.dbg_rhs_resid(True, 1e-3)[:3])     # res on levels 0 and 1, max|res|; the sum's order differs between the two


@row("dbg_rhs_resid_plain", ["msom_dbg_rhs_resid"], True, BOTH, random=False)
def _(h, rng, ctx):
    return list(h.dbg_rhs_resid(False, 1e-3)[:3])


@row("dbg_helm_relax", ["msom_dbg_helm_relax"], True, BOTH)
def _(h, rng, ctx):
    return [h.helm_relax(lev, *level_arrays(h, rng, lev), 4) for lev in (0, 1)]


@row("dbg_helm_residual", ["msom_dbg_helm_residual"], True, BOTH)
def _(h, rng, ctx):
    return list(h.helm_residual(like(h, rng), like(h, rng)))


def uniform_in_strict(strict):
    return dict(uniform_S=1) if strict else {}    # the chained smoother exists for the uniform-S column solver (opt-in in the strict build)


# every kernel name msom_bench_kernel takes on a layered handle; march*: on the one grid here where the solver itself may launch them
BENCH = ["sweep", "residual", "advection", "block2", "block2p", "rhs", "resid_correct", "resid_restrict", "red_prolong", "rhs_adv", "advance",
         "modes_project", "modes_energy", "spec_rows", "spec_transpose", "spec_cols", "spec_shells", "helm_sweep", "helm_residual"]
BENCH_MARCH = ["march2", "march3", "march4", "march3r", "march4p"]


def bench_row(kernel):
    def call(h, rng, ctx):
        assert h.bench_kernel(kernel, 1) >= 0.0    # a time: nothing to compare
        return []
    march = kernel in BENCH_MARCH
    row(f"bench_{kernel}", ["msom_bench_kernel"], True, (GM,) if march else (BOTH if kernel in ("rhs_adv", "resid_restrict", "resid_correct") else EVERY),
        setup=modes_setup if kernel.startswith("modes_") else None, hopts=uniform_in_strict if march else None)(call)


for _k in BENCH + BENCH_MARCH:
    bench_row(_k)


# ---- mutating rows: psi, q, S, the time, the limiter or the solver path change

def set_row(name, field, make, grids=BOTH, oracle=True, after=None):
    def call(h, rng, ctx):
        h.set(F[field], make(h, rng))
        if after:
            after(h)
        return [h.get(F[field])]
    row(name, ["msom_set_field"] + (["msom_set_const"] if after else []), False, grids, oracle=oracle)(call)


def fr_random(h, rng):
    return np.stack([h.param(f"Fr_{l}") * (1 + 0.3 * rng.uniform(-1, 1, (h.ny, h.nx))) for l in range(h.nl - 1)])


set_row("set_psi", "PSI", lambda h, rng: noisy(h.get(F["PSI"]), rng))
set_row("set_q", "Q", lambda h, rng: noisy(h.get(F["Q"]), rng))
set_row("set_qforc", "QFORC", lambda h, rng: like(h, rng, 1e-4))
set_row("set_topo", "TOPO", lambda h, rng: like(h, rng, 0.05, 1), after=lambda h: h.option("flag_topo", 1))
set_row("set_fr_set_const", "FR", fr_random, after=lambda h: h.set_const())


@row("set_const", ["msom_set_const"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    h.set_const()
    return []


@row("remove_mean", ["msom_remove_mean"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    h.remove_mean(F["PSI"])
    return []


@row("invertq", ["msom_invertq"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    psi, st = h.invertq(noisy(h.get(F["Q"]), rng), noisy(h.get(F["PSI"]), rng))
    return [psi, mg(st)]


@row("invertq_in_place", ["msom_invertq"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    if h.is_gpu:      # no caller arrays: MSOM_Q into MSOM_PSI from the psi the handle holds
        st = MGStats()
        assert h.L.msom_invertq(h.h, None, None, C.byref(st)) == 0
    else:
        st = h.invertq()[1]
    return [mg(st)]


@row("update", ["msom_update"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    dq, d = h.update(noisy(h.get(F["Q"]), rng), h.param("DT"))
    return [dq, d]


@row("update_in_place", ["msom_update"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    dq, d = h.update(None, h.param("DT"))
    return [dq, d]


@row("advance", ["msom_advance"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    q = h.get(F["Q"])
    return [h.advance(noisy(q, rng), like(h, rng, q.std()), 1e-3)]


@row("advance_in_place", ["msom_advance"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    dq = like(h, rng, h.get(F["Q"]).std())
    if h.is_gpu:      # no caller q: MSOM_Q = MSOM_Q + dt dq
        assert h.L.msom_advance(h.h, None, None, dq.ctypes.data_as(C.c_void_p), 1e-3) == 0
    else:
        h.advance(None, dq, 1e-3)
    return [h.get(F["Q"])]


def bfn_row(direction):
    def call(h, rng, ctx):
        tend = np.empty((h.nl, h.ny, h.nx))
        h.pystep_bfn(noisy(h.get(F["Q"]), rng), tend, direction, 1)
        return [tend]
    row("pystep_bfn_" + ("forward" if direction > 0 else "backward"), ["pystep_bfn"], False, BOTH, oracle=True)(call)


bfn_row(1.0)
bfn_row(-1.0)     # the signs of iRe, iRe4, Eks, Ekb stay flipped in the handle: the steps that follow run with them


@row("pyq2p", ["pyq2p"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    p = np.empty((h.nl, h.ny, h.nx))
    h.pyq2p(p, noisy(h.get(F["Q"]), rng))
    return [p]


@row("pyp2q", ["pyp2q"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    q = np.empty((h.nl, h.ny, h.nx))
    h.pyp2q(noisy(h.get(F["PSI"]), rng), q)
    return [q]


@row("comp_q", ["msom_comp_q"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    return [h.comp_q(noisy(h.get(F["PSI"]), rng))]


@row("pystep_de", ["pystep_de"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    outs = [np.empty((h.nl, h.ny, h.nx)) for _ in range(6)]
    h.pystep_de(noisy(h.get(F["PSI"]), rng), *outs, 0)
    return outs


@row("bfn_steps", ["msom_bfn_begin", "msom_bfn_steps"], False, BOTH)
def _(h, rng, ctx):
    h.bfn_begin()
    h.bfn_steps(2, 1e-3, 1.0, 0.0)
    return [h.get(F["Q"]), h.get(F["BFN_F2"])]


@row("bfn_steps_nudged", ["msom_bfn_begin", "msom_bfn_steps", "msom_bfn_misfit"], False, BOTH)
def _(h, rng, ctx):
    h.set(F["BFN_OBS"], noisy(h.get(F["Q"]), rng))
    h.bfn_begin()
    h.bfn_steps(2, 1e-3, 1.0, 0.5)
    return [h.get(F["Q"]), h.get(F["BFN_F2"]), h.bfn_misfit()]


def filter_row(dtflt):
    def call(h, rng, ctx):
        h.wavelet_filter(dtflt)
        return [h.get(F["QOF"])]
    row("wavelet_filter_" + ("plus" if dtflt > 0 else "minus"), ["msom_wavelet_filter"], False, BOTH, oracle=True)(call)


filter_row(0.25)
filter_row(-0.25)


@row("wavelet_apply", ["msom_dbg_wavelet_apply"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    h.wavelet_apply(F["PSI"])
    return []


@row("filter_de", ["msom_filter_de"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    h.energy_tend(0.01)
    h.filter_de(F["PO_MFT"], 0.25)
    return [h.get(F["DE_FT"])]


def write_psi_bas(h, rng, ctx):
    h.write_bas(F["PSI"], str(ctx.tmp / "po.bas"))
    return [(ctx.tmp / "po.bas").read_bytes()]


@row("read_bas", ["msom_read_bas", "msom_write_bas"], False, (GSQ,), oracle=True, early=write_psi_bas)
def _(h, rng, ctx):
    h.read_bas(F["PSI"], str(ctx.tmp / "po.bas"))     # the psi of one step earlier, rounded to float
    return []


def write_vars_nc(h, rng, ctx):
    h.write_nc(str(ctx.tmp / "restart.nc"))
    return [(ctx.tmp / "restart.nc").read_bytes()]


@row("read_nc", ["msom_read_nc", "msom_write_nc"], False, BOTH, early=write_vars_nc)
def _(h, rng, ctx):
    h.read_nc(F["PSI"], str(ctx.tmp / "restart.nc"), "psi", -1)
    h.read_nc(F["Q"], str(ctx.tmp / "restart.nc"), "q", 0)
    return []


def write_qforc(h, rng, ctx):
    h.set(F["QFORC"], like(h, rng, 1e-4))
    h.write_bas(F["QFORC"], str(ctx.tmp / f"qforc_{h.nl}l_N{h.nx}.bas"))
    return []


@row("read_inputs", ["msom_read_inputs"], False, (GSQ,), early=write_qforc)
def _(h, rng, ctx):
    h.read_inputs(str(ctx.tmp))     # leaves the handle without set_const: the next step makes it
    return [h.get(F["QFORC"])]


@row("run", ["msom_run"], False, (GSQ,))
def _(h, rng, ctx):
    h.run(str(ctx.tmp), 1)
    out = ctx.tmp / "outdir_0001"
    return [(p.name, p.read_bytes()) for p in sorted(out.iterdir())]


@row("set_tnext", ["msom_set_tnext"], False, BOTH, oracle=True)
def _(h, rng, ctx):
    h.set_tnext(h.t + 0.0371)      # dt is cut to land on it
    return []


# ---- option rows: to another value between two steps and back after the next one

def option_row(name, opts, oracle, grids=BOTH, moved=(), hopts=None, undo_returns=None, builds=(True, False)):
    """opts: key -> value, or key -> function(ctx, base) for the keys whose base value belongs to the configuration.  moved: parameters
    that must report another path after the call on the CACHED handle"""
    def base(h, ctx, key):
        if key in ctx.conf:
            return ctx.conf[key]
        if key == "TOLERANCE":
            return ctx.tol
        if key in DEFAULTS:
            return (ctx.hopts or {}).get(key, DEFAULTS[key])
        return ctx.stash[key]

    def call(h, rng, ctx):
        ctx.stash.update({k: h.param(k) for k in opts if k == "DT"})
        ctx.stash.update(NITERMAX=100, NITERMIN=1)
        watch = moved if h.is_gpu and ctx.conf is CACHED else ()
        before = [h.param(k) for k in watch]
        for k, v in opts.items():
            h.option(k, v(base(h, ctx, k)) if callable(v) else v)
        after = [h.param(k) for k in watch]
        assert all(a != b for a, b in zip(after, before)), f"{name}: {moved} did not all move: {before} -> {after}"
        return []

    def undo(h, rng, ctx):
        out = undo_returns(h) if undo_returns and h.is_gpu else []
        for k in reversed(list(opts)):
            h.option(k, base(h, ctx, k))
        return out
    row(name, ["msom_set_option"], False, grids, oracle=oracle, undo=undo, hopts=hopts, builds=builds)(call)


option_row("opt_TOLERANCE", dict(TOLERANCE=1e-5), True)
option_row("opt_NITERMAX", dict(NITERMAX=2), True)
option_row("opt_NITERMIN", dict(NITERMIN=3), True)
option_row("opt_DT", dict(DT=1e-3), True)
option_row("opt_fused", dict(fused=0), True, moved=("rhs_resid",))
option_row("opt_adv_fused", dict(adv_fused=0), True, moved=("rhs_resid",))
option_row("opt_rhs_variant", dict(rhs_variant=1), True)
option_row("opt_rhs_resid", dict(rhs_resid=lambda b: 1 - b), True, moved=("rhs_resid",))
option_row("opt_mg_fused", dict(mg_fused=0), True, moved=("rhs_resid",))
option_row("opt_prolong_fused", dict(prolong_fused=0), True)
option_row("opt_mg_coarse_0", dict(mg_coarse=0), True, moved=("relax_path_3",))     # level 3: 16 or 32 cells wide, in the coarse group by default
option_row("opt_mg_coarse_2", dict(mg_coarse=2), True, moved=("mg_coarse_lean",), builds=(False,))
option_row("opt_mg_coarse_2_restrict2", dict(mg_coarse=2, restrict2=0), True, moved=("restrict2",))
option_row("opt_restrict2", dict(restrict2=0), True, moved=("restrict2",))
option_row("opt_restrict_pyr", dict(restrict_pyr=0), True)
option_row("opt_block8", dict(block8=0), True, moved=("relax_path_0",))
option_row("opt_block_sweeps", dict(block_sweeps=1), True, moved=("relax_path_0",))
option_row("opt_graph", dict(graph=1), True)
option_row("opt_async_solve", dict(async_solve=lambda b: 1 - b), True)
option_row("opt_step_sync", dict(step_sync=lambda b: 1 - b), True)
option_row("opt_async_solve_fused", dict(async_solve=lambda b: 1 - b, fused=0), True, moved=("rhs_resid",))
option_row("opt_reference_chain", dict(march=0, block8=0, fused=0, mg_fused=0, mg_coarse=0, prolong_fused=0, adv_fused=0), True,
           moved=("relax_path_0", "relax_path_3", "rhs_resid"))     # REFERENCE_CHAIN of test_gpu_fullsize.py
# not against the oracle: it has the general column solver only, and no modal inversion
option_row("opt_uniform_S", dict(uniform_S=lambda b: 0), False, moved=("uniform_S",), builds=(False,))
option_row("opt_uniform_S_on", dict(uniform_S=lambda b: 1), False, moved=("uniform_S",), builds=(True,))
option_row("opt_mode_pv_invert", dict(mode_pv_invert=1), False, moved=("rhs_resid",),
           undo_returns=lambda h: [mg(h.modes_mgstats(m)) for m in range(h.nl)])
ROWS["opt_mode_pv_invert"].syms += ("msom_modes_mgstats",)
# the chained smoother: a level of 512 x 64 cells at least, uniform S
option_row("opt_march_2", dict(march=2), False, (GM,), moved=("relax_path_0", "march_levels"), hopts=uniform_in_strict)
option_row("opt_march_min", dict(march_min=16), False, (GM,), moved=("relax_path_0", "march_levels"), hopts=uniform_in_strict)
for _key, _v, _moved in (("march_k", 3, ("march_kmax",)), ("march_k", 2, ("march_kmax",)), ("march_prolong", 0, ()), ("march_correct", 0, ())):
    option_row(f"opt_{_key}_{_v}", {_key: _v}, False, (GM,), moved=_moved, hopts=lambda strict: dict(uniform_in_strict(strict), march=2))
option_row("opt_march_off", dict(march=0), False, (GM,), moved=("relax_path_0",), hopts=lambda strict: dict(uniform_in_strict(strict), march=2))


# ------------------------------------------------------------------ completeness (no GPU)

EXEMPT = {
    "msom_destroy": "ends the handle: nothing follows it",
}
# entry points without a handle argument are outside the table by construction; named here so that the reading of the header is checked
NO_HANDLE = {"msom_last_error", "msom_version", "msom_create", "msom_create_str", "msom_create_newqg", "msom_create_newqg_str", "msom_set_device",
             "msom_comm_unique_id", "msom_create_tiled", "msom_dbg_rccl_selftest", "msom_spec_layout"}


def handle_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "msom.h")).read(), flags=re.S)
    names = declared_symbols()
    takes = {n for n in names if re.search(r"\b" + n + r"\s*\(\s*msom_t\s*\*", txt)}
    return names, takes


def missing_rows(rows):
    names, takes = handle_entry_points()
    assert set(names) - takes == NO_HANDLE, sorted(set(names) - takes ^ NO_HANDLE)
    covered = {s for r in rows.values() for s in r.syms}
    assert covered <= takes, sorted(covered - takes)      # a row names what the header declares
    assert not covered & set(EXEMPT)
    return sorted(takes - covered - set(EXEMPT))


def test_every_entry_point_has_a_row():
    assert missing_rows(ROWS) == []
    # the check bites: without its row an entry point is reported
    assert missing_rows({k: r for k, r in ROWS.items() if k != "remove_mean"}) == ["msom_remove_mean"]


# ------------------------------------------------------------------ playing a row

_runs = [0]


def context(tmp_path, conf, tol, hopts):
    _runs[0] += 1
    d = tmp_path / f"run{_runs[0]}"
    d.mkdir()
    return types.SimpleNamespace(tmp=d, conf=conf, tol=tol, hopts=hopts, stash={})


def play(h, r, form, ctx, with_call=True):
    rng = np.random.default_rng(SEED)
    ret, dts = [], []
    if with_call and r.setup:
        ret += r.setup(h, rng, ctx) or []
    before = 2 if form == "lazy" else 1
    for n in range(before):
        if with_call and r.early and n == before - 1:
            ret += r.early(h, rng, ctx) or []
        dts.append(h.step())
    if with_call:
        ret += r.call(h, rng, ctx) or []
    for n in range(2 if form == "lazy" or r.undo else 1):
        dts.append(h.step())
        if with_call and r.undo and n == 0:
            ret += r.undo(h, rng, ctx) or []
    out = [state(h, dts)]
    h.close()
    return out, ret


def resolve(hopts, strict):
    return hopts(strict) if callable(hopts) else hopts


def run_gpu(r, grid, strict, conf, form, tol, tmp_path, with_call=True):
    hopts = resolve(r.hopts, strict)
    return play(gpu_handle(grid, strict, conf, tol, hopts), r, form, context(tmp_path, conf, tol, hopts), with_call)


_untouched = {}     # the CACHED run without any call, once per (grid, build, form, handle options)


def untouched(r, grid, strict, form, tmp_path):
    key = (grid, strict, form, tuple(sorted((resolve(r.hopts, strict) or {}).items())))
    if key not in _untouched:
        _untouched[key] = run_gpu(r, grid, strict, CACHED, form, 1e-3, tmp_path, with_call=False)[0]
    return _untouched[key]


TABLE = [pytest.param(name, grid, strict, id=f"{name}-{grid[0]}x{grid[1]}x{grid[2]}-{'strict' if strict else 'product'}")
         for name, r in ROWS.items() for grid in r.grids for strict in BUILDS if strict in r.builds]


@gpu
@pytest.mark.parametrize("name,grid,strict", TABLE)
def test_cached_equals_plain(name, grid, strict, tmp_path):
    r = ROWS[name]
    for form in FORMS:
        a, ra = run_gpu(r, grid, strict, CACHED, form, 1e-3, tmp_path)
        b, rb = run_gpu(r, grid, strict, PLAIN, form, 1e-3, tmp_path)
        same(a, b)
        same_returned(ra, rb, f"{name} {form}")
        if r.pure:
            assert a[0][3][0] == 1, a[0][3]    # one cycle per solve: the speculative passes are accepted (the state under test)
            same(a, untouched(r, grid, strict, form, tmp_path))


ORACLE_TABLE = [pytest.param(name, grid, tol, id=f"{name}-{grid[0]}x{grid[1]}x{grid[2]}-tol{tol:g}")
                for name, r in ROWS.items() if r.oracle and True in r.builds for grid in r.grids for tol in (1e-3, 1e-7)]


@gpu
@pytest.mark.parametrize("name,grid,tol", ORACLE_TABLE)
def test_strict_cached_equals_oracle(name, grid, tol, tmp_path):
    r = ROWS[name]
    for form in FORMS:
        a, ra = run_gpu(r, grid, True, CACHED, form, tol, tmp_path)
        b, rb = play(oracle_handle(grid, tol), r, form, context(tmp_path, CACHED, tol, None))
        same(a, b)
        if name != "get":     # the oracle row reads fewer fields
            same_returned(ra, rb, f"{name} {form}")
        if tol == 1e-7 and r.pure:
            assert a[0][3][0] > 1, a[0][3]     # several cycles: the speculative pass was discarded


@gpu
@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("grid", BOTH)
def test_the_cache_is_live(grid, strict):
    """without this nothing above tests the cache: the by-product really opens the solves of an untouched CACHED run, and a mutating call
    really sends the next solve back to the residual pass"""
    counts = {}
    for name in ("nothing", "set_q"):
        g = gpu_handle(grid, strict, CACHED, 1e-3, profile=1)
        assert g.param("rhs_resid") == 1
        g.step()
        g.profile_reset()
        g.step()
        ROWS[name].call(g, np.random.default_rng(SEED), None)
        g.step()
        g.sync()
        counts[name] = {k: g.profile_read(k)[1] for k in ("resid_restrict", "rhs")}
        assert g.mgstats().i == 1
        g.close()
    assert counts["nothing"] == dict(resid_restrict=0, rhs=4), counts
    assert counts["set_q"]["resid_restrict"] >= 1 and counts["set_q"]["rhs"] == 4, counts


# ------------------------------------------------------------------ random sequences

def drawable(r, grid, strict, need_oracle):
    return grid in r.grids and r.random and not r.early and not r.hopts and strict in r.builds and (r.oracle or not need_oracle)


def draw(seed, grid, strict, need_oracle):
    rng = np.random.default_rng(seed)
    pool = [name for name, r in ROWS.items() if drawable(r, grid, strict, need_oracle)]
    return [[pool[int(k)] for k in rng.integers(len(pool), size=int(rng.integers(1, 4)))] for _ in range(3)]


def play_sequence(h, seq, ctx):
    """three steps, the drawn calls before each; a row's setup goes right before its call, its undo after the step that follows"""
    rng = np.random.default_rng(SEED)
    ret, dts = [], []
    for names in seq:
        for name in names:
            r = ROWS[name]
            if r.setup:
                r.setup(h, rng, ctx)
            ret += r.call(h, rng, ctx) or []
        dts.append(h.step())
        for name in names:
            if ROWS[name].undo:
                ret += ROWS[name].undo(h, rng, ctx) or []
    out = [state(h, dts)]
    h.close()
    return out, ret


@gpu
@pytest.mark.parametrize("seed", range(8))
def test_random_sequences_strict_against_oracle(seed, tmp_path):
    grid, tol = BOTH[seed % 2], (1e-3, 1e-7)[(seed // 2) % 2]
    seq = draw(7000 + seed, grid, True, True)
    try:
        a, _ = play_sequence(gpu_handle(grid, True, CACHED, tol), seq, context(tmp_path, CACHED, tol, None))
        b, _ = play_sequence(oracle_handle(grid, tol), seq, context(tmp_path, CACHED, tol, None))
        same(a, b)
    except Exception as e:
        raise AssertionError(f"sequence {seq} on {grid} at TOLERANCE {tol:g}: {e}") from e


@gpu
@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("seed", range(8))
def test_random_sequences_cached_against_plain(seed, strict, tmp_path):
    grid = BOTH[seed % 2]
    seq = draw(8000 + seed, grid, strict, False)
    try:
        a, ra = play_sequence(gpu_handle(grid, strict, CACHED, 1e-3), seq, context(tmp_path, CACHED, 1e-3, None))
        b, rb = play_sequence(gpu_handle(grid, strict, PLAIN, 1e-3), seq, context(tmp_path, PLAIN, 1e-3, None))
        same(a, b)
        same_returned(ra, rb, "returned")
    except Exception as e:
        raise AssertionError(f"sequence {seq} on {grid}: {e}") from e
