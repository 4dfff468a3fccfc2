"""Wavenumber spectra and spectral fluxes on the device (msom_spec_*) against tests/spec_ref.py, the contract of include/msom.h in numpy.

Accuracy bar, measured here on the reference alone: d_ref is the distance between spec_ref in fp64 and spec_ref in numpy.longdouble on the
same input; the device must be within max(16 d_ref, 64 eps) of the longdouble result.  Distances are max |difference| per layer over
sqrt(max auto(a, a) * max auto(b, b)) of that layer, auto being spec_2D, the 1-D spectrum or the flux, whichever is compared: a
cross-spectrum that cancels is not held to its own small size.  Every check prints its ratio device / d_ref.

Shapes: 8 x 8 (two bins), 16 x 16, 64 x 32, 32 x 128, 128 x 128, 1024 x 512; 2048 x 64 / 64 x 2048 beside them because a line of up to
1024 has at most one butterfly per thread per stage and a longer one loops (lines of 8, 32, 128, 512, 2048 end on a radix-2 stage, the
others do not); 4096 x 32 / 32 x 4096, the longest line, whose column pass holds two of them in 139 KiB of LDS; 16 x 16 with 19 layers, more
than one batch of the work arrays.  Data: seeded normal fields with non-zero mean, or a = three single modes (one on the Nyquist row, one
on an axis) so that a mirrored or shifted index is a wrong location.  L0 = 1."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import newqg_ref as nq
import orc
import spec_ref as R
from msom_amd import FIELDS as F
from msom_amd import NewQG, QG
from test_gpu_hooks import DevBuf
from test_gpu_modes import random_fr
from test_gpu_stats import velocities
from test_gpu_tiled import run_tiled

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
LD = np.longdouble
ERR_ARG, ERR_CONFIG, ERR_STATE = -1, -3, -6
DP = C.POINTER(C.c_double)
BOTH = pytest.mark.parametrize("strict", [True, False], ids=["strict", "product"])
#          nx    ny  layers data
SHAPES = [(8, 8, 1, "random"), (16, 16, 3, "modes"), (64, 32, 6, "random"), (32, 128, 3, "modes"), (128, 128, 6, "random"),
          (1024, 512, 1, "modes"), (2048, 64, 1, "random"), (64, 2048, 3, "modes"), (4096, 32, 1, "modes"), (32, 4096, 1, "random"),
          (16, 16, 19, "random")]
IDS = [f"{s[0]}x{s[1]}x{s[2]}-{s[3]}" for s in SHAPES]
ALL = pytest.mark.parametrize("case", range(len(SHAPES)), ids=IDS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec_32.npz")


def params(nx, ny, nl, extra=""):
    return orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra, L0=1.0)


def mode_list(nx, ny):
    """(p, s, amplitude): one on the Nyquist row, one on the x axis, one general"""
    return [(3 % (nx // 2), ny // 2, 1.0), (2, 0, 0.5), (1, 3, 0.25)]


def data(nx, ny, layers, kind, seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((layers, ny, nx)) - 0.4
    if kind == "random":
        a = rng.standard_normal((layers, ny, nx)) + 0.7
    else:
        x, y = np.arange(nx)[None, :], np.arange(ny)[:, None]
        one = sum(amp * np.cos(2 * np.pi * (p * x / nx + s * y / ny)) for p, s, amp in mode_list(nx, ny))
        a = np.stack([(1 + l) * one for l in range(layers)])
    return a, b


class Ref:
    """inputs, spec_ref of them in fp64 and in longdouble -- (plane, spectrum, flux) per pair ab, aa, bb -- and the bar"""

    def __init__(self, a, b, D):
        self.a, self.b, self.D = a, b, D
        self.layers, self.ny, self.nx = a.shape
        self.p = {}
        for key, (x, y) in dict(ab=(a, b), aa=(a, a), bb=(b, b)).items():
            for dt in (np.float64, LD):
                s2 = R.spec_2d(x, y, D, dt)
                self.p[key, dt] = (s2, R.spec_1d_of(s2, D, dt), R.flux_of(s2, D, dt))

    def scale(self, key, which):
        mx = lambda k: np.abs(self.p[k, LD][which]).reshape(self.layers, -1).max(axis=1)   # noqa: E731
        s = mx(key) if key != "ab" else np.sqrt(mx("aa") * mx("bb"))
        return s.reshape((self.layers,) + (1,) * (self.p[key, LD][which].ndim - 1))

    def dist(self, got, key, which):
        return float((np.abs(got - self.p[key, LD][which]) / self.scale(key, which)).max())

    def check(self, got, key, which, what):
        d_ref = self.dist(self.p[key, np.float64][which], key, which)
        bar = max(16 * d_ref, 64 * EPS)
        err = self.dist(np.asarray(got), key, which)
        print(f"{what} {key} {('plane', 'spec', 'flux')[which]}: device {err:.3e}, d_ref {d_ref:.3e}, ratio {err / d_ref if d_ref else float('inf'):.2f}, bar {bar:.3e}")
        assert np.all(np.isfinite(got)) and err <= bar, (what, key, which, err, bar)


@functools.lru_cache(maxsize=None)
def ref(case):
    nx, ny, layers, kind = SHAPES[case]
    return Ref(*data(nx, ny, layers, kind, 100 + case), 1.0 / nx)


@functools.lru_cache(maxsize=None)
def handle(nx, ny, strict, nl=1):
    g = QG(params(nx, ny, nl), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    g.set_tnext(float("inf"))
    assert g.param("L0") == 1.0
    return g


# ------------------------------------------------------------------ 1. the plane

@BOTH
@ALL
def test_spec_2d_pointwise(case, strict):
    r = ref(case)
    g = handle(r.nx, r.ny, strict)
    assert g.spec_2d(r.a, r.b).shape == r.a.shape
    r.check(g.spec_2d(r.a, r.b), "ab", 0, IDS[case])
    r.check(g.spec_2d(r.a), "aa", 0, IDS[case])                       # a == b
    r.check(g.spec_2d(r.b, r.b.copy()), "bb", 0, IDS[case])           # the same values through the two-array route
    da, db, do = DevBuf(r.a), DevBuf(r.b), DevBuf(np.full(r.a.shape, -7.0))
    assert g.L.msom_spec_2d(g.h, da.ptr, db.ptr, r.layers, do.ptr) == 0
    dev = do.host()
    assert np.array_equal(dev, g.spec_2d(r.a, r.b))                   # device pointers: the same bits as host pointers
    assert g.L.msom_spec_2d(g.h, da.ptr, da.ptr, r.layers, do.ptr) == 0
    assert np.array_equal(do.host(), g.spec_2d(r.a))
    mixed = np.empty(r.a.shape)                                        # one host, one device input, host output
    assert g.L.msom_spec_2d(g.h, r.a.ctypes.data, db.ptr, r.layers, mixed.ctypes.data) == 0
    assert np.array_equal(mixed, dev)
    assert np.array_equal(da.host(), r.a) and np.array_equal(db.host(), r.b)
    for d_ in (da, db, do):
        d_.free()


# ------------------------------------------------------------------ 2. spectrum and flux

@BOTH
@ALL
def test_spec_cross_spectrum_and_flux(case, strict):
    r = ref(case)
    g = handle(r.nx, r.ny, strict)
    nb = R.nbins(r.nx, r.ny)
    assert g.spec_bins() == nb
    for key, (x, y) in dict(ab=(r.a, r.b), aa=(r.a, None), bb=(r.b, None)).items():
        sp, fl = g.spec_cross(x, y), g.spec_cross(x, y, flux=True)      # each with the other NULL
        assert sp.shape == fl.shape == (r.layers, nb)
        r.check(sp, key, 1, IDS[case])
        r.check(fl, key, 2, IDS[case])
        both_s, both_f = np.empty_like(sp), np.empty_like(fl)
        y_ = x if y is None else y
        assert g.L.msom_spec_cross(g.h, x.ctypes.data, y_.ctypes.data, r.layers, both_s.ctypes.data_as(DP), both_f.ctypes.data_as(DP)) == 0
        assert np.array_equal(both_s, sp) and np.array_equal(both_f, fl)
    da, db = DevBuf(r.a), DevBuf(r.b)
    sp = np.empty((r.layers, nb))
    assert g.L.msom_spec_cross(g.h, da.ptr, db.ptr, r.layers, sp.ctypes.data_as(DP), None) == 0
    assert np.array_equal(sp, g.spec_cross(r.a, r.b))
    da.free(); db.free()


# ------------------------------------------------------------------ 3. the reference's recording through the device

@BOTH
def test_golden_file_through_the_device(strict):
    gold = np.load(GOLDEN)
    N = int(gold["N"])
    g = handle(N, N, strict)
    a, b = gold["a"], gold["b"]
    r = Ref(a, b, float(gold["L0"]) / N)
    for which, (name, got) in enumerate((("spec_2d", g.spec_2d(a, b)), ("spec_1d", g.spec_cross(a, b)), ("flux", g.spec_cross(a, b, flux=True)))):
        r.check(got, "ab", which, "golden")
        d_ref = r.dist(r.p["ab", np.float64][which], "ab", which)
        recorded = r.dist(gold[name], "ab", which)        # the recording's own distance from the longdouble result
        err = float((np.abs(got - gold[name]) / r.scale("ab", which)).max())
        print(f"golden {name}: device - recording {err:.3e}, recording - longdouble {recorded:.3e}")
        assert err <= max(16 * d_ref, 64 * EPS) + recorded
    assert g.spec_bins() == int(gold["nbins"])


# ------------------------------------------------------------------ 4. identities on the device's numbers

@BOTH
@ALL
def test_identities(case, strict):
    r = ref(case)
    nx, ny, layers, kind = SHAPES[case]
    g = handle(nx, ny, strict)
    D = r.D
    s2, fl = g.spec_2d(r.a, r.b), g.spec_cross(r.a, r.b, flux=True)
    ab = (r.a.astype(LD) * r.b).sum(axis=(1, 2))
    bar2 = max(16 * r.dist(r.p["ab", np.float64][0], "ab", 0), 64 * EPS) * r.scale("ab", 0).ravel()
    # Parseval: every one of the nx ny points within its bar
    assert np.all(np.abs(s2.astype(LD).sum(axis=(1, 2)) / (nx * D) / (ny * D) - ab * D * D) <= nx * ny * bar2 / (nx * D) / (ny * D))
    # only the point (0, 0) lies inside radius 1
    want = (ab - nx * ny * r.a.astype(LD).mean(axis=(1, 2)) * r.b.astype(LD).mean(axis=(1, 2))) * D * D
    barf = max(16 * r.dist(r.p["ab", np.float64][2], "ab", 2), 64 * EPS) * r.scale("ab", 2).ravel()
    assert np.all(np.abs(fl[:, 0] - want) <= barf + 64 * EPS * np.abs(ab) * D * D)
    if kind == "modes":
        saa = g.spec_2d(r.a)
        on = np.zeros((ny, nx), dtype=bool)
        for p, s, amp in mode_list(nx, ny):
            for sg in (1, -1):   # signed indices; -n/2 stands for both +-n/2
                on[(sg * s + ny // 2) % ny, (sg * p + nx // 2) % nx] = True
        assert on.sum() == 6     # two points each: (p, -ny/2) and (-p, -ny/2) of the Nyquist-row mode are distinct because p != 0
        for l in range(layers):
            assert np.abs(saa[l][~on]).max() <= 64 * EPS * saa[l].max()
            assert np.all(saa[l][on] > 1e-3 * saa[l].max())
            assert abs(saa[l][on].sum() / ((r.a[l] ** 2).sum() * nx * ny * D ** 4) - 1) <= 64 * EPS


# ------------------------------------------------------------------ 5. energy spectra of the model state

#           nx  ny  nl  extra                     stratification
ECASES = [(64, 64, 3, "", "fr"), (64, 32, 6, "", "uniform"), (64, 64, 2, "sbc = -1\ntau0 = 0\n", "fr"), (32, 32, 1, "", "uniform")]
EIDS = [f"{c[0]}x{c[1]}x{c[2]}-{c[4]}" + ("-periodic" if "sbc = -1" in c[3] else "") for c in ECASES]
EALL = pytest.mark.parametrize("ecase", range(len(ECASES)), ids=EIDS)


@functools.lru_cache(maxsize=None)
def ehandle(ecase, strict):
    """set_const and two steps of the double gyre"""
    nx, ny, nl, extra, strat = ECASES[ecase]
    g = QG(params(nx, ny, nl, extra), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    if strat == "fr":
        g.set(F["FR"], random_fr(nl, ny, nx))
    g.set_const()
    g.set_tnext(float("inf"))
    for _ in range(2):
        assert g.step() > 0
    assert np.all(np.isfinite(g.get(F["PSI"])))
    return g


def auto_check(got, x_pairs, fac, D, what):
    """got [layers][nbins] against fac[l] * sum over the pairs of spec_1d(x, x), with the bar of the module docstring on that sum"""
    lo, hi = (sum(R.spec_1d(x, x, D, dt) for x in x_pairs) * fac.astype(dt)[:, None] for dt in (np.float64, LD))
    scale = np.abs(hi).max(axis=1, keepdims=True)
    d_ref = float((np.abs(lo - hi) / scale).max())
    err = float((np.abs(got - hi) / scale).max())
    bar = max(16 * d_ref, 64 * EPS)
    print(f"{what}: device {err:.3e}, d_ref {d_ref:.3e}, ratio {err / d_ref:.2f}, bar {bar:.3e}")
    assert np.all(np.isfinite(got)) and err <= bar, (what, err, bar)


@BOTH
@EALL
def test_spec_energy(ecase, strict):
    nx, ny, nl, extra, strat = ECASES[ecase]
    g = ehandle(ecase, strict)
    D = g.param("L0") / g.param("N")
    nb = R.nbins(nx, ny)
    psi = g.get(F["PSI"])
    dh = np.array([g.param(f"dh_{l}") for l in range(nl)])
    u, v = velocities(psi, "sbc = -1" in extra, 2.0 * D)
    ke, pe = g.spec_energy()
    assert ke.shape == (nl, nb) and pe.shape == (max(nl - 1, 0), nb)
    auto_check(ke, (u, v), 0.5 * dh, D, EIDS[ecase] + " ke")
    if nl > 1:
        dhc = 0.5 * (dh[:-1] + dh[1:])
        gg = np.sqrt(g.get(F["S"])[:nl - 1]) * (psi[1:] - psi[:-1]) / dhc[:, None, None]
        auto_check(pe, (gg,), 0.5 * dhc, D, EIDS[ecase] + " pe")
    # the bins overlap, so sum_r is no identity; instead the pair route against the generic call, one auto-spectrum at a time
    generic = 0.5 * dh[:, None] * (g.spec_cross(u) + g.spec_cross(v))
    assert np.abs(ke - generic).max() <= 64 * EPS * np.abs(generic).max()
    # either result alone; nl = 1 leaves pe alone
    only_ke, only_pe = np.full((nl, nb), -1.0), np.full((max(nl - 1, 1), nb), -1.0)
    assert g.L.msom_spec_energy(g.h, only_ke.ctypes.data_as(DP), None) == 0
    assert g.L.msom_spec_energy(g.h, None, only_pe.ctypes.data_as(DP)) == 0
    assert np.array_equal(only_ke, ke)
    assert np.array_equal(only_pe, pe) if nl > 1 else np.all(only_pe == -1.0)
    assert g.L.msom_spec_energy(g.h, None, None) == ERR_ARG


# ------------------------------------------------------------------ 6. the budget fluxes: two of the handle's fields

@BOTH
def test_spec_fields_of_the_budget_terms(strict):
    g = ehandle(0, strict)
    g.energy_tend(0.01)
    psi, j1 = g.get(F["PSI"]), g.get(F["DE_J1"])
    assert np.abs(j1).max() > 0
    for flux in (False, True):
        assert np.array_equal(g.spec_fields(F["PSI"], F["DE_J1"], flux=flux), g.spec_cross(psi, j1, flux=flux))
        assert np.array_equal(g.spec_fields(F["PSI"], F["PSI"], flux=flux), g.spec_cross(psi, flux=flux))
    # linear in each argument, so the sign of -p is the caller's (up to the rounding of another transform: 64 eps of the auto-fluxes)
    size = np.sqrt(np.abs(g.spec_cross(psi, flux=True)).max(axis=1) * np.abs(g.spec_cross(j1, flux=True)).max(axis=1))[:, None]
    assert np.all(np.abs(g.spec_cross(-psi, j1, flux=True) + g.spec_fields(F["PSI"], F["DE_J1"], flux=True)) <= 64 * EPS * size)
    x = (C.c_double * (3 * g.spec_bins()))()
    assert g.L.msom_spec_fields(g.h, F["PSI"], F["RD"], x, None) == ERR_ARG       # 3 layers against 1
    assert g.L.msom_spec_fields(g.h, F["PSI"], 99, x, None) == ERR_ARG
    assert g.L.msom_spec_fields(g.h, -1, F["PSI"], x, None) == ERR_ARG
    assert g.L.msom_spec_fields(g.h, F["PSI"], F["PSI"], None, None) == ERR_ARG


# ------------------------------------------------------------------ 7. - 9. determinism, reporting, no side effects

@BOTH
@pytest.mark.parametrize("case", [4, 5], ids=[IDS[4], IDS[5]])
def test_two_calls_give_identical_bits(case, strict):
    r = ref(case)
    g = handle(r.nx, r.ny, strict)
    for fn in (lambda: g.spec_2d(r.a, r.b), lambda: g.spec_cross(r.a, r.b), lambda: g.spec_cross(r.a, r.b, flux=True), lambda: g.spec_cross(r.a)):
        assert np.array_equal(fn(), fn())
    e = ehandle(0, strict)
    (k1, p1), (k2, p2) = e.spec_energy(), e.spec_energy()
    assert np.array_equal(k1, k2) and np.array_equal(p1, p2)


@BOTH
def test_kr_bins_and_bytes(strict):
    nx, ny = 64, 32
    g = QG(params(nx, ny, 2), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(2, ny, nx))
    g.set_const()
    D = 1.0 / nx
    assert g.spec_bins() == 30 and np.array_equal(g.spec_kr(), np.arange(1, 31) / (64 * D))
    assert np.allclose(g.spec_kr(), R.kr(nx, ny, D), rtol=4 * EPS, atol=0)
    assert g.param("spec_bytes") == 0            # asking for the layout allocates nothing
    g.spec_energy()
    first = g.param("spec_bytes")
    assert first >= 2 * 16 * nx * ny and g.param("spec_batch") >= 1
    g.spec_energy()
    assert g.param("spec_bytes") == first        # allocated once
    a = np.random.default_rng(0).standard_normal((2, ny, nx))
    g.spec_2d(a)                                 # host input and output: their device copies are counted too
    assert g.param("spec_bytes") > first
    g.set_const()
    assert g.param("spec_bytes") == 0
    g.spec_cross(a)
    assert g.param("spec_bytes") > 0
    g.close()


@BOTH
def test_no_side_effects(strict):
    g = ehandle(0, strict)
    nl, ny, nx = 3, 64, 64
    g.energy_tend(0.01)
    keys = ("PSI", "Q", "DQ", "ZETA", "S", "DE_J1")
    before = {k: g.get(F[k]) for k in keys}
    st, t, it = g.mgstats(), g.t, g.L.msom_iter(g.h)
    a = np.random.default_rng(5).standard_normal((nl, ny, nx))
    g.spec_2d(a); g.spec_cross(a, a + 1); g.spec_cross(a, flux=True); g.spec_fields(F["PSI"], F["DE_J1"], flux=True); g.spec_energy()
    g.spec_kr(); g.spec_bins()
    ms = C.c_double()
    for name in (b"spec_rows", b"spec_transpose", b"spec_cols", b"spec_shells"):
        assert g.L.msom_bench_kernel(g.h, name, 1, C.byref(ms)) == 0
    for k in keys:
        assert np.array_equal(g.get(F[k]), before[k]), k
    s2 = g.mgstats()
    assert (s2.i, s2.resb, s2.resa, s2.sum, s2.nrelax) == (st.i, st.resb, st.resa, st.sum, st.nrelax)
    assert g.t == t and g.L.msom_iter(g.h) == it
    assert g.step() > 0                          # and the run goes on


# ------------------------------------------------------------------ 10. call order, arguments, scope

def every_call(L, h, a, out, res):
    p, o = a.ctypes.data, out.ctypes.data
    r1, r2 = res[0].ctypes.data_as(DP), res[1].ctypes.data_as(DP)
    yield "msom_spec_bins", L.msom_spec_bins(h)
    yield "msom_spec_kr", L.msom_spec_kr(h, r1)
    yield "msom_spec_2d", L.msom_spec_2d(h, p, p, 1, o)
    yield "msom_spec_cross", L.msom_spec_cross(h, p, p, 1, r1, r2)
    yield "msom_spec_fields", L.msom_spec_fields(h, F["PSI"], F["Q"], r1, r2)
    yield "msom_spec_energy", L.msom_spec_energy(h, r1, r2)


def buffers(ny, nx, nl=3):
    return np.full((1, ny, nx), 7.0), np.full((1, ny, nx), 7.0), (np.full(nl * max(nx, ny), 7.0), np.full(nl * max(nx, ny), 7.0))


def untouched(a, out, res):
    return np.all(a == 7.0) and np.all(out == 7.0) and np.all(res[0] == 7.0) and np.all(res[1] == 7.0)


@BOTH
def test_call_order_and_argument_errors(strict):
    nx = ny = 32
    g = QG(params(nx, ny, 3), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], orc.synthetic_psi(3, ny, nx))
    a, out, res = buffers(ny, nx)
    for name, rc in every_call(g.L, g.h, a, out, res):                  # before msom_set_const
        assert rc == ERR_STATE, (name, rc)
    assert untouched(a, out, res) and g.param("spec_bytes") == 0
    g.set_const()
    L, h, p, o = g.L, g.h, a.ctypes.data, out.ctypes.data
    r1 = res[0].ctypes.data_as(DP)
    assert L.msom_spec_kr(h, None) == ERR_ARG
    assert L.msom_spec_2d(h, None, p, 1, o) == ERR_ARG and L.msom_spec_2d(h, p, None, 1, o) == ERR_ARG and L.msom_spec_2d(h, p, p, 1, None) == ERR_ARG
    assert L.msom_spec_2d(h, p, p, 0, o) == ERR_ARG and L.msom_spec_2d(h, p, p, -2, o) == ERR_ARG
    assert L.msom_spec_cross(h, None, p, 1, r1, None) == ERR_ARG and L.msom_spec_cross(h, p, None, 1, r1, None) == ERR_ARG
    assert L.msom_spec_cross(h, p, p, 0, r1, None) == ERR_ARG and L.msom_spec_cross(h, p, p, 1, None, None) == ERR_ARG
    assert L.msom_spec_fields(h, F["PSI"], F["Q"], None, None) == ERR_ARG and L.msom_spec_energy(h, None, None) == ERR_ARG
    assert untouched(a, out, res) and g.param("spec_bytes") == 0
    for name, rc in every_call(L, h, a, out, res):                      # and now they run
        assert rc == (nx // 2 - 2 if name == "msom_spec_bins" else 0), (name, rc)
    g.set(F["FR"], random_fr(3, ny, nx))                                  # a new stratification: msom_set_const is due again
    a, out, res = buffers(ny, nx)
    for name, rc in every_call(L, h, a, out, res):
        assert rc == ERR_STATE, (name, rc)
    assert untouched(a, out, res)
    g.close()


def test_tiled_handle_is_refused():
    nx, ny, nl = 64, 32, 2

    def fn(g, rank):
        a, out, res = buffers(g.ny, g.nx)
        codes = list(every_call(g.L, g.h, a, out, res))
        return dict(codes=codes, clean=bool(untouched(a, out, res)), bytes=g.param("spec_bytes"))

    for o in run_tiled(params(nx, ny, nl, "MGLEVELS = 5\n"), 2, 1, orc.synthetic_psi(nl, ny, nx), nsteps=0, strict=True, fn=fn):
        for name, rc in o["extra"]["codes"]:
            assert rc == ERR_CONFIG, (name, rc)
        assert o["extra"]["clean"] and o["extra"]["bytes"] == 0


@BOTH
def test_newqg_handle_is_refused(strict):
    g = NewQG(nq.sample_par(32).text(), strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], np.random.default_rng(2).standard_normal((1, 32, 32)))
    g.set_const()
    a, out, res = buffers(32, 32)
    for name, rc in every_call(g.L, g.h, a, out, res):
        assert rc == ERR_CONFIG, (name, rc)
        assert name in g.L.msom_last_error().decode(), name
    assert untouched(a, out, res)
    g.close()


# ------------------------------------------------------------------ 11. the measurement hook

@BOTH
def test_bench_kernel_names(strict):
    g = ehandle(1, strict)
    ms = C.c_double(-1.0)
    for name in (b"spec_rows", b"spec_transpose", b"spec_cols", b"spec_shells"):
        ms.value = -1.0
        assert g.L.msom_bench_kernel(g.h, name, 2, C.byref(ms)) == 0 and ms.value > 0, name
    assert g.L.msom_bench_kernel(g.h, b"spec_nothing", 2, C.byref(ms)) == ERR_ARG
    ke, _ = g.spec_energy()                      # the work arrays it overwrote are scratch: the next call is sound
    assert np.all(np.isfinite(ke)) and np.all(ke >= 0)
