"""Option rhs_resid: the tendency + advance pass (k_rhs_lpw, RES instantiation) emits the first residual of the next inversion --
res on levels 0 and 1, max|res|, the sum of q -- instead of a launch of k_residual2<write + restrict> on the same psi and q.

The by-product repeats k_residual2's operations one for one, so a run with the option on equals the run with it off BIT FOR BIT in both
builds: psi, q, every dt and (i, resb, resa, nrelax) of the last solve.  mgstats().sum alone is held to rel = 1e-12: it is a sum of
q over the grid whose order differs (per workgroup of the tendency pass / of the residual pass).

No power of two is a multiple of the 58-column strip, so every grid here has a ragged last strip."""
import gc

import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F

pytestmark = pytest.mark.gpu

# 64x64x1: no vertical term; 128x64x2: top and bottom layers only; 256x64x5: two strips of 5 wavefronts per workgroup, idle wavefronts
# and a last workgroup whose second strip lies past the right edge (the library takes powers of two only, so not 192 x 96);
# 128x16x3: fewer rows than one chunk
GRIDS = [(64, 64, 1), (128, 64, 2), (256, 64, 5), (256, 128, 6), (128, 16, 3)]
BUILDS = [True, False]


def params(nx, ny, nl, extra=""):
    return orc.double_gyre_params(nx, nl, extra=(f"Ny = {ny}\n" if ny != nx else "") + extra)


def fr_field(g, nx, ny, nl):
    """bench.py's spatially varying Froude field"""
    x, y = (np.arange(nx) + 0.5) / nx, (np.arange(ny) + 0.5) / ny
    shape = 1.0 + 0.3 * np.outer(np.sin(2 * np.pi * y), np.cos(2 * np.pi * x))
    if nl > 1:   # one layer: no interface
        g.set(F["FR"], np.stack([g.param(f"Fr_{l}") * shape for l in range(nl - 1)]))


def qforc_field(g, nx, ny, nl):
    g.set(F["QFORC"], 1e-4 * np.random.default_rng(5).standard_normal((nl, ny, nx)))


def handle(nx, ny, nl, strict, resid, extra="", pre=None, tol=1e-7, **opts):
    g = QG(params(nx, ny, nl, extra), strict=strict)
    g.option("quiet", 1)
    g.option("TOLERANCE", tol)
    if resid is not None:
        g.option("rhs_resid", resid)
    for k, v in opts.items():
        g.option(k, v)
    if pre:
        pre(g, nx, ny, nl)
    g.set(F["PSI"], orc.synthetic_psi(nl, ny, nx))
    g.set_const()
    return g


def snap(g, dts):
    st = g.mgstats()
    return g.get(F["PSI"]), g.get(F["Q"]), list(dts), (st.i, st.resb, st.resa, st.nrelax), st.sum


def run(nx, ny, nl, strict, resid, **kw):
    g = handle(nx, ny, nl, strict, resid, **kw)
    dts, out = [], []
    for n in range(3):
        dts.append(g.step())
        if n in (0, 2):
            out.append(snap(g, dts))
    g.close()
    return out


def same(a, b):
    for x, y in zip(a, b):
        assert np.array_equal(x[0], y[0]), "psi"
        assert np.array_equal(x[1], y[1]), "q"
        assert x[2] == y[2], "dt"
        assert x[3] == y[3], f"(i, resb, resa, nrelax): {x[3]} / {y[3]}"
        assert x[4] == pytest.approx(y[4], rel=1e-12), "sum"
    assert len(a) == len(b)


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("nx,ny,nl", GRIDS)
def test_steps_equal_option_off(nx, ny, nl, strict):
    same(run(nx, ny, nl, strict, 1), run(nx, ny, nl, strict, 0))


# chunk heights (rhs_dbg = rows << 8; the launcher raises a height below 8 to 8 first, so every height here is above that floor) that do
# not divide ny (10, 12: a ragged last chunk), odd ones, which the launcher makes even for the by-product (9 -> 10, 11 -> 12, 13 -> 14;
# none of those divides 64 or 128 either) while the run with the option off keeps the odd height, partial slip and free slip walls, a
# spatially varying S, a 3-D forcing, the ghost-line body everywhere
VARIANTS = {
    "rows10": dict(rhs_dbg=10 << 8),
    "rows12": dict(rhs_dbg=12 << 8),
    "rows9_odd": dict(rhs_dbg=9 << 8),
    "rows11_odd": dict(rhs_dbg=11 << 8),
    "rows13_odd": dict(rhs_dbg=13 << 8),
    "partial_slip": dict(extra="sbc = 2.0\n"),
    "free_slip": dict(extra="sbc = 0\n"),
    "fr": dict(pre=fr_field),
    "qforc": dict(pre=qforc_field),
    "fr_qforc_rows10": dict(pre=lambda g, *a: (fr_field(g, *a), qforc_field(g, *a)), rhs_dbg=10 << 8),
    "edge_body": dict(lpw_dbg=4),
    "edge_body_slip": dict(lpw_dbg=4, extra="sbc = 2.0\n"),
}


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("nx,ny,nl", [(256, 64, 5), (256, 128, 6)])
def test_variants_equal_option_off(nx, ny, nl, variant, strict):
    kw = VARIANTS[variant]
    same(run(nx, ny, nl, strict, 1, **kw), run(nx, ny, nl, strict, 0, **kw))


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("rows", [9, 13])
def test_odd_height_few_rows(rows, strict):
    """ny = 16 and an odd requested height: made even, two chunks, the second ragged (10 + 6, 14 + 2)"""
    kw = dict(rhs_dbg=rows << 8)
    same(run(128, 16, 3, strict, 1, **kw), run(128, 16, 3, strict, 0, **kw))


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("tol", [1e-7, 1e-3])   # several cycles per solve: the speculative pass is discarded; one: it is accepted
@pytest.mark.parametrize("async_solve", [0, 1])
def test_speculative_pass(async_solve, tol, strict):
    nx, ny, nl = 256, 64, 5
    a = run(nx, ny, nl, strict, 1, tol=tol, async_solve=async_solve)
    same(a, run(nx, ny, nl, strict, 0, tol=tol, async_solve=async_solve))
    same(a, run(nx, ny, nl, strict, 0, tol=tol, async_solve=0))


def seq_set_q(g, nx, ny, nl):
    g.set(F["Q"], g.get(F["Q"]) * 1.01)


def seq_set_psi(g, nx, ny, nl):
    g.set(F["PSI"], 0.5 * orc.synthetic_psi(nl, ny, nx))


def seq_pyq2p(g, nx, ny, nl):
    p = np.empty((nl, ny, nx))
    g.pyq2p(p, 0.9 * g.get(F["Q"]))


SEQUENCES = {"set_q": seq_set_q, "set_psi": seq_set_psi, "pyq2p": seq_pyq2p}


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("tol", [1e-7, 1e-3])
@pytest.mark.parametrize("seq", sorted(SEQUENCES))
def test_call_between_steps(seq, tol, strict):
    """a call that changes psi or q between two steps: nothing stale may open the next solve"""
    nx, ny, nl = 128, 64, 2
    out = []
    for resid in (1, 0):
        g = handle(nx, ny, nl, strict, resid, tol=tol)
        dts = [g.step()]
        SEQUENCES[seq](g, nx, ny, nl)
        dts.append(g.step())
        out.append([snap(g, dts)])
        g.close()
    same(*out)


@pytest.mark.parametrize("strict", BUILDS)
def test_option_toggled_between_steps(strict):
    nx, ny, nl = 128, 64, 2
    out = []
    for toggle in (True, False):
        g = handle(nx, ny, nl, strict, 1 if toggle else 0, tol=1e-3)
        dts = [g.step()]
        if toggle:
            g.option("rhs_resid", 0)
        dts.append(g.step())
        if toggle:
            g.option("rhs_resid", 1)
        dts.append(g.step())
        dts.append(g.step())
        out.append([snap(g, dts)])
        g.close()
    same(*out)


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("async_solve", [0, 1])
def test_profile_slots(async_solve, strict):
    """with the option on and solves of one cycle the pre-cycle residual pass is not launched after the first solve; the tendency pass
    is launched as often as before"""
    nx, ny, nl = 256, 64, 5
    counts = {}
    for resid in (1, 0):
        g = handle(nx, ny, nl, strict, resid, tol=1e-3, async_solve=async_solve, profile=1)
        g.step()
        g.profile_reset()
        for _ in range(3):
            g.step()
        g.sync()
        counts[resid] = {k: g.profile_read(k)[1] for k in ("resid_restrict", "rhs")}
        assert g.mgstats().i == 1
        g.close()
    assert counts[0]["resid_restrict"] == 6 and counts[1]["resid_restrict"] == 0
    assert counts[1]["rhs"] == counts[0]["rhs"] == 6


def split_cells(a, nx, ny, rp, sp):
    """owned cells of a raw split array [nl][rows][2 halves][rp / 2], one ghost row below and sp pad columns on each side of a half row
    -> mask.  rp and sp are the library's own (split_rp_<k>, split_pad)"""
    nl, ls = a.shape
    rows, hp, hk = ls // rp, rp // 2, nx // 2
    assert rows * rp == ls and rows >= ny + 2 and hp >= hk + 2 * sp
    m = np.zeros((rows, 2, hp), bool)
    m[1:ny + 1, :, sp:sp + hk] = True
    return np.broadcast_to(m.reshape(-1), (nl, ls))


@pytest.mark.parametrize("strict", BUILDS)
@pytest.mark.parametrize("variant", ["plain", "fr_qforc_rows10", "edge_body", "rows9_odd", "rows11_odd", "rows13_odd", "rows12"])
@pytest.mark.parametrize("nx,ny,nl", GRIDS)
def test_by_products_equal_residual_pass(nx, ny, nl, variant, strict):
    """one tendency pass with the by-product against k_residual2<write + restrict> on the same psi and q_out: res on levels 0 and 1
    (NaN-filled beforehand: what one kernel leaves alone the other does too), max|res|, the sum of q_out"""
    kw = dict(VARIANTS.get(variant, {}))
    g = handle(nx, ny, nl, strict, 0, **kw)
    g.step()
    dt = 0.5 * g.step()
    a = g.dbg_rhs_resid(True, dt)
    b = g.dbg_rhs_resid(False, dt)
    sp, rp = int(g.param("split_pad")), [int(g.param(f"split_rp_{k}")) for k in (0, 1)]
    g.close()
    own = [split_cells(b[k], nx >> k, ny >> k, rp[k], sp) for k in (0, 1)]
    for k in (0, 1):
        assert np.array_equal(a[k], b[k], equal_nan=True), f"level {k}"
        assert not np.isnan(b[k][own[k]]).any() and np.isnan(b[k][~own[k]]).all()
    assert a[2] == b[2] and a[2] == np.abs(b[0][own[0]]).max()
    assert a[3] == pytest.approx(b[3], rel=1e-12)


def test_default_resolves_by_size():
    g = handle(64, 64, 3, False, None)
    assert g.param("rhs_resid") == 0       # far below the size from which the by-product pays
    g.option("rhs_resid", 1)
    assert g.param("rhs_resid") == 1
    g.option("mg_fused", 0)                # no fused residual consumer in the solve: nothing is emitted, whatever the option says
    assert g.param("rhs_resid") == 0
    g.close()


@pytest.mark.parametrize("n,nl", [(4096, 6), (2048, 3)])
def test_full_size_default_equals_option_off(n, nl):
    """the metric size and the next one down, product build, default options against rhs_resid = 0, after 1 and 3 steps (hazards of this
    kernel family have shown only at full size)"""
    psi0 = orc.synthetic_psi(nl, n, n)
    ref = []
    for resid in (0, None):
        g = QG(params(n, n, nl), strict=False)
        g.option("quiet", 1)
        if resid is not None:
            g.option("rhs_resid", resid)
        g.set(F["PSI"], psi0)
        g.set_const()
        # the default must have resolved to on here: otherwise both handles run the same path and the comparison says nothing
        assert g.param("rhs_resid") == (0 if resid == 0 else 1)
        dts = []
        for k in range(3):
            dts.append(g.step())
            if k in (0, 2):
                st = g.mgstats()
                cur = (g.get(F["PSI"]), g.get(F["Q"]), list(dts), (st.i, st.resb, st.resa, st.nrelax), st.sum)
                if resid == 0:
                    ref.append(cur)
                else:
                    same([cur], [ref[k // 2]])
                    ref[k // 2] = None
                del cur
        g.close()
        gc.collect()
