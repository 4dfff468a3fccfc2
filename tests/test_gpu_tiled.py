"""Tiled (multi-GPU) code path on ONE GPU: px x py tiles run as host threads of one process
and exchange halos through the library's in-process transport (device-to-device copies), i.e.
exactly the pack / exchange / unpack / reduction logic that the RCCL transport drives with one
process per GPU.  Determinism gate of SURVEY 8(e): the tiled result must equal the single-tile
result of the same global grid bit for bit (same multigrid level count via MGLEVELS)."""
import os
import threading

import numpy as np
import pytest

import orc
from msom_amd import QG, FIELDS as F

pytestmark = pytest.mark.gpu


def run_tiled(params, px, py, psi, nsteps, strict, fn=None, opts=None, pre=None):
    n = px * py
    uid = b"MSOMLOCL" + os.urandom(8) + bytes(112)
    nl, gny, gnx = psi.shape
    tx, ty = gnx // px, gny // py
    out, errs = [None] * n, []

    def worker(rank):
        try:
            g = QG(params, strict=strict, tiled=(px, py, rank, uid))
            g.option("quiet", 1)
            for k_, v_ in (opts or {}).items():
                g.option(k_, v_)
            ix, iy = rank % px, rank // px
            assert g.tile == (px, py, ix, iy) and (g.nx, g.ny) == (tx, ty)
            g.set(F["PSI"], psi[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx])
            g.set_const()
            if pre:
                pre(g, rank)
            g.set_tnext(float("inf"))
            dts = [g.step() for _ in range(nsteps)]
            res = dict(q=g.get(F["Q"]), psi=g.get(F["PSI"]), ke=g.ke(), t=g.t, dts=dts, st=g.mgstats(), agg=g.param("agg_level"))
            if fn:
                res["extra"] = fn(g, rank)
            out[rank] = res
            g.close()
        except Exception as e:  # noqa: BLE001
            errs.append((rank, repr(e)))

    th = [threading.Thread(target=worker, args=(r,), daemon=True) for r in range(n)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=120)
    assert not errs, errs
    assert all(o is not None for o in out), "a tile thread hung"
    return out


def assemble(out, key, px, py):
    rows = []
    for iy in range(py):
        rows.append(np.concatenate([out[iy * px + ix][key] for ix in range(px)], axis=2))
    return np.concatenate(rows, axis=1)


@pytest.mark.parametrize("px,py,tile,nl", [(2, 1, 32, 3), (1, 2, 32, 3), (2, 2, 32, 6), (2, 4, 16, 2), (3, 1, 16, 3)])
@pytest.mark.parametrize("strict", [True, False])
def test_tiled_equals_single_tile_bit_for_bit(px, py, tile, nl, strict):
    gnx, gny = tile * px, tile * py
    levels = int(np.log2(tile))
    extra = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {levels}\n"
    if px == 3:
        pytest.skip("3 tiles per side needs a non-power-of-two global N; covered by create-time check")
    params = orc.double_gyre_params(gnx, nl, extra=extra)
    psi = orc.synthetic_psi(nl, gny, gnx)
    out = run_tiled(params, px, py, psi, nsteps=5, strict=strict)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    dts = [g.step() for _ in range(5)]
    assert g.nlevels() == levels
    for r in range(px * py):
        assert out[r]["dts"] == dts, r
        assert out[r]["t"] == g.t
        assert (out[r]["st"].i, out[r]["st"].resa, out[r]["st"].resb) == (g.mgstats().i, g.mgstats().resa, g.mgstats().resb)
        assert out[r]["ke"] == pytest.approx(g.ke(), rel=1e-13)   # sum order differs
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))


@pytest.mark.parametrize("strict", [True, False])
def test_large_tiles_default_agglomeration(strict):
    """2 x 2 tiles of 512^2 with the default options: level 0 exchanges halos after every colour, the levels
    from 256^2 per tile down are gathered (global 512^2 ... 4^2, the last five in one launch), the wide-level
    kernels (two cells per thread, LDS-tiled correction, fused tendency) run on tiles; equal to the single
    tile bit for bit."""
    px = py = 2
    tile, nl = 512, 2
    gn = tile * px
    params = orc.double_gyre_params(gn, nl, extra="MGLEVELS = 9\n")
    psi = orc.synthetic_psi(nl, gn, gn)
    out = run_tiled(params, px, py, psi, nsteps=3, strict=strict)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    dts = [g.step() for _ in range(3)]
    for r in range(px * py):
        assert out[r]["dts"] == dts, r
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))


@pytest.mark.parametrize("extra", ["", "ediag = 0\nafilt = 4\ndtflt = 0.02\n"])
def test_tiled_driver_loop_writes_the_same_files(tmp_path, extra):
    """msom_run on 2 x 2 tiles (collective gathers, rank 0 writes): po / qo .bas files, backup of the constant fields
    and NetCDF output identical to the single-tile run; restart from the written file on the tiles.  Second case: the
    wavelet filter and the energy budgets in the loop (pf / de_* files, msqg/qg.c:124-160)"""
    px = py = 2
    tile, nl = 32, 3
    gn = tile * px
    params = orc.double_gyre_params(gn, nl, extra="MGLEVELS = 5\n" + extra).replace("tend  = 500.", "tend = 0.04").replace("dtout = 1.", "dtout = 0.02")
    psi = orc.synthetic_psi(nl, gn, gn)
    d1, d4 = tmp_path / "single", tmp_path / "tiled"
    d1.mkdir(); d4.mkdir()
    g = QG(params)
    g.option("quiet", 1)
    g.set(F["PSI"], psi); g.set_const()
    g.run(str(d1))
    g.write_nc(str(d1 / "vars.nc"))

    def run(gt, rank):
        gt.run(str(d4))
        gt.write_nc(str(d4 / "vars.nc"))
        gt.read_bas(F["PSI"], str(d4 / "outdir_0001" / "po000000000.bas"))      # collective read: every tile takes its part
        return gt.get(F["PSI"])

    out = run_tiled(params, px, py, psi, nsteps=0, strict=False, fn=run)
    names = sorted(os.listdir(d1 / "outdir_0001"))
    assert names == sorted(os.listdir(d4 / "outdir_0001")) and any(n.startswith("po") for n in names) and len(names) >= 12
    assert not extra or (any(n.startswith("de_ft") for n in names) and any(n.startswith("pf") for n in names))
    for n in names:
        assert (d1 / "outdir_0001" / n).read_bytes() == (d4 / "outdir_0001" / n).read_bytes(), n
    assert (d1 / "vars.nc").read_bytes() == (d4 / "vars.nc").read_bytes()
    back = np.concatenate([np.concatenate([out[iy * px + ix]["extra"] for ix in range(px)], axis=2) for iy in range(py)], axis=1)
    assert np.array_equal(back, psi.astype("f4").astype("f8"))


def test_tiled_strict_matches_oracle():
    """The tiled strict build is bit-exact against the (untiled) CPU oracle as well."""
    px, py, tile, nl = 2, 2, 32, 3
    gn = tile * px
    params = orc.double_gyre_params(gn, nl, extra="MGLEVELS = 5\n")
    psi = orc.synthetic_psi(nl, gn, gn)
    out = run_tiled(params, px, py, psi, nsteps=4, strict=True)
    o = orc.Oracle(params, smoother=orc.GS_RB, quiet=1)
    assert o.nlevels() == 5
    o.set(orc.PSI, psi)
    o.set_const()
    for _ in range(4):
        o.step()
    assert np.array_equal(assemble(out, "q", px, py), o.get(orc.Q))
    assert np.array_equal(assemble(out, "psi", px, py), o.get(orc.PSI))


def test_tiled_tight_tolerance_multi_cycle_and_background_flow():
    """Several multigrid cycles per solve (adaptive nrelax path) + large-scale flow + remove_mean."""
    px, py, tile, nl = 2, 2, 32, 3
    gn = tile * px
    params = orc.double_gyre_params(gn, nl, extra="MGLEVELS = 5\nTOLERANCE = 1e-11\nupg = [0.3,0.1,0.0]\nvpg = [0.0,-0.2,0.05]\nflsrv = 1\n")
    psi = orc.synthetic_psi(nl, gn, gn) + 1e-4

    def extra(g, rank):
        g.remove_mean(F["PSI"])
        return g.get(F["PSI"])

    out = run_tiled(params, px, py, psi, nsteps=2, strict=True, fn=extra)
    g = QG(params, strict=True)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    for _ in range(2):
        g.step()
    assert g.mgstats().i > 1
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    g.remove_mean(F["PSI"])
    got = np.concatenate([np.concatenate([out[iy * px + ix]["extra"] for ix in range(px)], axis=2) for iy in range(py)], axis=1)
    assert np.abs(got - g.get(F["PSI"])).max() <= 1e-15 * np.abs(psi).max()   # mean: sum order differs


def test_rccl_library_resolves():
    """dlopen(librccl) + symbol table + ncclGetUniqueId through the C ABI (the N > 1 RCCL
    transport itself needs one GPU per rank and is exercised by bench.py --gpus N)."""
    import ctypes
    from msom_amd import load_library
    L = load_library()
    buf = (ctypes.c_char * 128)()
    assert L.msom_comm_unique_id(buf) == 0, L.msom_last_error()
    assert any(b != 0 for b in buf.raw)
    assert L.msom_set_device(0) == 0


def test_rccl_transport_selftest():
    """one-rank RCCL communicator: grouped ncclSend/ncclRecv to self, all-reduce, all-gather through
    comm_exchange / comm_allreduce / comm_allgather (the transport bench.py --gpus N uses)"""
    from msom_amd import load_library
    L = load_library()
    assert L.msom_set_device(0) == 0
    assert L.msom_dbg_rccl_selftest() == 0, L.msom_last_error().decode()


@pytest.mark.parametrize("px,py,tile,nl", [(2, 2, 32, 3), (2, 4, 16, 6), (2, 1, 64, 2)])
@pytest.mark.parametrize("agg_size,expect_level", [(64, 0), (8, None), (0, -1)])
@pytest.mark.parametrize("strict", [True, False])
def test_coarse_level_agglomeration_is_bit_identical(px, py, tile, nl, agg_size, expect_level, strict):
    """Below the agglomeration level every rank solves the gathered global coarse grid instead of
    exchanging halos after every colour: same arithmetic, so the result must not change by a bit
    -- whether all levels (agg_size 64), only the coarse ones (8) or none (0) are agglomerated."""
    gnx, gny = tile * px, tile * py
    levels = int(np.log2(tile))
    params = orc.double_gyre_params(gnx, nl, extra=(f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {levels}\nTOLERANCE = 1e-9\n")
    psi = orc.synthetic_psi(nl, gny, gnx)
    opts = {"agg_size": agg_size, "uniform_S": 1}
    out = run_tiled(params, px, py, psi, nsteps=3, strict=strict, opts=opts)
    lev = out[0]["agg"]
    if expect_level is None:
        assert 0 < lev < levels
    else:
        assert lev == expect_level
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.option("uniform_S", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    for _ in range(3):
        g.step()
    assert g.mgstats().i > 1            # several cycles per solve at this tolerance
    assert out[0]["st"].i == g.mgstats().i and out[0]["st"].resa == g.mgstats().resa
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))


@pytest.mark.parametrize("px,py,tx,ty,nl", [(2, 1, 512, 64, 3), (1, 2, 512, 64, 2), (2, 2, 512, 128, 6), (2, 2, 1024, 64, 4)])
@pytest.mark.parametrize("strict", [True, False])
def test_chained_smoother_on_tiles(px, py, tx, ty, nl, strict):
    """option march = 2 on tiles: a pass of chained half-sweeps reads 4 rows / cells of its neighbour tiles (one deep
    halo exchange per pass instead of one exchange per half-sweep) and re-computes the cone of dependence.  Strict build
    (uniform-S solver switched on): equal to the single tile, with and without the chained smoother, bit for bit.
    Product build: the levels that take the chained pass differ between a tile and the whole grid and FMA contraction is
    chosen per kernel, so the comparison is to fp64 round-off (1e-10 of max|psi|, same cycle counts)"""
    gnx, gny = tx * px, ty * py
    levels = int(np.log2(min(tx, ty)))
    params = orc.double_gyre_params(gnx, nl, extra=(f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {levels}\n")
    psi = orc.synthetic_psi(nl, gny, gnx)
    out = run_tiled(params, px, py, psi, nsteps=2, strict=strict, opts={"march": 2, "TOLERANCE": 1e-7, "uniform_S": 1})
    ref = []
    for march in (0, 2):
        g = QG(params, strict=strict)
        g.option("quiet", 1); g.option("march", march); g.option("TOLERANCE", 1e-7); g.option("uniform_S", 1)
        g.set(F["PSI"], psi)
        g.set_const()
        g.set_tnext(float("inf"))
        dts = [g.step() for _ in range(2)]
        assert g.param("uniform_S") == 1.0
        ref.append((dts, g.get(F["Q"]), g.get(F["PSI"]), g.mgstats().i))
        g.close()
    for r in range(px * py):
        assert out[r]["st"].i == ref[1][3]
    q, p = assemble(out, "q", px, py), assemble(out, "psi", px, py)
    if strict:
        for r in range(px * py):
            assert out[r]["dts"] == ref[1][0], r
        assert np.array_equal(q, ref[1][1]) and np.array_equal(p, ref[1][2])
        assert np.array_equal(ref[0][1], ref[1][1]) and np.array_equal(ref[0][2], ref[1][2])
    else:
        assert np.abs(p - ref[1][2]).max() <= 1e-10 * np.abs(ref[1][2]).max()
        assert np.abs(q - ref[1][1]).max() <= 1e-10 * np.abs(ref[1][1]).max()


@pytest.mark.parametrize("strict", [True, False])
def test_chained_smoother_default_on_big_tiles(strict):
    """default options on tiles that are big enough for the chained smoother to switch itself on (2 x 1 tiles of
    2048^2 x 4 = 2^24 cell-layers each): same comparison as above, one step"""
    px, py, tx, ty, nl = 2, 1, 2048, 2048, 4
    gnx, gny = tx * px, ty * py
    params = orc.double_gyre_params(gnx, nl, extra=f"Ny = {gny}\nMGLEVELS = 11\n")
    psi = orc.synthetic_psi(nl, gny, gnx)
    out = run_tiled(params, px, py, psi, nsteps=1, strict=strict, opts={"uniform_S": 1})
    g = QG(params, strict=strict)
    g.option("quiet", 1); g.option("uniform_S", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    g.step()
    p = assemble(out, "psi", px, py)
    if strict:
        assert np.array_equal(p, g.get(F["PSI"]))
    else:
        assert np.abs(p - g.get(F["PSI"])).max() <= 1e-10 * np.abs(g.get(F["PSI"])).max()
    assert out[0]["st"].i == g.mgstats().i


def test_tiled_passive_tracers_wide_halo_messages():
    """nptr = 5 on 2 x 2 tiles of 64^2 x 3: tracer fields carry nl * nptr = 15 layers and are exchanged whole, the
    largest halo message of the run (the staging buffers were sized for nl layers only).  Bit-identical to
    the single tile, tracers included."""
    px = py = 2
    tile, nl, nptr = 64, 3, 5
    gn = tile * px
    ex = f"MGLEVELS = 6\nnptr = {nptr}\nptr_r = [10,0,3.5,1,0]\nPe = [200,50,0,100,20]\n"
    params = orc.double_gyre_params(gn, nl, extra=ex)
    psi = orc.synthetic_psi(nl, gn, gn)
    rng = np.random.default_rng(5)
    c0, rl = 1e-3 * rng.standard_normal((nl * nptr, gn, gn)), 1e-3 * rng.standard_normal((nl * nptr, gn, gn))

    def sl(a, rank):
        ix, iy = rank % px, rank // px
        return a[:, iy * tile:(iy + 1) * tile, ix * tile:(ix + 1) * tile]

    def pre(g, rank):
        g.set(F["PTR"], sl(c0, rank)); g.set(F["PTR_RELAX"], sl(rl, rank))

    out = run_tiled(params, px, py, psi, nsteps=3, strict=True, pre=pre, fn=lambda g, r: g.get(F["PTR"]))
    g = QG(params, strict=True)
    g.option("quiet", 1)
    g.set(F["PSI"], psi); g.set_const()
    g.set(F["PTR"], c0); g.set(F["PTR_RELAX"], rl)
    g.set_tnext(float("inf"))
    for _ in range(3):
        g.step()
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "extra", px, py), g.get(F["PTR"]))
    assert np.abs(g.get(F["PTR"]) - c0).max() > 0


def test_baseline_c4_layout_2x4_tiles_of_2048x1024x6():
    """BASELINE config 4 exactly as written -- 4096^2 x 6 on 2 x 4 tiles of 2048 x 1024 -- through the in-process
    transport on ONE GPU (8 host threads, 8 x 1.8 GB of fields): one RK2 step, product build, default options (the
    chained smoother with 4-deep halos on the two finest tile levels, agglomerated coarse levels, overlapped ring
    exchanges).  Compared with the single tile on the same number of multigrid levels: the per-point arithmetic is the
    same but FMA contraction is chosen per kernel and the kernels differ between tile and whole grid, hence 1e-10."""
    px, py, tx, ty, nl = 2, 4, 2048, 1024, 6
    gn = 4096
    params = orc.double_gyre_params(gn, nl, extra="MGLEVELS = 10\n")
    psi = orc.synthetic_psi(nl, gn, gn)
    out = run_tiled(params, px, py, psi, nsteps=1, strict=False)
    g = QG(params)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    dt = g.step()
    p = assemble(out, "psi", px, py)
    ref = g.get(F["PSI"])
    assert p.shape == ref.shape == (nl, gn, gn)
    assert np.abs(p - ref).max() <= 1e-10 * np.abs(ref).max()
    for r in range(px * py):
        assert out[r]["dts"] == [dt] and out[r]["st"].i == g.mgstats().i


@pytest.mark.parametrize("px,py,tile,nl", [(2, 2, 32, 3), (2, 1, 32, 3), (1, 2, 32, 3), (2, 4, 16, 1), (2, 2, 512, 2)])
@pytest.mark.parametrize("strict", [True, False])
def test_periodic_domain_on_tiles(px, py, tile, nl, strict):
    """sbc = -1 (doubly periodic, msqg/qg.h:842-846) on tiles: the neighbours wrap around, no tile has a wall, with 1 or 2
    tiles per side both neighbours of an axis are the same rank (or the tile itself).  Equal to the periodic single tile bit
    for bit (strict and product builds), incl. the agglomerated periodic coarse grid."""
    gnx, gny = tile * px, tile * py
    levels = int(np.log2(tile))
    # Ly = L0 / 2: the double-gyre wind curl sin(2 pi y / L0) has a non-zero mean there, which a periodic domain cannot absorb
    # (the inversion stalls and raises nrelax to 100: slow, and not what is tested here)
    extra = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {levels}\nsbc = -1\nTOLERANCE = 1e-8\n" + ("tau0 = 0\n" if gny < gnx else "")
    params = orc.double_gyre_params(gnx, nl, extra=extra)
    x = (np.arange(gnx) + 0.5) / gnx
    y = (np.arange(gny) + 0.5) / gny
    psi = np.stack([1e-3 * (1 - 0.2 * l) * (np.outer(np.sin(2 * np.pi * y), np.cos(4 * np.pi * x)) + 0.5 * np.outer(np.cos(6 * np.pi * y + l), np.sin(2 * np.pi * x)))
                    for l in range(nl)])
    out = run_tiled(params, px, py, psi, nsteps=3, strict=strict)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    dts = [g.step() for _ in range(3)]
    for r in range(px * py):
        assert out[r]["dts"] == dts, r
        assert (out[r]["st"].i, out[r]["st"].resa) == (g.mgstats().i, g.mgstats().resa)
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))


@pytest.mark.parametrize("px,py", [(2, 1), (1, 2), (2, 2)])
@pytest.mark.parametrize("tx,ty", [(32, 16), (16, 32)])
@pytest.mark.parametrize("strict", [True, False])
def test_periodic_domain_on_tiles_that_are_not_square(px, py, tx, ty, strict):
    """sbc = -1 with 1 or 2 tiles per side, where one peer gets both messages of an axis (or all four, the tile being its own
    peer), on tiles of 32 x 16 and 16 x 32 cells: the W / E messages and the S / N messages differ in length on every level.  The
    in-process transport pairs messages by posting order as RCCL does (comm_order_inl.h), so an order that hands a W / E strip
    to a S / N edge is a count error here and one that swaps the two edges of an axis a tag error; with square tiles the first
    cannot show.  Equal to the periodic single tile bit for bit, strict and product builds."""
    nl = 2
    gnx, gny = tx * px, ty * py
    extra = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {int(np.log2(min(tx, ty)))}\nsbc = -1\nTOLERANCE = 1e-8\n" + ("tau0 = 0\n" if gny < gnx else "")
    params = orc.double_gyre_params(gnx, nl, extra=extra)
    x = (np.arange(gnx) + 0.5) / gnx
    y = (np.arange(gny) + 0.5) / gny
    psi = np.stack([1e-3 * (1 - 0.2 * l) * (np.outer(np.sin(2 * np.pi * y), np.cos(4 * np.pi * x)) + 0.5 * np.outer(np.cos(6 * np.pi * y + l), np.sin(2 * np.pi * x)))
                    for l in range(nl)])
    out = run_tiled(params, px, py, psi, nsteps=3, strict=strict)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    dts = [g.step() for _ in range(3)]
    for r in range(px * py):
        assert out[r]["dts"] == dts, r
        assert (out[r]["st"].i, out[r]["st"].resa) == (g.mgstats().i, g.mgstats().resa)
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))


@pytest.mark.parametrize("px,py,tile,nl", [(2, 2, 32, 3), (2, 1, 32, 3), (1, 2, 32, 1), (4, 2, 16, 3), (2, 2, 16, 2)])
@pytest.mark.parametrize("strict", [True, False])
def test_periodic_tiles_with_the_large_scale_flow(px, py, tile, nl, strict):
    """sbc = -1 with upg / vpg on tiles: psi_pg = vpg x - upg y is not periodic, its ghosts on the DOMAIN edges are
    dirichlet(vpg x - upg y) (msqg/qg.h:1105-1114) and the wrapped exchange values everywhere else.  Steps and the ghost
    cells of psi_pg equal to the single tile's bit for bit."""
    gnx, gny = tile * px, tile * py
    up = ",".join(["0.3", "0.1", "0.0"][:nl]); vp = ",".join(["0.0", "-0.2", "0.05"][:nl])
    extra = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {int(np.log2(tile))}\nsbc = -1\nTOLERANCE = 1e-8\nupg = [{up}]\nvpg = [{vp}]\nflsrv = 1\n" + ("tau0 = 0\n" if gny < gnx else "")
    params = orc.double_gyre_params(gnx, nl, extra=extra)
    x = (np.arange(gnx) + 0.5) / gnx
    y = (np.arange(gny) + 0.5) / gny
    psi = np.stack([1e-3 * (1 - 0.2 * l) * (np.outer(np.sin(2 * np.pi * y), np.cos(4 * np.pi * x)) + 0.5 * np.outer(np.cos(6 * np.pi * y + l), np.sin(2 * np.pi * x)))
                    for l in range(nl)])
    out = run_tiled(params, px, py, psi, nsteps=3, strict=strict, fn=lambda g, r: g.get(F["ZETAPG"]))
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    dts = [g.step() for _ in range(3)]
    for r in range(px * py):
        assert out[r]["dts"] == dts, r
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))
    # zeta_pg = del2(psi_pg) reads every ghost cell of psi_pg, corners of the domain included
    zpg = np.concatenate([np.concatenate([out[iy * px + ix]["extra"] for ix in range(px)], axis=2) for iy in range(py)], axis=1)
    assert np.array_equal(zpg, g.get(F["ZETAPG"]))


@pytest.mark.parametrize("px,py,tile,nl,extra", [(2, 2, 32, 3, ""), (2, 1, 32, 2, ""), (2, 4, 16, 2, ""), (2, 2, 32, 2, "sbc = -1\n")])
@pytest.mark.parametrize("strict", [True, False])
def test_wavelet_filter_on_tiles(px, py, tile, nl, extra, strict):
    """msom_wavelet_filter (msqg/qg.h:509-560) on tiles: the pyramid levels that still have a cell of every tile live on
    the tile (halo exchange with corners per level), the levels above are gathered and transformed by every rank with the
    same arithmetic; coefficients sig_lev from a non-uniform Rd.  Equal to the single tile bit for bit, and the model keeps
    stepping on the filtered state."""
    gnx, gny = tile * px, tile * py
    levels = int(np.log2(tile))
    ex = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {levels}\nafilt = 4\nTOLERANCE = 1e-10\n" + extra
    params = orc.double_gyre_params(gnx, nl, extra=ex)
    psi = orc.synthetic_psi(nl, gny, gnx)
    if extra:
        x = (np.arange(gnx) + 0.5) / gnx
        y = (np.arange(gny) + 0.5) / gny
        psi = np.stack([1e-3 * (1 - 0.2 * l) * np.outer(np.sin(2 * np.pi * y), np.cos(4 * np.pi * x)) for l in range(nl)])
    Rd = np.ones((1, gny, gnx)); Rd[0, :, gnx // 2:] = 3.0; Rd[0, : gny // 4] = 0.5
    ty, tx = gny // py, gnx // px

    def pre(g, rank):
        ix, iy = rank % px, rank // px
        g.set(F["RD"], Rd[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx])
        g.set_const()

    def fn(g, rank):
        g.wavelet_filter(0.5)
        res = [g.get(F["PSI"]), g.get(F["Q"]), g.get(F["QOF"])]
        g.step()
        return res + [g.get(F["Q"])]

    out = run_tiled(params, px, py, psi, nsteps=0, strict=strict, pre=pre, fn=fn)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["RD"], Rd)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    g.wavelet_filter(0.5)
    ref = [g.get(F["PSI"]), g.get(F["Q"]), g.get(F["QOF"])]
    g.step()
    ref.append(g.get(F["Q"]))
    for k in range(4):
        got = np.concatenate([np.concatenate([out[iy * px + ix]["extra"][k] for ix in range(px)], axis=2) for iy in range(py)], axis=1)
        assert np.array_equal(got, ref[k]), k


@pytest.mark.parametrize("px,py,tile,nl", [(2, 2, 32, 3), (2, 1, 64, 2)])
@pytest.mark.parametrize("strict", [True, False])
def test_stochastic_steps_on_tiles(px, py, tile, nl, strict):
    """-D_STOCHASTIC (msqg/qg_stochastic.h) with the counter-based device noise on tiles: the same fields as one tile,
    bit for bit (product build: relaxation + noise folded into the tendency pass; validation build: separate kernels)."""
    gnx, gny = tile * px, tile * py
    extra = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {int(np.log2(tile))}\ntr_stoch = 50\namp_stoch = 1e-5\n"
    params = orc.double_gyre_params(gnx, nl, extra=extra)
    psi = orc.synthetic_psi(nl, gny, gnx)
    sig = np.abs(np.random.default_rng(5).standard_normal((nl, gny, gnx)))
    opts = {"stochastic": 1, "noise_mode": 1, "seed": 3}
    tx, ty = gnx // px, gny // py

    def pre(g, r):
        ix, iy = r % px, r // px
        g.set(F["SIGMA"], np.ascontiguousarray(sig[:, iy * ty:(iy + 1) * ty, ix * tx:(ix + 1) * tx]))

    out = run_tiled(params, px, py, psi, nsteps=4, strict=strict, opts=opts, pre=pre)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    for k, v in opts.items():
        g.option(k, v)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set(F["SIGMA"], sig)
    g.set_tnext(float("inf"))
    for _ in range(4):
        g.step()
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))


@pytest.mark.parametrize("px,py,tile,nl,extra", [(2, 2, 32, 3, "Re = 800\nEks = 0.003\n"), (2, 1, 32, 2, ""), (1, 2, 32, 3, "sbc = -1\n")])
@pytest.mark.parametrize("strict", [True, False])
def test_energy_budgets_on_tiles(px, py, tile, nl, extra, strict):
    """energy_tend / filter_de (msqg/qg_energy.h:28-242) on tiles: the budget fields of every tile equal the blocks of the
    single-tile fields bit for bit (1-cell stencils on exchanged halos, the tiled wavelet filter for de_ft)."""
    gnx, gny = tile * px, tile * py
    ex = (f"Ny = {gny}\n" if gny != gnx else "") + f"MGLEVELS = {int(np.log2(tile))}\nediag = 0\nafilt = 4\ndtflt = 0.25\n" + extra
    params = orc.double_gyre_params(gnx, nl, extra=ex)
    psi = orc.synthetic_psi(nl, gny, gnx)
    names = ("DE_BF", "DE_VD", "DE_J1", "DE_J2", "DE_J3", "DE_FT", "PO_MFT")

    def budget_run(g, rank=None):
        for _ in range(3):
            g.energy_tend(0.02)
            g.step()
        before = {k: g.get(F[k]) for k in names}
        g.filter_de(F["PO_MFT"], 0.25)
        return before, {k: g.get(F[k]) for k in names}

    out = run_tiled(params, px, py, psi, nsteps=0, strict=strict, fn=budget_run)
    g = QG(params, strict=strict)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    g.set_tnext(float("inf"))
    ref = budget_run(g)
    for stage in (0, 1):
        for k in names:
            got = np.concatenate([np.concatenate([out[iy * px + ix]["extra"][stage][k] for ix in range(px)], axis=2) for iy in range(py)], axis=1)
            assert np.array_equal(got, ref[stage][k]), (stage, k, np.abs(got - ref[stage][k]).max())
    assert np.abs(ref[0]["DE_J1"]).max() > 0 and np.abs(ref[1]["DE_FT"]).max() > 0


def test_serial_noise_stream_is_refused_on_tiles():
    """noise_mode = 0 replays the reference's serial rand() stream: one stream per process would give every tile the same
    numbers, so a tiled model refuses it instead of forcing wrongly."""
    params = orc.double_gyre_params(64, 2, extra="MGLEVELS = 5\ntr_stoch = 50\namp_stoch = 1e-5\n")
    psi = orc.synthetic_psi(2, 64, 64)

    def step(g, r):
        try:
            g.step()
        except Exception as e:  # noqa: BLE001
            return repr(e)
        return "stepped"

    out = run_tiled(params, 2, 1, psi, nsteps=0, strict=False, opts={"stochastic": 1, "noise_mode": 0}, fn=step)
    assert all("noise_mode = 1" in o["extra"] for o in out), [o["extra"] for o in out]


@pytest.mark.parametrize("px,py,tx,ty,nl", [(2, 1, 512, 64, 3), (2, 2, 512, 64, 2), (1, 2, 512, 128, 6), (2, 2, 512, 128, 6)])
def test_march_on_periodic_tiles(px, py, tx, ty, nl):
    """periodic tiles have no walls, so big ones take the chained smoother by default, yet every periodic
    tiled test stayed below march_min.  Forced here (march = 2): sbc = -1 on 2 x 1 / 2 x 2 / 1 x 2 tiles through the in-process
    transport -- both neighbours of an axis are the same rank or the tile itself, deep halos of the residual, the correction
    and the coarse correction (prolongation rider), correction rider on the finest level (the nl = 6 cases have a coarse level
    of >= 8 cells) -- equal to the periodic single tile bit for bit in the strict build"""
    gnx, gny = tx * px, ty * py
    extra = (f"Ny = {gny}\n" if gny != gnx else "") + "sbc = -1\ntau0 = 0\n" + f"MGLEVELS = {int(np.log2(min(tx, ty)))}\n"
    params = orc.double_gyre_params(gnx, nl, extra=extra)
    psi = orc.synthetic_psi(nl, gny, gnx)
    opts = {"march": 2, "uniform_S": 1, "TOLERANCE": 1e-8}
    out = run_tiled(params, px, py, psi, nsteps=2, strict=True, opts=opts)
    g = QG(params, strict=True)
    g.option("quiet", 1)
    g.set(F["PSI"], psi)
    g.set_const()
    for k_, v_ in opts.items():
        g.option(k_, v_)
    g.set_tnext(float("inf"))
    dts = [g.step() for _ in range(2)]
    for r in range(px * py):
        assert out[r]["dts"] == dts, r
        assert (out[r]["st"].i, out[r]["st"].resa) == (g.mgstats().i, g.mgstats().resa)
    assert np.array_equal(assemble(out, "q", px, py), g.get(F["Q"]))
    assert np.array_equal(assemble(out, "psi", px, py), g.get(F["PSI"]))
