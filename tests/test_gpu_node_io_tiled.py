"""NetCDF files and the driver msomn_run of the vertex model on tiles (option io_tiles): px x py tiles as host threads of one process
write the single tile's vars.nc byte for byte, read it back into their windows, and run and resume through the driver's checkpoints.
Bits and bytes are compared as such; the one exception is text printed from sums whose order differs on tiles (diag_1d.dat): those
numbers are compared at 1e-6 relative -- "%e" prints seven digits, and the order effect is bounded at 1e-13 by
test_gpu_node_tiled.check_against_single.  Without the option every call here answers MSOM_ERR_CONFIG."""
import os

import numpy as np
import pytest

import orn
from msom_amd import MsomError, NodeQG
from msom_amd.state import read_state
from msom_amd.tiling import node_assemble, node_tile_window
from test_gpu_node_state_tiled import bare_tiled
from test_gpu_node_tiled import OPTION_KEYS, inputs, params, run_tiled, single

pytestmark = pytest.mark.gpu

MSOM_ERR_STATE = -6


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("px,py", [(2, 2), (4, 2)])
def test_write_nc_and_read_nc_on_tiles(px, py, strict, tmp_path):
    N, nl = 32, 3
    par, inp = params(N, nl), inputs(N, nl)
    pt, ps = str(tmp_path / "tiled.nc"), str(tmp_path / "single.nc")

    def writer(g, rank):
        for _ in range(2):        # two appended records
            g.step(True)
            g.write_nc(pt)
        return {k: g.param(k) for k in OPTION_KEYS}
    opts = dict(run_tiled(par, px, py, inp, strict, writer, opts=dict(mg_coarse=8, io_tiles=1))[0])
    g = single(par, inp, strict, opts)
    for _ in range(2):
        g.step(True)
        g.write_nc(ps)
    psi = g.get("PSI")
    g.close()
    a, b = open(pt, "rb").read(), open(ps, "rb").read()
    assert len(a) > 2 * 2 * nl * (N + 1) ** 2 * 4 and a == b
    assert sorted(os.listdir(tmp_path)) == ["single.nc", "tiled.nc"]
    # the file stores float32: both sides read the same rounded fields.  Fresh tiled handles take their windows, shared vertices and
    # halos included, and step on like a single tile that read the same file
    g = single(par, inp, strict, opts)
    g.read_nc("PSI", ps, "psi")
    g.read_nc("PSIPG", ps, "q", 0)
    g.comp_q()
    want = dict(psi=g.get("PSI"), pg=g.get("PSIPG"))
    g.step(True)
    want["q"] = g.get("Q")
    g.close()

    def reader(g, rank):
        g.read_nc("PSI", pt, "psi")
        g.read_nc("PSIPG", pt, "q", 0)
        g.comp_q()
        res = dict(psi=g.get("PSI"), pg=g.get("PSIPG"))
        e0 = g.param("exchanges")
        try:
            g.read_nc("PSI", str(tmp_path / "none.nc"), "psi")
            res["missing"] = 0
        except MsomError as e:
            res["missing"] = e.code
        res["posted"] = g.param("exchanges") - e0
        g.step(True)
        res["q"] = g.get("Q")
        return res
    out = run_tiled(par, px, py, inp, strict, reader, opts=dict(opts, io_tiles=1))
    for r, o in enumerate(out):
        sy, sx = node_tile_window(N, px, py, r)
        assert np.array_equal(o["psi"], want["psi"][:, sy, sx]) and np.array_equal(o["pg"], want["pg"][:, sy, sx])
        assert o["missing"] == -2 and o["posted"] == 0      # MSOM_ERR_IO on every rank, nothing posted
    assert np.array_equal(node_assemble([o["q"] for o in out], N, px, py, check_shared=True), want["q"])
    assert not np.array_equal(want["psi"], psi)       # (what was read is the float32 of what was written)


def diag_numbers(text):
    rows = [l for l in text.splitlines()]
    return rows[0], np.array([[float(v) for v in l.split(",")] for l in rows[1:]])


@pytest.mark.parametrize("strict", [True, False])
def test_driver_runs_and_resumes_on_tiles(strict, tmp_path):
    """test_driver_resumes_from_its_checkpoint of test_gpu_node_state.py on 2 x 2 tiles, held to the single tile's run"""
    px, py, N, nl = 2, 2, 32, 2
    par = orn.node_params(N, nl, bc_fac=1.0, extra="tend = 0.4\ndtout = 0.1\ndtdiag = 0.05\n")
    inp = inputs(N, nl)
    whole, died, one = tmp_path / "whole", tmp_path / "died", tmp_path / "one"
    for d in (whole, died, one):
        d.mkdir()
    common = dict(mg_coarse=8, io_tiles=1)

    def run_whole(g, rank):
        return g.run(str(whole)), {k: g.param(k) for k in OPTION_KEYS}
    out = run_tiled(par, px, py, inp, strict, run_whole, opts=dict(common, ckpt_steps=5))
    n_whole = out[0][0]
    assert all(o[0] == n_whole for o in out) and n_whole > 10          # the same return value on every rank
    assert sorted(os.listdir(whole)) == ["outdir_0001", "state.msom"]      # one directory, made by rank 0
    # the single tile's run, with the option values the tiles report
    g = single(par, inp, strict, dict(out[0][1], ckpt_steps=5))
    assert g.run(str(one)) == n_whole
    g.close()
    assert (whole / "outdir_0001" / "vars.nc").read_bytes() == (one / "outdir_0001" / "vars.nc").read_bytes()
    assert (whole / "outdir_0001" / "params.in").read_text() == par
    ht, dt_ = diag_numbers((whole / "outdir_0001" / "diag_1d.dat").read_text())
    h1, d1 = diag_numbers((one / "outdir_0001" / "diag_1d.dat").read_text())
    assert ht == h1 and dt_.shape == d1.shape == (8, 4)
    print(np.abs(dt_ - d1).max())
    assert np.allclose(dt_, d1, rtol=1e-6, atol=0)
    assert (whole / "state.msom").read_bytes()[:64] == (one / "state.msom").read_bytes()[:64]
    a, b = read_state(whole / "state.msom"), read_state(one / "state.msom")
    for k in a["records"]:                                                  # the run record names the size of diag_1d.dat: text
        assert np.array_equal(a["records"][k], b["records"][k]), k

    # a run that dies after 8 steps, having written past its last checkpoint; new handles with nothing but the file resume it
    def run_died(g, rank):
        n = g.run(str(died), 8)
        g.write_nc(str(died / "outdir_0001" / "vars.nc"))
        if rank == 0:
            with open(died / "outdir_0001" / "diag_1d.dat", "a") as f:
                f.write("%e, %e, %e, %e\n" % (g.t, 1.0, 2.0, 3.0))
        return n
    assert run_tiled(par, px, py, inp, strict, run_died, opts=dict(common, ckpt_steps=5)) == [8] * 4
    st = read_state(died / "state.msom")
    assert st["iter"] == 5 and list(st["records"]["run"][3:5]) == [1, 1]

    def make(rank, uid):
        g = NodeQG(par, strict=strict, tiled=(px, py, rank, uid))
        for k, v in dict(common, resume=1).items():
            g.set_option(k, v)
        return g
    res = bare_tiled(make, px, py, lambda g, rank: (g.run(str(died)), g.t))
    assert all(r[0] == n_whole and abs(r[1] - 0.4) < 1e-12 for r in res)
    assert sorted(os.listdir(died)) == ["outdir_0001", "state.msom"]
    for name in ("vars.nc", "diag_1d.dat"):
        a, b = (whole / "outdir_0001" / name).read_bytes(), (died / "outdir_0001" / name).read_bytes()
        assert len(a) > 100 and a == b, name


def test_driver_without_constants_is_refused_on_every_rank(tmp_path):
    par = orn.node_params(32, 2, bc_fac=1.0, extra="tend = 0.4\ndtout = 0.1\n")

    def make(rank, uid):
        g = NodeQG(par, strict=False, tiled=(2, 1, rank, uid))
        g.set_option("io_tiles", 1)
        return g

    def body(g, rank):
        codes = []
        for resume in (0, 1):         # resume = 1 with no state.msom in the directory starts like a run without it
            g.set_option("resume", resume)
            try:
                g.run(str(tmp_path))
                codes.append((0, ""))
            except MsomError as e:
                codes.append((e.code, str(e)))
        return codes
    for codes in bare_tiled(make, 2, 1, body):
        assert all(c[0] == MSOM_ERR_STATE and "msomn_set_const" in c[1] for c in codes), codes
    assert os.listdir(tmp_path) == []
