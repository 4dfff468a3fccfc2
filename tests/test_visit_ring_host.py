"""The compact grid of wall-ring chunks around the fused finest-level visit (option march_visit_ring, msom_visit_ring):
host arithmetic only, no device.  The band table must name exactly the chunks that the skip rule of the two passes admits when
it is applied to every chunk of the full grid, and the chunks that run must cover what the level needs:
every cell is written by a fused chunk or a ring CORR chunk, and every cell a ring CORR chunk reads was written by a ring PL
chunk.  Set equalities and inclusions, no tolerances."""
import ctypes as C

import numpy as np
import pytest

from msom_amd import api

K = 4            # half-sweeps per pass
FUSED_OW = 48    # own half-columns of a fused strip
PASS = {0: (56, 4), 1: (60, 2)}   # pass -> (own half-columns of a strip, halo lanes per side): PL, CORR

SIZES = [(4096, 4096), (2048, 2048), (1024, 512), (2048, 1024),
         (1000, 602), (776, 330), (4000, 3002), (1300, 97), (130, 50), (258, 4100), (128, 40), (128, 44)]
RING_ROWS = (6, 8, 14, 16)
VISIT_ROWS = (14, 20, 28, 42)
PAIRS = (1, 2)


def ring(hk, ny, ring_rows, visit_rows, pairs, corr):
    L = api.load_library()
    f = L.msom_visit_ring
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_int)] * 2
    geom, bands = (C.c_int * 5)(), (C.c_int * 16)()
    n = f(hk, ny, ring_rows, visit_rows, pairs, corr, geom, bands)
    if n < 0:
        return None
    chunks = []
    for b in range(4):
        s0, ns, c0, nc = bands[b], bands[4 + b], bands[8 + b], bands[12 + b]
        assert ns >= 0 and nc >= 0
        # the order the kernel prologue decodes a linear index in: strips fastest inside a band
        chunks += [(s0 + i % ns, c0 + i // ns) for i in range(ns * nc)]
    assert n == len(chunks)
    return dict(H=geom[0], vy0=geom[1], nc=geom[2], vx0=geom[3], ns=geom[4]), chunks


def skip_rects(g, Hc):
    """the rectangles launch_relax_visit hands to the two passes ("Walls")"""
    my, vy1, vx1 = Hc + K, g["vy0"] + g["nc"] * g["H"], g["vx0"] + g["ns"] * FUSED_OW
    return {0: (g["vy0"] + my, vy1 - my, g["vx0"] + 64, vx1 - 64), 1: (g["vy0"], vy1, g["vx0"], vx1)}


def brute_force(hk, ny, corr, Hc, skip):
    """the skip test of k_relax_march_dma on every chunk of the full grid"""
    ow, hl = PASS[corr]
    sy0, sy1, sx0, sx1 = skip
    out = set()
    for c in range((ny + Hc - 1) // Hc):
        y0, y1 = c * Hc, min(ny, c * Hc + Hc)
        for s in range((hk + ow - 1) // ow):
            kx0 = s * ow - hl
            if sy1 > sy0 and y0 >= sy0 and y1 <= sy1 and kx0 + hl >= sx0 and min(kx0 + 64 - hl, hk) <= sx1:
                continue
            out.add((s, c))
    return out


def combos(nx, ny):
    for rr in RING_ROWS:
        for vr in VISIT_ROWS:
            for pairs in PAIRS:
                yield rr, vr, pairs


@pytest.mark.parametrize("nx,ny", SIZES)
def test_compact_ring_is_the_skip_rule(nx, ny):
    hk = nx // 2
    for rr, vr, pairs in combos(nx, ny):
        for corr in (0, 1):
            r = ring(hk, ny, rr, vr, pairs, corr)
            if r is None:
                continue
            g, chunks = r
            assert g["H"] == vr and g["ns"] % pairs == 0
            want = brute_force(hk, ny, corr, rr, skip_rects(g, rr)[corr])
            assert len(chunks) == len(set(chunks)), (rr, vr, pairs, corr)
            assert set(chunks) == want, (rr, vr, pairs, corr)


@pytest.mark.parametrize("nx,ny", SIZES)
def test_ring_and_fused_chunks_cover_the_level(nx, ny):
    hk = nx // 2
    for rr, vr, pairs in combos(nx, ny):
        pl, co = ring(hk, ny, rr, vr, pairs, 0), ring(hk, ny, rr, vr, pairs, 1)
        assert (pl is None) == (co is None)
        if pl is None:
            continue
        g = pl[0]
        assert g == co[0]
        # fused chunks: inside the level with their whole cone (wave A reads rows y0 - 2K .. y1 + 2K - 1 and 8 halo lanes)
        fy0, fy1, fx0, fx1 = g["vy0"], g["vy0"] + g["nc"] * g["H"], g["vx0"], g["vx0"] + g["ns"] * FUSED_OW
        assert fy0 - 2 * K >= 0 and fy1 + 2 * K <= ny and fx0 - 8 >= 0 and fx1 + 8 <= hk
        written = np.zeros((ny, hk), dtype=bool)        # psi_out
        written[fy0:fy1, fx0:fx1] = True
        for s, c in co[1]:
            written[c * rr:min(ny, c * rr + rr), s * 60:min(hk, s * 60 + 60)] = True
        assert written.all(), (rr, vr, pairs)
        have = np.zeros((ny, hk), dtype=bool)           # da_alt after the ring PL pass
        for s, c in pl[1]:
            have[c * rr:min(ny, c * rr + rr), s * 56:min(hk, s * 56 + 56)] = True
        for s, c in co[1]:
            y0, y1, kx0 = c * rr, min(ny, c * rr + rr), s * 60 - 2
            assert have[max(0, y0 - K):min(ny, y1 + K), max(0, kx0):min(hk, kx0 + 64)].all(), (rr, vr, pairs, s, c)


def test_benchmark_geometry():
    """4096^2: the numbers the launch code is sized by: 21 x 145 fused workgroups of two pairs, about 1 370 ring PL
    and 1 020 ring CORR chunks instead of the 37 x 293 and 36 x 293 wavefronts of the full chunk grids"""
    g, pl = ring(2048, 4096, 0, 0, 2, 0)
    _, co = ring(2048, 4096, 0, 0, 2, 1)
    assert (g["H"], g["vy0"], g["nc"], g["vx0"], g["ns"]) == (28, 8, 145, 8, 42)
    assert 1200 < len(pl) < 1500 and 900 < len(co) < 1100
    assert ring(60, 4096, 0, 0, 2, 0) is None and ring(2048, 4096, 0, 0, 3, 0) is None
