"""The fused visit on the levels below the finest: host arithmetic only, no device.  The chunk height follows the level
(msom_visit_rows: the rule by rounds of the device's wave-pair slots), and with that height the chunks that run must cover what the
level needs, as tests/test_visit_ring_host.py argues for the finest level: every cell of the level's correction is written by a
fused chunk or by a chunk of the second ring, at most once by either kind, and every cell a second-ring chunk reads was written by
a first-ring (PL) chunk.  "Exactly once" over both kinds together does not hold for this geometry, on the finest level either: the
skip rule drops a ring chunk only when ALL its own cells lie inside the fused rectangle, so the chunks that straddle its edge write
a band of it again (same bits); the test bounds that band instead.  Equalities and inclusions, no tolerances."""
import ctypes as C

import numpy as np
import pytest

from msom_amd import api
from test_visit_ring_host import ring

K = 4
FUSED_OW = 48
HK = (256, 384, 512, 1024, 2048)
NY = (32, 40, 64, 96, 128, 256, 1024, 2048, 4096)   # 32, 40: no 28-row chunk fits (ny - 16 < 28), the minimiser is searched all the same
PAIRS = (1, 2)
SLOTS = (512, 1024)


def rows(hk, ny, pairs, slots):
    f = api.load_library().msom_visit_rows
    f.restype = C.c_int
    f.argtypes = [C.c_int] * 4
    return f(hk, ny, pairs, slots)


def grid(hk, ny, H, pairs):
    """chunk rows and strips of the fused grid (visit_geom): wave A reads 2 K rows beyond the chunk and 8 lanes beyond the strip"""
    return (ny - 4 * K) // H, ((hk - 64) // FUSED_OW + 1) // pairs * pairs


def steps(hk, ny, H, pairs, slots):
    nc, ns = grid(hk, ny, H, pairs)
    return -(-nc * ns // slots) * (H + 4 * K - 1)


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("pairs", PAIRS)
def test_height_rule(pairs, slots):
    for hk in HK:
        for ny in NY:
            H = rows(hk, ny, pairs, slots)
            nc, ns = grid(hk, ny, H, pairs)
            assert H >= 14 and H % 2 == 0 and nc > 0 and ns > 0, (hk, ny)
            g, _ = ring(hk, ny, 0, H, pairs, 0)
            assert (g["H"], g["nc"], g["ns"]) == (H, nc, ns)
            nc28, ns28 = grid(hk, ny, 28, pairs)
            if nc28 > 0 and nc28 * ns28 > 3 * slots:
                assert H == 28, (hk, ny)
                continue
            cand = [h for h in range(14, ny + 1, 2) if grid(hk, ny, h, pairs)[0] > 0]
            best = min(steps(hk, ny, h, pairs, slots) for h in cand)
            assert steps(hk, ny, H, pairs, slots) == best, (hk, ny, H)
            assert H == min(h for h in cand if steps(hk, ny, h, pairs, slots) == best), (hk, ny, H)   # the smallest on a tie


def test_levels_too_low_for_28_rows():
    """ny < 44: every height that fits (14 .. ny - 16) gives one chunk row, so the number of rounds does not depend on H and the
    shortest chunk is the minimiser, also with more strips than slots.  ny = 30: only 14 fits; ny = 29: none"""
    assert rows(1024, 40, 2, 1024) == 14 and rows(1024, 32, 1, 512) == 14
    assert rows(4096, 40, 1, 64) == 14     # 85 strips on 64 slots: two rounds of 29 steps; 24 rows would be two of 39
    assert rows(1024, 30, 2, 1024) == 14 and rows(1024, 29, 2, 1024) == -1


def test_benchmark_levels():
    """the numbers DESIGN.md argues with, 1024 pair slots: the finest level of 4096^2 keeps 28 rows (5.9 rounds), its 2048^2 level
    takes 40 (1000 pairs, one round of 55 steps instead of two of 43)"""
    assert rows(2048, 4096, 2, 1024) == 28
    assert rows(1024, 2048, 2, 1024) == 40 and grid(1024, 2048, 40, 2) == (50, 20)
    assert rows(60, 4096, 2, 1024) == -1 and rows(1024, 2048, 3, 1024) == -1


@pytest.mark.parametrize("hk", HK)
def test_plain_chunks_cover_the_level_once(hk):
    for ny in NY:
        for pairs in PAIRS:
            for slots in SLOTS:
                H = rows(hk, ny, pairs, slots)
                for rr in (0, 8):
                    Hc = rr or 14
                    pl, co = ring(hk, ny, rr, H, pairs, 0), ring(hk, ny, rr, H, pairs, 1)
                    g = pl[0]
                    assert g == co[0]
                    fy0, fy1, fx0, fx1 = g["vy0"], g["vy0"] + g["nc"] * g["H"], g["vx0"], g["vx0"] + g["ns"] * FUSED_OW
                    assert fy0 - 2 * K >= 0 and fy1 + 2 * K <= ny and fx0 - 8 >= 0 and fx1 + 8 <= hk
                    # the level's correction: once by the fused chunks (a grid), once by the chunks of the second ring among
                    # themselves, every cell by one of the two
                    fused = np.zeros((ny, hk), dtype=bool)
                    fused[fy0:fy1, fx0:fx1] = True
                    written = np.zeros((ny, hk), dtype=np.int8)
                    for s, c in co[1]:
                        written[c * Hc:min(ny, c * Hc + Hc), s * 60:min(hk, s * 60 + 60)] += 1
                    assert written.max() == 1, (ny, pairs, slots, rr)
                    assert (fused | (written == 1)).all(), (ny, pairs, slots, rr)
                    # a ring chunk runs whole when one of its own cells lies outside the fused rectangle, so a chunk that straddles the
                    # rectangle's edge writes up to Hc - 1 rows / 59 half-columns of it a second time (the same bits: same arithmetic
                    # on the same inputs; nothing reads the correction inside the visit).  No cell deeper inside is written twice
                    both = fused & (written == 1)
                    deep = np.zeros((ny, hk), dtype=bool)
                    deep[fy0 + Hc - 1:fy1 - Hc + 1, fx0 + 59:fx1 - 59] = True
                    assert not (both & deep).any(), (ny, pairs, slots, rr)
                    have = np.zeros((ny, hk), dtype=bool)           # the other buffer after the ring PL chunks
                    for s, c in pl[1]:
                        have[c * Hc:min(ny, c * Hc + Hc), s * 56:min(hk, s * 56 + 56)] = True
                    for s, c in co[1]:
                        y0, y1, kx0 = c * Hc, min(ny, c * Hc + Hc), s * 60 - 2
                        assert have[max(0, y0 - K):min(ny, y1 + K), max(0, kx0):min(hk, kx0 + 64)].all(), (ny, pairs, slots, rr, s, c)
