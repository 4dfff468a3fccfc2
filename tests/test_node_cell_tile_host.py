"""The index arithmetic of the cell tile layer of the vertex model (the ctile_* functions of msom_amd/csrc/node_tile_inl.h: cell windows,
even origins of the tiled levels, ring sources, the piece offsets of the cell gather and the global noise counter) against brute force
over every global cell, in a stand-alone program built with AddressSanitizer and UBSan (tools/node_cell_tile_host_check.cpp); and the
Python helpers that cut a global cell field into tile windows and put it together again.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from msom_amd.tiling import cell_assemble, cell_tile_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cell_tile_index_arithmetic_equals_brute_force_under_sanitizers(tmp_path):
    exe = str(tmp_path / "node_cell_tile_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "node_cell_tile_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # N in {8 .. 256} x px, py in {1, 2, 4, 8}: 96 decompositions, of which the 7 with N = 8 and 8 tiles a side have one-cell tiles
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 89
    assert "89 decompositions checked, 7 refused, 0 failures" in r.stdout


def gather_level(N, px, py, mg_coarse):
    """ntile_kg of node_tile_inl.h"""
    lim, k = max(mg_coarse, px, py), 0
    while (N >> k) >= 2 and (N >> k) > lim:
        k += 1
    return 1 if px * py > 1 and k == 0 else k


def test_cell_windows_round_trip_a_global_field_on_every_level():
    rng = np.random.default_rng(3)
    seen = 0
    for N in (8, 16, 32, 64, 128, 256):
        for px in (1, 2, 4, 8):
            for py in (1, 2, 4, 8):
                if px * py > 1 and (N // px < 2 or N // py < 2):
                    with pytest.raises(ValueError):
                        cell_tile_window(N, px, py, 0)
                    continue
                for mgc in (0, 4, 8, 32):
                    kg = gather_level(N, px, py, mgc)
                    for k in range(kg + 1):                     # the tiled levels and the pieces of the gather
                        n = N >> k
                        a = rng.standard_normal((2, n, n))
                        wins = [cell_tile_window(N, px, py, r, k) for r in range(px * py)]
                        count = np.zeros((n, n), int)
                        for sy, sx in wins:
                            assert (sy.stop - sy.start, sx.stop - sx.start) == (n // py, n // px)
                            count[sy, sx] += 1
                        assert np.all(count == 1)               # a cell belongs to exactly one tile
                        assert np.array_equal(cell_assemble([a[:, sy, sx] for sy, sx in wins], N, px, py, k), a)
                        seen += 1
    assert seen > 300
    with pytest.raises(ValueError):
        cell_assemble([np.zeros((4, 4))] * 3, 8, 2, 2)
    with pytest.raises(ValueError):
        cell_assemble([np.zeros((4, 4)), np.zeros((4, 3))], 8, 2, 1)
    with pytest.raises(ValueError):
        cell_tile_window(8, 2, 1, 2)
    with pytest.raises(ValueError):
        cell_tile_window(8, 4, 1, 0, k=2)                       # 2 cells for 4 tiles a side
