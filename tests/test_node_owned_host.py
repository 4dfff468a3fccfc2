"""Who owns a shared vertex of the vertex model on tiles (ntile_owned_range of msom_amd/csrc/node_tile_inl.h, node_owned_window of
msom_amd/tiling.py): the owned windows cover every vertex exactly once and lie inside the held windows, and the record digest of a
global array is the sum of the digests the tiles form over what they own, with the global indices.  The C++ side runs in a stand-alone
program built with AddressSanitizer and UBSan (tools/node_owned_host_check.cpp).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from msom_amd import state
from msom_amd.tiling import node_owned_window, node_tile_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES, SIDES = (8, 32, 64), (1, 2, 4, 8)
DECOMPOSITIONS = [(N, px, py) for N in SIZES for px in SIDES for py in SIDES if px * py == 1 or (N // px >= 2 and N // py >= 2)]


def test_owned_windows_equal_brute_force_under_sanitizers(tmp_path):
    exe = str(tmp_path / "node_owned_host_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "node_owned_host_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    # N = 8 with 8 tiles a side has one-cell tiles: 7 of the 48 decompositions are refused
    assert len(DECOMPOSITIONS) == 41
    assert "FAIL" not in r.stdout and r.stdout.count(": ok") == 41
    assert "41 decompositions checked, 7 refused, 0 failures" in r.stdout


@pytest.mark.parametrize("N,px,py", DECOMPOSITIONS)
def test_node_owned_window_counts_every_vertex_once(N, px, py):
    count = np.zeros((N + 1, N + 1), int)
    for r in range(px * py):
        (oy, ox), (hy, hx) = node_owned_window(N, px, py, r), node_tile_window(N, px, py, r)
        assert (oy.start, ox.start) == (hy.start, hx.start)                       # from the tile's origin ...
        assert hy.stop - oy.stop == (r // px != py - 1) and hx.stop - ox.stop == (r % px != px - 1)   # ... without the edge it shares
        count[oy, ox] += 1
    assert np.all(count == 1)
    # brute force: vertex (I, J) belongs to the tile whose cells [ox, ox + tx) x [oy, oy + ty) it is the origin of one, the last tile
    # of a row taking the wall
    tx, ty = N // px, N // py
    J, I = np.mgrid[0:N + 1, 0:N + 1]
    want = np.minimum(J // ty, py - 1) * px + np.minimum(I // tx, px - 1)
    got = np.full((N + 1, N + 1), -1)
    for r in range(px * py):
        got[node_owned_window(N, px, py, r)] = r
    assert np.array_equal(got, want)


def test_bad_decompositions_are_refused():
    for N, px, py, rank in ((8, 8, 1, 0), (32, 3, 1, 0), (32, 2, 2, 4), (32, 2, 2, -1)):
        with pytest.raises(ValueError):
            node_owned_window(N, px, py, rank)


def owned_digest(a, N, px, py, rank):
    """what k_state_rows sums on a tile: the terms of the vertices the tile owns, with their index in the global record"""
    sy, sx = node_owned_window(N, px, py, rank)
    k = np.arange(a.size, dtype=np.uint64).reshape(a.shape)[:, sy, sx]
    bits = np.ascontiguousarray(a[:, sy, sx]).view(np.uint64)
    with np.errstate(over="ignore"):
        return int(state._mix64(bits + np.uint64(0x9E3779B97F4A7C15) * (k + np.uint64(1))).sum(dtype=np.uint64))


@pytest.mark.parametrize("N,px,py", [d for d in DECOMPOSITIONS if d[0] >= 32])
def test_the_digest_is_the_sum_of_the_owned_digests(N, px, py):
    a = np.random.default_rng(N + 10 * px + py).standard_normal((3, N + 1, N + 1))
    parts = sum(owned_digest(a, N, px, py, r) for r in range(px * py)) % (1 << 64)
    assert parts == state.digest(a)
    if px * py > 1:   # over the held windows the shared vertices count twice: not the digest
        held = 0
        for r in range(px * py):
            sy, sx = node_tile_window(N, px, py, r)
            k = np.arange(a.size, dtype=np.uint64).reshape(a.shape)[:, sy, sx]
            with np.errstate(over="ignore"):
                held += int(state._mix64(np.ascontiguousarray(a[:, sy, sx]).view(np.uint64) + np.uint64(0x9E3779B97F4A7C15) * (k + np.uint64(1))).sum(dtype=np.uint64))
        assert held % (1 << 64) != state.digest(a)
