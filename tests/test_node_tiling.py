"""The numpy helpers of the vertex model's tile decomposition (msom_amd/tiling.py: node_tile_window, node_assemble): tiles HOLD the
vertices on their interior edges, so windows overlap by one column or row and the assembly can check that all holders of a shared
vertex agree bit for bit.  Every tiling of tools/node_tile_host_check.cpp's list at N = 16.  No GPU."""
import numpy as np
import pytest

from msom_amd.tiling import node_assemble, node_tile_window, tile_of_rank

N = 16
TILINGS = [(px, py) for px in (1, 2, 4, 8) for py in (1, 2, 4, 8)]


def split(x, px, py):
    return [x[(Ellipsis,) + node_tile_window(N, px, py, r)].copy() for r in range(px * py)]


@pytest.mark.parametrize("px,py", TILINGS)
def test_windows_hold_their_interior_edges(px, py):
    tx, ty = N // px, N // py
    count = np.zeros((N + 1, N + 1), int)
    for r in range(px * py):
        sy, sx = node_tile_window(N, px, py, r)
        ix, iy = tile_of_rank(r, px, py)
        assert (sx.start, sx.stop, sy.start, sy.stop) == (ix * tx, ix * tx + tx + 1, iy * ty, iy * ty + ty + 1)
        count[sy, sx] += 1
    i = np.arange(N + 1)
    seam_x = (i % tx == 0) & (i > 0) & (i < N)
    seam_y = (i % ty == 0) & (i > 0) & (i < N)
    assert np.array_equal(count, np.outer(1 + seam_y, 1 + seam_x))   # 1 inside a tile, 2 on a seam, 4 at a cross point


@pytest.mark.parametrize("px,py", TILINGS)
@pytest.mark.parametrize("lead", [(), (3,)])
def test_assemble_of_split_is_the_identity(px, py, lead):
    rng = np.random.default_rng(100 * px + py)
    x = rng.standard_normal(lead + (N + 1, N + 1))
    x[..., 3, 5] = -0.
    pieces = split(x, px, py)
    assert pieces[0].shape == lead + (N // py + 1, N // px + 1)
    for check in (True, False):
        y = node_assemble(pieces, N, px, py, check_shared=check)
        assert y.dtype == x.dtype and np.array_equal(y.view(np.uint64), x.view(np.uint64))


@pytest.mark.parametrize("px,py", [t for t in TILINGS if t != (1, 1)])
def test_a_flipped_bit_in_one_holder_of_a_shared_vertex_raises(px, py):
    rng = np.random.default_rng(7)
    x = rng.standard_normal((2, N + 1, N + 1))
    # every shared vertex in turn would be slow: one on each kind of seam, and a cross point where there is one
    tx, ty = N // px, N // py
    spots = []
    if px > 1:
        spots.append((ty // 2, tx))
    if py > 1:
        spots.append((ty, tx // 2))
    if px > 1 and py > 1:
        spots.append((ty, tx))
    for J, I in spots:
        holders = [r for r in range(px * py) if all(s.start <= v < s.stop for s, v in zip(node_tile_window(N, px, py, r), (J, I)))]
        assert len(holders) == (4 if (J, I) == (ty, tx) and px > 1 and py > 1 else 2)
        for r in holders:
            pieces = split(x, px, py)
            sy, sx = node_tile_window(N, px, py, r)
            v = pieces[r][1, J - sy.start:J - sy.start + 1, I - sx.start].view(np.uint64)
            v ^= np.uint64(1)   # the lowest mantissa bit of this holder's copy
            with pytest.raises(ValueError, match="shared vertex"):
                node_assemble(pieces, N, px, py)
            node_assemble(pieces, N, px, py, check_shared=False)   # unchecked: either copy is taken


def test_signed_zero_and_nan_payload_count_as_different():
    x = np.zeros((N + 1, N + 1))
    pieces = split(x, 2, 1)
    pieces[1][4, 0] = -0.
    with pytest.raises(ValueError, match="shared vertex"):
        node_assemble(pieces, N, 2, 1)
    x[:] = np.nan
    assert np.isnan(node_assemble(split(x, 2, 1), N, 2, 1)).all()   # the same NaN on both holders agrees


@pytest.mark.parametrize("args", [(16, 3, 1, 0), (16, 2, 2, 4), (16, 16, 1, 0), (24, 2, 2, 0), (16, 2, 2, -1)])
def test_bad_decompositions_are_refused(args):
    with pytest.raises(ValueError):
        node_tile_window(*args)
