"""Host-side helpers of the 2-D tile decomposition (one process per GPU): rank <-> tile
mapping, neighbour table and bootstrap of the library's communicator through
torch.distributed (RCCL on GPUs, gloo in the CPU tests).  Mirrors what the library does
internally (msom_create_tiled: rank r owns tile (r % px, r // px))."""
import ctypes

import numpy as np

TILE_GRIDS = {1: (1, 1), 2: (2, 1), 4: (2, 2), 8: (2, 4)}
# direction order of the library (comm.h): W E S N SW SE NW NE
DIRS = {"W": (-1, 0), "E": (1, 0), "S": (0, -1), "N": (0, 1), "SW": (-1, -1), "SE": (1, -1), "NW": (-1, 1), "NE": (1, 1)}


def tile_grid(world):
    if world not in TILE_GRIDS:
        raise ValueError(f"no tile grid defined for {world} ranks (use 1, 2, 4 or 8)")
    return TILE_GRIDS[world]


def tile_of_rank(rank, px, py):
    return rank % px, rank // px


OPPOSITE = dict(W="E", E="W", S="N", N="S", SW="NE", NE="SW", SE="NW", NW="SE")


def neighbours(rank, px, py, periodic=False):
    """periodic (sbc = -1 on tiles, msqg/qg.h:842-846): the neighbours wrap around; with 1 or 2 tiles per side both
    neighbours of an axis are the same rank (or the tile itself)"""
    ix, iy = tile_of_rank(rank, px, py)
    out = {}
    for name, (dx, dy) in DIRS.items():
        jx, jy = ix + dx, iy + dy
        if periodic:
            out[name] = (jy % py) * px + jx % px
        else:
            out[name] = jy * px + jx if (0 <= jx < px and 0 <= jy < py) else -1
    return out


def walls(rank, px, py, periodic=False):
    ix, iy = tile_of_rank(rank, px, py)
    if periodic:
        return dict(W=False, E=False, S=False, N=False)
    return dict(W=ix == 0, E=ix == px - 1, S=iy == 0, N=iy == py - 1)


def exchange_order(names):
    """posting order of one exchange (comm.hip): sends in the order of the direction they travel in, receives in the order
    of the direction the INCOMING message travels in (the opposite of the edge), so that two messages between the same
    pair of ranks pair up"""
    order = list(DIRS)
    sends = sorted(names, key=order.index)
    recvs = sorted(names, key=lambda n: order.index(OPPOSITE[n]))
    return sends, recvs


def tile_slice(rank, px, py, nx, ny):
    """(slice_y, slice_x) of this rank's tile in a global [.., gny, gnx] array."""
    ix, iy = tile_of_rank(rank, px, py)
    return slice(iy * ny, (iy + 1) * ny), slice(ix * nx, (ix + 1) * nx)


def _node_tile_cells(N, px, py):
    for name, v in (("N", N), ("px", px), ("py", py)):
        if v < 1 or v & (v - 1):
            raise ValueError(f"{name} = {v} must be a power of two")
    if N % px or N % py or (px * py > 1 and (N // px < 2 or N // py < 2)):
        raise ValueError(f"{px} x {py} tiles of at least 2 cells a side do not divide N = {N}")
    return N // px, N // py


def node_tile_window(N, px, py, rank):
    """(slice_y, slice_x) of this rank's vertices in a global [.., N + 1, N + 1] array of the vertex model.  A tile of
    Tx x Ty cells holds (Tx + 1) x (Ty + 1) vertices, the ones on its interior edges included: neighbouring windows
    overlap by one column or row (msom_amd/csrc/node_tile_inl.h)."""
    tx, ty = _node_tile_cells(N, px, py)
    if not 0 <= rank < px * py:
        raise ValueError(f"rank {rank} outside 0 .. {px * py - 1}")
    ix, iy = tile_of_rank(rank, px, py)
    return slice(iy * ty, (iy + 1) * ty + 1), slice(ix * tx, (ix + 1) * tx + 1)


def node_owned_window(N, px, py, rank):
    """(slice_y, slice_x) of the vertices this rank OWNS in a global [.., N + 1, N + 1] array: its held window without the
    last column unless the tile is the last of its row of tiles, rows likewise (ntile_owned_range of node_tile_inl.h).  The
    owned windows of all ranks cover every vertex exactly once: what a state file's records and digests count."""
    tx, ty = _node_tile_cells(N, px, py)
    if not 0 <= rank < px * py:
        raise ValueError(f"rank {rank} outside 0 .. {px * py - 1}")
    ix, iy = tile_of_rank(rank, px, py)
    return slice(iy * ty, (iy + 1) * ty + (iy == py - 1)), slice(ix * tx, (ix + 1) * tx + (ix == px - 1))


def node_assemble(pieces, N, px, py, check_shared=True):
    """Global [.., N + 1, N + 1] array from the px * py tile arrays [.., Ty + 1, Tx + 1] (in rank order) of the vertex model.
    check_shared: raise ValueError if two holders of a shared vertex disagree in any bit (-0. against 0. and different NaN
    payloads count)."""
    tx, ty = _node_tile_cells(N, px, py)
    if len(pieces) != px * py:
        raise ValueError(f"{len(pieces)} pieces for {px} x {py} tiles")
    pieces = [np.ascontiguousarray(p) for p in pieces]
    lead, dtype = pieces[0].shape[:-2], pieces[0].dtype
    bits = np.dtype(f"u{dtype.itemsize}") if dtype.kind in "fc" and dtype.itemsize in (2, 4, 8) else dtype
    out = np.empty(lead + (N + 1, N + 1), dtype)
    seen = np.zeros((N + 1, N + 1), bool)
    for rank, p in enumerate(pieces):
        if p.shape != lead + (ty + 1, tx + 1) or p.dtype != dtype:
            raise ValueError(f"piece of rank {rank}: {p.dtype}{p.shape}, expected {dtype}{lead + (ty + 1, tx + 1)}")
        sy, sx = node_tile_window(N, px, py, rank)
        if check_shared:
            shared = seen[sy, sx]
            differ = (out[..., sy, sx].view(bits) != p.view(bits)) & shared
            if differ.any():
                j, i = np.argwhere(differ.reshape((-1,) + differ.shape[-2:]).any(0))[0]
                raise ValueError(f"shared vertex ({sx.start + i}, {sy.start + j}): rank {rank} disagrees with a lower rank "
                                 f"({int(differ.sum())} values differ)")
        out[..., sy, sx] = p
        seen[sy, sx] = True
    return out


def cell_tile_window(N, px, py, rank, k=0):
    """(slice_y, slice_x) of this rank's cells in a global [.., N >> k, N >> k] array of level k of a cell pyramid of the vertex model
    (the noise, the wavelet filter).  A cell belongs to exactly one tile: the windows do not overlap.  Level k must have at least one
    cell a tile side (the library tiles the levels below param agg_level, which have two)."""
    _node_tile_cells(N, px, py)
    if not 0 <= rank < px * py:
        raise ValueError(f"rank {rank} outside 0 .. {px * py - 1}")
    n = N >> k
    if k < 0 or n < px or n < py:
        raise ValueError(f"level {k} of N = {N} has fewer than one cell a tile side on {px} x {py} tiles")
    tx, ty = n // px, n // py
    ix, iy = tile_of_rank(rank, px, py)
    return slice(iy * ty, (iy + 1) * ty), slice(ix * tx, (ix + 1) * tx)


def cell_assemble(pieces, N, px, py, k=0):
    """Global [.., N >> k, N >> k] array of cell level k from the px * py tile windows [.., Ty >> k, Tx >> k] in rank order."""
    if len(pieces) != px * py:
        raise ValueError(f"{len(pieces)} pieces for {px} x {py} tiles")
    pieces = [np.asarray(p) for p in pieces]
    n = N >> k
    out = np.empty(pieces[0].shape[:-2] + (n, n), pieces[0].dtype)
    for rank, p in enumerate(pieces):
        sy, sx = cell_tile_window(N, px, py, rank, k)
        want = pieces[0].shape[:-2] + (sy.stop - sy.start, sx.stop - sx.start)
        if p.shape != want:
            raise ValueError(f"piece of rank {rank}: {p.shape}, expected {want}")
        out[..., sy, sx] = p
    return out


def broadcast_unique_id(dist, make_id, device="cpu"):
    """Rank 0 creates the 128-byte communicator id (ncclUniqueId), everybody receives it."""
    import torch

    uid = torch.zeros(128, dtype=torch.uint8)
    if dist.get_rank() == 0:
        uid = torch.frombuffer(bytearray(make_id()), dtype=torch.uint8).clone()
    uid = uid.to(device)
    dist.broadcast(uid, 0)
    return uid.cpu().numpy().tobytes()


def rccl_unique_id(lib):
    buf = (ctypes.c_char * 128)()
    if lib.msom_comm_unique_id(buf) != 0:
        raise RuntimeError(lib.msom_last_error().decode())
    return buf.raw


def synthetic_tile(psi_fn, rank, px, py, nl, nx, ny):
    """Sample a global analytic field on this rank's tile: psi_fn(l, y01, x01) with normalised
    cell-centre coordinates of the GLOBAL domain."""
    ix, iy = tile_of_rank(rank, px, py)
    x = (np.arange(ix * nx, (ix + 1) * nx) + 0.5) / (nx * px)
    y = (np.arange(iy * ny, (iy + 1) * ny) + 0.5) / (ny * py)
    return np.stack([psi_fn(l, y, x) for l in range(nl)])
