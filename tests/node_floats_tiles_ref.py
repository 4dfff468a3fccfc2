"""Numpy restatement of the vertex model's Lagrangian floats on tiles (include/msomn_floats.h, DESIGN.md section 8l "On tiles"): the
owner rule of msom_amd/csrc/floats_inl.h (nfloats_owner_axis, nfloats_local, floats_hop without the periodic case) and one migration
pass of two phases with messages of K records.  The arithmetic of a stage is tests/node_floats_ref.py's: on tiles a float moves
exactly as on the single tile, so a run is the single tile's run plus the bookkeeping of who holds which float, and of the floats a
full message leaves behind (NaN from then on).  x * idx is one rounding in both builds, so there is one owner rule, not two.

Also the hand-staged case the GPU tests run (tests/test_gpu_node_floats_tiled.py): N = 64, nl = 3, the mask, topography and psi_pg of
tests/test_gpu_node_tiled.py::inputs, psi frozen, a seeded 1000 floats plus placed ones; tests/test_node_floats_tiles_ref.py asserts
on the CPU what those tests rely on."""
import numpy as np

import node_floats_ref as nr
from floats_tiles_ref import first_k, hop, last_k, leaving, random_k  # noqa: F401  (the choices of a full message: the layered model's)

N, NL, L0 = 64, 3, 100.0
NSTEPS = 6
TILINGS = [(2, 1), (1, 2), (2, 2), (2, 4)]


class Tiling:
    def __init__(self, geom, px, py):
        assert geom.N % px == 0 and geom.N % py == 0
        self.g, self.px, self.py = geom, int(px), int(py)
        self.tx, self.ty = geom.N // px, geom.N // py          # cells of a tile: it holds (tx + 1) x (ty + 1) vertices


def owner_axis(i0, tn, p):
    """i0 / tn: the seam's vertex is the first of the upper tile's cells; i0 <= N - 1, so x = L0 belongs to the last tile"""
    return np.minimum(np.maximum(i0, 0) // tn, p - 1)


def owner(t, x, y):
    """(col, row, ok, i0, j0) of positions; ok False: the position cannot be located (the float is lost and stays where it is)"""
    i0, j0, a, b, _, _ = nr.locate(t.g, x, y)
    ok = ~(np.isnan(a) | np.isnan(b))
    return owner_axis(i0, t.tx, t.px), owner_axis(j0, t.ty, t.py), ok, i0, j0


def local_corners(t, col, row, i0, j0):
    """the lower corner in the owner's indices: (i0 - ox, j0 - oy); the cell's corners are these and these + 1"""
    return i0 - col * t.tx, j0 - row * t.ty


def home(t, x, y):
    """the rank that owns positions (begin: no message is needed)"""
    col, row, ok, _, _ = owner(t, x, y)
    assert ok.all()
    return row * t.px + col


def migrate(t, where, hx, hy, K, pick=first_k, rng=None):
    """One pass behind a stage: where[id] = rank that holds id (row * px + col), (hx, hy) the positions the next stage evaluates.
    x phase (W / E), then y phase (S / N) over all residents, arrivals included.  Of the floats that want into one message the
    K that `pick` names go, the rest are unsent; so is a float whose owner is farther than a neighbour.  Walls on every side.
    Returns (where, unsent ids, stats): stats counts records per direction W E S N, diagonal movers, far ones, owner changes."""
    where = where.copy()
    col, row, ok, _, _ = owner(t, hx, hy)
    dead = ~ok
    unsent = []
    moved = np.zeros((2, where.size), dtype=bool)
    stats = dict(W=0, E=0, S=0, N=0, diag=0, far=0, changed=0)
    for ph in (0, 1):
        p = t.py if ph else t.px
        at = where // t.px if ph else where % t.px
        h = hop(row if ph else col, at, p, False)
        h[dead] = 0
        far = np.flatnonzero(h == 2)
        stats["far"] += far.size
        unsent.extend(far.tolist())
        dead[far] = True
        new = where.copy()
        for r in range(t.px * t.py):
            for d in (-1, 1):
                ids = np.flatnonzero((where == r) & (h == d))
                if not ids.size:
                    continue
                go = pick(ids, min(K, ids.size), rng)
                stay = np.setdiff1d(ids, go)
                unsent.extend(stay.tolist())
                dead[stay] = True
                ix, iy = r % t.px, r // t.px
                if ph:
                    iy += d
                else:
                    ix += d
                assert 0 <= ix < t.px and 0 <= iy < t.py        # no message across a wall
                new[go] = iy * t.px + ix
                moved[ph, go] = True
                stats[("SN" if ph else "WE")[d == 1]] += go.size
        where = new
    stats["diag"] = int((moved[0] & moved[1]).sum())
    stats["changed"] = int((moved[0] | moved[1]).sum())
    return where, np.array(sorted(unsent), dtype=np.int64), stats


def explain(t, where, hx, hy, K, unsent, tries=200):
    """the pass that leaves behind exactly `unsent`: (where, unsent ids, stats) of migrate, or None when no choice does"""
    want = np.asarray(sorted(unsent), dtype=np.int64)
    for seed in [None] + list(range(tries)):
        res = migrate(t, where, hx, hy, K, leaving(unsent, seed))
        if np.array_equal(res[1], want):
            return res
    return None


# ------------------------------------------------------------------ the hand-staged case

def case_inputs():
    """MASK, PSI, TOPO, PSIPG of the tiled model tests: an island across the vertical seam, land over the cross point, a bay on the
    north wall"""
    from test_gpu_node_tiled import inputs
    return inputs(N, NL)


def placed_floats(g, mask):
    """the placed floats, the same for every tiling of TILINGS (vertical seam at N / 2, horizontal seams at N / 4, N / 2, 3 N / 4):
    exactly on the seams, on the cross points, on the wall vertices at the seam ends, in all-land cells on either side of a seam, on
    the nextafter neighbours of seam positions, at x = L0 and at y = L0, and rows of floats a little to either side of every seam.
    Returns x, y, dict name -> index array"""
    n, L = g.N, g.L0
    D = L / n
    sx, sy = [n // 2 * D], [n // 4 * D, n // 2 * D, 3 * n // 4 * D]
    xs, ys, groups = [], [], {}

    def add(name, px, py):
        px, py = np.broadcast_arrays(np.atleast_1d(np.asarray(px, dtype=float)), np.atleast_1d(np.asarray(py, dtype=float)))
        k0 = len(xs)
        xs.extend(px.tolist())
        ys.extend(py.tolist())
        groups[name] = np.concatenate([groups.get(name, np.zeros(0, dtype=np.int64)), np.arange(k0, len(xs))])

    along = np.array([0.37 * D, 3.5 * D, 7.21 * D, 20.4 * D, 41.77 * D, L - 2.6 * D])
    for s in sx:
        add("seam", s, along)
        add("wall_at_seam", [s, s], [0.0, L])
        add("next", [np.nextafter(s, 0), np.nextafter(s, L)] * 3, np.repeat(along[1:4], 2))
    for s in sy:
        add("seam", along, s)
        add("wall_at_seam", [0.0, L], [s, s])
        add("next", np.repeat(along[1:4], 2), [np.nextafter(s, 0), np.nextafter(s, L)] * 3)
    for a in sx:
        for b in sy:
            add("cross", a, b)
            add("next", [np.nextafter(a, 0), np.nextafter(a, L), a, np.nextafter(a, 0)], [np.nextafter(b, L), b, np.nextafter(b, 0), np.nextafter(b, 0)])
            for q in (0.1, 0.03, 0.01, 0.003):                  # every quadrant, ever closer: whichever way the flow goes there, some
                for ox, oy in ((-1, -1), (1, 1), (-1, 1), (1, -1), (-1.2, 0.8), (0.8, -1.2), (0.9, 1.1)):   # cross both seams in one stage
                    add("around_cross", a + q * ox * D, b + q * oy * D)
    # all-land cells whose edge is a seam: the island across the vertical seam, the land over the cross point
    li, lj = nr.land_cells(mask)
    for s, line, other in [(n // 2, li, lj)] + [(k, lj, li) for k in (n // 4, n // 2, 3 * n // 4)]:
        for c in (s - 1, s):                                   # the cell below the seam and the one above it
            for o in other[line == c][:3]:
                p, q = (c + (0.8 if c < s else 0.15)) * D, (o + 0.45) * D
                add("land_at_seam", *((p, q) if line is li else (q, p)))
    assert groups["land_at_seam"].size >= 8 and np.all(nr.on_land(g, mask, np.array(xs)[groups["land_at_seam"]], np.array(ys)[groups["land_at_seam"]]))
    add("east", [L, L, L], [0.23 * L, n // 2 * D, 0.58 * L])
    add("north", [0.12 * L, n // 2 * D, 0.87 * L], [L, L, L])
    add("corner", [L], [L])
    fine = (np.arange(40) + 0.29) * L / 40
    for s in sx:
        for off in (-0.3 * D, -0.07 * D, 0.05 * D, 0.3 * D):
            add("beside", s + off, fine)
    for s in sy:
        for off in (-0.3 * D, -0.07 * D, 0.05 * D, 0.3 * D):
            add("beside", fine, s + off)
    return np.array(xs), np.array(ys), groups


def stage_dt(g, P, frac=0.4):
    """dt with which a stage moves a float by at most about frac cells: a velocity component is at most max |difference of
    neighbouring vertices| * idx"""
    dmax = max(np.abs(np.diff(P, axis=1)).max(), np.abs(np.diff(P, axis=2)).max())
    return frac / (dmax * g.idx * g.idx)


class Case:
    """the inputs, the frozen stream function P = PSI + PSIPG, the floats and the dt of the stages; one for all tilings"""

    def __init__(self, nseed=1000, seed=11):
        self.inp = case_inputs()
        self.mask = self.inp["MASK"][0]
        self.g = nr.Geom(N, L0)
        self.P = self.inp["PSI"] + self.inp["PSIPG"]
        x, y, lay = nr.seeded_floats(self.g, nseed, NL, seed=seed)
        wx, wy, self.groups = placed_floats(self.g, self.mask)
        self.groups = {k: v + nseed for k, v in self.groups.items()}
        self.x, self.y = np.concatenate([x, wx]), np.concatenate([y, wy])
        self.layer = np.concatenate([lay, (np.arange(wx.size) % NL).astype(np.int32)])
        self.n = self.x.size
        self.dt = stage_dt(self.g, self.P)

    def tiling(self, px, py):
        return Tiling(self.g, px, py)


def run(t, P, x, y, layer, dt, nsteps, K, pick=first_k, seed=0):
    """nsteps RK2 steps with P frozen and a migration pass behind every stage.  Returns the positions after every step (unsent
    floats NaN), the rank of every id after every pass, the statistics of every pass, and their sums."""
    rng = np.random.default_rng(seed)
    g = t.g
    x, y = x.copy(), y.copy()
    where = home(t, x, y)
    tot = dict(W=0, E=0, S=0, N=0, diag=0, far=0, changed=0, unsent=0)
    pos, wh, per = [], [], []
    xh, yh = x.copy(), y.copy()
    with np.errstate(invalid="ignore"):
        for _ in range(nsteps):
            for stage in (1, 2):
                if stage == 1:
                    xh, yh = nr.stage1(g, P, x, y, layer, dt)
                    hx, hy = xh, yh
                else:
                    x, y = nr.stage2(g, P, x, y, xh, yh, layer, dt)
                    hx, hy = x, y
                where, uns, st = migrate(t, where, hx, hy, K, pick, rng)
                st["unsent"] = uns.size
                for k in st:
                    tot[k] += st[k]
                for a in (x, y, xh, yh):
                    a[uns] = np.nan
                wh.append(where.copy())
                per.append(st)
            pos.append((x.copy(), y.copy()))
    return pos, wh, per, tot
