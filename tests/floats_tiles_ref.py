"""Numpy restatement of the Lagrangian floats on tiles (include/msom_floats.h, DESIGN.md section 8k "On tiles"): the owner rule of
msom_amd/csrc/floats_inl.h (floats_owner_axis, floats_hop) and one migration pass of two phases with messages of K records.  The
arithmetic of a stage is tests/floats_ref.py's: on tiles a float moves exactly as on the single tile, so a run is the single tile's
run plus the bookkeeping of who holds which float, and of the floats a full message leaves behind (NaN from then on).

Also the hand-staged case the GPU tests run (tests/test_gpu_floats_tiled.py): psi frozen, 16-cell tiles, a seeded 1000 floats plus
placed ones; tests/test_floats_tiles_ref.py asserts on the CPU what those tests rely on."""
from fractions import Fraction

import numpy as np

import floats_ref as fr

L0 = 80.0
TILE = 16


class Tiling:
    def __init__(self, geom, px, py):
        assert geom.nx % px == 0 and geom.ny % py == 0
        self.g, self.px, self.py = geom, int(px), int(py)
        self.tnx, self.tny = geom.nx // px, geom.ny // py


def owner_axis(i0, tn):
    """max(i0, 0) / tn: the ghost column -1 of a wall belongs to the first tile"""
    return np.maximum(i0, 0) // tn


def lower_corner(x, idx, n, periodic, fused=False):
    """(i0, ok) of floats_axis.  fused: xi = x * idx - 0.5 rounded once, as the product build's fused multiply-add forms it (the strict
    build and floats_ref round the product first); the two differ for a float within an ulp of a cell-centre line"""
    x = np.asarray(x, dtype=np.float64)
    if fused:
        xi = np.full(x.shape, np.nan)
        for k in np.flatnonzero(np.isfinite(x) & (np.abs(x) < 1e300)):
            xi[k] = float(Fraction(float(x[k])) * Fraction(float(idx)) - Fraction(1, 2))
    else:
        xi = x * np.float64(idx) - 0.5
    ok = np.isfinite(xi)
    f = np.floor(np.where(ok, xi, 0.0))
    if periodic:
        f = np.fmod(f, float(n))
        f = np.clip(np.where(f < 0, f + n, f), 0, n - 1)
    else:
        f = np.clip(f, -1, n - 1)
    return f.astype(np.int64), ok


def owner(t, x, y, fused=False):
    """(col, row, ok) of positions; ok False: the position cannot be located (the float is lost and stays where it is)"""
    i0, okx = lower_corner(x, t.g.idx, t.g.nx, t.g.periodic, fused)
    j0, oky = lower_corner(y, t.g.idx, t.g.ny, t.g.periodic, fused)
    return owner_axis(i0, t.tnx), owner_axis(j0, t.tny), okx & oky, i0, j0


def hop(own, at, p, periodic):
    """0 stays, +1 / -1 to the upper / lower neighbour (periodic: wrapped; both the same tile: the upper), 2 farther"""
    own, at = np.asarray(own), np.asarray(at)
    h = np.full(own.shape, 2, dtype=np.int64)
    lo = (own == at - 1) | ((own == (at - 1 + p) % p) if periodic else False)
    hi = (own == at + 1) | ((own == (at + 1) % p) if periodic else False)
    h[lo] = -1
    h[hi] = 1          # after lo: where both neighbours are one tile, the upper
    h[own == at] = 0
    return h


def first_k(ids, k, rng=None):
    return ids[:k]


def last_k(ids, k, rng=None):
    return ids[len(ids) - k:]


def random_k(ids, k, rng):
    return np.sort(rng.permutation(ids)[:k])


def leaving(unsent, seed=None):
    """the choice a run was seen to make: of the floats that want into one message, those in `unsent` are left behind first.  Where
    more of them want into a message of the x phase than it must leave behind (the others were left behind by the y phase), which
    ones is not seen: in turn (seed None) or drawn"""
    unsent = np.asarray(sorted(unsent), dtype=np.int64)
    draw = None if seed is None else np.random.default_rng(seed)

    def pick(ids, k, rng=None):
        last = ids[np.isin(ids, unsent)]
        if draw is not None:
            last = draw.permutation(last)
        return np.sort(np.concatenate([ids[~np.isin(ids, unsent)], last])[:k])
    return pick


def explain(t, where, hx, hy, K, unsent, fused=False, tries=200):
    """the pass that leaves behind exactly `unsent`: (where, unsent ids, stats) of migrate, or None when no choice does"""
    for seed in [None] + list(range(tries)):
        res = migrate(t, where, hx, hy, K, leaving(unsent, seed), fused=fused)
        if np.array_equal(res[1], np.asarray(sorted(unsent), dtype=np.int64)):
            return res
    return None


def migrate(t, where, hx, hy, K, pick=first_k, rng=None, fused=False):
    """One pass behind a stage: where[id] = rank that holds id (row * px + col), (hx, hy) the positions the next stage evaluates.
    x phase (W / E), then y phase (S / N) over all residents, arrivals included.  Of the floats that want into one message the
    K that `pick` names go, the rest are unsent; so is a float whose owner is farther than a neighbour.
    Returns (where, unsent ids, stats): stats counts records per direction W E S N, diagonal movers, far ones, owner changes."""
    where = where.copy()
    col, row, ok, _, _ = owner(t, hx, hy, fused)
    dead = ~ok
    unsent = []
    moved = np.zeros((2, where.size), dtype=bool)
    stats = dict(W=0, E=0, S=0, N=0, diag=0, far=0, changed=0)
    for ph in (0, 1):
        p = t.py if ph else t.px
        at = where // t.px if ph else where % t.px
        h = hop(row if ph else col, at, p, t.g.periodic)
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
                    iy = (iy + d) % t.py
                else:
                    ix = (ix + d) % t.px
                new[go] = iy * t.px + ix
                moved[ph, go] = True
                stats[("SN" if ph else "WE")[d == 1]] += go.size
        where = new
    stats["diag"] = int((moved[0] & moved[1]).sum())
    stats["changed"] = int((moved[0] | moved[1]).sum())
    return where, np.array(sorted(unsent), dtype=np.int64), stats


def home(t, x, y, fused=False):
    """the rank that owns positions (begin: no message is needed)"""
    col, row, ok, _, _ = owner(t, x, y, fused)
    assert ok.all()
    return row * t.px + col


# ------------------------------------------------------------------ the hand-staged case

def case_psi(nl, ny, nx):
    """a frozen stream function with flow across every seam in both directions: two gyres and a shorter wave, other signs per layer"""
    D = L0 / nx
    X, Y = np.meshgrid((np.arange(nx) + 0.5) * D, (np.arange(ny) + 0.5) * D)
    Lx, Ly = L0, L0 * ny / nx
    base = np.sin(2 * np.pi * X / Lx) * np.sin(np.pi * Y / Ly) + 0.6 * np.sin(np.pi * X / Lx) * np.sin(2 * np.pi * Y / Ly)
    wave = 0.35 * np.sin(3 * np.pi * X / Lx + 0.4) * np.sin(3 * np.pi * Y / Ly + 0.9)
    return np.array([(1.0 if l % 2 == 0 else -0.8) * base + (0.5 + 0.25 * l) * wave for l in range(nl)])


def placed_floats(g, px, py, nl):
    """on the seams, on the corners where four tiles meet, on a wall at a seam, on the cell-centre lines next to a seam, and a row
    of floats a little to either side of every seam; layers in turn, around the corners every point in every layer"""
    D = g.Lx / g.nx
    sx = [k * TILE * D for k in range(1, px)]
    sy = [k * TILE * D for k in range(1, py)]
    x, y = [], []
    ty = np.array([0.0, 0.37 * D, 3.5 * D, 7.21 * D, g.Ly - 2.6 * D, g.Ly])    # along a seam in x: the walls at its ends included
    tx = np.array([0.0, 0.37 * D, 3.5 * D, 7.21 * D, g.Lx - 2.6 * D, g.Lx])
    for s in sx:
        for off in (0.0, -0.5 * D, 0.5 * D, -0.11 * D, 0.13 * D):
            x += [s + off] * ty.size
            y += ty.tolist()
        fine = (np.arange(40) + 0.29) * g.Ly / 40
        for off in (-0.07 * D, 0.05 * D, 0.43 * D, 0.515 * D):   # beside the seam, beside the centre line where the owner changes
            x += [s + off] * fine.size
            y += fine.tolist()
    for s in sy:
        for off in (0.0, -0.5 * D, 0.5 * D, -0.11 * D, 0.13 * D):
            y += [s + off] * tx.size
            x += tx.tolist()
        fine = (np.arange(40) + 0.29) * g.Lx / 40
        for off in (-0.07 * D, 0.05 * D, 0.43 * D, 0.515 * D):
            y += [s + off] * fine.size
            x += fine.tolist()
    # the corners of four tiles and, half a cell on, the points where the owner changes in both directions; their neighbourhoods
    for a in [s + h for s in sx for h in (0.0, 0.5 * D)]:
        for b in [s + h for s in sy for h in (0.0, 0.5 * D)]:
            for ox, oy in ((0, 0), (-0.1, -0.1), (0.1, 0.1), (-0.1, 0.1), (0.1, -0.1), (-0.5, -0.5), (0.5, 0.5), (-0.5, 0.5), (0.5, -0.5),
                           (-0.02, -0.02), (0.02, 0.02), (-0.02, 0.02), (0.02, -0.02), (-0.005, 0.004), (0.004, -0.005)):
                x.append(a + ox * D)
                y.append(b + oy * D)
    lay = np.arange(len(x)) % nl
    nc = (px - 1) * (py - 1) * 4 * 15
    if nc:                             # the corner points once more per further layer
        x, y = x + x[-nc:] * (nl - 1), y + y[-nc:] * (nl - 1)
        lay = np.concatenate([lay] + [(lay[-nc:] + k) % nl for k in range(1, nl)])
    return np.array(x), np.array(y), lay.astype(np.int32)


class Case:
    """px x py tiles of 16 cells, nl = 2, walls: psi, its ghosted form, the floats and the dt of the stages"""

    def __init__(self, px, py, nl=2, nseed=1000):
        self.px, self.py, self.nl = px, py, nl
        self.nx, self.ny = TILE * px, TILE * py
        self.g = fr.Geom(self.nx, self.ny, L0)
        self.t = Tiling(self.g, px, py)
        self.psi = case_psi(nl, self.ny, self.nx)
        self.G = fr.ghosted_dirichlet(self.psi)
        x, y, lay = fr.seeded_floats(self.g, nseed, nl, seed=11)
        wx, wy, wl = placed_floats(self.g, px, py, nl)
        self.x, self.y = np.concatenate([x, wx]), np.concatenate([y, wy])
        self.layer = np.concatenate([lay, wl])
        self.n = self.x.size
        self.dt = stage_dt(self.g, self.G)


def stage_dt(g, G, frac=0.4):
    """dt with which a stage moves a float by at most about frac cells: a velocity component is at most max |difference of
    neighbouring psi| * idx"""
    dmax = max(np.abs(np.diff(G, axis=1)).max(), np.abs(np.diff(G, axis=2)).max())
    return frac / (dmax * g.idx * g.idx)


def run(t, G, x, y, layer, dt, nsteps, K, pick=first_k, seed=0):
    """nsteps RK2 steps with psi frozen (G ghosted, global) and a migration pass behind every stage.  Returns the positions after
    every step (unsent floats NaN), the rank of every id after every pass, and the sums of the passes' statistics."""
    rng = np.random.default_rng(seed)
    g = t.g
    x, y = x.copy(), y.copy()
    where = home(t, x, y)
    tot = dict(W=0, E=0, S=0, N=0, diag=0, far=0, changed=0, unsent=0)
    pos, wh = [], []
    xh, yh = x.copy(), y.copy()
    for _ in range(nsteps):
        for stage in (1, 2):
            if stage == 1:
                xh, yh = fr.stage1(g, G, x, y, layer, dt)
                hx, hy = xh, yh
            else:
                x, y = fr.stage2(g, G, x, y, xh, yh, layer, dt)
                hx, hy = x, y
            where, uns, st = migrate(t, where, hx, hy, K, pick, rng)
            for k in st:
                tot[k] += st[k]
            tot["unsent"] += uns.size
            for a in (x, y, xh, yh):
                a[uns] = np.nan
            wh.append(where.copy())
        pos.append((x.copy(), y.copy()))
    return pos, wh, tot
