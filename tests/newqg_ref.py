"""numpy restatement of the newqg dialect (msom_create_newqg): the cell-centred one-layer model of newqg/qg.h with the Helmholtz
("1.5-layer", gp_low) inversion.

Written from the rules include/msom.h documents for the dialect -- ghost fills of psi and of zeta / q with the corner rule, comp_q, the
tendency in its expression order, the limiter, one iteration of run() -- and from helm_ref for the inversion.  Every operation is a
plain IEEE double operation in the documented order, so the strict build can be held to the same bits.

Conventions: fields are [ny][nx]; a padded field carries one ghost ring ([ny + 2][nx + 2]); D = L0 / nx."""
import math

import numpy as np

import helm_ref

SAMPLE = """#!sh
# input parameter files

N  = 128
L0 = 100

f0 = 46.5
hEkb  = 0.0
tau0 = 1e-3
nu = 0.5
beta = 0.5
# sbc = 0: free slip, 100: no slip
sbc = 0.
# dh must be an array
dh   = [1.0]
gp_low = 2500.

# timestepping
DT    = 5.e-2
tend  = 200.
dtout = 0.1
CFL   = 0.2
TOLERANCE = 1e-5
"""


class Par:
    """parameters and their derived values (newqg/extra.h:71, newqg/qg.h:295,348-354)"""

    def __init__(self, N=64, Ny=None, L0=1.0, DT=1e10, CFL=0.5, TOLERANCE=1e-3, f0=1.0, beta=0.0, hEkb=0.0, tau0=0.0, nu=0.0, gp_low=0.0,
                 sbc=0.0, dh0=1.0, tend=1.0, dtout=1.0):
        self.nx, self.ny = N, N if Ny is None else Ny
        self.L0, self.CFL, self.tol = float(L0), float(CFL), float(TOLERANCE)
        self.f0, self.beta, self.hEkb, self.tau0, self.nu, self.gp_low, self.sbc, self.dh0 = (float(v) for v in (f0, beta, hEkb, tau0, nu, gp_low, sbc, dh0))
        self.D = self.L0 / N
        sq = self.D * self.D
        self.DT_in, self.tend, self.dtout = float(DT), float(tend), float(dtout)
        self.DT = float(DT)
        if self.nu != 0:
            self.DT = 0.5 * min(self.DT, sq / self.nu / 4.0)
        self.bc_fac = self.sbc / ((0.5 * self.sbc + 1) * sq)
        self.iRd2_low = -(self.f0 * self.f0) / (self.gp_low * self.dh0) if self.gp_low != 0 else 0.0
        self.periodic = self.sbc == -1
        self.cek = self.hEkb * self.f0 / (2 * self.dh0)
        n = 0
        while (self.nx >> n) >= 2 and (self.ny >> n) >= 2 and ((self.nx >> n) << n) == self.nx and ((self.ny >> n) << n) == self.ny:
            n += 1
        self.dims = [(self.nx >> k, self.ny >> k) for k in range(n)]

    def text(self, **extra):
        """a params.in of this model"""
        keys = dict(N=self.nx, Ny=self.ny, L0=self.L0, DT=self.DT_in, tend=self.tend, dtout=self.dtout, CFL=self.CFL, TOLERANCE=self.tol, f0=self.f0, beta=self.beta, hEkb=self.hEkb, tau0=self.tau0,
                    nu=self.nu, gp_low=self.gp_low, sbc=self.sbc)
        keys.update(extra)
        return "".join(f"{k} = {v!r}\n" for k, v in keys.items()) + f"dh = [{self.dh0!r}]\n"


def sample_par(N, Ny=None, **over):
    """the constants of newqg/params.in at another size"""
    kw = dict(N=N, Ny=Ny, L0=100, f0=46.5, hEkb=0.0, tau0=1e-3, nu=0.5, beta=0.5, sbc=0.0, dh0=1.0, gp_low=2500.0, DT=5e-2, tend=200.0, dtout=0.1, CFL=0.2,
              TOLERANCE=1e-5)
    kw.update(over)
    return Par(**kw)


def pad_psi(psi, periodic):
    """psi with its ghost ring: dirichlet(0) -- edges -v, corners by the y rule over the x-ghost column, +v -- or wrapped"""
    return helm_ref.pad(psi[None], periodic)[0]


def pad_zq(f, pp, bc_fac, periodic):
    """zeta / q with their ghost ring: bc_fac * (psi[interior] - psi[ghost]), x sides first, then the y sides over every column, the
    x-ghost columns included (a corner is bc_fac * (psi[x-ghost, interior row] - psi[corner ghost])); or wrapped.  pp: padded psi"""
    if periodic:
        return helm_ref.pad(f[None], True)[0]
    ny, nx = f.shape
    g = np.zeros((ny + 2, nx + 2))
    g[1:-1, 1:-1] = f
    g[1:-1, 0] = bc_fac * (pp[1:-1, 1] - pp[1:-1, 0])
    g[1:-1, -1] = bc_fac * (pp[1:-1, -2] - pp[1:-1, -1])
    g[0, :] = bc_fac * (pp[1, :] - pp[0, :])
    g[-1, :] = bc_fac * (pp[-2, :] - pp[-1, :])
    return g


def lap(p, D):
    """((((E + W) + N) + S) - 4 c) / (D*D) on the interior of a padded field"""
    return ((((p[1:-1, 2:] + p[1:-1, :-2]) + p[2:, 1:-1]) + p[:-2, 1:-1]) - 4 * p[1:-1, 1:-1]) / (D * D)


def comp_q(psi, par):
    """q = lap(psi); gp_low != 0: q = q + iRd2_low * psi"""
    q = lap(pad_psi(psi, par.periodic), par.D)
    if par.gp_low != 0:
        q = q + par.iRd2_low * psi
    return q


def jacobian(p, z, D):
    """the Arakawa Jacobian J(psi, zeta) of padded fields, the ten terms summed left to right, / ((12 D) D)"""
    c = (slice(1, -1), slice(1, -1))
    E, W, N, S = (slice(1, -1), slice(2, None)), (slice(1, -1), slice(None, -2)), (slice(2, None), slice(1, -1)), (slice(None, -2), slice(1, -1))
    NE, NW, SE, SW = (slice(2, None), slice(2, None)), (slice(2, None), slice(None, -2)), (slice(None, -2), slice(2, None)), (slice(None, -2), slice(None, -2))
    s = (p[E] - p[W]) * (z[N] - z[S])
    s = s + (p[S] - p[N]) * (z[E] - z[W])
    s = s + p[E] * (z[NE] - z[SE])
    s = s - p[W] * (z[NW] - z[SW])
    s = s - p[N] * (z[NE] - z[NW])
    s = s + p[S] * (z[SE] - z[SW])
    s = s + z[N] * (p[NE] - p[NW])
    s = s - z[S] * (p[SE] - p[SW])
    s = s - z[E] * (p[NE] - p[SE])
    s = s + z[W] * (p[NW] - p[SW])
    return s / ((12.0 * D) * D)


def tendency(psi, par, qforc=None):
    """(zeta, dq) of update_qg after the inversion, in the documented order"""
    D = par.D
    pp = pad_psi(psi, par.periodic)
    zeta = lap(pp, D)
    zp = pad_zq(zeta, pp, par.bc_fac, par.periodic)
    dq = 0.0 + ((-jacobian(pp, zp, D)) - (par.beta * (pp[1:-1, 2:] - pp[1:-1, :-2])) / (2 * D))
    dq = dq + par.nu * lap(zp, D)
    dq = dq - par.cek * zeta
    if qforc is not None:
        dq = dq + qforc
    return zeta, dq


def umax(psi, par):
    """max |u| over the faces, u = (0.25 * (((a - b) + c) - d)) / D as advection_pv writes it (newqg/qg.h:207)"""
    p = pad_psi(psi, par.periodic)
    ny, nx = psi.shape
    # x faces (i = 0 .. nx, j = 0 .. ny - 1), padded indices +1: psi[0,1] - psi[0,-1] + psi[-1,1] - psi[-1,-1]
    ux = 0.25 * (((p[2:, 1:] - p[:-2, 1:]) + p[2:, :-1]) - p[:-2, :-1]) / par.D
    # y faces (i = 0 .. nx - 1, j = 0 .. ny), the same expression with the directions exchanged
    uy = 0.25 * (((p[1:, 2:] - p[1:, :-2]) + p[:-1, 2:]) - p[:-1, :-2]) / par.D
    return max(float(np.abs(ux).max()), float(np.abs(uy).max()))


class Limiter:
    """the dt limiter of advection_pv (newqg/qg.h:202-219) with its static `previous`"""

    def __init__(self):
        self.previous = 0.0

    def __call__(self, um, dtmax, par):
        dtmax = dtmax / par.CFL
        if um != 0.0:
            dt = par.D / um
            if dt < dtmax:
                dtmax = dt
        dtmax = dtmax * par.CFL
        if dtmax > self.previous:
            dtmax = (self.previous + 0.1 * dtmax) / 1.1
        self.previous = dtmax
        return dtmax


def invert(psi, q, par, tol=None, **kw):
    """poisson(psi, q, lambda = iRd2_low): returns (psi, Stats)"""
    ibu = helm_ref.ibu_levels([par.iRd2_low], len(par.dims))
    pm, st = helm_ref.solve(psi[None], q[None], ibu, par.dims, par.L0, par.tol if tol is None else tol, par.periodic, **kw)
    return pm[0], st[0]


def dtnext(t, tnext, dt):
    """dtnext() of Basilisk"""
    if tnext != math.inf and tnext > t:
        n = int((tnext - t) / dt)
        if n == 0:
            dt = tnext - t
        else:
            dt1 = (tnext - t) / n
            if dt1 > dt * (1.0 + 1e-9):
                dt = (tnext - t) / (n + 1)
            elif dt1 < dt:
                dt = dt1
            tnext = t + dt
    else:
        tnext = t + dt
    return dt, tnext


class Model:
    """state of one handle: psi, q, zeta, dq, the limiter, time"""

    def __init__(self, par, psi, qforc=None, tol=None):
        self.par, self.tol = par, par.tol if tol is None else tol
        self.psi = np.array(psi, dtype=np.float64)
        self.qforc = qforc
        self.q = comp_q(self.psi, par)   # set_const
        self.zeta = np.zeros_like(self.psi)
        self.dq = np.zeros_like(self.psi)
        self.lim = Limiter()
        self.t, self.tnext, self.iter, self.dt = 0.0, math.inf, 0, 0.0
        self.stats = None

    def update(self, q, dtmax):
        self.psi, self.stats = invert(self.psi, q, self.par, self.tol)
        self.zeta, self.dq = tendency(self.psi, self.par, self.qforc)
        return self.lim(umax(self.psi, self.par), dtmax, self.par)

    def step(self):
        self.dt, tnext = dtnext(self.t, self.tnext, self.update(self.q, self.par.DT))
        pred = self.q + self.dq * (self.dt / 2.0)
        self.update(pred, self.dt)
        self.q = self.q + self.dq * self.dt
        self.t = tnext
        self.iter += 1
        return self.dt

    def ke_terms(self):
        """the terms -0.5 * psi * lap(psi) * D^2 of newqg/qg.c:89-91"""
        D = self.par.D
        return -0.5 * self.psi * lap(pad_psi(self.psi, self.par.periodic), D) * (D * D)
