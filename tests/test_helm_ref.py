"""helm_ref (the numpy restatement of the modal PV inversion) against the layered CPU oracle and against comp_q, and the
properties of the seeded right-hand side that tests/test_gpu_modal_invert.py relies on.  No GPU."""
import functools

import numpy as np
import pytest

import helm_ref as H
import modes_ref as R
import orc

CASES = [(16, 3), (32, 6)]
IDS = [f"{n}x{n}x{nl}" for n, nl in CASES]
SEED = 7          # unit-normal q whose per-mode cycle counts differ and whose residuals stay clear of TOLERANCE (asserted below)
TOL_LOOSE = 1e-3


def unit_normal_q(nl, ny, nx, seed=SEED):
    return np.random.default_rng(seed).standard_normal((nl, ny, nx))


def levels(nx, ny):
    """the cell-centred levels of a walled N x Ny grid down to minlevel = 1 (the coarsest has 2 cells across its shorter side)"""
    d = [(nx, ny)]
    while min(d[-1]) > 2:
        d.append((d[-1][0] // 2, d[-1][1] // 2))
    return d


class Setup:
    def __init__(self, N, nl):
        self.N, self.nl = N, nl
        self.txt = orc.double_gyre_params(N, nl)
        o = orc.Oracle(self.txt, quiet=1)
        o.set(orc.PSI, np.zeros((nl, N, N)))
        o.set_const()
        self.L0 = o.param("L0")
        self.dh = np.array([o.param(f"dh_{l}") for l in range(nl)])
        self.S = o.get(orc.S)[:nl - 1, 0, 0]              # uniform table
        self.ibu, self.m2l, self.l2m, _ = R.modes_eigh(self.S, self.dh)
        self.A = R.amat(self.S, self.dh)
        self.dims = levels(N, N)
        assert [o.level_dims(k) for k in range(o.nlevels())] == self.dims
        self.q = unit_normal_q(nl, N, N)

    def comp_q(self, psi):
        """lap(psi) - amat psi with the Dirichlet ghosts of psi (amat's eigenvalues are -iBu)"""
        D = self.L0 / self.N
        p = H.pad(psi, False)
        lap = (p[:, 1:-1, 2:] + p[:, 1:-1, :-2] + p[:, 2:, 1:-1] + p[:, :-2, 1:-1] - 4 * psi) / (D * D)
        return lap - np.einsum("lk,kyx->lyx", self.A, psi)

    def invert(self, tol, **kw):
        return H.invert(self.q, self.l2m, self.m2l, H.ibu_levels(self.ibu, len(self.dims)), self.dims, self.L0, tol, False, **kw)


@functools.lru_cache(maxsize=None)
def setup(case):
    return Setup(*CASES[case])


@functools.lru_cache(maxsize=None)
def tight(case):
    return setup(case).invert(1e-12)


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_modal_psi_satisfies_comp_q(case):
    s = setup(case)
    psi, _, st = tight(case)
    err = np.abs(s.q - s.comp_q(psi)).max() / np.abs(s.q).max()
    print("max|q - comp_q(psi)| / max|q| =", err, "cycles", [t.i for t in st])
    assert err <= 1e-10


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_modal_psi_equals_layered_oracle(case):
    s = setup(case)
    psi, _, _ = tight(case)
    o = orc.Oracle(s.txt, quiet=1, TOLERANCE=1e-12)
    o.set(orc.PSI, np.zeros_like(s.q))
    o.set_const()
    ref = o.pyq2p(s.q)
    err = np.abs(psi - ref).max() / np.abs(ref).max()
    print("rel =", err)
    assert err <= 1e-10


@pytest.mark.parametrize("case", range(len(CASES)), ids=IDS)
def test_loose_tolerance_freezes_modes_at_different_cycles(case):
    s = setup(case)
    _, _, st = s.invert(TOL_LOOSE)
    counts = [t.i for t in st]
    print("cycles per mode", counts, "nrelax", [t.nrelax for t in st])
    assert len(set(counts)) >= 2
    for m, t in enumerate(st):
        for c, r in enumerate(t.history):
            print(f"mode {m} cycle {c + 1}: resa / TOLERANCE = {r / TOL_LOOSE:.4g}")
            assert abs(r / TOL_LOOSE - 1) >= 0.01     # round-off cannot flip a stopping decision
            assert min(abs(t.ratios[c] / 1.2 - 1), abs(t.ratios[c] / 10 - 1)) >= 0.01, t.ratios[c]   # ... nor a step of nrelax
