"""tests/spec_ref.py (the contract of msom_spec_* in numpy) against the recorded output of the reference's own fftlib.py, and the
identities the contract implies.  No GPU.

tests/golden/spec_32.npz holds data only: two seeded random fields [3][32][32] with non-zero mean and, per layer, what
msqg/scripts/fftlib.py's get_spec_2D, get_spec_1D and get_flux return for them with Delta = L0 / N, L0 = 1, plus get_len_wavenumber(N,
Delta).  It was written once on a CPU with

    a = default_rng(20261019).standard_normal((3, 32, 32)) + 0.7;  b = <the same generator>.standard_normal((3, 32, 32)) - 0.4
    spec_2d[l] = fftlib.get_spec_2D(a[l], b[l], 1 / 32);  spec_1d[l] = fftlib.get_spec_1D(...);  flux[l] = fftlib.get_flux(...)

(the command is also in the file's README entry)."""
import os

import numpy as np
import pytest

import spec_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "spec_32.npz")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLDEN)


def test_reproduces_the_reference_recording(gold):
    D = float(gold["L0"]) / int(gold["N"])
    for name, fn in (("spec_2d", R.spec_2d), ("spec_1d", R.spec_1d), ("flux", R.flux)):
        got, want = fn(gold["a"], gold["b"], D), gold[name]
        assert got.shape == want.shape
        err = np.abs(got - want).max() / np.abs(want).max()
        print(name, err)
        assert err <= 1e-13, name


def test_bin_count_of_the_reference(gold):
    N = int(gold["N"])
    assert int(gold["nbins"]) == N // 2 - 2 == R.nbins(N, N) == gold["spec_1d"].shape[1]


@pytest.mark.parametrize("nx,ny", [(32, 32), (64, 16), (8, 32)])
def test_parseval_and_first_flux(nx, ny):
    rng = np.random.default_rng(nx * 100 + ny)
    a, b = rng.standard_normal((2, ny, nx)) + 0.5, rng.standard_normal((2, ny, nx)) - 1.5
    D = 1. / nx
    s2 = R.spec_2d(a, b, D)
    ab = (a * b).sum(axis=(1, 2))
    assert np.allclose(s2.sum(axis=(1, 2)) / (nx * D) / (ny * D), ab * D * D, rtol=1e-12, atol=0)
    # only the point (0, 0) lies inside radius 1
    want = (ab - nx * ny * a.mean(axis=(1, 2)) * b.mean(axis=(1, 2))) * D * D
    assert np.allclose(R.flux(a, b, D)[:, 0], want, rtol=1e-11, atol=0)


@pytest.mark.parametrize("nx,ny,p,s", [(32, 32, 3, 5), (64, 16, 7, 8), (16, 32, 0, 4), (16, 16, 8, 0)])
def test_a_single_mode_sits_on_plus_minus_its_wavenumber(nx, ny, p, s):
    x, y = np.arange(nx)[None, :], np.arange(ny)[:, None]
    a = np.cos(2 * np.pi * (p * x / nx + s * y / ny))
    s2 = R.spec_2d(a, a, 1.)
    on = np.zeros((ny, nx), dtype=bool)
    for sg in (1, -1):   # signed indices; -n/2 stands for both +-n/2
        i, j = (sg * p + nx // 2) % nx, (sg * s + ny // 2) % ny
        on[j, i] = True
    assert np.abs(s2[~on]).max() <= 1e-12 * s2.max()
    assert np.isclose(s2[on].sum(), (a * a).sum() * nx * ny, rtol=1e-12)


def test_longdouble_runs_natively():
    a = np.random.default_rng(3).standard_normal((16, 16))
    lo, hi = R.spec_1d(a, a, 1 / 16), R.spec_1d(a, a, 1 / 16, np.longdouble)
    assert hi.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    assert 0 < float(np.abs(lo - hi).max() / np.abs(hi).max()) < 1e-14
