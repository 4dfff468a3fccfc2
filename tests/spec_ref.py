"""The contract of the msom_spec_* block (include/msom.h) in numpy, written from its formulas: integer bin membership on the signed
wavenumber indices and numpy.fft.fft2.  Every function takes a dtype, so that the same code runs in numpy.longdouble (numpy transforms it
natively) and gives the tests their measure of fp64 rounding.  Arrays are [layers][ny][nx] or [ny][nx]."""
import numpy as np


def r2(nx, ny):
    """R2(i, j) = (i sx)^2 + (j sy)^2 on the fftshift-ed plane [ny][nx], exact integers"""
    nmax = max(nx, ny)
    i = np.arange(-nx // 2, nx // 2, dtype=np.int64) * (nmax // nx)
    j = np.arange(-ny // 2, ny // 2, dtype=np.int64) * (nmax // ny)
    return j[:, None] ** 2 + i[None, :] ** 2


def nbins(nx, ny):
    return max(nx, ny) // 2 - 2


def _ranges(nx, ny):
    """the points of the plane sorted by R2, and per bin r the slices of that order with r^2 <= R2 <= (r + 1)^2 and (r + 1)^2 <= R2"""
    R2 = r2(nx, ny).ravel()
    order = np.argsort(R2, kind="stable")
    R2s = R2[order]
    r = np.arange(nbins(nx, ny), dtype=np.int64)
    lo = np.searchsorted(R2s, r * r, side="left")
    hi = np.searchsorted(R2s, (r + 1) ** 2, side="right")
    flo = np.searchsorted(R2s, (r + 1) ** 2, side="left")
    return order, lo, hi, flo


def count(nx, ny):
    _, lo, hi, _ = _ranges(nx, ny)
    return hi - lo


def kr(nx, ny, D, dtype=np.float64):
    return np.arange(1, nbins(nx, ny) + 1).astype(dtype) / (dtype(max(nx, ny)) * dtype(D))


def spec_2d(a, b, D, dtype=np.float64):
    """Re(fft2(a) conj fft2(b)) D^4, fftshift-ed on the last two axes"""
    a, b = np.asarray(a, dtype=dtype), np.asarray(b, dtype=dtype)
    A, B = np.fft.fft2(a), np.fft.fft2(b)
    assert A.real.dtype == dtype
    s = (A.real * B.real + A.imag * B.imag) * dtype(D) ** 4
    return np.fft.fftshift(s, axes=(-2, -1))


def spec_1d(a, b, D, dtype=np.float64):
    """spec[..., r] = 2 pi kr[r] (sum over bin r of spec_2D) / count[r]"""
    return spec_1d_of(spec_2d(a, b, D, dtype), D, dtype)


def flux(a, b, D, dtype=np.float64):
    """flux[..., r] = (sum over (r + 1)^2 <= R2 of spec_2D) / (nx D) / (ny D)"""
    return flux_of(spec_2d(a, b, D, dtype), D, dtype)


def spec_1d_of(s2, D, dtype=np.float64):
    """spec_1d from a plane spec_2d already holds"""
    assert s2.dtype == dtype
    ny, nx = s2.shape[-2:]
    order, lo, hi, _ = _ranges(nx, ny)
    s2 = s2.reshape(s2.shape[:-2] + (-1,))[..., order]
    k = kr(nx, ny, D, dtype)
    two_pi = 2 * (np.pi if dtype is np.float64 else np.arctan(dtype(1)) * 4)
    out = np.empty(s2.shape[:-1] + (len(k),), dtype=dtype)
    for r in range(len(k)):
        out[..., r] = two_pi * k[r] * s2[..., lo[r]:hi[r]].sum(axis=-1) / dtype(hi[r] - lo[r])
    return out


def flux_of(s2, D, dtype=np.float64):
    """flux from a plane spec_2d already holds"""
    assert s2.dtype == dtype
    ny, nx = s2.shape[-2:]
    order, _, _, flo = _ranges(nx, ny)
    s2 = s2.reshape(s2.shape[:-2] + (-1,))[..., order]
    dk2 = (1 / (dtype(nx) * dtype(D))) * (1 / (dtype(ny) * dtype(D)))
    out = np.empty(s2.shape[:-1] + (len(flo),), dtype=dtype)
    ends = list(flo[1:]) + [s2.shape[-1]]      # the rings (r + 1)^2 <= R2 < (r + 2)^2 (the last one open), summed from the outside in
    tail = np.zeros(s2.shape[:-1], dtype=dtype)
    for r in range(len(flo) - 1, -1, -1):
        tail = tail + s2[..., flo[r]:ends[r]].sum(axis=-1)
        out[..., r] = tail * dk2
    return out
